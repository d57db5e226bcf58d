"""How far the fp32 specification of the Philox-to-normal transform sits from float64, on every reachable input.

    python tools/normal_margins.py                      # CPU only: writes profiles/normal_transform.txt
    python tools/normal_margins.py --device margins.jsonl   # appends what the GPU test measured (SKR_PARITY_MARGINS=margins.jsonl
                                                            # pytest -m gpu tests/test_normal_transform_gpu.py)

The factors r, cos, sin of the fp32 specification (tests/normal_cases.py::oracle_parts) are evaluated over the 83,886,080 exactly
representable words and the rounding words and compared with the float64 evaluation of the same fp32 uniforms; the maxima and the bound
they compose to are the constants tests/test_normal_transform_gpu.py holds the device to (x 1.5)."""

import argparse
import json
import os
import platform
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "normal_transform.txt")
KEYS = (("E_r", "max |r - exact|"), ("E_c", "max |cos - exact|"), ("E_s", "max |sin - exact|"), ("rel_r", "max relative error of r, units of 2^-24"),
        ("composed", "composed bound E_r + R max(E_c, E_s) + R 2^-24"))  # fmt: skip


def lines_of(title: str, rep: dict) -> list[str]:
    return [title] + [f"  {k:<9} {rep[k]:.6e}   {what}" for k, what in KEYS]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", help="SKR_PARITY_MARGINS file of a GPU run of tests/test_normal_transform_gpu.py: append its figures")
    args = ap.parse_args()
    if args.device:
        rep = {}
        for line in open(args.device):
            rec = json.loads(line)
            if rec["family"] == "normal transform factors":
                rep[rec["measure"]] = rec["value"]
        with open(OUT, "a") as fh:
            fh.write("\n".join(lines_of("\ndevice (MI355X, v_log_f32 / v_sqrt_f32 / v_cos_f32 / v_sin_f32 as skr_philox.h uses them) against float64, same words:", rep)) + "\n")
        return
    import normal_cases as NC
    import numpy as np
    import torch

    rep = NC.factor_report(NC.oracle_parts, NC.representative_words(), NC.rounding_words())
    text = [
        "Philox-to-normal transform: distance of the fp32 specification (oracle noise.py::box_muller) from float64",
        f"words: the {NC.N_REPRESENTATIVE} exactly representable ones and {NC.rounding_words().numel()} rounding words (tests/normal_cases.py)",
        f"host: numpy {np.__version__}, torch {torch.__version__}, {platform.machine()}",
        "",
        *lines_of("fp32 specification against float64:", rep),
        f"  conditions that need no measurement: {'all hold' if not rep['violations'] else rep['violations']}",
    ]
    with open(OUT, "w") as fh:
        fh.write("\n".join(text) + "\n")
    print("\n".join(text))


if __name__ == "__main__":
    main()
