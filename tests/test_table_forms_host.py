"""tests/table_cases.py held to account without a GPU: its float64 reference and bound accept an fp32 evaluation in the kernels' order and
reject the errors a table-form kernel could make, on the very operands and rows tests/test_table_forms_gpu.py launches; and its grid
is what csrc/skr_step_fast.hip instantiates."""

import ctypes
import os
import re

import numpy as np
import pytest
import table_cases as TC
import torch
from conftest import ROOT

from skrample_amd import _hip

BATCH, SAMPLE = TC.SMALL[0]
CASES = [TC.Case("k1", 1), TC.Case("k1", 4, noise="on"), TC.Case("k1", 13, noise="on"), TC.Case("k1", 16, noise="on"), TC.Case("k1", 16), TC.Case("k2", 14, 1, noise="both"),
         TC.Case("k2", 4, 1, noise="zeta1"), TC.Case("rk1", 5, noise="on", kinds=(1, 2)), TC.Case("rk1", 8, kinds=(3, 3))]  # fmt: skip


def int_view(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Sample:
    "sample b of a case on the host: operands, row, normals -- each of them replaceable, which is how an error is seeded"

    def __init__(self, case: TC.Case, dtype: str, b: int, r: int, rows, present):
        self.case, self.dtype, self.td, self.b = case, dtype, TC.DTYPES[dtype], b
        self.row, self.present = rows[r], present[r]
        self.seed = TC.seeds_for(BATCH)[b]
        self.x64 = TC.operands64(case, dtype, BATCH, SAMPLE)[:, b, :]
        self.x32 = self.x64.float().numpy()
        narrow = TC.pool(dtype, BATCH, SAMPLE)[0]
        self.conv = None
        if case.family == "rk1":
            s_, o_ = (narrow[j, b * SAMPLE : (b + 1) * SAMPLE] for j in (0, 1))
            self.conv = TC.conversion_reference(s_, o_, case.kinds, tuple(self.row.convert_k))

    def normals(self, seed=None, row=None):
        seed, row = self.seed if seed is None else seed, self.row if row is None else row
        return tuple(TC.normal(seed, s, SAMPLE).astype(np.float32) for s in (row.stream0, row.stream1))

    def reference(self):
        return TC.reference64(self.case, self.td, self.x64, self.row, self.present, self.seed, self.conv)

    def emulate(self, x32=None, row=None, present=None, normals=None):
        z0, z1 = self.normals() if normals is None else normals
        return TC.emulate32(self.case, self.td, self.x32 if x32 is None else x32, self.row if row is None else row,
                            self.present if present is None else present, z0, z1, self.conv)  # fmt: skip


def samples(case, dtype, rolling=True):
    rows, present = TC.build_rows(case, rolling)
    return [Sample(case, dtype, b, r, rows, present) for b, r in zip(range(BATCH), (0, 2, len(rows) - 1, 3))], rows, present


def ratios(sample: Sample, outs: dict) -> float:
    return max(TC.worst_ratio(outs[name], ref, allowed) for name, (ref, allowed) in sample.reference().items())


@pytest.mark.parametrize("dtype", list(TC.DTYPES))
def test_the_reference_accepts_the_kernels_order(dtype):
    "an fp32 evaluation in the kernels' order (on bit_model.fma32, the correctly rounded fma) meets the float64 bound with ratio <= 1"
    worst = 0.0
    for case in CASES:
        if dtype not in TC.FAMILY_DTYPES[case.family]:
            continue
        for s in samples(case, dtype)[0]:
            worst = max(worst, ratios(s, s.emulate()))
    assert 0.0 < worst <= 1.0, worst


def swapped(row, i, j):
    other = _hip.StepRowC.from_buffer_copy(row)
    other.coef0[i], other.coef0[j] = row.coef0[j], row.coef0[i]
    other.coef1[i], other.coef1[j] = row.coef1[j], row.coef1[i]
    return other


@pytest.mark.parametrize("dtype", list(TC.DTYPES))
def test_seeded_errors_are_rejected(dtype):
    """one operand dropped, two coefficients swapped, operand j + 12 read for j, the neighbouring sample's noise, the neighbouring
    sample's row: each lands outside the bound or changes bits in 16-bit dtypes, and outside the bound in fp32, for every sample it can touch"""
    seen = set()
    for case in CASES:
        if dtype not in TC.FAMILY_DTYPES[case.family]:
            continue
        group, rows, present = samples(case, dtype)
        for n, s in enumerate(group):
            good = s.emulate()
            neighbour = group[(n + 1) % len(group)]
            first = 2 if case.family == "rk1" else 0  # (the conversion pair enters out1 through its coefficients like any operand, and out0 bit for bit)
            errors = {}
            live = [j for j in s.present if j >= first]
            if len(s.present) > 1 and live:
                errors["dropped"] = s.emulate(present=tuple(j for j in s.present if j != live[len(live) // 2]))
            read = s.row.coef1 if case.family == "rk1" else s.row.coef0  # (two slots whose coefficients the kernel reads and that differ)
            pair = next(((i, j) for i in s.present for j in s.present if i < j and read[i] != read[j]), None)
            if pair is not None:
                errors["swapped"] = s.emulate(row=swapped(s.row, *pair))
            if case.family == "k1" and case.slots >= 13 and 0 in s.present and 12 in s.present:
                x = s.x32.copy()
                x[0] = x[12]
                errors["j+12"] = s.emulate(x32=x)
            if case.draws and any(getattr(s.row, z) != 0.0 for z in (("zeta1",) if case.family == "rk1" else ("zeta0", "zeta1") if case.family == "k2" else ("zeta0",))):
                errors["neighbour's noise"] = s.emulate(normals=s.normals(seed=neighbour.seed))
            errors["neighbour's row"] = s.emulate(row=neighbour.row, present=neighbour.present, normals=s.normals(row=neighbour.row))
            for what, outs in errors.items():
                outside = ratios(s, outs) > 1.0
                changed = any(not torch.equal(int_view(outs[k]), int_view(good[k])) for k in outs)
                assert outside or (changed and dtype != "fp32"), (what, case, dtype, s.b)
                assert changed, (what, case, dtype, s.b)
                seen.add(what)
    assert seen == {"dropped", "swapped", "j+12", "neighbour's noise", "neighbour's row"}, seen


def test_the_grid_is_what_the_source_instantiates():
    src = open(os.path.join(ROOT, "skrample_amd", "csrc", "skr_step_fast.hip")).read()
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    row_terms = int(re.search(r"#define SKR_ROW_TERMS (\d+)", header).group(1))
    assert row_terms == _hip.ROW_TERMS == TC.ROW_TERMS == 16
    assert ctypes.sizeof(_hip.StepRowC) == 8 * (2 * row_terms + 3 + 2 + 4)
    counts = re.search(r"using TwoOutCounts = TwoOutList<(.*?)>;", src, re.S).group(1)
    pairs = [(int(a), int(b)) for a, b in re.findall(r"TwoOut<(\d+), (\d+), \w+>", counts)]
    assert len(pairs) == 14 and tuple(p for p in pairs if sum(p) <= row_terms) == TC.K2_PAIRS
    assert "constexpr bool TABLE = NA + NB <= SKR_ROW_TERMS;" in src
    assert "with_count<1, ONE_TRIP_MAX_K>" in src and "with_form<T, (N <= 8), (N <= SKR_ROW_TERMS)>" in src
    assert TC.K1_COUNTS == tuple(range(1, row_terms + 1))
    lo, hi = map(int, re.search(r"with_count<(\d), (\d)>\(args\.n_terms, \[&\]\(auto n\) \{\s*constexpr int N = decltype\(n\)::value;\s*RkOneTripArgs", src).groups())
    assert TC.RK1_COUNTS == tuple(range(lo, hi + 1))
    assert "with_form<T, false, true>" in src  # every step_kernel_rk1 count has its table forms
    assert all(f"launch_rk1<T, {n}, {blk}>" in src for n in ("true", "false") for blk in TC.RK1_BLOCKS)
    assert set(TC.MAPPED_K1) <= set(TC.K1_COUNTS) and set(TC.MAPPED_RK1) <= set(TC.RK1_COUNTS) and set(TC.MAPPED_K2) <= set(TC.K2_PAIRS)
    assert len(TC.full_grid("k1")) == 32 and len(TC.full_grid("rk1")) == 7 * 3 * 2 * 2 and len(TC.full_grid("k2")) == 40


def test_rows_and_index_vectors_cover_what_they_claim():
    "every table has >= 5 dense rows that differ in every field, a zero-zeta row and a stream above 2^32; rolling tables add the absent sets; the index vectors stay inside the table"
    for family in ("k1", "rk1", "k2"):
        for case in TC.full_grid(family):
            rows, present = TC.build_rows(case, rolling=True)
            dense = rows[: TC.N_DENSE]
            for field in ("chain", "stream0", "stream1") + (("zeta1",) if case.draws and case.noise != "zeta0" else ()) + (("zeta0",) if case.draws and family != "rk1" and case.noise != "zeta1" else ()):
                assert len({getattr(r, field) for r in dense}) >= TC.N_DENSE - 1, (case, field)
            assert len({tuple(r.coef0[: case.slots]) for r in dense}) == TC.N_DENSE and len({tuple(r.coef1[: case.slots]) for r in dense}) == TC.N_DENSE
            assert len({tuple(r.convert_k) for r in dense}) == TC.N_DENSE
            assert any(r.stream0 > 2**32 for r in dense) and any(r.stream1 > 2**32 for r in dense)
            if case.draws:
                assert any(r.zeta0 == 0.0 and r.zeta1 == 0.0 for r in dense)
            lacks = [tuple(j for j in range(case.slots) if j not in p) for p in present[TC.N_DENSE :]]
            assert all(p for p in present) and (family != "rk1" or all(p[:2] == (0, 1) for p in present))
            if family == "k1" and case.slots >= 13:
                assert (0,) in lacks and (12,) in lacks  # 12 slots apart, in both orders
            if family == "k2" and case.nb:
                assert (case.na,) in lacks
            if case.slots >= 3 + (2 if family == "rk1" else 0):
                first = 2 if family == "rk1" else 0
                assert (first,) in lacks and (case.slots - 1,) in lacks and any(first < l[0] < case.slots - 1 for l in lacks if len(l) == 1)
            for off in (0, 1):
                for form in TC.FORMS:
                    vectors = TC.pick_lists(form, len(rows) if form == "rolling" else TC.N_DENSE, 4, off, 3)
                    assert all(p < 0 or 0 <= p + off < len(rows) for v in vectors for p in v)
                    if form == "rolling":
                        assert {p + off for v in vectors for p in v if p >= 0} == set(range(off, len(rows))) and any(p < 0 for v in vectors for p in v)
    assert any(s >= 2**40 for s in TC.SEEDS) and any(s >= 2**63 for s in TC.SEEDS)
