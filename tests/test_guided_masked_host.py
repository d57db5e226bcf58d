"""Guided in-painting without a device: the declaration of skr_guided_masked_step_launch and its binding, the launch table it stays out
of, and set_inpaint(fuse_guidance=True) on CPU tensors, where the flag changes nothing and nothing is launched."""

import os
import re

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "skr_guided_masked_step_launch"


def test_header_binding_library_and_launch_table():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skrample_hip.h")).read(), flags=re.S)
    declared = re.search(r"^int " + NAME + r"\((.*?)\);", header, flags=re.S | re.M)
    assert declared is not None and NAME in _hip.EXPORTS and _hip.GUIDED_MASKED == NAME and callable(_hip.launch_guided_masked_step)
    assert len(getattr(_hip.load(), NAME).argtypes) == len(declared.group(1).split(",")) == 9
    names = [name for name, _ in _hip.ENTRIES.values()]  # the launch table stays as it is: 22 keys, and the new entry is none of its names
    assert len(_hip.ENTRIES) == 22 and NAME not in names and not NAME.startswith("skr_step_launch")
    assert sorted(names) == sorted(n for n in _hip.EXPORTS if n.startswith(("skr_step_launch", "skr_guidance_rescale_factor")))


@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("sampler", [lambda: PT.DPM(order=2), lambda: PT.UniPC(order=2)], ids=["dpm2", "unipc2"])
def test_on_cpu_tensors_the_flag_changes_nothing_and_launches_nothing(sampler, phi):
    shape, g = (2, 4, 8, 8), torch.Generator().manual_seed(11)
    orig, nz, xa, mask = *(torch.randn(shape, generator=g).bfloat16() for _ in range(3)), torch.rand((2, 1, 8, 8), generator=g)
    fused, plain = (PD.SkrampleWrapperScheduler(sampler(), PS.Karras(PS.Scaled())) for _ in range(2))
    fused.set_timesteps(4), plain.set_timesteps(4)
    fused.set_inpaint(mask, orig, nz, fuse_guidance=True), plain.set_inpaint(mask, orig, nz)
    xb, _hip.trace = xa, []
    try:
        for t in plain.timesteps.tolist():
            u, c = (torch.randn(shape, generator=g).bfloat16() for _ in range(2))
            xa, pa = fused.step_guided(u, c, 7.3, t, xa, return_dict=False, guidance_rescale=phi)
            xb, pb = plain.step(lazy.Guidance(u, c, 7.3, phi).torch_lines(), t, xb, return_dict=False)  # the default route on the host: torch's lines
            pa, pb = (v.materialize() if isinstance(v, lazy.LazyTensor) else v for v in (pa, pb))
            assert torch.equal(xa.view(torch.int16), xb.view(torch.int16)) and torch.equal(pa.view(torch.int16), pb.view(torch.int16))
        assert _hip.trace == []
    finally:
        _hip.trace = None
    fused.clear_inpaint()
    assert fused._inpaint is None and not fused._inpaint_fuse
