"""Helpers of tests/test_table_forms_gpu.py and tests/test_table_forms_host.py: the case grid of the table-form step kernels, the
builders of rows, plans and index vectors, the float64 reference with its bound, and a host emulation of the kernels' fp32 order (on
bit_model.fma32, the correctly rounded fma).

The table forms are the launches that take their scalars from a `skr_step_row` in device memory (include/skrample_hip.h):
skr_step_launch_indexed ("whole"), skr_step_launch_indexed_per_sample ("per_sample") and skr_step_launch_rolling ("rolling").
Nothing in this module needs a GPU."""

from __future__ import annotations

import ctypes
import functools
import random
from dataclasses import dataclass

import bit_model as BM
import numpy as np
import torch
from skr_oracle import noise as ON

from skrample_amd import _hip

CHUNK = 2048  # elements per workgroup of the one-trip kernels (BLOCK * VEC)
GUARD = 2048  # elements in front of and behind every output
ROW_TERMS = 16

# ---- the grid ---------------------------------------------------------------------------------------------------------------------
# What skrample_amd/csrc/skr_step_fast.hip instantiates in a table form.  `with_form` gives a kernel its table instantiations when its
# operands fit a device-resident row (`SKR_ROW_TERMS`, 16):
#   step_kernel_k1   launch_k1: with_count<1, ONE_TRIP_MAX_K> cut at N <= SKR_ROW_TERMS            -> 1..16 operands, noise on / off
#   step_kernel_rk1  launch_rk1: with_count<2, 8>, BLK 128 and 256                                  -> 2..8 operands
#   step_kernel_k2   the (NA, NB) entries of `TwoOutCounts` with NA + NB <= SKR_ROW_TERMS           -> the ten pairs below, 16-bit only
# tests/test_table_forms_host.py reads these three facts back from the source, so a change there fails here.
K1_COUNTS = tuple(range(1, 17))
RK1_COUNTS = tuple(range(2, 9))
RK1_BLOCKS = (128, 256)
K2_PAIRS = ((2, 0), (3, 0), (4, 0), (4, 1), (6, 1), (7, 1), (8, 1), (10, 1), (12, 1), (14, 1))
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
FAMILY_DTYPES = {"k1": ("bf16", "fp16", "fp32"), "rk1": ("bf16", "fp16", "fp32"), "k2": ("bf16", "fp16")}
FORMS = ("whole", "per_sample", "rolling")
RK_KINDS = ((1, 2), (0, 1), (3, 3))
K2_NOISE = ("off", "both", "zeta0", "zeta1")
# reduced grid of the mapped geometry (64 samples of 3 chunks: a non-identity XCD chunk map and the dividing chunk -> sample form)
MAPPED_K1 = (1, 4, 9, 13, 16)
MAPPED_RK1 = (2, 5, 8)
MAPPED_K2 = ((4, 1), (8, 1), (14, 1))

SMALL = tuple((4, CHUNK * c) for c in (1, 2, 3))  # (samples, elements per sample): bps_shift 0, 1, -3 (rk1 at 128 threads: 1, 2, -6)
MAPPED = (64, CHUNK * 3)
# geometry x row_offset of the full grid: every geometry, both offsets, the dividing form under both
SMALL_COMBOS = ((SMALL[0], 0), (SMALL[1], 1), (SMALL[2], 0), (SMALL[2], 1))

EPS_OUT = {torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11, torch.float32: 2.0**-24}
NORMAL_BAR = 4e-6  # device normal against oracle philox_normal: the bar tests/test_noise_gpu.py::test_random_generator asserts
SEEDS = (11, 2**40 + 5, 2**63 + 9, 77)  # as test_in_kernel_philox_matches_oracle_spec, one more


@dataclass(frozen=True)
class Case:
    family: str  # "k1" | "rk1" | "k2"
    na: int  # operands of the launch's own dtype
    nb: int = 0  # fp32 operands behind them (k2 only)
    noise: str = "off"  # k1 / rk1: "off" | "on"; k2: one of K2_NOISE
    kinds: tuple = (0, 0)  # rk1: (convert_to, convert_from)
    blk: int = 0  # rk1: forced workgroup size

    @property
    def slots(self) -> int:
        return self.na + self.nb

    @property
    def draws(self) -> bool:
        return self.noise != "off"


def full_grid(family: str):
    if family == "k1":
        return [Case("k1", k, noise=nz) for k in K1_COUNTS for nz in ("off", "on")]
    if family == "rk1":
        return [Case("rk1", k, noise=nz, kinds=kinds, blk=blk) for k in RK1_COUNTS for kinds in RK_KINDS for nz in ("off", "on") for blk in RK1_BLOCKS]
    return [Case("k2", na, nb, noise=nz) for na, nb in K2_PAIRS for nz in K2_NOISE]


def mapped_grid(family: str):
    if family == "k1":
        return [Case("k1", k, noise=nz) for k in MAPPED_K1 for nz in ("off", "on")]
    if family == "rk1":
        return [Case("rk1", k, noise=("on" if k != 5 else "off"), kinds=RK_KINDS[n % 3], blk=blk) for n, k in enumerate(MAPPED_RK1) for blk in RK1_BLOCKS]
    return [Case("k2", na, nb, noise=nz) for (na, nb), nz in zip(MAPPED_K2, ("both", "zeta1", "off"))]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def seeds_for(batch: int) -> list[int]:
    return [(SEEDS[b % 4] + 7919 * (b // 4)) % 2**64 for b in range(batch)]


def seeds_tensor(seeds) -> torch.Tensor:
    return torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64).copy())


@functools.lru_cache(maxsize=None)
def pool(dtype_name: str, batch: int, sample: int):
    """The operands every case of one dtype and geometry draws from, on the host: `narrow` [16, batch * sample] in the dtype and `wide`
    [batch * sample] fp32 (the fp32 state of a two-output step).  Scales differ per operand; the first 64 elements of every sample
    of operand 0 and the first 32 of operand 1 are exact zeros (signed-zero sums, and a rounded conversion of zeros)."""
    td = DTYPES[dtype_name]
    g = torch.Generator().manual_seed(1000 + batch * 7 + sample // CHUNK)
    n = batch * sample
    scales = (1.0, 0.5, 2.0, 0.25, 1.5, 0.75, 3.0, 1.0, 0.125, 2.5, 1.0, 0.5, 4.0, 1.25, 0.3, 1.75)
    narrow = torch.stack([(torch.randn(n, generator=g) * s).to(td) for s in scales])
    wide = torch.randn(n, generator=g) * 1.5
    narrow.view(ROW_TERMS, batch, sample)[0, :, :64] = 0
    narrow.view(ROW_TERMS, batch, sample)[1, :, :32] = 0
    return narrow, wide


@functools.lru_cache(maxsize=4)
def pool64(dtype_name: str, batch: int, sample: int):
    "the same operands in float64, [16, batch, sample] and [batch, sample]"
    narrow, wide = pool(dtype_name, batch, sample)
    return narrow.double().view(ROW_TERMS, batch, sample), wide.double().view(batch, sample)


@functools.lru_cache(maxsize=4096)
def normal(seed: int, stream: int, n: int) -> np.ndarray:
    return ON.philox_normal(seed, stream, n).astype(np.float64)


# ---- rows -------------------------------------------------------------------------------------------------------------------------
N_DENSE = 6
CHAINS = (-0.4375, 1.0, 0.3125, -1.0, 0.75, 0.0625)
ZETAS = (0.625, 0.0, -0.75, 0.5, 1.25, 0.375)  # fp32 numbers; row 1 skips its draw
STREAMS = (5, 2**32 + 7, 11, 300, 2**40 + 1, 9)
# (k0 .. k3 of the rounded conversion, as sigma-like numbers; one negative k0)
CONVERT_K = tuple((0.9 - 0.07 * r if r != 3 else -0.55, 0.09999999999999998 + 0.11 * r, 0.7310585786300049 + 0.05 * r, 0.35 + 0.06 * r) for r in range(N_DENSE))


def _coef(rng: random.Random) -> float:
    kind = rng.randrange(4)
    c = (1.0, -1.0, rng.uniform(-3, 3), rng.uniform(-1e-2, 1e-2))[kind]
    return c if c != 0.0 else 0.5


def absent_sets(case: Case) -> list[tuple]:
    "the operand sets the sparse rows of a rolling table lack: leading, interior and trailing slots, 12 slots apart in both orders, the fp32 state"
    n, first = case.slots, (2 if case.family == "rk1" else 0)  # (the pair of a rounded conversion is always present)
    sets: list[tuple] = []
    if n - first >= 2 or (n - first == 1 and first == 2):
        sets += [(first,), (n - 1,)]
    if n - first >= 3:
        sets += [((first + n) // 2,), tuple(range(first + 1, n, 2))]
    if case.family == "k1" and n >= 13:
        hi = n - 13
        sets += [(0,), (12,), (hi,), (hi + 12,), (0, hi) if hi else (0, 5), tuple(j for j in range(n) if j % 12 != 0) if n > 12 else ()]
    if case.family == "k2" and case.nb:
        sets += [(case.na,), (case.na - 1, case.na)]
    out = []
    for s in sets:
        s = tuple(sorted(set(j for j in s if first <= j < n)))
        if s and len(s) < n and s not in out:
            out.append(s)
    return out


def build_rows(case: Case, rolling: bool):
    """The table of one case: six dense rows that differ in every field, then (rolling) one sparse row per absent set.
    Returns (ctypes array of StepRowC, [tuple of present operands per row])."""
    rng = random.Random(f"{case.family}/{case.na}/{case.nb}")
    n = case.slots
    lacks = [()] * N_DENSE + (absent_sets(case) if rolling else [])
    rows = (_hip.StepRowC * len(lacks))()
    present = []
    for r, (row, lack) in enumerate(zip(rows, lacks)):
        d = r % N_DENSE
        for j in range(n):
            row.coef0[j], row.coef1[j] = (_coef(rng), _coef(rng)) if n >= 3 else (rng.uniform(0.2, 3) * (-1) ** r, rng.uniform(-3, -0.2) * (-1) ** (r // 2))
        if n >= 3:
            row.coef0[r % n], row.coef1[(r + 1) % n] = 1.0, -1.0
        elif d in (2, 3):  # (one or two operands: the rows must still differ, so only two of them carry the exact units)
            row.coef0[0], row.coef1[n - 1] = (1.0, -1.0) if d == 2 else (-1.0, 1.0)
        for j in range(n, ROW_TERMS):  # slots the launch does not have: never read
            row.coef0[j], row.coef1[j] = 1e30, -1e30
        for i, j in enumerate(lack):
            row.coef0[j], row.coef1[j] = (0.0, -0.0) if (i + r) % 2 else (-0.0, 0.0)
        row.chain = CHAINS[d] * (1.0 if r < N_DENSE else -0.5)
        z0, z1 = ZETAS[d], ZETAS[(d + 3) % N_DENSE] if d != 1 else 0.0
        if case.family == "rk1" or case.noise == "zeta1":
            z0 = 0.0  # (a Runge-Kutta stage draws on out1 alone)
        if case.noise == "zeta0":
            z1 = 0.0
        row.zeta0, row.zeta1 = z0, z1
        row.stream0, row.stream1 = STREAMS[d] + 17 * (r // N_DENSE), STREAMS[(d + 2) % N_DENSE] + 1000 + r
        for i in range(4):
            row.convert_k[i] = CONVERT_K[d][i] * (1.0 if r < N_DENSE else 1.25)
        present.append(tuple(j for j in range(n) if j not in lack))
    return rows, present


def rows_tensor(rows) -> torch.Tensor:
    return torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8)


def pick_lists(form: str, n_rows: int, batch: int, off: int, salt: int) -> list[list[int]]:
    """Index vectors (entries BEFORE row_offset is added; -1 / -2 = inactive) for one case: whole-batch two single indices, per-sample
    two shuffled vectors, rolling enough vectors that every row of the table is used, each with inactive samples."""
    rng = random.Random(salt * 31 + off)
    usable = list(range(off, n_rows))
    if form == "whole":
        return [[r - off] for r in rng.sample(usable, 2)]
    if form == "per_sample":
        out = []
        for _ in range(2):
            rows = [usable[(i * 5 + rng.randrange(len(usable))) % len(usable)] for i in range(batch)]
            rng.shuffle(rows)
            out.append([r - off for r in rows])
        return out
    order = usable[N_DENSE - off :] + usable[: N_DENSE - off]  # sparse rows first
    rng.shuffle(order)
    per = max(1, batch - max(1, batch // 4))  # a quarter of the samples inactive
    out = []
    for at in range(0, len(order), per):
        rows = order[at : at + per]
        rows += [order[i % len(order)] for i in range(per - len(rows))]
        vec = [r - off for r in rows] + [(-1 if (at + i) % 3 else -2) for i in range(batch - per)]
        rng.shuffle(vec)
        out.append(vec)
    if batch <= 8:
        out.append([-1 if i % 2 else -2 for i in range(batch)])  # nobody active
    return out


# ---- plans ------------------------------------------------------------------------------------------------------------------------
def make_plan(case: Case, code: int, sample: int) -> _hip.StepPlanC:
    "the structure of a table launch; every scalar a row carries is garbage here -- a table form must ignore it"
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a = case.slots, case.na, code
    plan.dtype_b = _hip.F32 if case.nb else code
    plan.out0_dtype = _hip.F32 if case.family == "k2" else code
    plan.out1_dtype = _hip.NONE if case.family == "k1" else code
    plan.noise_mode, plan.sample_numel = int(case.draws), sample
    plan.convert_to, plan.convert_from = case.kinds
    for k in range(case.slots):
        plan.coef0[k], plan.coef1[k] = 1e30, -1e30
    plan.chain, plan.zeta0, plan.zeta1, plan.stream0, plan.stream1 = 1e30, 1e30, 1e30, 0xDEAD, 0xDEAD
    for i in range(4):
        plan.convert_k[i] = 1e30
    return plan


def narrow_plan(case: Case, plan: _hip.StepPlanC, row, present) -> _hip.StepPlanC:
    "the skr_step_launch a sample's result must have the bits of: the row's scalars, the present operands only, in slot order"
    one = _hip.StepPlanC()
    ctypes.memmove(ctypes.byref(one), ctypes.byref(plan), ctypes.sizeof(plan))
    one.n_terms = len(present)
    one.n_group_a = sum(1 for j in present if j < case.na)
    for k in range(_hip.MAX_TERMS):
        one.coef0[k] = one.coef1[k] = 0.0
    for i, j in enumerate(present):
        one.coef0[i], one.coef1[i] = row.coef0[j], row.coef1[j]
    one.chain, one.zeta0, one.zeta1, one.stream0, one.stream1 = row.chain, row.zeta0, row.zeta1, row.stream0, row.stream1
    for i in range(4):
        one.convert_k[i] = row.convert_k[i]
    return one


# ---- references -------------------------------------------------------------------------------------------------------------------
def conversion_reference(s_: torch.Tensor, o_: torch.Tensor, kinds, k) -> torch.Tensor:
    "out0 of a rounded conversion, one torch op at a time in the tensors' dtype (tests/test_step_gpu.py::test_rounded_conversion_equals_torch_op_by_op)"
    to_kind, from_kind = kinds
    x = {0: lambda: o_, 1: lambda: (s_ - k[0] * o_) / k[1], 2: lambda: k[1] * s_ - k[0] * o_, 3: lambda: o_ * k[0]}[to_kind]()
    return {0: lambda: x, 1: lambda: (s_ - k[2] * x) / k[3], 2: lambda: (k[2] * s_ - x) / k[3], 3: lambda: x / k[2]}[from_kind]()


def operands64(case: Case, dtype_name: str, batch: int, sample: int) -> torch.Tensor:
    "[slots, batch, sample] float64: the case's operands in slot order (the fp32 state last)"
    narrow, wide = pool64(dtype_name, batch, sample)
    return torch.cat([narrow[: case.na], wide[None]]) if case.nb else narrow[: case.na]


def reference64(case: Case, td: torch.dtype, x: torch.Tensor, row, present, seed: int, conv: torch.Tensor | None = None) -> dict:
    """One sample in float64.  x [slots, sample] float64; `conv` the rounded conversion of an rk1 case (its out0, compared bit for bit
    elsewhere, enters out1 as the value the kernel chains).  Returns {output: (reference, allowed error)} with the bound of
    test_random_linear_forms_vs_float64 -- (present operands + 4) * 2^-23 * sum |c| |x| + one rounding of the output (+ 2^-25 for
    fp16's subnormals) -- plus the device-versus-oracle bar of a normal times the zetas that reach the output."""
    n = x.shape[1]
    c0 = torch.tensor([row.coef0[j] if j in present else 0.0 for j in range(case.slots)], dtype=torch.float64)
    c1 = torch.tensor([row.coef1[j] if j in present else 0.0 for j in range(case.slots)], dtype=torch.float64)
    eps_acc, terms = 2.0**-23, len(present) + 4
    z0 = torch.from_numpy(normal(seed, row.stream0, n)) if case.draws and row.zeta0 != 0.0 else None
    z1 = torch.from_numpy(normal(seed, row.stream1, n)) if case.draws and row.zeta1 != 0.0 else None

    def allowed(ref, mag, od, zeta_reach):
        a = terms * eps_acc * mag + EPS_OUT[od] * ref.abs() * 1.01 + 1e-30 + zeta_reach * NORMAL_BAR  # (1e-30 as there: an exact zero allows an exact zero)
        return a + 2.0**-25 if od == torch.float16 else a

    out = {}
    if case.family == "rk1":
        d = conv.double()
        ref1 = row.chain * d + c1 @ x
        mag1 = abs(row.chain) * d.abs() + c1.abs() @ x.abs()
        if z1 is not None:
            ref1 = ref1 + row.zeta1 * z1
        out["out1"] = (ref1, allowed(ref1, mag1, td, abs(row.zeta1) if z1 is not None else 0.0))
        return out
    ref0, mag0 = c0 @ x, c0.abs() @ x.abs()
    if z0 is not None:
        ref0 = ref0 + row.zeta0 * z0
    reach0 = abs(row.zeta0) if z0 is not None else 0.0
    out["out0"] = (ref0, allowed(ref0, mag0, torch.float32 if case.family == "k2" else td, reach0))
    if case.family == "k2":
        ref1 = row.chain * ref0 + c1 @ x
        mag1 = abs(row.chain) * mag0 + c1.abs() @ x.abs()
        if z1 is not None:
            ref1 = ref1 + row.zeta1 * z1
        out["out1"] = (ref1, allowed(ref1, mag1, td, abs(row.chain) * reach0 + (abs(row.zeta1) if z1 is not None else 0.0)))
    return out


# ---- host emulation of the kernels' order --------------------------------------------------------------------------------------------
def emulate32(case: Case, td: torch.dtype, x32: np.ndarray, row, present, z0, z1, conv: torch.Tensor | None = None) -> dict:
    """The kernels' arithmetic on the host: fp32 coefficients, one fma per present operand in slot order, then the noise fma, then `chain`
    (rk1: chain before its noise), one rounding to the output dtype.  x32 [slots, sample] float32; z0 / z1 float32 normals or None.
    Returns {output: tensor of the output dtype}."""
    zero = np.zeros(x32.shape[1], dtype=np.float32)

    def accumulate(coefs):
        s = zero
        for j in present:
            s = BM.fma32(np.float32(coefs[j]), x32[j], s)
        return s

    def rounded(s, od):
        return torch.from_numpy(s).to(od)

    use0 = case.draws and row.zeta0 != 0.0 and z0 is not None
    use1 = case.draws and row.zeta1 != 0.0 and z1 is not None
    if case.family == "rk1":
        s1 = accumulate(row.coef1)
        s1 = BM.fma32(np.float32(row.chain), conv.float().numpy(), s1)
        if use1:
            s1 = BM.fma32(np.float32(row.zeta1), z1, s1)
        return {"out1": rounded(s1, td)}
    s0 = accumulate(row.coef0)
    if use0:
        s0 = BM.fma32(np.float32(row.zeta0), z0, s0)
    if case.family == "k1":
        return {"out0": rounded(s0, td)}
    s1 = accumulate(row.coef1)
    s1 = BM.fma32(np.float32(row.chain), s0, s1)
    if use1:
        s1 = BM.fma32(np.float32(row.zeta1), z1, s1)
    return {"out0": rounded(s0, torch.float32), "out1": rounded(s1, td)}


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, allowed: torch.Tensor) -> float:
    "max err / allowed (inf for a NaN)"
    err = (got.double() - ref).abs()
    ratio = err / allowed
    return float("inf") if torch.isnan(ratio).any() else ratio.max().item()
