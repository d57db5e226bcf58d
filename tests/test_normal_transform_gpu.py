"""The Philox-to-normal transform of skr_philox.h on the MI355X, on every reachable input.

Every random number of the engine is skr::normal4: Philox4x32-10, then a Box-Muller on the raw v_log_f32 / v_sqrt_f32 / v_cos_f32 /
v_sin_f32.  skr_normal_u32 runs that transform on caller-provided words, so each factor -- r(u0), cos(2 pi u1), sin(2 pi u1), one fp32
uniform each -- is compared with float64 on all 83,886,080 exactly representable words plus the words the conversion has to round
(tests/normal_cases.py); the factor maxima bound every one of the 2^64 pairs.  The bar is the fp32 specification's own distance from
float64 (profiles/normal_transform.txt) x 1.5.  Then the production form (parts = 0) is tied to the factors bit for bit, the shipped
generators to the production form, and the raw Philox words to a torch int64 restatement at the counter, seed and stream edges."""

import ctypes

import pytest
import torch

import normal_cases as NC
from conftest import note_margin
from skrample_amd import _hip

pytestmark = pytest.mark.gpu
ORACLE = NC.ORACLE  # profiles/normal_transform.txt: E_r 3.955e-7, E_c 3.797e-7, E_s 4.163e-7, rel_r 2.870 x 2^-24, composed 3.615e-6


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def normal_u32(words: torch.Tensor, parts: int) -> torch.Tensor:
    "[n, 4] int64 words on the device -> [n, 4] fp32 of skr_normal_u32"
    w = NC.as_u32_bits(words).contiguous()
    out = torch.empty(w.shape, dtype=torch.float32, device=w.device)
    _hip.check(_hip.load().skr_normal_u32(out.data_ptr(), w.data_ptr(), w.shape[0], parts, _hip.current_stream_ptr(w.device)), "normal_u32")
    return out


def philox_u32(seed: int, stream: int, first: int, n: int, dev) -> torch.Tensor:
    "[n, 4] int64 words of skr_philox_u32"
    out = torch.empty(n, 4, dtype=torch.int32, device=dev)
    _hip.check(_hip.load().skr_philox_u32(out.data_ptr(), seed, stream, first, n, _hip.current_stream_ptr(dev)), "philox")
    return out.to(torch.int64) & 0xFFFFFFFF


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def factors(dev):
    "parts = 1 over every representative and rounding word, the word in the x slot (r) and in the y slot (cos, sin): measured once"
    product_differs = [0]

    def parts_of(words: torch.Tensor):
        quad = torch.zeros(words.numel(), 4, dtype=torch.int64, device=dev)
        quad[:, 0] = words
        quad[:, 1] = words
        out = normal_u32(quad, 1)
        product_differs[0] += int((bits(out[:, 3]) != bits(out[:, 0] * out[:, 1])).sum())
        return out[:, 0].clone(), out[:, 1].clone(), out[:, 2].clone()

    rep = NC.factor_report(parts_of, NC.representative_words(dev), NC.rounding_words(dev))
    rep["product_differs"] = product_differs[0]
    for k in ("E_r", "E_c", "E_s", "rel_r", "composed"):
        note_margin("normal transform factors", k, rep[k], NC.SLACK * ORACLE[k] if k in ("rel_r", "composed") else None)
    print("\nnormal transform, device against float64:", {k: rep[k] for k in ("E_r", "E_c", "E_s", "rel_r", "composed")})
    return rep


def test_factor_conditions_on_every_reachable_input(factors):
    """finite; r = 0 exactly where u = 1 and positive elsewhere; r <= R (1 + 2^-22); |cos|, |sin| <= 1; their signs; a rounding word
    has the bits of its round-to-nearest-even representative; out[3] is the fp32 product of out[0] and out[1]"""
    assert factors["violations"] == []
    assert factors["product_differs"] == 0


def test_factors_no_further_from_float64_than_the_fp32_specification(factors):
    """the composed bound of every z and the relative error of r (the one a log2 that cancels near u -> 1 fails), each at most 1.5 x what
    the fp32 specification itself measures against float64"""
    assert NC.bar_violations(factors, ORACLE) == []


def test_production_form_is_the_product_of_the_factors(dev, factors):
    "parts = 0 on 2^24 Philox words: bit for bit the fp32 products of the parts = 1 factors, and within the composed bound of float64"
    w = NC.philox_words(2**40 + 7, 3 * 256, 0, 1 << 22, dev)
    z = normal_u32(w, 0)
    a, b = normal_u32(w, 1), normal_u32(w[:, [2, 3, 0, 1]], 1)
    want = torch.stack([a[:, 0] * a[:, 1], a[:, 0] * a[:, 2], b[:, 0] * b[:, 1], b[:, 0] * b[:, 2]], -1)
    assert torch.equal(bits(z), bits(want))
    assert torch.equal(bits(a[:, 3]), bits(want[:, 0])) and torch.equal(bits(b[:, 3]), bits(want[:, 2]))
    u = NC.uniform(w)
    exact = torch.empty(w.shape, dtype=torch.float64, device=dev)
    for x, y in ((0, 1), (2, 3)):
        r, _, _ = NC.exact_parts(u[:, x])
        _, c, s = NC.exact_parts(u[:, y])
        exact[:, x], exact[:, y] = r * c, r * s
    worst = note_margin("normal transform production form", "max |z - float64|", (z.double() - exact).abs().max().item(), factors["composed"])
    assert worst <= factors["composed"], (worst, factors["composed"])


def test_shipped_generators_are_the_production_form(dev):
    """one stream over 2^24 elements is skr_normal_u32(skr_philox_u32(...), parts = 0): skr_noise_random through its packed route and
    its generic route (base off by one element), bit for bit, and skr_noise_brownian with one stream of weight 1 and scale 1 (whose
    fma(1, z, 0) turns a -0 into +0, so its values are compared)"""
    lib, s = _hip.load(), _hip.current_stream_ptr(dev)
    n, seed, stream = 1 << 24, 2**40 + 7, 5 * 256 + 1
    want = normal_u32(philox_u32(seed, stream, 0, n // 4, dev), 0).reshape(-1)
    seeds = torch.tensor([seed], dtype=torch.int64, device=dev)
    buf = torch.zeros(n + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    for off in (0, 1):
        out = buf[off : off + n]
        _hip.check(lib.skr_noise_random(out.data_ptr(), _hip.F32, seeds.data_ptr(), stream, 1, n, s), "random")
        assert torch.equal(bits(out), bits(want)), off
        assert (buf[off + n :] == 0).all() and (buf[:off] == 0).all()
        buf.zero_()
    ids, one, zero = (ctypes.c_uint64 * 1)(stream), (ctypes.c_double * 1)(1.0), (ctypes.c_double * 1)(0.0)
    _hip.check(lib.skr_noise_brownian(buf.data_ptr(), _hip.F32, seeds.data_ptr(), ids, one, zero, 1, 1.0, None, 0, 1, n, s), "brownian")
    assert torch.equal(buf[:n], want) and not torch.isnan(want).any()


FIRST_BLOCKS = (0, 2**32 - 2**19, 2**63, 2**64 - 2**19)  # the carry into the counter's high word; wrap-around
SEEDS = (0, 1, 2**40 + 7, 2**64 - 3)
STREAMS = (0, 5 * 256 + 255, 2**32 + 7, 2**63, 2**64 - 1)  # 1 << 63 is the Brownian generator's base


@pytest.mark.parametrize("first", FIRST_BLOCKS)
def test_raw_philox_at_the_counter_seed_and_stream_edges(dev, first):
    for seed in SEEDS:
        for stream in STREAMS:
            assert torch.equal(philox_u32(seed, stream, first, 1 << 20, dev), NC.philox_words(seed, stream, first, 1 << 20, dev)), (seed, stream)


def test_random123_known_answers_on_the_device(dev):
    "the kat_vectors of tests/test_oracle_golden.py::test_philox_known_answers through skr_philox_u32"
    for (seed, stream, first), want in NC.PHILOX_KATS:
        got = philox_u32(seed, stream, first, 1, dev)[0].tolist()
        assert got == list(want), [hex(v) for v in got]
        assert NC.philox_words(seed, stream, first, 1, dev)[0].tolist() == list(want)
