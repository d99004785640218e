"""What tests/test_gpu_gemm_exact.py rests on, checked without a GPU: the exactness premise of every case of the matrix
(tests/gemm_cases.py), the dropout draw against the attention tests' statement of it, the route of every case (hero_gemm_route,
host only) and the coverage of the launch tables, the measured GELU tolerances, and the sharpness of the comparison itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_cases as GC
from tests import gemm_reference as R
from tests import tvc_reference as TR


@pytest.fixture(scope="module")
def lib():
    from hero_amd import build
    build.build()
    from hero_amd import _lib as L
    return L.lib()


def compute_units(lib):
    from hero_amd import _lib as L
    probe = np.zeros(16, dtype=np.int32)
    plain = L.GemmEpilogue(None, None, None, 0, 0, 0.0, 1, L.no_dropout(), None, 0, 0, 0)
    assert lib.hero_gemm_route(24000, 3072, 768, 768, 768, 3072, 0, 0, L.BF16, C.byref(plain), probe.ctypes.data, probe.size) == 12
    return int(probe[4])                             # 2000 tiles: one persistent workgroup per compute unit


# ---- the exactness premise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted({(c["dt"], c["lay"], c["M"], c["N"], c["K"]) for c in GC.CASES}), ids=lambda s: "%s_%s_%dx%dx%d" % s)
def test_exactness_precondition(shape):
    """Every partial sum of every case is an fp32 number: sum_k |a_mk b_kn| - a bound on ANY partial sum in ANY order - stays
    under 2^24 grid steps, the accumulator round-trips through fp32, and it is a whole number of grid steps."""
    _, a, b, acc = GC._operands(*shape)
    assert float((np.abs(a) @ np.abs(b)).max()) < R.MAG_BOUND
    assert np.array_equal(acc.astype(np.float32).astype(np.float64), acc)
    assert np.array_equal(np.rint(acc / R.GRID_STEP) * R.GRID_STEP, acc)
    assert shape[4] * 3 * 4 / 32 < R.MAG_BOUND


@pytest.mark.parametrize("case", [c for c in GC.CASES if c["M"] < 1000], ids=lambda c: c["name"])
def test_epilogue_values_are_fp32(case):
    """The exact epilogues end in fp32 numbers (so fp32 outputs have ONE correct bit pattern and bf16 outputs are one rounding
    of it), their column sums are exact in any order, and the pre-activations of the GELU cases lie on the grid the tolerances
    were measured on."""
    seed, a, b, acc, x, ref = GC.reference(case)
    e = case["epi"]
    act = e.get("act", "none")
    if act in R.EXACT_ACTS:
        assert R.is_fp32(ref["out"])
        if e.get("colsum"):
            assert float(np.abs(ref["out"]).sum(axis=0).max()) < 2.0 ** 24 * 2.0 ** -9      # mul_aux: grid step 2^-7 * 2^-2
            assert R.is_fp32(ref["colsum"])
    else:
        pre = x["aux_in"] if act == "gelu_bwd" else acc + x["bias"]
        assert float(np.abs(pre).max()) <= GC.PREACT_RANGE and np.array_equal(np.rint(pre * 32) / 32, pre)
        assert float(np.std(pre)) > 1.0                      # across the curved range, not only where GELU saturates
    if e.get("slabs"):
        for s in R.split_slabs(a, b, 128 if case["dt"] == "bf16" else 64, 3):
            assert R.is_fp32(s)


# ---- dropout ---------------------------------------------------------------------------------------------------------------------------
def test_dropout_keep_is_the_attention_tests_draw():
    """Lk % 4 == 0: the attention index ((n H + h) Lq + i) * round_up(Lk, 4) + j is the flat index of an [N H Lq, Lk] matrix."""
    N, H, Lq, Lk = 2, 3, 5, 12
    for seed, site, thr in ((0x0123456789ABCDEF, 7, 6554), (0xFFFFFFFFFFFFFFFF, 0, 32768), (5, 1 << 40, 60000)):
        mult = TR.dropout_multipliers(seed, site, thr, 2.0, N, H, Lq, Lk).reshape(-1).numpy()
        keep = R.dropout_keep(seed, site, thr, np.arange(N * H * Lq * Lk))
        assert np.array_equal(keep, mult != 0)
        assert 0 < keep.sum() < keep.size
    keep = R.dropout_keep(11, 3, 6554, np.arange(1 << 16))
    assert abs(keep.mean() - 0.9) < 0.01


def test_dropout_params():
    assert R.dropout_params(0.5) == (32768, 2.0)
    thr, scale = R.dropout_params(0.1)
    assert thr == 6554 and scale == float(np.float32(1.0) / np.float32(0.9))


# ---- routes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GC.CASES, ids=lambda c: c["name"])
def test_case_routes_to_the_launch_it_names(lib, case):
    if case["name"] in GC.MULTI_ROUND and compute_units(lib) != 256:
        pytest.skip("the multi-round shapes are sized for 256 compute units; this library reports %d" % compute_units(lib))
    if case["force"] < 0 and case["expect"][0] != GC.SKINNY and compute_units(lib) != 256:
        pytest.skip("heuristic routes depend on the compute-unit count")
    w = GC.route_words(lib, case)
    assert GC.named_launch(w) == tuple(case["expect"]), w
    if case["name"] in GC.MULTI_ROUND:
        bm, bn = case["expect"][1:3]
        tiles = -(-case["M"] // bm) * -(-case["N"] // bn)
        assert tiles > 256 and w[4] == 256, (tiles, w)         # persistent workgroups walk more than one tile
    if case["epi"].get("slabs") or case["epi"].get("split_k", 1) > 1 and case["expect"][0] != GC.WS_OO:
        assert w[7] == lib.hero_gemm_splits(case["K"], case["epi"]["split_k"], 1 if case["dt"] == "bf16" else 0) == 3


def test_cases_cover_every_table_row():
    reached = {GC.table_row(c) for c in GC.CASES}
    missing = [r for r in GC.TABLE_ROWS if r not in reached]
    assert not missing, missing
    assert reached <= set(GC.TABLE_ROWS), reached - set(GC.TABLE_ROWS)
    assert GC.UNREACHABLE not in reached
    print("reached %d rows: %s" % (len(reached), sorted(reached)))


def test_no_route_reaches_the_unreachable_instantiation(lib):
    """gemm_ws_kernel<2, 3, true, 0> (128 x 192, O,O) is documented as unreachable: O,O problems under every force config, and
    the heuristic, never name it."""
    for case in [c for c in GC.CASES if c["lay"] == "OO" and c["dt"] == "bf16"]:
        for force in (-1, 8, 9, 10, 13, 14):
            w = GC.route_words(lib, dict(case, force=force))
            assert not (w[0] == GC.WS_OO and (w[1], w[2]) != (192, 192)), (case["name"], force, w)


# ---- tolerances -------------------------------------------------------------------------------------------------------------------------
def test_gelu_tolerances():
    """The recorded errors (gemm_cases.py's header) are what the two references give on every multiple of 1/32 in [-60, 60]."""
    x = np.arange(-60 * 32, 60 * 32 + 1, dtype=np.float64) / 32
    g64, d64 = R.gelu64(x), R.gelu_grad64(x)
    xt = torch.tensor(x, dtype=torch.float32, requires_grad=True)
    y = torch.nn.functional.gelu(xt)
    y.sum().backward()
    e32 = float(np.abs(y.detach().double().numpy() - g64).max()), float(np.abs(xt.grad.double().numpy() - d64).max())
    ga, da = R.gelu_as_f32(x)
    eas = float(np.abs(ga.astype(np.float64) - g64).max()), float(np.abs(da.astype(np.float64) - d64).max())
    print("fp32 torch gelu / gelu' max abs error: %.3g / %.3g; A&S 7.1.26 float32: %.3g / %.3g" % (e32 + eas))
    for measured, recorded in zip(e32 + eas, (GC.E32_GELU, GC.E32_GRAD, GC.EAS_GELU, GC.EAS_GRAD)):
        assert recorded * 0.5 <= measured * GC.FACTOR <= recorded * 1.25, (measured, recorded)   # (libm / SIMD width may move the last digit)
    assert max(eas) < 2.0 ** -21                             # common.h: "2^-23-class" - within a factor of four of 2^-23


# ---- sharpness ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["glds_bf16_128x128_bias", "glds_f32_128x128_bias", "glds_bf16_128x128_out_f32", "ws_192x192_bias_res_drop10"])
def test_one_grid_step_in_one_element_is_rejected(name):
    """The comparison of the GPU tests rejects ONE accumulator element moved by ONE grid step (2^-7) - where that step survives
    the output format at all: an fp32 output always, a bf16 output where |value| < 2 (half a bf16 ulp there is 2^-8 < 2^-7)."""
    case = next(c for c in GC.CASES if c["name"] == name)
    seed, a, b, acc, x, ref = GC.reference(case)
    bf16_out = case["dt"] == "bf16" and not case["epi"].get("out_f32")
    good = torch.from_numpy(R.bf16_rne(ref["out"]) if bf16_out else ref["out"])
    got = good.to(torch.bfloat16 if bf16_out else torch.float32)
    assert R.same_bits(got, ref["out"], bf16_out)
    small = np.argwhere(np.abs(ref["out"]) < 1.0) if bf16_out else np.argwhere(np.abs(ref["out"]) >= 0)
    for r, c in (small[0], small[len(small) // 2], small[-1]):
        for step in (R.GRID_STEP, -R.GRID_STEP):
            bad = acc.copy()
            bad[r, c] += step
            e = case["epi"]
            wrong = R.epilogue_ref(bad, bias=x["bias"], act=e.get("act", "none"), aux_in=x["aux_in"], drop=x["drop"], residual=x["res"])["out"]
            if wrong[r, c] == ref["out"][r, c]:
                continue                                     # a dropped element: the perturbation is multiplied by zero
            bad_got = torch.from_numpy(R.bf16_rne(wrong) if bf16_out else wrong).to(got.dtype)
            assert not R.same_bits(bad_got, ref["out"], bf16_out), (r, c, step)
            assert "1 of" in R.first_mismatches(bad_got, ref["out"], bf16_out)


def test_bf16_rne():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0078125, 257.0, 0.0, 1e-3, 788.0])
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).double().numpy()      # fp32 values: one rounding either way
    assert np.array_equal(R.bf16_rne(x), want)
    assert R.bf16_rne(np.array([1.00390625]))[0] == 1.0 and R.bf16_rne(np.array([1.01171875]))[0] == 1.015625    # ties to even
    assert R.bf16_half_ulp(np.array([1.5]))[0] == 2.0 ** -8 and R.bf16_half_ulp(np.array([300.0]))[0] == 1.0
