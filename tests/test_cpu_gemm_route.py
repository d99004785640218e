"""hero_gemm_route (host only) against the kernel trace of the commit that tests/golden/gemm_routes.json names: for every
recorded case the route must name the kernel that ran there, with its grid and workgroup size, and a pre-scale launch
exactly where the trace shows scale_f32_kernel first.  The table was recorded once (tools/gemm_routes.py) and is the
reference; it is never regenerated from the code under test."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")))
ACT = dict(none=0, gelu=1, relu=2, gelu_bwd=3, relu_bwd=4, gelu_dg=5, mul_aux=6)
SKINNY, WS_KK, WS_OO, GLDS_KK, GLDS_OO, STAGED = 1, 2, 3, 4, 5, 6
CFG = {(128, 128): "2, 2, 2, 2", (192, 128): "2, 2, 3, 2", (256, 256): "2, 4, 4, 2", (64, 64): "2, 2, 1, 1"}
# Dynamic LDS per kernel as the kernels' own geometry structs define it (Cfg::LDS, GldsRing::LDS, ws::Geo::LDS, 64 KiB for the
# transposing O,O kernel): the tracer reports 0 bytes for every dispatch, so the recorded column cannot hold the routes to it.
LDS = {(GLDS_KK, 128, 128): 65536, (GLDS_KK, 192, 128): 81920, (GLDS_KK, 256, 256): 131072, (GLDS_KK, 64, 64): 65536,
       (STAGED, 128, 128): 65536, (STAGED, 256, 256): 131072, (GLDS_OO, 128, 128): 65536}


@pytest.fixture(scope="module")
def lib():
    from hero_amd import build
    build.build()
    from hero_amd import _lib as L
    return L.lib()


def kernel_name(case, w):
    """The demangled name of the instantiation that route words `w` denote."""
    family, bm, bn, ek = w[0], w[1], w[2], w[3]
    t = "unsigned short" if case["dt"] == "bf16" else "float"
    if family == SKINNY:
        return "gemm_skinny_f32_kernel(float const*, float const*, float*, float const*, int, int, int, int, int, int)"
    if family in (WS_KK, WS_OO):
        return "void hero::ws::gemm_ws_kernel<%d, %d, %s, %d>(hero::ws::WsArgs)" % (bm // 64, bn // 64, "true" if family == WS_OO else "false", ek)
    if family == GLDS_KK:
        return "void hero::gemm_glds_kernel<%s, hero::Cfg<%s>, %d>(hero::GemmArgs)" % (t, CFG[bm, bn], ek)
    if family == GLDS_OO:
        return "hero::gemm_glds_tr_kernel(hero::GemmArgs)"
    assert family == STAGED, w
    return "void hero::gemm_kernel<%s, %d, %d, hero::Cfg<%s> >(hero::GemmArgs)" % (t, case["lay"][0] == "O", case["lay"][1] == "O", CFG[bm, bn])


def route(lib, case):
    from hero_amd import _lib as L
    e, M, N, K = case["epi"], case["M"], case["N"], case["K"]
    p = lambda flag: 64 if flag else None                       # the route reads pointers as null / non-null only
    drop = L.Dropout(64, 1, 6554, 1.0 / 0.9) if e.get("drop") else L.no_dropout()
    epi = L.GemmEpilogue(p(e.get("bias")), p(e.get("residual")), p(e.get("aux")), ACT[e.get("act", "none")], 1 if e.get("out_f32") else 0,
                         float(e.get("beta", 0.0)), int(e.get("split_k", 1)), drop, p(e.get("colsum")), 1 if e.get("colsum") == "partial" else 0, 0,
                         M * N if e.get("slabs") else 0)
    al, bl = (L.LAYOUT_K if ch == "K" else L.LAYOUT_O for ch in case["lay"])
    ld = lambda layout, outer: K if layout == L.LAYOUT_K else outer
    out = np.zeros(16, dtype=np.int32)
    n = lib.hero_gemm_route(M, N, K, ld(al, M), ld(bl, N), N, al, bl, L.BF16 if case["dt"] == "bf16" else L.F32, C.byref(epi), out.ctypes.data, out.size)
    assert n == 12, (n, lib.hero_last_error())
    return [int(x) for x in out[:n]]


@pytest.mark.parametrize("case", GOLD["cases"], ids=[c["name"] for c in GOLD["cases"]])
def test_route_is_the_recorded_launch(lib, case):
    probe = np.zeros(16, dtype=np.int32)
    from hero_amd import _lib as L
    plain = L.GemmEpilogue(None, None, None, 0, 0, 0.0, 1, L.no_dropout(), None, 0, 0, 0)
    assert lib.hero_gemm_route(24000, 3072, 768, 768, 768, 3072, 0, 0, L.BF16, C.byref(plain), probe.ctypes.data, probe.size) == 12
    if probe[4] != GOLD["cus"]:                      # 2000 tiles: one persistent workgroup per compute unit
        pytest.skip("the golden routes were recorded on %d compute units; this library reports %d" % (GOLD["cus"], probe[4]))
    lib.hero_gemm_force_config(case["force"])
    try:
        w = route(lib, case)
    finally:
        lib.hero_gemm_force_config(-1)
    launches = list(case["launches"])
    scaled = launches[0]["kernel"].startswith("scale_f32_kernel") or launches[0]["kernel"].startswith("hero::scale_f32_kernel")
    assert bool(w[10]) == scaled, (w, launches)
    if scaled:
        launches.pop(0)
    assert len(launches) == 1, launches
    got = dict(kernel=kernel_name(case, w), grid=w[4], threads=w[5])
    want = {k: launches[0][k] for k in got}
    assert got == want, (w, launches)
    if launches[0]["lds"]:
        assert w[6] == launches[0]["lds"]
    family = w[0]
    lds = 163840 if family in (WS_KK, WS_OO) else 32 * min(case["K"], 1024) * 4 + 16 if family == SKINNY else LDS[family, w[1], w[2]]
    assert w[6] == lds, w


def test_route_validates_like_hero_gemm(lib):
    from hero_amd import _lib as L
    out = np.zeros(12, dtype=np.int32)
    e = L.GemmEpilogue(None, None, None, 0, 0, 0.0, 1, L.no_dropout(), None, 0, 0, 0)
    call = lambda *a, epi=e, cap=12: lib.hero_gemm_route(*a, C.byref(epi), out.ctypes.data, cap)
    assert call(64, 64, 64, 64, 64, 64, 0, 0, L.BF16, cap=11) == -1                # capacity
    assert call(64, 66, 64, 64, 64, 68, 0, 0, L.BF16) == -1                        # N % 4
    assert call(64, 64, 68, 68, 68, 64, 0, 0, L.BF16) == -1                        # bf16 K % 8
    assert call(64, 64, 68, 68, 68, 64, 0, 0, L.F32) == 12                         # f32 K % 4
    assert call(64, 64, 64, 64, 64, 64, 0, 0, 2) == -1                             # dtype
    split = L.GemmEpilogue(64, None, None, 0, 1, 0.0, 4, L.no_dropout(), None, 0, 0, 0)
    assert call(64, 64, 512, 512, 512, 64, 0, 0, L.BF16, epi=split) == -1          # split_k with a bias
    assert call(0, 64, 64, 64, 64, 64, 0, 0, L.BF16) == 12 and out[0] == 0         # empty output: nothing to launch
