"""The case matrix of the bit-exact GEMM tests: one entry per (kernel instantiation, epilogue, shape), each NAMING the launch
it is meant to be - (family, tile rows, tile columns, compile-time epilogue kind, reduction split or not, pre-scale launch or
not).  tests/test_cpu_gemm_reference.py proves through hero_gemm_route (host only) that every case is that launch and that the
cases together reach every row of the two launch tables; tests/test_gpu_gemm_exact.py runs them.

The cases, their expected launches and TABLE_ROWS are written by hand from include/hero_hip.h and gemm_route.h's comments; nothing
of them is read from the library (route_words at the end only ASKS the library, for the tests to compare).

Tolerances of the three epilogues that are not exact (GELU, GELU_DG, GELU_BWD), measured by
test_cpu_gemm_reference.py::test_gelu_tolerances on every multiple of 1/32 in [-60, 60] (a superset of the pre-activations
the cases produce: test_exactness_precondition checks that), maximum ABSOLUTE error against float64:
  torch's own fp32 gelu        5.69e-07     torch's own fp32 gelu' (autograd)      1.68e-07
  A&S 7.1.26 in float32 numpy  3.69e-07     its gelu'                              2.68e-07
The bounds use 4 x these: a different but equally legitimate fp32 evaluation order (fp32 dtype, libm erff), and the 1-ulp
hardware exp / reciprocal of the fast form (bf16 dtype).  How they enter a comparison is in test_gpu_gemm_exact.py's header."""

import ctypes as C
import functools
import zlib

import numpy as np

from tests import gemm_reference as R

SKINNY, WS_KK, WS_OO, GLDS_KK, GLDS_OO, STAGED = 1, 2, 3, 4, 5, 6
GEN = 0x100                                    # the run-time-flag epilogue; else a mask of 1 bias, 2 GELU, 4 residual, 8 dropout, 16 gelu'
FACTOR = 4.0
E32_GELU, E32_GRAD = FACTOR * 5.69e-07, FACTOR * 1.68e-07
EAS_GELU, EAS_GRAD = FACTOR * 3.69e-07, FACTOR * 2.68e-07
PREACT_RANGE = 60.0

TILE4 = {0: (128, 128), 1: (192, 128), 2: (256, 256), 3: (64, 64)}            # hero_gemm_force_config 0..3 (+ 4: register staging)
TILE_WS = {9: (192, 192), 10: (128, 192), 13: (64, 128), 14: (64, 192)}       # hero_gemm_force_config 9 / 10 / 13 / 14

# name -> (epilogue fields, EK of the bf16 direct-to-LDS instantiation, EK of the wave-specialised one or None, 64-row tiles only)
EPILOGUES = {
    "plain": ({}, 0, 0),
    "bias": (dict(bias=1), 1, 1),
    "bias_res_drop50": (dict(bias=1, res=1, drop=0.5), 13, 13),
    "bias_res_drop10": (dict(bias=1, res=1, drop=0.1), 13, 13),
    "bias_res": (dict(bias=1, res=1), 13, 13),                         # the dropout instantiation with dropout off
    "bias_gelu": (dict(bias=1, act="gelu"), 3, 3),
    "bias_gelu_dg": (dict(bias=1, act="gelu_dg"), 3, 3),
    "res": (dict(res=1), 4, 4),
    "gelu_bwd": (dict(act="gelu_bwd"), 16, 16),
    "mul_aux": (dict(act="mul_aux"), 16, 16),
    "gelu_bwd_colsum": (dict(act="gelu_bwd", colsum="acc"), 16, 16),
    "mul_aux_colsum": (dict(act="mul_aux", colsum="acc"), 16, 16),
    "mul_aux_colsum_partial": (dict(act="mul_aux", colsum="partial"), 16, 16),
    "relu": (dict(bias=1, act="relu"), GEN, 3),                        # wave-specialised: ReLU on the GELU slot
    "relu_res": (dict(bias=1, act="relu", res=1), GEN, 7),             # wave-specialised: the 64-row tiles only
    "relu_bwd": (dict(act="relu_bwd"), GEN, None),
    "out_f32": (dict(out_f32=1), GEN, None),
}

CASES = []


def _case(name, dt, lay, M, N, K, force, expect, **epi):
    assert all(c["name"] != name for c in CASES), name
    CASES.append(dict(name=name, dt=dt, lay=lay, M=M, N=N, K=K, force=force, expect=expect, epi=epi))


# ---- 4-wave direct-to-LDS K,K: every tile x every epilogue kind, bf16 and fp32 ----------------------------------------------------
GLDS_SHAPE = {0: (293, 264, 320), 1: (421, 264, 320), 2: (549, 520, 320), 3: (165, 136, 320)}
GLDS_SHAPE_F32 = {0: (293, 260, 160), 1: (421, 260, 160), 2: (549, 516, 160), 3: (165, 132, 160)}
for cfg, (bm, bn) in TILE4.items():
    for ename, (fields, ek, _) in EPILOGUES.items():
        _case("glds_bf16_%dx%d_%s" % (bm, bn, ename), "bf16", "KK", *GLDS_SHAPE[cfg], cfg, (GLDS_KK, bm, bn, ek, False, False), **fields)
        if ename != "out_f32":
            _case("glds_f32_%dx%d_%s" % (bm, bn, ename), "f32", "KK", *GLDS_SHAPE_F32[cfg], cfg, (GLDS_KK, bm, bn, GEN, False, False), **fields)
_case("glds_bf16_128x128_out_f32_beta", "bf16", "KK", *GLDS_SHAPE[0], 0, (GLDS_KK, 128, 128, GEN, False, False), out_f32=1, beta=0.5)

# ---- 4-wave register-staged: 128 x 128 (force 4) and 256 x 256 (force 6), all four layout pairs, reduction tails ----------------
for dt, vec in (("bf16", 8), ("f32", 4)):
    for cfg, (bm, bn) in ((4, (128, 128)), (6, (256, 256))):
        for lay in ("KK", "KO", "OK", "OO"):
            M = (296 if lay[0] == "O" else 293) if bm == 128 else (552 if lay[0] == "O" else 549)
            N = (33 if bm == 128 else 65) * vec
            K = (325 if dt == "bf16" else 163) if lay == "OO" else (328 if dt == "bf16" else 164)
            for ename in ("plain", "bias_res_drop50", "bias_gelu", "mul_aux_colsum" if lay == "KK" else "relu_bwd"):
                _case("staged_%s_%s_%dx%d_%s" % (dt, lay, bm, bn, ename), dt, lay, M, N, K, cfg, (STAGED, bm, bn, GEN, False, False),
                      **EPILOGUES[ename][0])

# ---- the transposing direct-to-LDS kernel (bf16 O,O) ----------------------------------------------------------------------------
TR = ("bf16", "OO", 296, 264, 325, 0)
_case("tr_plain", *TR, (GLDS_OO, 128, 128, GEN, False, False))
_case("tr_out_f32_beta0", *TR, (GLDS_OO, 128, 128, GEN, False, False), out_f32=1, beta=0.0)
_case("tr_out_f32_beta05", *TR, (GLDS_OO, 128, 128, GEN, False, False), out_f32=1, beta=0.5)
_case("tr_split3_atomics_beta0", *TR, (GLDS_OO, 128, 128, GEN, True, True), out_f32=1, beta=0.0, split_k=3)
_case("tr_split3_atomics_beta05", *TR, (GLDS_OO, 128, 128, GEN, True, True), out_f32=1, beta=0.5, split_k=3)
_case("tr_split3_atomics_beta1", *TR, (GLDS_OO, 128, 128, GEN, True, False), out_f32=1, beta=1.0, split_k=3)
_case("tr_split3_slabs", *TR, (GLDS_OO, 128, 128, GEN, True, False), out_f32=1, split_k=3, slabs=1)

# ---- split-K on the 4-wave K,K kernels: atomics (pre-scaled) and slabs ---------------------------------------------------------------
for name, dt, shape, cfg, fam in (("glds_bf16", "bf16", (293, 264, 320), 0, GLDS_KK), ("staged_bf16", "bf16", (293, 264, 328), 4, STAGED),
                                  ("glds_f32", "f32", (293, 260, 160), 0, GLDS_KK), ("staged_f32", "f32", (293, 260, 164), 4, STAGED)):
    _case(name + "_split3_atomics_beta0", dt, "KK", *shape, cfg, (fam, 128, 128, GEN, True, True), out_f32=1, beta=0.0, split_k=3)
    _case(name + "_split3_atomics_beta05", dt, "KK", *shape, cfg, (fam, 128, 128, GEN, True, True), out_f32=1, beta=0.5, split_k=3)
    _case(name + "_split3_slabs", dt, "KK", *shape, cfg, (fam, 128, 128, GEN, True, False), out_f32=1, split_k=3, slabs=1)

# ---- a forced locality group of 3 M-tiles on the 64 x 64 tiles: 6 tile rows (M = 5 * 64 + 5, two whole groups) and 5 tile rows
# (M = 4 * 64 + 5: tile_coord's SHORT last group of 2) ------------------------------------------------------------------------------
for M in (325, 261):
    for ename in ("plain", "bias_res_drop50"):
        _case("glds_bf16_64x64_group3_M%d_%s" % (M, ename), "bf16", "KK", M, 136, 320, 3 | (3 << 8),
              (GLDS_KK, 64, 64, EPILOGUES[ename][1], False, False), **EPILOGUES[ename][0])

# ---- wave-specialised K,K: every geometry x every epilogue kind ------------------------------------------------------------------
WS_SHAPE = {9: (421, 392, 320), 10: (293, 392, 320), 13: (165, 264, 448), 14: (165, 392, 320)}
for cfg, (bm, bn) in TILE_WS.items():
    for ename, (fields, _, ek) in EPILOGUES.items():
        if ek is None or (ek == 7 and bm != 64):
            continue
        _case("ws_%dx%d_%s" % (bm, bn, ename), "bf16", "KK", *WS_SHAPE[cfg], cfg, (WS_KK, bm, bn, ek, False, False), **fields)

# ---- ... with more tiles than compute units (256): the persistent workgroups walk several tiles --------------------------------
WS_ROUNDS = {13: (2117, 1032, 448),        # 34 x 9 = 306 tiles of 64 x 128
             14: (2117, 1416, 320),        # 34 x 8 = 272 tiles of 64 x 192
             10: (2117, 2888, 256),        # 17 x 16 = 272 tiles of 128 x 192
             9: (3100, 2888, 256)}         # 17 x 16 = 272 tiles of 192 x 192
for cfg, shape in WS_ROUNDS.items():
    for ename in ("plain", "bias_res_drop50"):
        _case("ws_%dx%d_rounds_%s" % (*TILE_WS[cfg], ename), "bf16", "KK", *shape, cfg, (WS_KK, *TILE_WS[cfg], EPILOGUES[ename][2], False, False),
              **EPILOGUES[ename][0])

# ---- wave-specialised O,O (the weight-gradient accumulate): the route cuts 33 k-steps into 7 ranges of 5 ------------------------------
for beta, pre in ((0.0, True), (1.0, False), (0.5, True)):
    _case("ws_oo_beta%g" % beta, "bf16", "OO", 392, 392, 2100, 9, (WS_OO, 192, 192, 0, True, pre), out_f32=1, beta=beta)
_case("ws_oo_split_hint4", "bf16", "OO", 392, 392, 2100, 9, (WS_OO, 192, 192, 0, True, False), out_f32=1, beta=1.0, split_k=4)

# ---- skinny fp32 (heuristic only) --------------------------------------------------------------------------------------------------
for M, N, K in ((32, 772, 260), (5, 772, 1300)):
    _case("skinny_M%d_plain" % M, "f32", "KK", M, N, K, -1, (SKINNY, 32, 8, 0, False, False))
    _case("skinny_M%d_bias" % M, "f32", "KK", M, N, K, -1, (SKINNY, 32, 8, 0, False, False), bias=1)

MULTI_ROUND = [c["name"] for c in CASES if "_rounds_" in c["name"]]

# ---- every row of the two launch tables, by hand: (family, dtype, A layout, B layout, tile rows, tile columns, EK) --------------------
TABLE_ROWS = []
for bm, bn in ((128, 128), (192, 128), (256, 256), (64, 64)):                 # 4 tiles x (7 bf16 kinds + 1 fp32) = 32
    for ek in (GEN, 0, 1, 13, 3, 4, 16):
        TABLE_ROWS.append((GLDS_KK, "bf16", "K", "K", bm, bn, ek))
    TABLE_ROWS.append((GLDS_KK, "f32", "K", "K", bm, bn, GEN))
for dt in ("bf16", "f32"):                                                    # 2 dtypes x 2 tiles x 4 layout pairs = 16 staged
    for bm, bn in ((128, 128), (256, 256)):
        for al in "KO":
            for bl in "KO":
                TABLE_ROWS.append((STAGED, dt, al, bl, bm, bn, GEN))
TABLE_ROWS.append((GLDS_OO, "bf16", "O", "O", 128, 128, GEN))                 # 1 transposing
for bm, bn in ((192, 192), (128, 192), (64, 128), (64, 192)):                 # 6 x 4 wave-specialised K,K
    for ek in (0, 1, 13, 3, 4, 16):
        TABLE_ROWS.append((WS_KK, "bf16", "K", "K", bm, bn, ek))
TABLE_ROWS.append((WS_KK, "bf16", "K", "K", 64, 128, 7))                      # + 2: ReLU + residual on the 64-row tiles
TABLE_ROWS.append((WS_KK, "bf16", "K", "K", 64, 192, 7))
TABLE_ROWS.append((WS_OO, "bf16", "O", "O", 192, 192, 0))                     # + 1 O,O
TABLE_ROWS.append((SKINNY, "f32", "K", "K", 32, 8, 0))                        # 1 skinny (not in a table: its own launch)
UNREACHABLE = (WS_OO, "bf16", "O", "O", 128, 192, 0)                          # gemm_ws_kernel<2, 3, true, 0>: instantiated, no route
assert len(TABLE_ROWS) == 49 + 27 + 1 and len(set(TABLE_ROWS)) == len(TABLE_ROWS)


def table_row(case):
    fam, bm, bn, ek = case["expect"][:4]
    return (fam, case["dt"], case["lay"][0], case["lay"][1], bm, bn, ek)


# ---- a case's operands, reference and route (shared by the CPU and the GPU tests) ------------------------------------------------------
def operands(case):
    """(A [M, K], B [K, N]) float64 on the grids, one draw per (dtype, layouts, shape): shared by all epilogues of a shape."""
    return _operands(case["dt"], case["lay"], case["M"], case["N"], case["K"])


@functools.lru_cache(maxsize=4)
def _operands(dt, lay, M, N, K):
    seed = zlib.crc32(("%s %s %d %d %d" % (dt, lay, M, N, K)).encode())
    a, b = R.grid_x(seed, (M, K)), np.ascontiguousarray(R.grid_w(seed, (N, K)).T)
    return seed, a, b, a @ b


def epilogue_inputs(case, seed):
    """The epilogue's operands of a case, float64 on their grids: dict(bias, res, aux_in, c0, drop)."""
    e, M, N = case["epi"], case["M"], case["N"]
    act = e.get("act", "none")
    out = dict(bias=R.grid_bias(seed, N) if e.get("bias") else None, res=R.grid_quarter(seed, (M, N)) if e.get("res") else None,
               aux_in=None, c0=None, drop=None)
    if act in ("mul_aux", "relu_bwd"):
        out["aux_in"] = R.grid_quarter(seed, (M, N), tag=6)
    elif act == "gelu_bwd":
        out["aux_in"] = R.grid_preact(seed, (M, N))
    if e.get("beta", 0.0) != 0.0:
        out["c0"] = R.grid_quarter(seed, (M, N), tag=7)
    if e.get("drop"):
        out["drop"] = (0x5DEECE66D1234567 ^ seed, 3 + seed % 5) + R.dropout_params(e["drop"])
    return out


def reference(case):
    seed, a, b, acc = operands(case)
    x = epilogue_inputs(case, seed)
    e = case["epi"]
    ref = R.epilogue_ref(acc, bias=x["bias"], act=e.get("act", "none"), aux_in=x["aux_in"], drop=x["drop"], residual=x["res"],
                         beta=e.get("beta", 0.0), c0=x["c0"], tile_rows=case["expect"][1] if e.get("colsum") == "partial" else 0)
    return seed, a, b, acc, x, ref


def route_words(lib, case):
    """hero_gemm_route for a case under its force config, with the padded leading dimensions the GPU test passes."""
    from hero_amd import _lib as L
    e, M, N, K = case["epi"], case["M"], case["N"], case["K"]
    vec = 8 if case["dt"] == "bf16" else 4
    p = lambda flag: 64 if flag else None
    act = e.get("act", "none")
    thr, scale = R.dropout_params(e["drop"]) if e.get("drop") else (0, 1.0)
    split = int(e.get("split_k", 1))
    epi = L.GemmEpilogue(p(e.get("bias")), p(e.get("res")), p(act != "none"), R.ACT[act], 1 if e.get("out_f32") else 0, float(e.get("beta", 0.0)),
                         split, L.Dropout(64 if thr else None, 1, thr, scale), p(e.get("colsum")), 1 if e.get("colsum") == "partial" else 0, 0,
                         (M + 1) * (N + vec) if e.get("slabs") else 0)
    al, bl = (L.LAYOUT_K if ch == "K" else L.LAYOUT_O for ch in case["lay"])
    lda, ldb = (K if al == L.LAYOUT_K else M) + vec, (K if bl == L.LAYOUT_K else N) + vec
    out = np.zeros(16, dtype=np.int32)
    lib.hero_gemm_force_config(case["force"])
    try:
        n = lib.hero_gemm_route(M, N, K, lda, ldb, N + vec, al, bl, L.BF16 if case["dt"] == "bf16" else L.F32, C.byref(epi), out.ctypes.data, out.size)
    finally:
        lib.hero_gemm_force_config(-1)
    assert n == 12, (case["name"], n, lib.hero_last_error())
    return [int(x) for x in out[:n]]


def named_launch(w):
    return (w[0], w[1], w[2], w[3], w[7] > 1, bool(w[10]))
