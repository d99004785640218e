"""hero_gemm, hero_fold_slabs, hero_wgrad_group and hero_wgrad_batch on operands for which every correct kernel gives the
same bits (tests/gemm_reference.py): one case per kernel instantiation x epilogue (tests/gemm_cases.py), each proven through
hero_gemm_route to be the launch it names before it runs, compared with `torch.equal` against the float64 restatement of the
header's contract - an fp32 output is that number, a bf16 output its round-to-nearest-even.

The three epilogues that are not exact get bounds derived from references, never from the kernels (measured values and what
they were measured against: tests/gemm_cases.py's header; re-measured by test_cpu_gemm_reference.py::test_gelu_tolerances):
  E32  = 4 x the maximum absolute error of torch's own fp32 gelu (5.69e-07) / gelu' (1.68e-07) against float64,
  E_as = 4 x the maximum absolute error of a float32 numpy restatement of Abramowitz-Stegun 7.1.26 (3.69e-07 / 2.68e-07),
both on every multiple of 1/32 in [-60, 60].  With f = gelu or gelu', u the pre-activation (exact) and ref the float64 value:
  GELU / GELU_DG, fp32 dtype:   |got - ref| <= E32 (|ref| + 1)
  GELU / GELU_DG, bf16 dtype:   |got - ref| <= half a bf16 ulp at ref + E_as            (exactly ONE output rounding)
  GELU_BWD (out = acc f'(aux)): the error of f' reaches the output through the exact factor acc, and the product is one more
                                fp32 rounding:  |acc| * (E32 (|f'| + 1)  or  E_as) + 2^-23 |ref|  (+ half a bf16 ulp at ref)
The saved pre-activation and everything in front of the nonlinearity stay exact.

Every case passes leading dimensions one vector wider than the logical widths, pre-fills C / aux / the column-sum table with
a NaN bit pattern and guard rows, and holds every pad column and guard row bitwise untouched afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_cases as GC
from tests import gemm_reference as R

pytestmark = pytest.mark.gpu

GUARD = 3                       # rows behind the last one of C / aux, all sentinel
PAD_IN = 8192.0                 # pad columns of the operands: finite, so that a kernel may load (not use) them
SENT = {torch.bfloat16: (torch.int16, 0x7FD5), torch.float32: (torch.int32, 0x7FC12345)}      # quiet NaNs with a payload


@pytest.fixture(scope="module")
def Lb():
    from hero_amd import _lib
    _lib.lib()
    return _lib


def bits(t):
    return t.view(SENT[t.dtype][0])


def sentinel(rows, ld, dtype):
    it, pattern = SENT[dtype]
    return torch.full((rows, ld), pattern, dtype=it, device="cuda").view(dtype)


def padded_in(x64, vec, dtype):
    """An operand [rows, cols] in a [rows, cols + vec] buffer."""
    rows, cols = x64.shape
    buf = torch.full((rows, cols + vec), PAD_IN, dtype=dtype, device="cuda")
    buf[:, :cols] = torch.from_numpy(np.ascontiguousarray(x64)).to(dtype)
    return buf


def padded_out(rows, cols, ld, dtype, init64=None, guard=GUARD):
    buf = sentinel(rows + guard, ld, dtype)
    if init64 is not None:
        buf[:rows, :cols] = torch.from_numpy(np.ascontiguousarray(init64)).to(dtype)
    return buf


def outside_untouched(buf, rows, cols):
    b = bits(buf).clone()
    b[:rows, :cols] = SENT[buf.dtype][1]
    return bool((b == SENT[buf.dtype][1]).all())


def region(buf, rows, cols):
    return buf[:rows, :cols].cpu()


def assert_exact(got, want64, what):
    bf16 = got.dtype == torch.bfloat16
    assert R.same_bits(got, want64, bf16), "%s: %s" % (what, R.first_mismatches(got, want64, bf16))


def assert_within(got, ref64, bound, what):
    assert not bool(torch.isnan(got).any()), what + ": NaN left in the output"
    ok, ratio = R.within(got, ref64, bound)
    print("%s: worst error / bound = %.3f" % (what, ratio))
    assert ok, "%s: error is %.3f x the bound" % (what, ratio)


def seed_tensor(word):
    return torch.tensor([word - (1 << 64) if word >= (1 << 63) else word], dtype=torch.int64, device="cuda")


def nonlinear_bound(ref64, f32_dtype, bf16_out, e32, eas, acc=None, factor=None):
    """The bounds of the header."""
    if acc is None:
        b = e32 * (np.abs(ref64) + 1.0) if f32_dtype else np.full(ref64.shape, eas)
    else:
        b = np.abs(acc) * (e32 * (np.abs(factor) + 1.0) if f32_dtype else eas) + 2.0 ** -23 * np.abs(ref64)
    return b + (R.bf16_half_ulp(ref64) if bf16_out else 0.0)


def run_case(Lb, case):
    lib = Lb.lib()
    e, M, N, K, lay = case["epi"], case["M"], case["N"], case["K"], case["lay"]
    bf16 = case["dt"] == "bf16"
    T, vec = (torch.bfloat16, 8) if bf16 else (torch.float32, 4)
    OT = torch.float32 if e.get("out_f32") else T
    act = e.get("act", "none")
    seed, a, b, acc, x, ref = GC.reference(case)

    # ---- the launch is the instantiation the case names
    w = GC.route_words(lib, case)
    assert GC.named_launch(w) == tuple(case["expect"]), w
    splits, k_per_split = w[7], w[8]

    dA = padded_in(a if lay[0] == "K" else a.T, vec, T)
    dB = padded_in(b.T if lay[1] == "K" else b, vec, T)
    ldc = N + vec
    slabs = bool(e.get("slabs"))
    stride = (M + 1) * ldc
    if slabs:
        dC = sentinel(splits + 1, stride, torch.float32)                   # one guard slab behind the last
    else:
        dC = padded_out(M, N, ldc, OT, x["c0"])
    bias = torch.from_numpy(x["bias"]).float().cuda() if x["bias"] is not None else None
    res = padded_in(x["res"], vec, T) if x["res"] is not None else None
    aux = aux_before = None
    if act in ("gelu_bwd", "relu_bwd", "mul_aux"):
        aux = padded_out(M, N, ldc, T, x["aux_in"])
        aux_before = bits(aux).clone()
    elif act != "none":
        aux = padded_out(M, N, ldc, T)
    colsum = cs0 = None
    if e.get("colsum") == "acc":
        cs0 = R.grid_quarter(seed, (1, N), tag=8)
        colsum = padded_out(1, N, N + 4, torch.float32, cs0, guard=1)
    elif e.get("colsum") == "partial":
        colsum = padded_out((M + 63) // 64, N, N, torch.float32, guard=2)
    drop, seed_dev = Lb.no_dropout(), None
    if x["drop"]:
        seed_dev = seed_tensor(x["drop"][0])
        drop = Lb.Dropout(seed_dev.data_ptr(), x["drop"][1], x["drop"][2], x["drop"][3])
    p = lambda t: t.data_ptr() if t is not None else None
    epi = Lb.GemmEpilogue(p(bias), p(res), p(aux), R.ACT[act], 1 if e.get("out_f32") else 0, float(e.get("beta", 0.0)), int(e.get("split_k", 1)),
                          drop, p(colsum), 1 if e.get("colsum") == "partial" else 0, 0, stride if slabs else 0)
    al, bl = (Lb.LAYOUT_K if ch == "K" else Lb.LAYOUT_O for ch in lay)
    lib.hero_gemm_force_config(case["force"])
    try:
        Lb.check(lib.hero_gemm(dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), M, N, K, dA.shape[1], dB.shape[1], ldc, al, bl, Lb.BF16 if bf16 else Lb.F32,
                               C.byref(epi), Lb.stream()))
    finally:
        lib.hero_gemm_force_config(-1)
    torch.cuda.synchronize()
    name = case["name"]

    if slabs:
        assert splits == lib.hero_gemm_splits(K, e["split_k"], Lb.BF16 if bf16 else Lb.F32)
        want = R.split_slabs(a, b, k_per_split, splits)
        for s in range(splits):
            slab = dC[s].view(M + 1, ldc)
            assert_exact(region(slab, M, N), want[s], "%s slab %d" % (name, s))
            assert outside_untouched(slab, M, N), "%s: slab %d written outside [M, N]" % (name, s)
        assert outside_untouched(dC[splits:], 0, 0), name + ": the slab behind the last was written"
        for out_dtype in (torch.float32, torch.bfloat16):
            out = sentinel(1, M * ldc + 8, out_dtype)
            Lb.check(lib.hero_fold_slabs(dC.data_ptr(), splits, stride, out.data_ptr(), M * ldc, Lb.dt(out), Lb.stream()))
            torch.cuda.synchronize()
            assert_exact(out[0, :M * ldc].view(M, ldc)[:, :N].cpu(), R.fold_slabs(want), "%s fold to %s" % (name, out_dtype))
            assert outside_untouched(out[:, M * ldc:], 0, 0), name + ": fold wrote past n"
        assert R.is_fp32(acc) and np.array_equal(R.fold_slabs(want), acc)
        return

    # ---- the output
    got = region(dC, M, N)
    assert not bool(torch.isnan(got).any()), name + ": an output element still holds the NaN it was pre-filled with"
    bf16_out = OT == torch.bfloat16
    if act in R.EXACT_ACTS:
        assert_exact(got, ref["out"], name)
    elif act == "gelu_bwd":
        assert_within(got, ref["out"], nonlinear_bound(ref["out"], not bf16, bf16_out, GC.E32_GRAD, GC.EAS_GRAD, acc, ref["factor"]), name)
    else:
        assert_within(got, ref["out"], nonlinear_bound(ref["out"], not bf16, bf16_out, GC.E32_GELU, GC.EAS_GELU), name)
    assert outside_untouched(dC, M, N), name + ": C written outside [M, N]"

    # ---- aux
    if aux_before is not None:
        assert torch.equal(bits(aux), aux_before), name + ": the epilogue wrote to an aux it only reads"
    elif aux is not None:
        if act == "gelu_dg":
            assert_within(region(aux, M, N), ref["aux"], nonlinear_bound(ref["aux"], not bf16, bf16, GC.E32_GRAD, GC.EAS_GRAD), name + " aux")
        else:
            assert_exact(region(aux, M, N), ref["aux"], name + " aux")        # GELU: the pre-activation; RELU: its output
        assert outside_untouched(aux, M, N), name + ": aux written outside [M, N]"

    # ---- column sums of the values written to C, before rounding
    if colsum is not None:
        if e["colsum"] == "acc":
            got_cs, want_cs, rows = region(colsum, 1, N), cs0 + ref["colsum"].reshape(1, N), 1
        else:
            rows = (M + 63) // 64
            got_cs, want_cs = region(colsum, rows, N), ref["partial"]
        if act in R.EXACT_ACTS:
            assert_exact(got_cs, want_cs, name + " colsum")
        else:       # the elements' bounds add up, and M fp32 additions of numbers whose magnitudes sum to S lose at most M 2^-24 S
            be = nonlinear_bound(ref["out"], not bf16, False, GC.E32_GRAD, GC.EAS_GRAD, acc, ref["factor"])
            S = np.abs(ref["out"]).sum(axis=0) + np.abs(cs0).reshape(-1)
            assert_within(got_cs, want_cs, (be.sum(axis=0) + M * 2.0 ** -24 * S).reshape(1, N), name + " colsum")
        assert outside_untouched(colsum, rows, N), name + ": column sums written outside the table"


@pytest.mark.parametrize("case", GC.CASES, ids=lambda c: c["name"])
def test_gemm_case(Lb, case):
    run_case(Lb, case)


def test_beta_zero_overwrites_nan(Lb):
    """With beta = 0 a NaN already in C must not survive - in the epilogue's store and in the pre-scale launch of the atomics
    paths (both store rather than multiply): the cases above pre-fill C with NaN and demand exact results; this one makes sure
    such cases are in the matrix."""
    names = {c["name"] for c in GC.CASES if c["epi"].get("out_f32") and c["epi"].get("beta", 0.0) == 0.0 and not c["epi"].get("slabs")}
    assert {"tr_out_f32_beta0", "tr_split3_atomics_beta0", "glds_bf16_split3_atomics_beta0", "staged_f32_split3_atomics_beta0", "ws_oo_beta0"} <= names


# ---- weight gradients ------------------------------------------------------------------------------------------------------------------
def _ints(shape, seed, lo=-3, hi=4):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g, device="cuda")


def _wgrad_setup(Lb, K, shapes, seed, dbias_from=None):
    """Problems dw_i [M_i, N_i] += dy[:, cols_i]^T x_i over K rows: dy is ONE [K, sum M_i + 8] matrix (column slices, as the fused
    QKV gradient passes them), x_i and dw_i carry a pad vector, dw_i guard rows.  -> (probs, keep-alive, checks)."""
    Ms = [m for m, _ in shapes]
    dy = torch.full((K, sum(Ms) + 8), PAD_IN, dtype=torch.bfloat16, device="cuda")
    dy[:, :sum(Ms)] = _ints((K, sum(Ms)), seed).to(torch.bfloat16)
    probs = (Lb.WgradProblem * len(shapes))()
    keep, checks, col0 = [dy], [], 0
    for i, (m, n) in enumerate(shapes):
        x = torch.full((K, n + 8), PAD_IN, dtype=torch.bfloat16, device="cuda")
        x[:, :n] = _ints((K, n), seed + 1 + i).to(torch.bfloat16)
        dw0 = _ints((m, n), seed + 50 + i, -8, 9).double() / 4
        dw = sentinel(m + GUARD, n + 4, torch.float32)
        dw[:m, :n] = dw0.float()
        prod = dy[:, col0:col0 + m].double().t() @ x[:, :n].double()
        assert float((dy[:, col0:col0 + m].double().abs().t() @ x[:, :n].double().abs()).max()) < 2.0 ** 24    # integers: exact in fp32
        db = db0 = None
        if dbias_from is not None and i >= dbias_from:
            db0 = _ints((m,), seed + 90 + i, -8, 9).double() / 4
            db = sentinel(1, m + 4, torch.float32)
            db[0, :m] = db0.float()
        probs[i] = Lb.WgradProblem(dy[:, col0:].data_ptr(), x.data_ptr(), dw.data_ptr(), m, n, dy.shape[1], x.shape[1], dw.shape[1], 4,
                                   db.data_ptr() if db is not None else None)
        keep += [x, dw, db]
        checks.append((dw, dw0, prod, db, db0, dy[:, col0:col0 + m].double().sum(dim=0)))
        col0 += m
    return probs, keep, checks


def _wgrad_check(checks, times, what):
    for i, (dw, dw0, prod, db, db0, dysum) in enumerate(checks):
        m, n = dw0.shape
        want = dw0 + times * prod
        assert torch.equal(dw[:m, :n].double(), want), "%s: dw of problem %d: %d elements differ" % (what, i, int((dw[:m, :n].double() != want).sum()))
        assert outside_untouched(dw, m, n), "%s: dw of problem %d written outside [M, N]" % (what, i)
        if db is not None:
            assert torch.equal(db[0, :m].double(), db0 + times * dysum), "%s: dbias of problem %d" % (what, i)
            assert outside_untouched(db, 1, m), "%s: dbias of problem %d written past M" % (what, i)


BERT_LAYER_MINUS_FFN2 = [(2304, 768), (768, 768), (3072, 768)]          # fused QKV, attention output, FFN1: 48 + 16 + 64 tiles of 192 x 192


@pytest.mark.parametrize("K,path", [(1032, "stream-K"), (520, "hero_gemm fallback")], ids=["stream_k", "fallback"])
def test_wgrad_group(Lb, K, path):
    """hero_wgrad_group accumulates into non-zero dw from column slices of one dy.  K = 1032: its stream-K kernel (bf16,
    K >= 1024 with a tail of 8 rows, 128 tiles x 17 k-steps >= 8 x 256 compute units); K = 520: one hero_gemm per problem."""
    assert (128 * ((K + 63) // 64) >= 8 * 256 and K >= 1024) == (path == "stream-K")
    lib = Lb.lib()
    probs, keep, checks = _wgrad_setup(Lb, K, BERT_LAYER_MINUS_FFN2, seed=7)
    ms, flops, launches = C.c_double(), C.c_double(), C.c_longlong()
    lib.hero_prof_enable(1)                 # slot 9 counts the wave-specialised O,O launches: the stream-K kernel, not the fallback's GEMMs
    try:
        for times in (1, 2):
            Lb.check(lib.hero_wgrad_group(probs, len(BERT_LAYER_MINUS_FFN2), K, Lb.BF16, Lb.stream()))
            torch.cuda.synchronize()
            _wgrad_check(checks, times, "hero_wgrad_group (%s), launch %d" % (path, times))
        Lb.check(lib.hero_prof_read(9, C.byref(ms), C.byref(flops), C.byref(launches)))
    finally:
        lib.hero_prof_enable(0)
    assert launches.value == (2 if path == "stream-K" else 0), launches.value


@pytest.mark.parametrize("K,shapes,what", [(520, [(768, 768)], "sliced tail only: 16 tiles"),
                                           (456, [(3072, 768)] * 4, "one whole round: 256 tiles")], ids=["tail_only", "whole_round"])
def test_wgrad_batch(Lb, K, shapes, what):
    """hero_wgrad_batch: a group that is only a sliced tail, and the smallest group with a whole round of 256 tiles - at the
    shortest reduction the plan takes (8 k-steps of 64: K > 448; shorter ones, K = 200 for one, are hero_wgrad_group's and the plan
    says so with 0 words).  dbias on all problems but the first, a second launch accumulates once more."""
    lib = Lb.lib()
    probs, keep, checks = _wgrad_setup(Lb, K, shapes, seed=11, dbias_from=1)
    buf = np.zeros(8 + 8 * 256 * 16, dtype=np.int32)
    assert lib.hero_wgrad_batch_plan(probs, len(shapes), 200, buf.ctypes.data, buf.size) == 0
    words = lib.hero_wgrad_batch_plan(probs, len(shapes), K, buf.ctypes.data, buf.size)
    assert words > 8, (words, lib.hero_last_error())
    assert buf[6] == sum(-(-m // 192) * -(-n // 192) for m, n in shapes)
    plan = torch.from_numpy(buf[:words].copy()).cuda()
    for times in (1, 2):
        Lb.check(lib.hero_wgrad_batch(probs, len(shapes), K, Lb.BF16, plan.data_ptr(), words, Lb.stream()))
        torch.cuda.synchronize()
        _wgrad_check(checks, times, "hero_wgrad_batch (%s), launch %d" % (what, times))
