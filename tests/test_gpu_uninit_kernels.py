"""No kernel result may depend on what an uninitialised buffer held: every kernel family run twice on identical inputs, once
with every buffer the library allocates uninitialised (outputs, saved probabilities and statistics, LayerNorm statistics and
column partials, split-K slabs, workspaces) pre-filled with 0.0 and once with NaN; every result must be finite and
bit-identical between the two (tests/uninit.py).  No tolerance anywhere.  Needs a real MI355X (-m gpu).

Shapes: the smallest of each dispatch class, taken from the tests that pin those classes (test_gpu_dropout_masks.ATTN_CASES,
tests/gemm_cases.CASES, test_gpu_kernels.py)."""

import pytest
import torch

from tests import dropout_reference as DR
from tests import gemm_cases as GC
from tests import uninit
from tests.test_gpu_dropout_masks import LN_DTYPES, LN_IDS
from tests.test_gpu_kernels import rnd

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SEED = 0x5EED0123456789AB
SITE = (1 << 32) + 7
H = 2

# Every element that a comparison leaves out, and why.  Nothing else is excluded: whatever an op returns to its caller as a
# result (ctx, dqkv, y, dx, dgamma / dbeta / dbias, GEMM outputs, losses, gradients) is compared in full.
EXCLUSIONS = {
    "attention.saved, packed batch":
        "k_attn_fwd's saved tensor is [S, H, Lm, Lm] probabilities or [S, H, Lm, 2] row statistics with Lm the LONGEST sequence; "
        "a packed sequence of L < Lm rows has no query row i >= L and no key j >= L, the forward writes (i < L, j < L) only "
        "and the backward must not let the rest reach dqkv - which the full comparison of dqkv checks",
    "k_gather_rows(tail_rows=n), rows behind the result":
        "spare rows of the same storage that a following row stack writes before anything reads them; the returned view "
        "[:rows] is compared in full",
    "k_dec_attn_step, cache rows behind the step's position":
        "the key/value cache [N, Tcap, 2D] is filled one row per decode step; rows > pos are written by later steps and the "
        "step at pos must not read them - which the full comparison of its ctx checks; rows <= pos are compared",
}
# (the third exclusion the contract allows - probabilities of a forward-only call that nothing reads - is not used: the
# forward-only case below is padded, writes its whole probability tensor, and is compared in full)


@pytest.fixture(scope="module")
def HF():
    from hero_amd import functional
    return functional


@pytest.fixture(scope="module")
def Lb():
    from hero_amd import _lib
    _lib.lib()
    return _lib


def _drop(Lb, seed_word, p, site=SITE):
    if not p:
        return None
    return Lb.Dropout(seed_word.data_ptr(), site, max(1, int(round(p * 65536.0))), 1.0 / (1.0 - p))


def _seed_word():
    return torch.tensor([SEED], dtype=torch.int64, device="cuda")


def _lens(L):
    return [max(1, L - 3 * i) for i in range(3)]


# ==== attention =====================================================================================================================
# (id, dtype, lens, packed, save_probs, ctx to the backward, backward, pairs per wave): one per row of the dispatch table in
# test_gpu_dropout_masks.ATTN_CASES
ATTN = [("f32-%d" % n, F32, _lens(n), False, False, True, True, 0) for n in (9, 23, 61, 70, 150)] + \
       [("bf16-%d-%s" % (n, "probs" if sp else "stats"), BF16, _lens(n), False, sp, True, True, 0) for n in (15, 31, 37, 64) for sp in (False, True)] + \
       [("bf16-%d-long" % n, BF16, _lens(n), False, False, True, True, 0) for n in (65, 130, 256)] + \
       [("bf16-70-valu-bwd", BF16, _lens(70), False, False, False, True, 0),
        ("bf16-257-fwd", BF16, _lens(257), False, False, True, False, 0),
        ("bf16-31-ppw3", BF16, _lens(31), False, False, True, True, 3),
        ("f32-packed-24", F32, [24, 9, 1, 17], True, False, True, True, 0)] + \
       [("bf16-packed-%d-%s" % (lens[0], "probs" if sp else "stats"), BF16, lens, True, sp, True, True, 0)
        for lens in ([60, 33, 5], [56, 20, 3]) for sp in (False, True)] + \
       [("bf16-packed-31-probs-scalar", BF16, [31, 9, 1], True, True, True, True, 0),      # Lm % 4 != 0: the scalar branch of probs_row
        ("bf16-packed-31-stats", BF16, [31, 9, 1], True, False, True, True, 0),
        ("bf16-packed-201-long", BF16, [201, 130, 31], True, False, True, True, 0)]


def _saved_defined(geo, saved_shape):
    """EXCLUSIONS["attention.saved, packed batch"]: the live (row, key) region of the probabilities, the live rows of the statistics."""
    live = geo.live()
    if len(saved_shape) == 4:
        return live[:, None].expand(-1, H, -1, -1)
    return live.any(-1)[:, None, :, None].expand(-1, H, -1, 2).reshape(-1)


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop"])
@pytest.mark.parametrize("case", ATTN, ids=[c[0] for c in ATTN])
def test_attention(HF, Lb, case, p):
    name, dtype, lens, packed, save_probs, give_ctx, backward, ppw = case
    geo = DR.Geometry(lens, max(lens), packed)
    Lm, D, n_seq = geo.Lm, H * 64, geo.S

    def build():
        madd = geo.key_mask()
        if lens[1] > 1:
            madd[1, 0] = DR.MASKED                                   # the first key of sequence 1
        return dict(qkv=rnd(geo.rows, 3 * D, dtype=dtype, seed=1), dctx=rnd(geo.rows, D, dtype=dtype, seed=2), madd=madd.cuda(),
                    off=geo.seq_off().cuda() if packed else None, seed=_seed_word())

    def run(t):
        drop = _drop(Lb, t["seed"], p)
        ctx, saved = HF.k_attn_fwd(t["qkv"], t["madd"], n_seq, Lm, H, drop=drop, seq_off=t["off"])
        out = {"ctx": ctx, "saved": saved}
        if backward:
            out["dqkv"] = HF.k_attn_bwd(t["qkv"], saved, t["dctx"], n_seq, Lm, H, drop=drop, seq_off=t["off"],
                                        ctx=ctx if give_ctx else None, mask_add=t["madd"])
        return out

    stats = dtype == BF16 and not save_probs and bool(Lb.lib().hero_attention_stats_ok(Lb.BF16, Lm))
    defined = {"saved": _saved_defined(geo, (n_seq * H * Lm * 2,) if stats else (n_seq, H, Lm, Lm))} if packed else None
    HF.ATTN_SAVE_PROBS = save_probs
    Lb.check(Lb.lib().hero_attention_force_ppw(ppw))
    try:
        out = uninit.assert_fill_independent(build, run, defined)
    finally:
        HF.ATTN_SAVE_PROBS = False
        Lb.check(Lb.lib().hero_attention_force_ppw(0))
    assert (out["saved"].dim() == 1) == stats
    assert backward or Lm > Lb.lib().hero_attention_max_len(Lb.BF16, 1)


# ==== LayerNorm =====================================================================================================================
LN_SHAPES = [(r, c) for c in (132, 256, 516, 768, 1028, 4352) for r in (9, 70)] + [(4101, 132), (4101, 256)]


def _ln_build(rows, cols, xdt, dt):
    def build():
        x = rnd(rows, cols, dtype=xdt, seed=1) * 2 + 0.5
        g = torch.Generator().manual_seed(6)
        return dict(x=x, g=rnd(cols, seed=2) * 0.1 + 1, b=rnd(cols, seed=3) * 0.1, dy=rnd(rows, cols, dtype=dt, seed=4),
                    t0=rnd(50, cols, seed=4), t1=rnd(7, cols, seed=5),
                    i0=torch.randint(0, 50, (rows,), generator=g).int().cuda(), i1=torch.randint(0, 7, (rows,), generator=g).int().cuda(),
                    seed=_seed_word())
    return build


@pytest.mark.parametrize("dts", LN_DTYPES, ids=LN_IDS)
@pytest.mark.parametrize("rows,cols", LN_SHAPES, ids=["%dx%d" % s for s in LN_SHAPES])
def test_layernorm_forward(HF, Lb, rows, cols, dts):
    """k_ln_fwd: plain, with the output dropout, and with embedding tables, indices and the saved pre-normalisation sum."""
    xdt, ydt = dts

    def run(t):
        out = {}
        for tag, kw in (("plain", {}), ("drop", dict(drop=_drop(Lb, t["seed"], 0.1))),
                        ("tables", dict(tabs=[t["t0"], t["t1"], t["t1"][3:4]], idxs=[t["i0"], t["i1"], None], want_pre=True))):
            if tag == "tables" and xdt != F32:
                continue                                              # the tables are fp32 and are added to an fp32 x
            y, mean, rstd, pre = HF.k_ln_fwd(t["x"], t["g"], t["b"], 1e-12, ydt, rows, cols, **kw)
            out.update({tag + ".y": y, tag + ".mean": mean, tag + ".rstd": rstd})
            if pre is not None:
                out[tag + ".pre"] = pre
        return out

    uninit.assert_fill_independent(_ln_build(rows, cols, xdt, ydt), run)


@pytest.mark.parametrize("dts", LN_DTYPES, ids=LN_IDS)
@pytest.mark.parametrize("rows,cols", LN_SHAPES, ids=["%dx%d" % s for s in LN_SHAPES])
def test_layernorm_backward(HF, Lb, rows, cols, dts):
    """k_ln_bwd: fresh dgamma / dbeta, both dropouts, accumulation (grad_beta = 1) into pre-set dgamma / dbeta, and
    want_params=False with the feeding linear's bias gradient (the library has it up to 1024 columns)."""
    xdt, dt = dts

    def run(t):
        x, g, dy = t["x"], t["g"], t["dy"]
        _, mean, rstd, _ = HF.k_ln_fwd(x, g, t["b"], 1e-12, dt, rows, cols)
        d_out, d_in = _drop(Lb, t["seed"], 0.1), _drop(Lb, t["seed"], 0.1, site=11)
        out = {}
        out["a.dx"], _, out["a.dgamma"], out["a.dbeta"] = HF.k_ln_bwd(x, dy, g, mean, rstd)
        out["b.dx"], out["b.dx_dropped"], out["b.dgamma"], out["b.dbeta"] = HF.k_ln_bwd(x, dy, g, mean, rstd, drop_out=d_out, drop_in=d_in)
        dg, db = torch.ones(cols, device="cuda"), torch.full((cols,), 2.0, device="cuda")
        out["c.dx"], _, _, _ = HF.k_ln_bwd(x, dy, g, mean, rstd, drop_out=d_out, dgamma=dg, dbeta=db, grad_beta=1.0)
        out["c.dgamma"], out["c.dbeta"] = dg, db
        dg, db = torch.ones(cols, device="cuda"), torch.full((cols,), 2.0, device="cuda")
        dbias = torch.full((cols,), 3.0, device="cuda") if cols <= 1024 else None
        out["d.dx"], out["d.dx_dropped"], _, _ = HF.k_ln_bwd(x, dy, g, mean, rstd, drop_out=d_out, drop_in=d_in, dgamma=dg, dbeta=db,
                                                            grad_beta=1.0, want_params=False, dbias_in=dbias)
        out["d.dgamma"], out["d.dbeta"] = dg, db
        if dbias is not None:
            out["d.dbias_in"] = dbias
        out["e.dx"], _, _, _ = HF.k_ln_bwd(x, dy, g, mean, rstd, want_params=False)
        return out

    uninit.assert_fill_independent(_ln_build(rows, cols, xdt, dt), run)


class _LnDeferred(torch.autograd.Function):
    """k_ln_bwd inside a backward pass, where the library defers the fold of its per-block partials to hero_colsum_multi."""

    @staticmethod
    def forward(ctx, x, pack):
        ctx.pack = pack
        return x.clone()

    @staticmethod
    def backward(ctx, dy):
        HF, t, out = ctx.pack
        dx, _, _, _ = HF.k_ln_bwd(t["x"], t["dy"], t["g"], t["mean"], t["rstd"], dgamma=out["dgamma"], dbeta=out["dbeta"],
                                   grad_beta=1.0, want_params=False, dbias_in=out["dbias_in"])
        out["dx"] = dx
        out["queued"] = torch.tensor(len(HF._CQ.jobs))
        return dx.to(dy.dtype), None


@pytest.mark.parametrize("dts", LN_DTYPES, ids=LN_IDS)
@pytest.mark.parametrize("rows,cols", [(9, 132), (70, 768), (4101, 256)])
def test_layernorm_backward_deferred_fold(HF, Lb, rows, cols, dts):
    """The deferred fold: hero_layernorm_bwd(defer_fold) into a torch.empty table of per-block partials, then hero_colsum_multi
    over it at the end of the backward pass."""
    xdt, dt = dts

    def run(t):
        _, t["mean"], t["rstd"], _ = HF.k_ln_fwd(t["x"], t["g"], t["b"], 1e-12, dt, rows, cols)
        out = dict(dgamma=torch.ones(cols, device="cuda"), dbeta=torch.full((cols,), 2.0, device="cuda"),
                   dbias_in=torch.full((cols,), 3.0, device="cuda"))
        leaf = torch.zeros(rows, cols, dtype=dt, device="cuda", requires_grad=True)
        _LnDeferred.apply(leaf, (HF, t, out)).backward(t["dy"])
        assert int(out["queued"]) == 3 and not HF._CQ.jobs           # three folds were deferred, and flushed with the pass
        return out

    uninit.assert_fill_independent(_ln_build(rows, cols, xdt, dt), run)


# ==== column sums ===================================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [0, 3, 300])
def test_column_sums(HF, Lb, dtype, rows):
    """k_colsum and hero_colsum_multi: no rows (hero_colsum only: the multi-sum refuses a problem without rows), fewer rows than a
    workgroup has row lanes, several row blocks; a column offset into a wider source; overwrite and accumulate."""
    def build():
        return dict(src=rnd(max(rows, 1), 776, dtype=dtype, seed=1), part=rnd(max(rows, 1), 3 * 16, seed=2))     # (0 rows: a real address)

    def colsum(src, o, beta, col0, n):
        if rows:
            return HF.k_colsum(src, out=o, beta=beta, col0=col0, ncols=n)
        ws = HF._workspace(256 * n, src.device)                       # k_colsum's own launch, told that the source has no rows
        Lb.check(Lb.lib().hero_colsum(src.data_ptr() + col0 * src.element_size(), o.data_ptr(), 0, n, src.shape[1], Lb.dt(src), beta,
                                      ws.data_ptr(), Lb.stream()))
        return o

    def run(t):
        src, out = t["src"], {}
        for beta in (0.0, 1.0):
            out["colsum.beta%d" % beta] = colsum(src, torch.full((768,), 0.5, device="cuda"), beta, 8, 768)
        out["colsum.fresh"] = colsum(src, torch.empty((776,), dtype=F32, device="cuda"), 0.0, 0, 776)
        specs = [(src, 8, 768, 1.0), (src, 0, 776, 0.0), (t["part"], 16, 16, 1.0)]
        outs = [torch.full((n,), 0.5, device="cuda") for _, _, n, _ in specs]
        probs = (Lb.Colsum * len(specs))(*[Lb.Colsum(s.data_ptr() + c0 * s.element_size(), o.data_ptr(), rows, n, s.shape[1], Lb.dt(s), beta)
                                           for (s, c0, n, beta), o in zip(specs, outs)])
        ws = torch.empty(Lb.lib().hero_colsum_multi_workspace_bytes(probs, len(specs)) // 4 + 1, device="cuda")
        rc = Lb.lib().hero_colsum_multi(probs, len(specs), ws.data_ptr(), Lb.stream())
        if not rows:
            assert rc != 0                                            # hero_colsum_multi takes no problem without rows: refused, nothing launched
            return out
        Lb.check(rc)
        out.update({"multi.%d" % i: o for i, o in enumerate(outs)})
        return out

    uninit.assert_fill_independent(build, run)


# ==== GEMM family ===================================================================================================================
@pytest.mark.parametrize("case", GC.CASES, ids=lambda c: c["name"])
def test_gemm_case(Lb, case):
    """Every case of tests/gemm_cases.CASES through test_gpu_gemm_exact.run_case, inside both fills.  The fill has NO effect on
    these launches: that path allocates nothing with torch.empty - C, aux, slabs and column-sum tables are torch.full buffers
    of a NaN pattern of its own - and hero_gemm uses no cached workspace.  What the cases show is what run_case shows by
    itself (a NaN left in an output buffer does not survive, nothing is written outside [M, N]); they are here because this
    call path is the one asked for.  The GEMM outputs that the LIBRARY allocates uninitialised are compared under the fills
    by the functional-level tests below (k_linear, k_dgrad, k_dgrad_t, k_wgrad with and without a split, the slab path)."""
    from tests.test_gpu_gemm_exact import run_case
    for fill in uninit.FILLS:
        with uninit.filled(fill):
            run_case(Lb, case)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(1, 8, 8), (200, 136, 96), (131, 768, 768)])
def test_linear_epilogues_and_dgrad(HF, Lb, dtype, M, N, K):
    """k_linear with the GELU / ReLU aux and residual epilogues and dropout, k_dgrad with the gelu' epilogue, k_wgrad (one
    split: no atomics at these row counts) with beta 0 and 1, and k_wgrad(dbias=...) outside a backward pass - there the bias
    gradient is a hero_colsum of its own, NOT the ride on hero_wgrad_batch (that one runs under the fills in the step tests
    and in test_wgrad_batch_ignores_what_lies_behind_a_column_slice)."""
    def build():
        return dict(x=rnd(M, K, dtype=dtype, seed=1), w=rnd(N, K, dtype=dtype, seed=2, scale=0.05), b=rnd(N, seed=3),
                    res=rnd(M, N, dtype=dtype, seed=4), dy=rnd(M, N, dtype=dtype, seed=5), u=rnd(M, K, dtype=dtype, seed=6),
                    r=rnd(M, K, dtype=dtype, seed=7), seed=_seed_word())

    def run(t):
        x, w, b, dy = t["x"], t["w"], t["b"], t["dy"]
        out = {"y": HF.k_linear(x, w, b)}
        out["gelu.aux"] = torch.empty_like(out["y"])
        out["gelu.y"] = HF.k_linear(x, w, b, act=Lb.ACT_GELU, aux=out["gelu.aux"])
        out["relu.aux"] = torch.empty_like(out["y"])
        out["relu.y"] = HF.k_linear(x, w, b, act=Lb.ACT_RELU, aux=out["relu.aux"], residual=t["res"])
        out["drop.y"] = HF.k_linear(x, w, b, residual=t["res"], drop=_drop(Lb, t["seed"], 0.1))
        out["dx"] = HF.k_dgrad(dy, w)
        out["dx.gelu"] = HF.k_dgrad(dy, w, act=Lb.ACT_GELU_BWD, aux=t["u"], residual=t["r"])
        out["dw"] = HF.k_wgrad(dy, x)
        acc = torch.full((N, K), 0.5, device="cuda")
        out["dw.beta1"] = HF.k_wgrad(dy, x, out=acc, beta=1.0)
        db = torch.full((N,), 0.25, device="cuda")
        out["dw.with_dbias"] = HF.k_wgrad(dy, x, out=torch.full((N, K), 0.5, device="cuda"), beta=1.0, dbias=db)
        out["dbias.colsum"] = db
        return out

    assert HF._split_for(N, K, M, 64 if dtype == BF16 else 32) == 1      # (a split merges with fp32 atomics: other bits run to run)
    uninit.assert_fill_independent(build, run)


@pytest.mark.parametrize("M,N,K", [(300, 136, 64), (1000, 768, 3072)])
def test_dgrad_t_per_tile_column_sums(HF, Lb, M, N, K):
    """k_dgrad_t with the multiply-by-aux epilogue and the [ceil(M / 64), N] table of per-tile column sums in a torch.empty
    buffer: the kernel writes every row of it (zeros in the rows of a tile's other 64-row blocks)."""
    def build():
        return dict(dy=rnd(M, K, dtype=BF16, seed=5), wt=rnd(N, K, dtype=BF16, seed=6, scale=0.05), aux=rnd(M, N, dtype=BF16, seed=7))

    def run(t):
        part = torch.empty((-(-M // 64), N), dtype=F32, device="cuda")
        du = HF.k_dgrad_t(t["dy"], t["wt"], act=Lb.ACT_MUL_AUX, aux=t["aux"], colsum=part, colsum_partial=True)
        return {"du": du, "partials": part, "dbias": HF.k_colsum(part)}

    uninit.assert_fill_independent(build, run)


def test_split_slabs_and_fold(HF, Lb):
    """The split-slab path of test_gemm_split_slabs_and_fold with the slabs in a torch.empty buffer, and the long-reduction
    dgrad that the library builds on it (its smallest shape)."""
    M, N, K = 256, 512, 64 * 37

    def build():
        return dict(a=rnd(M, K, dtype=BF16, seed=1), b=rnd(N, K, dtype=BF16, seed=2, scale=0.05),
                    dy=rnd(360, 8200, dtype=BF16, seed=1, scale=0.05), wt=rnd(768, 8200, dtype=BF16, seed=2, scale=0.05))

    def run(t):
        n = Lb.lib().hero_gemm_splits(K, 8, Lb.BF16)
        slabs = torch.empty((n, M, N), dtype=F32, device="cuda")
        HF.k_gemm(t["a"], t["b"], slabs, M, N, K, K, K, N, Lb.LAYOUT_K, Lb.LAYOUT_K, Lb.BF16, out_f32=True, split_k=8, split_stride=M * N)
        out = {"slabs": slabs}
        for dt_ in (F32, BF16):
            o = torch.empty((M, N), dtype=dt_, device="cuda")
            Lb.check(Lb.lib().hero_fold_slabs(Lb.ptr(slabs), n, M * N, Lb.ptr(o), M * N, Lb.dt(o), Lb.stream()))
            out["fold.%s" % dt_] = o
        out["dgrad_long"] = HF.k_dgrad_t(t["dy"], t["wt"])
        return out

    uninit.assert_fill_independent(build, run)


@pytest.mark.parametrize("which", ["group-1032", "group-520", "batch-tail_only", "batch-whole_round"])
def test_wgrad_group_and_batch(Lb, which):
    """hero_wgrad_group at K = 1032 (stream-K) and 520 (fallback), hero_wgrad_batch at the two shapes of test_wgrad_batch,
    through test_gpu_gemm_exact's own problems (integer operands: the float64 product's bits are demanded).  As in
    test_gemm_case the fill has no effect here: dW, dbias and the operands are torch.full / torch.randint buffers."""
    from tests import test_gpu_gemm_exact as GE
    import numpy as np
    lib = Lb.lib()
    for fill in uninit.FILLS:
        with uninit.filled(fill):
            if which.startswith("group"):
                K = int(which.split("-")[1])
                probs, keep, checks = GE._wgrad_setup(Lb, K, GE.BERT_LAYER_MINUS_FFN2, seed=7)
                for times in (1, 2):
                    Lb.check(lib.hero_wgrad_group(probs, len(GE.BERT_LAYER_MINUS_FFN2), K, Lb.BF16, Lb.stream()))
                    torch.cuda.synchronize()
                    GE._wgrad_check(checks, times, "%s, fill %r, launch %d" % (which, fill, times))
            else:
                K, shapes = (520, [(768, 768)]) if which == "batch-tail_only" else (456, [(3072, 768)] * 4)
                probs, keep, checks = GE._wgrad_setup(Lb, K, shapes, seed=11, dbias_from=1)
                buf = np.zeros(8 + 8 * 256 * 16, dtype=np.int32)
                words = lib.hero_wgrad_batch_plan(probs, len(shapes), K, buf.ctypes.data, buf.size)
                assert words > 8
                plan = torch.from_numpy(buf[:words].copy()).cuda()
                for times in (1, 2):
                    Lb.check(lib.hero_wgrad_batch(probs, len(shapes), K, Lb.BF16, plan.data_ptr(), words, Lb.stream()))
                    torch.cuda.synchronize()
                    GE._wgrad_check(checks, times, "%s, fill %r, launch %d" % (which, fill, times))


# ==== row kernels ===================================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_gather_rows(HF, dtype):
    """k_gather_rows from the a and the b source with -1 (zero) rows, plain and with spare rows behind the result."""
    def build():
        idx = torch.randint(-31, 50, (200,), generator=torch.Generator().manual_seed(3)).int()
        idx[idx == -1] = 5
        idx[::17] = -1
        return dict(a=rnd(50, 128, dtype=dtype, seed=1), b=rnd(30, 128, dtype=dtype, seed=2), idx=idx.cuda())

    def run(t):
        tail = HF.k_gather_rows(t["a"], t["b"], t["idx"], 200, 128, tail_rows=7)
        assert tail.shape == (200, 128)                              # EXCLUSIONS: the 7 spare rows are not part of the result
        return {"out": HF.k_gather_rows(t["a"], t["b"], t["idx"], 200, 128), "out.tail": tail}

    uninit.assert_fill_independent(build, run)


def test_csr_gather_sum_and_expand_rows(HF):
    """CsrGatherSumFn forward / backward on the frame map of test_csr_gather_and_elementwise; ExpandRowsFn forward / backward on
    an index that names rows several times and leaves one out."""
    from hero_amd.model.model import build_frame_map

    def build():
        return dict(src=rnd(3 * 5, 64, seed=1).requires_grad_(True), x=rnd(6, 3, 64, dtype=BF16, seed=2).requires_grad_(True),
                    idx=torch.tensor([0, 0, 2, 5, 2, 2, 1, 5, 0], device="cuda"), dy=rnd(9, 3, 64, dtype=BF16, seed=3))

    def run(t):
        offs, ent, inv = build_frame_map([2, 1], [[(0, [0, 1]), (1, [3])], [(0, [2, 0])]], 2, 4, 5, torch.device("cuda"))
        out = HF.CsrGatherSumFn.apply(t["src"], offs, ent, inv, 8)
        out.backward(torch.ones_like(out) * 2)
        y = HF.ExpandRowsFn.apply(t["x"], t["idx"])
        y.backward(t["dy"])
        return {"csr.out": out, "csr.dsrc": t["src"].grad, "expand.out": y, "expand.dx": t["x"].grad}

    uninit.assert_fill_independent(build, run)


@pytest.mark.parametrize("rows,n_dst,cols,dtype", [(257, 2, 4352, F32), (1300, 37, 768, F32), (1300, 37, 768, BF16)])
def test_scatter_add_sorted(HF, rows, n_dst, cols, dtype):
    """hero_segment_sort (order and sort workspace are torch.empty int32: zero under both fills) + hero_scatter_add_sorted with
    its cached fp32 workspace (functional._WS, filled by the harness)."""
    def build():
        idx = torch.randint(0, n_dst, (rows,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3), dtype=torch.int32)
        idx[::7] = 5 % n_dst
        idx[1::11] = 1 % n_dst
        idx[2::13] = -1
        return dict(idx=idx, src=rnd(rows, cols, dtype=dtype, seed=4))

    def run(t):
        dst = torch.full((n_dst, cols), 0.5, device="cuda")
        HF.k_scatter_add_sorted(t["src"], t["idx"], dst, 1 % n_dst)
        return {"dst": dst, "order": HF.segment_order(t["idx"], n_dst, 1 % n_dst)}

    uninit.assert_fill_independent(build, run)


def test_cast_and_weight_copies(HF):
    """k_cast both ways; packed / packed_t compute copies, then refresh_weight_cache (hero_copy_multi) after the masters moved -
    the shapes of test_one_launch_weight_refresh_equals_per_tensor_casts."""
    def build():
        g = torch.Generator().manual_seed(0)
        return dict(x=rnd(1001, seed=2), ws=[torch.nn.Parameter(torch.randn(n, 96, generator=g).cuda()) for n in (64, 130, 40)],
                    bs=[torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in (64, 130, 40)])

    def run(t):
        lo = HF.k_cast(t["x"], BF16)
        out = {"cast.bf16": lo, "cast.f32": HF.k_cast(lo, F32)}
        W, Wt, B = HF.packed(t["ws"], BF16), HF.packed_t(t["ws"], BF16), HF.packed(t["bs"], F32)
        out.update({"packed": W.clone(), "packed_t": Wt.clone(), "packed.bias": B.clone()})
        with torch.no_grad():
            for prm in t["ws"] + t["bs"]:
                prm.mul_(1.5).add_(0.25)
        HF.notify_weights_updated()
        HF.refresh_weight_cache()
        assert HF.packed(t["ws"], BF16) is W and HF.packed_t(t["ws"], BF16) is Wt
        out.update({"refreshed": W, "refreshed_t": Wt, "refreshed.bias": HF.packed(t["bs"], F32)})
        return out

    try:
        uninit.assert_fill_independent(build, run)
    finally:
        HF.clear_weight_cache()


# ==== loss ==========================================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols,ld", [(5, 100, 100), (64, 1931, 1936)])
def test_cross_entropy(HF, dtype, rows, cols, ld):
    """CrossEntropyFn forward and backward; ld > cols: the gradient's pad columns are part of the result (zeros)."""
    def build():
        y = torch.randint(0, cols, (rows,), generator=torch.Generator().manual_seed(2)).cuda()
        y[0] = -1
        return dict(x=rnd(rows, ld, dtype=dtype, seed=1, scale=3.0).requires_grad_(True), y=y, w=rnd(rows, seed=3).abs() + 0.5)

    def run(t):
        loss = HF.cross_entropy(t["x"], t["y"], ncols=cols, ignore_index=-1, inv_temp=1.0 / 0.7)
        (loss * t["w"]).sum().backward()
        return {"loss": loss, "dlogits": t["x"].grad}

    uninit.assert_fill_independent(build, run)


# ==== heads =========================================================================================================================
# One call of each wrapper, at the smallest parametrisation (with a mask) of the wrapper's own test_gpu_*_kernels.py, through
# that file's own input builders.
def test_head_wrappers():
    """head.py: QueryPoolFn, RowNormFn, VideoRankLossFn, StEdLossFn (its zero-between-calls workspace is left alone)."""
    from hero_amd.head import QueryPoolFn, RowNormFn, StEdLossFn, VideoRankLossFn
    from tests import test_gpu_head_kernels as T

    def build():
        B, Lq, D = 3, 7, 260
        mask = torch.ones(B, Lq)
        mask[0, Lq - 2:] = 0
        mask[1, :] = 0
        mask[2, 1:] = 0
        qn, cn, vmask = T._video_rank_inputs(7, 13, 2, 128, 0)
        sted = [t.cuda() for t in T._sted_inputs(6, 3, 128, 15, BF16)]
        for i in (0, 1, 3, 4):
            sted[i].requires_grad_(True)
        return dict(q=T.gen(B, Lq, D, seed=1, dtype=BF16).cuda().requires_grad_(True), w=T.gen(1, D, seed=2, scale=0.2).cuda().requires_grad_(True),
                    g=T.gen(B, D, seed=3).cuda(), mask=mask.cuda(), x=T.gen(6, 260, seed=1).cuda().requires_grad_(True), gx=T.gen(6, 260, seed=2).cuda(),
                    qn=qn.cuda().requires_grad_(True), cn=cn.cuda().requires_grad_(True), vmask=vmask.cuda(), sted=sted)

    def run(t):
        out = {}
        out["pool"] = QueryPoolFn.apply(t["q"], t["mask"], t["w"])
        out["pool"].backward(t["g"])
        out["pool.dq"], out["pool.dw"] = t["q"].grad, t["w"].grad
        out["norm"] = RowNormFn.apply(t["x"], 1e-5)
        out["norm"].backward(t["gx"])
        out["norm.dx"] = t["x"].grad
        lc, lq = VideoRankLossFn.apply(t["qn"], t["cn"], t["vmask"], (0, 7), 0.1, True, True, 3, 10.0, 8.0, 8.0)
        (1.7 * lc - 0.6 * lq).backward()
        out.update({"rank.l_ctx": lc, "rank.l_q": lq, "rank.dqn": t["qn"].grad, "rank.dcn": t["cn"].grad})
        s = t["sted"]
        loss = StEdLossFn.apply(s[0], s[1], s[2], s[3], s[4], s[5], 0.7)
        (2.5 * loss).backward()
        out.update({"sted.loss": loss, "sted.dq2": s[0].grad, "sted.dctx": s[1].grad, "sted.dw_st": s[3].grad, "sted.dw_ed": s[4].grad})
        return out

    uninit.assert_fill_independent(build, run)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_violin_and_qa_wrappers(dtype):
    """violin.py: FramePoolFn, BceHeadFn; qa.py: QaPoolFn."""
    from tests import test_gpu_qa_pool_kernels as TQ
    from tests import test_gpu_violin_kernels as TV

    def build():
        return dict(pool=TV.pool_data("short_L", dtype), full=TV.pool_data("fully_masked", dtype), head=TV.head_data("S5_K256", dtype),
                    qa=TQ.case_data("odd_A_short_L", dtype))

    def run(t):
        out = {}
        for tag in ("pool", "full"):
            out[tag + ".pooled"], out[tag + ".dseq"], out[tag + ".dw"] = TV.run_pool(t[tag])
        out["head.loss"], out["head.logits"], out["head.dh"], out["head.dw"], out["head.db"] = TV.run_head(t["head"])
        out["qa.qa"], out["qa.se"], out["qa.dseq"], out["qa.dwq"], out["qa.dws"] = TQ.run_kernels(t["qa"])
        return out

    uninit.assert_fill_independent(build, run)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_tvc_wrappers(Lb, dtype):
    """tvc.py: DecAttnCoreFn in both operand forms (causal, below one tile) and with ragged key masks and dropout; smooth_ce
    and smooth_ce_mean with padding columns."""
    from hero_amd.tvc import smooth_ce, smooth_ce_mean
    from tests import test_gpu_tvc_kernels as TT

    def build():
        c = TT.loss_data("C1000_ld1024", dtype, 0.1)
        return dict(causal=TT.attn_data("below_tile", dtype), ragged=TT.attn_data("ragged_small", dtype), seed=_seed_word(),
                    x=c["x"].clone().requires_grad_(True), x2=c["x"].clone().requires_grad_(True), labels=c["labels"], w=c["w"])

    def run(t):
        out = {}
        for tag, form, p in (("causal", "fused", 0.0), ("causal", "separate", 0.1), ("ragged", "separate", 0.0), ("ragged", "separate", 0.1)):
            res = TT.run_attention(t[tag], form, drop=_drop(Lb, t["seed"], p))
            out.update({"%s.%s.%g.%s" % (tag, form, p, n): v for n, v in zip(("ctx", "dq", "dk", "dv"), res)})
        rows, pair = smooth_ce(t["x"], t["labels"], 0.1, ncols=1000)
        (rows * t["w"]).sum().backward()
        mean = smooth_ce_mean(t["x2"], t["labels"], 0.1, ncols=1000)
        (mean * 0.5).backward()
        out.update({"smooth.rows": rows, "smooth.pair": pair, "smooth.dlogits": t["x"].grad, "smooth.mean": mean, "smooth.mean.dlogits": t["x2"].grad})
        return out

    uninit.assert_fill_independent(build, run)


def test_caption_retrieval_and_eval_wrappers():
    """caption.py: k_caption_score on the golden captions; retrieval.py: k_topk_rows (k > n: the (0, -1) slots), k_st_ed_probs,
    k_moment_topk; pretrain_eval.py: ce_eval with predictions, feat_eval."""
    from hero_amd import pretrain_eval as E
    from hero_amd import retrieval as HR
    from hero_amd.caption import k_caption_score
    from tests import pretrain_eval_reference as PR
    from tests import test_gpu_caption_kernels as TC
    from tests import test_gpu_pretrain_eval_kernels as TE
    from tests import test_gpu_retrieval_kernels as TR

    def build():
        g = torch.Generator().manual_seed(22)
        nq, nv, ln, k, taps = TR.PROBS[0]
        ld = (nv * ln + 3) // 4 * 4 + 4
        lens = torch.randint(1, ln + 1, (nv,), generator=g)
        lens[0] = 1
        sel = torch.randint(0, nv, (nq, k), generator=g).to(torch.int32)
        sel[-1, -1] = -1
        st, ed, w = TR.soft_probs(3, 4, 12, seed=15)
        logits, labels = TE._device_case(PR.CE_SHAPES[0], BF16)
        p, tg, _, _ = TE._feat(PR.FEAT_ROWS[-1], PR.FEAT_COLS[0])
        return dict(refs=TC.fixture_case(), ids=TC.id_rows(TC.HYPS, TC.TCAP + 5), clip=torch.arange(TC.C, dtype=torch.int32).cuda(),
                    s=torch.randn(4, 52, generator=g).cuda(), sim=(torch.randn(nq, ld, generator=g) * 2).cuda(),
                    mask=(torch.arange(ln).view(1, ln) < lens.view(nv, 1)).float().cuda(), sel=sel.cuda(),
                    w_st=(torch.randn(taps, generator=g) * 0.5).cuda(), w_ed=(torch.randn(taps, generator=g) * 0.5).cuda(), ln=ln,
                    st=st.cuda(), ed=ed.cuda(), w=w.cuda(), logits=logits, labels=labels, ncols=PR.CE_SHAPES[0][1],
                    p=torch.from_numpy(p.copy()).cuda().to(BF16), tg=torch.from_numpy(tg.copy()).cuda().to(BF16))

    def run(t):
        out = {}
        out["cap.stats"], out["cap.rouge"], out["cap.cider"], out["cap.lcs"] = k_caption_score(t["ids"], t["clip"], t["refs"], TC.EOS, tcap=TC.TCAP, want_lcs=True)
        out["topk.val"], out["topk.idx"] = HR.k_topk_rows(t["s"], 128, n=50)
        out["topk_exp.val"], out["topk_exp.idx"] = HR.k_topk_rows(t["s"], 16, alpha=20.0, n=50)
        out["probs.st"], out["probs.ed"] = HR.k_st_ed_probs(t["sim"], t["mask"], t["sel"], t["w_st"], t["w_ed"], t["ln"])
        out["moment.score"], out["moment.flat"] = HR.k_moment_topk(t["st"], t["ed"], t["w"], 1, 4, 12)
        out["ce.acc"], out["ce.pred"] = E.ce_eval(t["logits"], t["labels"], ncols=t["ncols"], ignore_index=PR.CE_IGNORE, inv_temp=0.7, want_pred=True)
        out["feat.acc"] = E.feat_eval(t["p"], t["tg"])
        return out

    uninit.assert_fill_independent(build, run)


# ==== memory behind an operand ======================================================================================================
def test_wgrad_batch_ignores_what_lies_behind_a_column_slice(Lb):
    """hero_wgrad_batch on column slices dY[:, col0:col0 + 128] of one matrix, 128 < the 192-column tile, with NaN in the rows
    BEHIND dY and x (where the allocator's leftovers are in a training step): the tile of the slice at col0 = 256 reaches, in
    the last row of the reduction, col0 elements past the end of dY.  Those columns belong to no output, but the bias-gradient
    ride adds them - times 0 - to the sums of the wave's other column blocks.  Found by test_gpu_uninit_steps.py on the video-QA
    batch (value.bias gradient NaN in one element); this is the same read with the memory behind dY under the test's control.
    Integer operands: dW and dbias must be the exact sums, twice (the second launch accumulates)."""
    import numpy as np
    from tests import test_gpu_gemm_exact as GE
    lib, K, n, m = Lb.lib(), 520, 3, 128
    dy = GE.sentinel(K + 2, n * m + 8, BF16)
    dy[:K] = GE.PAD_IN
    dy[:K, :n * m] = GE._ints((K, n * m), 21).to(BF16)
    probs, keep, checks = (Lb.WgradProblem * n)(), [], []
    for i in range(n):
        x = GE.sentinel(K + 2, m + 8, BF16)
        x[:K] = GE.PAD_IN
        x[:K, :m] = GE._ints((K, m), 22 + i).to(BF16)
        dw, db = torch.full((m, m), 0.25, device="cuda"), torch.full((m,), 0.5, device="cuda")
        probs[i] = Lb.WgradProblem(dy[:, i * m:].data_ptr(), x.data_ptr(), dw.data_ptr(), m, m, dy.shape[1], x.shape[1], m, 4, db.data_ptr())
        sl = dy[:K, i * m:(i + 1) * m].double()
        keep.append(x)
        checks.append((dw, db, sl.t() @ x[:K, :m].double(), sl.sum(0)))
    buf = np.zeros(8 + 8 * 256 * 16, dtype=np.int32)
    words = lib.hero_wgrad_batch_plan(probs, n, K, buf.ctypes.data, buf.size)
    assert words > 8, (words, lib.hero_last_error())
    plan = torch.from_numpy(buf[:words].copy()).cuda()
    for times in (1, 2):
        Lb.check(lib.hero_wgrad_batch(probs, n, K, Lb.BF16, plan.data_ptr(), words, Lb.stream()))
        torch.cuda.synchronize()
        for i, (dw, db, prod, colsum) in enumerate(checks):
            assert bool(torch.isfinite(db).all()), "dbias of slice %d: %d of %d elements not finite, first at %d" % (
                i, int((~torch.isfinite(db)).sum()), m, int((~torch.isfinite(db)).nonzero()[0]))
            assert torch.equal(dw.double(), 0.25 + times * prod), "dw of slice %d, launch %d" % (i, times)
            assert torch.equal(db.double(), 0.5 + times * colsum), "dbias of slice %d, launch %d" % (i, times)


# ==== split-K weight gradient =======================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_wgrad_with_a_split_reduction(HF, dtype):
    """k_wgrad where functional._split_for cuts the reduction: the output comes from torch.empty, a pre-scale launch stores
    beta * dW (beta = 0: a store, not a product with what was there) and the splits add their partial sums with fp32 atomics.
    Integer operands: the sums are exact in any order, so the bits are reproducible and equal the float64 product."""
    M, N, K = 2048, 128, 128

    def build():
        g = torch.Generator().manual_seed(31)
        return dict(dy=torch.randint(-3, 4, (M, N), generator=g).to(dtype).cuda(), x=torch.randint(-3, 4, (M, K), generator=g).to(dtype).cuda())

    def run(t):
        acc = torch.full((N, K), 0.25, device="cuda")
        return {"dw": HF.k_wgrad(t["dy"], t["x"]), "dw.beta1": HF.k_wgrad(t["dy"], t["x"], out=acc, beta=1.0)}

    assert HF._split_for(N, K, M, 64 if dtype == BF16 else 32) > 1
    out = uninit.assert_fill_independent(build, run)
    t = build()
    want = t["dy"].double().t() @ t["x"].double()
    assert torch.equal(out["dw"].double(), want) and torch.equal(out["dw.beta1"].double(), 0.25 + want)


# ==== decoding and post-processing wrappers =========================================================================================
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_tvc_decode_wrappers(HF, Lb, dtype):
    """tvc.py: k_dec_attn_row (ragged key masks), k_dec_attn_step on a key/value cache from torch.empty - the rows behind the
    step's position hold the fill, the step must not see them - and DecAttentionFn in its self and cross forms."""
    from hero_amd.tvc import DecAttentionFn, k_dec_attn_step
    from tests import test_gpu_tvc_decode_kernels as TD
    N, Lq, Lk, D = 2, 5, 9, 128

    def build():
        g = torch.Generator().manual_seed(41)
        prm = lambda *shape: torch.nn.Parameter((torch.randn(*shape, generator=g) * 0.1).cuda())      # noqa: E731
        mask = torch.zeros(N, Lk)
        mask[1, 3:] = -10000.0
        return dict(step=TD.step_data("below_wave", dtype), cross=TD.cross_data("ragged_small", dtype), seed=_seed_word(),
                    x=torch.randn(N, Lq, D, generator=g).to(dtype).cuda().requires_grad_(True),
                    enc=torch.randn(N, Lk, D, generator=g).to(dtype).cuda().requires_grad_(True),
                    dy=torch.randn(N, Lq, D, generator=g).to(dtype).cuda(), mask=mask.cuda(),
                    w=[prm(D, D) if i % 2 == 0 else prm(D) for i in range(6)], w2=[prm(D, D) if i % 2 == 0 else prm(D) for i in range(6)])

    def run(t):
        out = {"row.ctx": TD.run_cross(t["cross"])}
        c = t["step"]
        n, h, pos, tcap = c["dims"]
        cache = torch.empty((n, tcap, 2 * h * 64), dtype=dtype, device="cuda")
        cache[:, :pos] = c["hist"]
        out["step.ctx"] = k_dec_attn_step(c["qkv"], cache, pos, n, h)
        out["step.cache"] = cache[:, :pos + 1]                       # the rows behind the position belong to later steps
        for tag, enc, mask, w, p in (("self", None, None, t["w"], 0.0), ("cross", t["enc"], t["mask"], t["w2"], 0.1)):
            y = DecAttentionFn.apply(t["x"], enc, mask, H, _drop(Lb, t["seed"], p), *w)
            y.backward(t["dy"])
            out[tag + ".ctx"] = y
            out.update({"%s.dparam%d" % (tag, i): prm.grad for i, prm in enumerate(w)})
        out["dx"], out["denc"] = t["x"].grad, t["enc"].grad
        return out

    HF.set_grad_sink(None)
    try:
        uninit.assert_fill_independent(build, run)
    finally:
        HF.clear_weight_cache()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_beam_and_sample_select(dtype):
    """tvc.py: k_beam_select and k_sample_select, two steps each, on the tables as the decoder makes them - a BeamTables built
    INSIDE the fill (cum, fin, len, ids, anc and the workspace come from torch.empty) and reset as a decode resets it."""
    from hero_amd import tvc as T
    from hero_amd.model.tvc import BeamTables
    from tests import test_gpu_tvc_sample_kernels as TS
    from tests import tvc_beam_reference as RB
    from tests import tvc_sample_reference as RS
    N, B, V = 5, 3, 160
    params = RS.SELECT_PARAMS[1]

    def build():
        return dict(beam=RB.select_case(N, B, V, dtype, False)["logits"].cuda(), sample=RS.select_case(N, B, V, dtype, False, params)["logits"].cuda(),
                    seed=TS.seed_word(RS.SELECT_SEED))

    def run(t):
        out = {}
        tb = BeamTables(N, B, RB.SELECT_TCAP, "cuda", True).reset()
        last = torch.empty((N * B,), dtype=torch.int32, device="cuda")
        for step in (0, 1):
            T.k_beam_select(t["beam"][:, :V], tb.cum, tb.fin, tb.len, tb.ids, tb.anc, last, tb.ws, step, N, B, V, RB.SELECT_EOS)
            out.update({"beam%d.%s" % (step, k): getattr(tb, k).clone() for k in ("cum", "fin", "len", "ids", "anc")})
            out["beam%d.last" % step] = last.clone()
        ts = BeamTables(N, B, RS.SELECT_TCAP, "cuda", True).reset_sampling()
        for step in (0, 1):
            T.k_sample_select(t["sample"][:, :V], ts.cum, ts.fin, ts.len, ts.ids, last, ts.kept, t["seed"], step, N, B, V, RS.SELECT_EOS, *params)
            out.update({"sample%d.%s" % (step, k): getattr(ts, k).clone() for k in ("cum", "fin", "len", "ids", "kept")})
            out["sample%d.last" % step] = last.clone()
        return out

    uninit.assert_fill_independent(build, run)


def test_moment_nms_and_first_hit():
    """retrieval.py: k_moment_nms and k_first_hit at the first size past one wave of test_gpu_postproc_kernels.py's grids (65
    candidates, vacant rows and tails included); all integer outputs - zero under both fills - so this holds the calls in the
    sweep and shows that every slot of keep / count / first is written."""
    import numpy as np
    from hero_amd import retrieval as HR
    from tests import test_gpu_postproc_kernels as TP
    p, n_pred = 65, 40

    def build():
        rng = np.random.default_rng(1000 + p)
        video, st, ed = TP.rows(rng, p)
        g0 = rng.integers(0, 80, size=7) * 1.5
        gt_ts = np.stack([g0, g0 + rng.integers(1, 12, size=7) * 1.5], axis=1).astype(np.float32)
        return dict(video=TP.dev(video), st=TP.dev(st), ed=TP.dev(ed), gt_video=TP.dev(np.array([0, 1, 2, 3, 5, 0, 1], dtype=np.int32)),
                    gt_ts=TP.dev(gt_ts), thds=torch.tensor([0.5, 0.7], device="cuda"), np=(video, st, ed))

    def run(t):
        keep, count = HR.k_moment_nms(t["video"], t["st"], t["ed"], 0.5, 100, n_pred)
        first = HR.k_first_hit(t["video"], t["gt_video"], t["st"], t["ed"], t["gt_ts"], 1.5, t["thds"], n_pred)
        return {"nms.keep": keep, "nms.count": count, "first": first, "first.vr": HR.k_first_hit(t["video"], t["gt_video"], n_pred=n_pred)}

    out = uninit.assert_fill_independent(build, run)
    want_keep, want_count = HR.nms_rows_host(*build()["np"], 0.5, 100, n_pred)
    assert np.array_equal(out["nms.keep"].cpu().numpy(), want_keep) and np.array_equal(out["nms.count"].cpu().numpy(), want_count)
