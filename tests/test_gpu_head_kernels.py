"""The loss-head kernels of hero_amd/csrc/head.hip (hero_query_pool_*, hero_rownorm_*, hero_score_max_*, hero_rank_loss,
hero_st_ed_*, hero_sums_scaled) at the benchmark's shapes, at the second trips and tails of their loops, and on exact ties.

A. Exact tests: integer / bit comparisons, no tolerance (first-maximum rule, exactly representable inputs through the real
   GEMM, bit reproducibility and workspace hygiene of hero_st_ed_bwd, `own` slices).
B. Parity, element-wise (tests.util.elem_rel_err), with the float64 references of tests/head_reference.py.  Inputs are drawn
   once in the kernel's input dtype and the same rounded values go to the reference.

Tolerances of B (none is taken from a kernel's output)
-----------------------------------------------------
fp32 outputs: the error of the fp32 PyTorch formulation of the same op (tests/test_gpu_head.py / model/pretrain.py, fp32, same
inputs, on the GPU) against the float64 reference, measured per op over the cases of this file's grid (the worst case is listed;
it is the largest shape unless noted), times 4 (another summation order, the __expf / __logf intrinsics), floored at
16 * 2^-24 = 9.54e-7.  Loss scalars: the same constant, relative to max(1, |ref|).  bf16-stored outputs (dq, dx, dctx with bf16
inputs): per element |a - b| <= 2^-8 |b| + TOL * rms(b) (bf16 rounding is 2^-9; the factor 2 covers an fp32 accumulation error
that moves a value across a rounding boundary).  Every test prints the kernel's and PyTorch-fp32's error per output (-s).

Measured on an AMD Instinct MI355X (gfx950), ROCm PyTorch, this file's inputs:

    op            worst PyTorch-fp32 elem_rel_err (case)                     x 4        TOL
    query_pool    1.878e-04  (dq,   fp32 B=5 L=70 D=1536)                          7.51e-04   7.51e-04
    rownorm       1.306e-07  (dx,   fp32 1920 x 768)                               5.22e-07   9.54e-07 (floor)
    video_rank    3.771e-07  (dqn,  N=32 L=100 D=768 lse, 3 hard negatives)        1.51e-06   1.51e-06
    rank_loss     5.606e-07  (ds_q, nv=260 hinge, 20 hard negatives)               2.24e-06   2.24e-06
    st_ed         6.511e-06  (dctx, fp32 B=160 L=60 D=768 K=5)                     2.60e-05   2.60e-05
    sums_scaled   2.399e-08  (4 segments of 984)                                   9.60e-08   9.54e-07 (floor)

The kernels' own worst figures in the same run, for the record (they are not where the constants come from): query_pool 6.6e-06,
rownorm 1.5e-07, video_rank 1.35e-06 (dcn at N=32 L=100; PyTorch-fp32 has 1.32e-06 on dcn at N=60 L=10 per=5), rank_loss
1.4e-07, st_ed 7.2e-06 (dctx at D=1536), sums_scaled 5.9e-08.  PyTorch-fp32's query_pool figure is that large because of its fp32
matmul path on this device, not because of the mathematics; the constant is kept as the rule gives it.
A note on the bf16 bound: the unit roundoff of bf16 (8 significant bits, round to nearest even) is 2^-8, not 2^-9, so
2^-8 |b| leaves no factor 2: a correctly rounded store meets it only through |fl(x) - x| <= u/(1+u) |x| plus the rms floor.
It is kept as written; every bf16 output passes it.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_reference as R
from tests.util import elem_rel_err

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
TOL = {"query_pool": 4 * 1.878e-4, "rownorm": FLOOR, "video_rank": 4 * 3.771e-7, "rank_loss": 4 * 5.606e-7, "st_ed": 4 * 6.511e-6,
       "sums_scaled": FLOOR}
EASY_W = float(np.float32(0.1))                        # the kernel's easy weight is the float 0.1f


def gen(*shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


class Report:
    """Prints kernel / PyTorch-fp32 errors of every output, collects the misses, asserts once at the end."""

    def __init__(self, op, case):
        self.op, self.case, self.tol, self.bad = op, case, TOL[op], []

    def _line(self, name, ek, et, ok):
        print("\n[head-parity] %-11s %-34s %-8s kernel %.3e  torch-fp32 %s  tol %.3e %s"
              % (self.op, self.case, name, ek, "%.3e" % et if et is not None else "   -     ", self.tol, "" if ok else "MISS"), end="")
        if not ok:
            self.bad.append((name, ek, self.tol))

    def tensor(self, name, got, ref, t32=None, sel=None):
        ref = ref.detach()
        ek = elem_rel_err(got, ref, sel)
        et = elem_rel_err(t32, ref, sel) if t32 is not None else None
        if got.dtype == torch.bfloat16:
            a, b = got.detach().double().cpu(), ref.double().cpu()
            if sel is not None:
                a, b = a[sel.bool().cpu()], b[sel.bool().cpu()]
            ok = bool(((a - b).abs() <= 2.0 ** -8 * b.abs() + self.tol * b.pow(2).mean().sqrt()).all())
        else:
            ok = ek <= self.tol
        self._line(name, ek, et, ok)

    def scalar(self, name, got, ref, t32=None):
        ref = float(ref)
        d = max(1.0, abs(ref))
        ek = abs(float(got) - ref) / d
        self._line(name, ek, abs(float(t32) - ref) / d if t32 is not None else None, ek <= self.tol)

    def done(self):
        assert not self.bad, (self.op, self.case, self.bad)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


# =================================================================================================================================
# A. exact tests
# =================================================================================================================================
@pytest.mark.parametrize("L,extra", [(1, 0), (13, 0), (64, 0), (65, 0), (100, 0), (256, 0), (300, 0), (100, 8)])
def test_score_max_fwd_first_maximum_exact(L, extra):
    """hero_score_max_fwd through the C ABI: with a 0/1 mask s*k + (1-k)*-10000 is exact, so out is where(mask, s, -10000).max
    BITWISE and arg the first arg-max EXACTLY.  Scores from 8 values: most pairs have tied maxima.  Ties placed on purpose:
    same lane (frames l, l+64), different lanes with the earlier frame in the higher lane's second trip (70 and 3), a fully
    masked video, a video whose only valid frame is the last."""
    from hero_amd import _lib as Lb
    M, N = 5, 7                                                            # 35 pairs: the last workgroup has 3 of its 4 waves
    rng = np.random.RandomState(L)
    vals = (np.arange(8, dtype=np.float32) - 3.5) / 4
    s = vals[rng.randint(0, 8, size=(M, N, L))]
    mask = np.ones((N, L), np.float32)
    mask[1, L // 2 + 1:] = 0
    mask[2, :] = 0                                                         # fully masked: every frame is exactly -10000
    mask[3, :L - 1] = 0                                                    # only the last frame is valid
    if L >= 2:
        mask[5, 0] = 0                                                     # first frame masked
    top = np.float32(2.0)
    if L > 64:
        s[0, 0, :] = vals[0]
        s[0, 0, [0, 64]] = top                                             # same lane, two trips
    if L > 70:
        s[1, 0, :] = vals[0]
        s[1, 0, [3, 70]] = top                                             # lane 6's second trip (70) against lane 3's first (3)
        s[2, 4, :] = vals[0]
        s[2, 4, [63, 64]] = top                                            # lane 63 against lane 0's second trip
    if L > 200:
        s[3, 6, :] = vals[0]
        s[3, 6, [130, 194, 199]] = top
    s[4, 6, :] = vals[7]                                                   # all frames equal
    ld = ((N * L + 3) & ~3) + extra
    sp = np.full((M, ld), 77.0, np.float32)                                # the padding is larger than any score
    sp[:, :N * L] = s.reshape(M, N * L)
    v = np.where(mask[None] != 0, s, np.float32(-10000.0))
    want_out, want_arg = v.max(-1), v.argmax(-1).astype(np.int32)
    ties = int(((v == want_out[..., None]).sum(-1) > 1).sum())
    assert ties >= ((M * N) // 2 if L >= 64 else 5 if L > 1 else 0), ties
    sd, md = torch.from_numpy(sp).cuda(), torch.from_numpy(mask).cuda()
    out = torch.full((M, N), -1.0, device="cuda")
    arg = torch.full((M, N), -1, dtype=torch.int32, device="cuda")
    a = Lb.ScoreMax()
    a.s, a.mask, a.out, a.arg = Lb.ptr(sd), Lb.ptr(md), Lb.ptr(out), Lb.ptr(arg)
    a.M, a.N, a.L, a.D, a.ld_s = M, N, L, 4, ld
    Lb.check(Lb.lib().hero_score_max_fwd(C.byref(a), Lb.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(arg.cpu().numpy(), want_arg), (arg.cpu().numpy(), want_arg)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want_out.view(np.int32))


def test_video_rank_loss_exactly_representable_inputs():
    """VideoRankLossFn forward + backward with entries of qn, cn in {-2..2}/16: every product is a multiple of 2^-8 and every
    partial sum far below 2^24 of that unit, so the fp32 GEMM gives the scores exactly, in any order, identical to float64.
    Ties between frames are then EXACT ties and the first-maximum rule is tested through GEMM + max + loss + both backward
    kernels.  Hinge, margin 0.1: every hinge argument is >= 0.4/256 from zero (0.1 * 256 = 25.6) - asserted below."""
    from hero_amd.head import VideoRankLossFn
    N, per, Lc, D = 37, 2, 70, 768                                         # N % 4 = 1; N*L = 2590 is padded to 2592 for the GEMM
    M = N * per
    g = torch.Generator().manual_seed(11)
    qn = (torch.randint(-2, 3, (M, D), generator=g).float() / 16)
    cn = (torch.randint(-2, 3, (N, Lc, D), generator=g).float() / 16)
    mask = torch.ones(N, Lc)
    mask[3, 40:] = 0
    mask[10, 1:] = 0
    qb, cb = R.leaf(qn), R.leaf(cn)
    lc_r, lq_r, q2v, arg, s = R.video_rank_losses(qb, cb, mask.double(), per, 0.1, False, False, 20, 10.0)
    q2v.retain_grad()
    (1.7 * lc_r - 0.6 * lq_r).backward()
    # preconditions, from the float64 scores
    assert float((s.detach() * 256 - (s.detach() * 256).round()).abs().max()) == 0           # multiples of 2^-8: exact in fp32
    v = R.mask_logits(s.detach(), mask.double().unsqueeze(0))
    tied = (v == q2v.detach().unsqueeze(-1)).sum(-1) > 1
    assert int((tied & (q2v.grad != 0)).sum()) > 10                        # exact ties that carry gradient: the rule is exercised
    own = torch.arange(M) // per
    pos = q2v.detach()[torch.arange(M), own]
    is_pos = own[:, None] == torch.arange(N)[None, :]
    h_ctx = (0.1 + q2v.detach() - pos[:, None])[~is_pos]
    h_q = (0.1 + q2v.detach().t()[own] - pos[:, None])[~is_pos.t()[own]]
    assert float(h_ctx.abs().min()) > 1e-3 and float(h_q.abs().min()) > 1e-3
    qd, cd = qn.cuda().requires_grad_(True), cn.cuda().requires_grad_(True)
    lc, lq = VideoRankLossFn.apply(qd, cd, mask.cuda(), (0, N), 0.1, False, False, 20, 10.0)
    (1.7 * lc - 0.6 * lq).backward()
    rep = Report("video_rank", "exact inputs N=37 per=2 L=70 D=768")
    rep.scalar("l_ctx", lc.detach(), lc_r)
    rep.scalar("l_q", lq.detach(), lq_r)
    rep.tensor("dqn", qd.grad, qb.grad)
    rep.tensor("dcn", cd.grad, cb.grad)
    # frames that are the (first) arg-max of no pair get exactly nothing - in particular the LATER frame of every tie
    is_arg = torch.zeros(N, Lc, dtype=torch.bool)
    is_arg[torch.arange(N).unsqueeze(0).expand(M, N), arg] = True
    assert float(cd.grad.cpu()[~is_arg].abs().max()) == 0.0
    assert float(cb.grad[~is_arg].abs().max()) == 0.0
    rep.done()


def _sted_inputs(B, L, D, K, dtype, seed=0):
    q2 = gen(B, D, seed=seed + 1, scale=0.2)
    ctx = gen(B, L, D, seed=seed + 2, dtype=dtype)
    w_st, w_ed = gen(1, 1, K, seed=seed + 3, scale=0.5), gen(1, 1, K, seed=seed + 4, scale=0.5)
    rng = np.random.RandomState(seed + 5)
    valid = rng.randint(max(1, (3 * L) // 10), L + 1, size=B)             # ragged: 30 % .. 100 % of the frames
    valid[0] = L
    mask = (np.arange(L)[None, :] < valid[:, None]).astype(np.float32)
    tg = np.stack([rng.randint(0, valid), rng.randint(0, valid)], 1).astype(np.int64)
    tg[0] = (0, L - 1)                                                     # frame 0 and the last frame
    if B > 1:
        tg[1] = (L - 1, 0)
        mask[1, :] = 1
    if B > 2 and L > 1:
        mask[2, L - 1] = 0
        tg[2] = (L - 1, L - 1)                                             # a masked frame as target
    if B > 4:
        tg[3, 0] = -1
        tg[4, 1] = -1
    assert (tg[:, 0] != -1).any() and (tg[:, 1] != -1).any()
    assert ((tg == -1) | ((tg >= 0) & (tg < L))).all()
    return q2, ctx, torch.from_numpy(mask), w_st, w_ed, torch.from_numpy(tg)


def test_st_ed_bwd_bit_reproducible_and_leaves_its_ticket_at_zero():
    """Two backward calls through the same cached workspace at B > 64 (three chunks of shares): identical bits for every
    output, the arrival counter (last word group of the workspace) reads 0 after each, and dw_st / dw_ed ACCUMULATE."""
    from hero_amd import _lib as Lb
    from hero_amd.head import StEdLossFn, _sted_workspace
    B, L, D, K = 130, 23, 64, 5
    q2, ctx, mask, w_st, w_ed, tg = [t.cuda() for t in _sted_inputs(B, L, D, K, torch.float32)]
    rows = torch.empty(B, device="cuda")
    saved = torch.empty(3, B, L, device="cuda")
    a = StEdLossFn._args(q2, ctx, mask, w_st, w_ed, tg, saved, K)
    a.loss_rows = Lb.ptr(rows)
    Lb.check(Lb.lib().hero_st_ed_fwd(C.byref(a), Lb.stream()))
    ws = _sted_workspace(B, q2.device)
    assert ws.numel() == B * 32 + 4
    gup = torch.tensor([2.5], device="cuda")
    init = torch.tensor([3.0, -1.0, 0.5, 0.0, 7.0], device="cuda")
    outs = []
    for _ in range(2):
        dq2, dctx = torch.full_like(q2, 9.0), torch.full_like(ctx, 9.0)
        dws, dwe = init.clone(), (-init).clone()
        a.g, a.g_scale = Lb.ptr(gup), 0.7
        a.dq2, a.dctx, a.dw_st, a.dw_ed, a.ws = Lb.ptr(dq2), Lb.ptr(dctx), Lb.ptr(dws), Lb.ptr(dwe), Lb.ptr(ws)
        Lb.check(Lb.lib().hero_st_ed_bwd(C.byref(a), Lb.stream()))
        torch.cuda.synchronize()
        assert bits(ws[B * 32:]).tolist() == [0, 0, 0, 0]
        outs.append((dq2, dctx, dws, dwe))
    for x, y in zip(*outs):
        assert torch.equal(bits(x), bits(y))
    # += : the same call on zeroed accumulators gives (out - init) up to the one rounding of the final add
    dq2, dctx = torch.empty_like(q2), torch.empty_like(ctx)
    z_st, z_ed = torch.zeros(K, device="cuda"), torch.zeros(K, device="cuda")
    a.dq2, a.dctx, a.dw_st, a.dw_ed = Lb.ptr(dq2), Lb.ptr(dctx), Lb.ptr(z_st), Lb.ptr(z_ed)
    Lb.check(Lb.lib().hero_st_ed_bwd(C.byref(a), Lb.stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(init + z_st), bits(outs[0][2])) and torch.equal(bits(-init + z_ed), bits(outs[0][3]))
    assert float(z_st.abs().min()) > 0


@pytest.mark.parametrize("per", [1, 5])
def test_video_rank_loss_own_slices(per):
    """Rows [n0, n0 + n_own) of dcn are bit-equal to the full run's rows, every other row is exactly 0, dqn does not depend on
    the slice - first, middle, last and empty slices, one and five queries per video."""
    from hero_amd.head import VideoRankLossFn
    N, Lc, D = 6, 9, 64
    M = N * per
    qn = F.normalize(gen(M, D, seed=1), dim=-1).cuda().requires_grad_(True)
    cn = F.normalize(gen(N, Lc, D, seed=2), dim=-1).cuda().requires_grad_(True)
    mask = torch.ones(N, Lc).cuda()
    mask[4, 5:] = 0

    def run(own):
        qn.grad = cn.grad = None
        lc, lq = VideoRankLossFn.apply(qn, cn, mask, own, 0.1, False, False, 20, 10.0)
        (lc + 0.5 * lq).backward()
        return qn.grad.clone(), cn.grad.clone()
    dq_full, dc_full = run((0, N))
    assert float(dc_full.abs().sum()) > 0
    for n0, n_own in [(0, 2), (2, 3), (4, 2), (5, 1), (3, 0), (0, 0), (6, 0)]:
        dq, dc = run((n0, n_own))
        assert torch.equal(bits(dq), bits(dq_full)), (n0, n_own)
        assert torch.equal(bits(dc[n0:n0 + n_own]), bits(dc_full[n0:n0 + n_own])), (n0, n_own)
        assert not bits(dc[:n0]).any() and not bits(dc[n0 + n_own:]).any(), (n0, n_own)


# =================================================================================================================================
# B. parity with the float64 references
# =================================================================================================================================
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,L,D", [(32, 20, 768), (5, 70, 1536), (3, 7, 260), (6, 65, 4)])
def test_query_pool_parity(dtype, B, L, D):
    from hero_amd.head import QueryPoolFn
    q, w, g = gen(B, L, D, seed=1, dtype=dtype), gen(1, D, seed=2, scale=0.2), gen(B, D, seed=3)
    mask = torch.ones(B, L)
    mask[0, L - 2:] = 0
    mask[1, :] = 0                                                         # a fully masked query: uniform attention, zero ds
    mask[2, 1:] = 0
    qd, wd = q.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    out = QueryPoolFn.apply(qd, mask.cuda(), wd)
    out.backward(g.cuda())
    qr, wr = R.leaf(q), R.leaf(w)
    ref, att = R.query_pool(qr, mask.double(), wr)
    ref.backward(g.double())
    assert float((att[1] - 1.0 / L).abs().max()) < 1e-15
    qt, wt = q.float().cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    m = mask.cuda()
    a32 = F.softmax((qt @ wt.t()) * m.unsqueeze(2) + (1 - m.unsqueeze(2)) * -1e4, dim=1)
    t32 = torch.einsum("blm,bld->bmd", a32, qt)[:, 0]
    t32.backward(g.cuda())
    rep = Report("query_pool", "%s B=%d L=%d D=%d" % (str(dtype)[6:], B, L, D))
    rep.tensor("pooled", out, ref, t32)
    rep.tensor("dq", qd.grad, qr.grad, qt.grad)
    rep.tensor("dw", wd.grad, wr.grad, wt.grad)
    rep.done()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(1920, 768), (8, 4), (5, 64), (6, 260), (7, 768)])
def test_rownorm_parity(dtype, rows, cols):
    """rows % 4 in {0, 1, 2, 3}, cols in {4, 64, 260, 768}; a zero row, a row of norm 1e-7 (below eps, non-zero: dx = dy / eps)
    and a row just above eps.  The three kinds of row are compared separately (their dx differ by 1e5 in size)."""
    from hero_amd.head import RowNormFn
    eps = 1e-5
    x, g = gen(rows, cols, seed=1), gen(rows, cols, seed=2)
    x[1] = 0
    x[2] = x[2] / x[2].norm() * 1e-7
    x[4] = x[4] / x[4].norm() * 1.5e-5
    x = x.to(dtype)
    n = x.double().norm(dim=-1)
    assert n[1] == 0 and 0 < n[2] < eps / 10 and eps * 1.2 < n[4] < eps * 2
    kinds = {"normal": n > 1e-3, "clamped": n < eps, "near-eps": (n > eps) & (n < 1e-3)}
    assert int(kinds["normal"].sum()) == rows - 3
    xd = x.cuda().requires_grad_(True)
    y = RowNormFn.apply(xd, eps)
    y.backward(g.cuda())
    xr = R.leaf(x)
    yr = R.rownorm(xr, eps)
    yr.backward(g.double())
    xt = x.float().cuda().requires_grad_(True)
    yt = F.normalize(xt, dim=-1, eps=eps)
    yt.backward(g.cuda())
    rep = Report("rownorm", "%s %dx%d" % (str(dtype)[6:], rows, cols))
    for kind, sel in kinds.items():
        sel = sel.unsqueeze(1).expand(rows, cols)
        rep.tensor("y/" + kind, y, yr, yt, sel)
        rep.tensor("dx/" + kind, xd.grad, xr.grad, xt.grad, sel)
    rep.done()


def _ragged_mask(N, L, seed, lo=0.3):
    rng = np.random.RandomState(seed)
    valid = rng.randint(int(lo * L) or 1, L + 1, size=N)
    return torch.from_numpy((np.arange(L)[None, :] < valid[:, None]).astype(np.float32))


def _torch32_video_rank(qn, cn, mask, per, margin, lse, hard, pool, hard_w, w):
    from tests.test_gpu_head import torch_rank_losses
    qt, ct = qn.cuda().requires_grad_(True), cn.cuda().requires_grad_(True)
    m = mask.cuda()
    sc = torch.einsum("md,nld->mln", qt, ct)
    q2v = (sc * m.t().unsqueeze(0) + (1 - m.t().unsqueeze(0)) * -1e4).max(dim=1)[0]
    lc, lq = torch_rank_losses(q2v, per, margin, lse, hard, pool, hard_w)
    (w[0] * lc + w[1] * lq).backward()
    return lc.detach(), lq.detach(), qt.grad, ct.grad


# (N, L, per, D, lse, hard, pool, (w_ctx, w_q), seed).  Hinge with random inputs only where a seed meets the gap precondition
# (the larger hinge shapes are in test_video_rank_loss_exactly_representable_inputs and test_rank_loss_abi_parity).
VIDEO_RANK_CASES = [
    (32, 60, 1, 768, False, False, 20, (8.0, 8.0), 0),                     # bench: 32 videos x 60 frames
    (32, 60, 5, 768, True, True, 20, (8.0, 8.0), 0),                       # bench: five queries per video (M = 160)
    (32, 100, 1, 768, True, True, 3, (1.0, 1.0), 0),                       # ragged TVR: 30-100 valid frames of 100
    (9, 256, 1, 768, True, False, 20, (1.0, 1.0), 0),                      # long video; N % 4 = 1
    (260, 8, 1, 128, True, True, 20, (1.0, 1.0), 0),                       # N > 256: second trip of the staging / candidate loops
    (60, 10, 5, 128, True, True, 1, (1.0, 1.0), 1),                        # nq = 300 > 256
    (6, 13, 1, 1536, False, True, 100, (1.0, 1.0), 0),                     # D > 1024; N % 4 = 2; pool >= the number of negatives
    (7, 13, 2, 128, False, False, 20, (0.0, 8.0), 0),                      # N % 4 = 3; w_ctx = 0
    (7, 13, 1, 128, True, True, 3, (8.0, 0.0), 0),                         # w_q = 0
]


def _video_rank_inputs(N, L, per, D, seed):
    qn = F.normalize(gen(N * per, D, seed=100 + seed), dim=-1)
    cn = F.normalize(gen(N, L, D, seed=200 + seed), dim=-1)
    mask = _ragged_mask(N, L, 300 + seed)
    return qn, cn, mask


def video_rank_preconditions(q2v, s, mask, per, margin, lse, hard, pool):
    """From the float64 reference: (top-2 gap of every pair's frame scores, smallest |hinge argument|, smallest gap across the
    hard / easy boundary of a row or column).  The fp32 scores are within ~1e-7 of these: with the gaps asserted by the caller,
    fp32 and float64 choose the same frame, the same active set and the same hard negatives."""
    v = R.mask_logits(s, mask.double().unsqueeze(0))
    valid2 = mask.sum(1) > 1                                               # (a video with one valid frame has no runner-up)
    top2 = v.topk(2, dim=-1)[0]
    gap = float((top2[..., 0] - top2[..., 1])[:, valid2].min())
    nq, nv = q2v.shape
    own = torch.arange(nq) // per
    pos = q2v[torch.arange(nq), own]
    is_pos = own[:, None] == torch.arange(nv)[None, :]
    hinge = 1.0
    if not lse:
        hinge = min(float((margin + q2v - pos[:, None]).abs()[~is_pos].min()),
                    float((margin + q2v.t()[own] - pos[:, None]).abs()[~is_pos.t()[own]].min()))
    edge = 1.0
    if hard:
        for mat, neg in ((q2v, ~is_pos), (q2v.t(), (~is_pos).t())):
            srt = torch.where(neg, mat, torch.full_like(mat, -1e9)).sort(dim=1, descending=True)[0]
            if pool < int(neg.sum(1).min()):
                edge = min(edge, float((srt[:, pool - 1] - srt[:, pool]).min()))
    return gap, hinge, edge


@pytest.mark.parametrize("N,L,per,D,lse,hard,pool,w,seed", VIDEO_RANK_CASES)
def test_video_rank_loss_parity(N, L, per, D, lse, hard, pool, w, seed):
    from hero_amd.head import VideoRankLossFn
    qn, cn, mask = _video_rank_inputs(N, L, per, D, seed)
    qb, cb = R.leaf(qn), R.leaf(cn)
    lc_r, lq_r, q2v, arg, s = R.video_rank_losses(qb, cb, mask.double(), per, 0.1, lse, hard, pool, 10.0)
    gs = (1.7, -0.6)
    (gs[0] * w[0] * lc_r + gs[1] * w[1] * lq_r).backward()
    gap, hinge, edge = video_rank_preconditions(q2v.detach(), s.detach(), mask, per, 0.1, lse, hard, pool)
    assert gap > 1e-6 and hinge > 1e-4 and edge > 1e-6, (gap, hinge, edge)
    qd, cd = qn.cuda().requires_grad_(True), cn.cuda().requires_grad_(True)
    lc, lq = VideoRankLossFn.apply(qd, cd, mask.cuda(), (0, N), 0.1, lse, hard, pool, 10.0, w[0], w[1])
    (gs[0] * lc + gs[1] * lq).backward()
    tc, tq, tdq, tdc = _torch32_video_rank(qn, cn, mask, per, 0.1, lse, hard, pool, 10.0, (gs[0] * w[0], gs[1] * w[1]))
    rep = Report("video_rank", "N=%d L=%d per=%d D=%d %s%s" % (N, L, per, D, "lse" if lse else "hinge", " hard%d" % pool if hard else ""))
    rep.scalar("l_ctx", lc.detach(), w[0] * lc_r, w[0] * tc)
    rep.scalar("l_q", lq.detach(), w[1] * lq_r, w[1] * tq)
    rep.tensor("dqn", qd.grad, qb.grad, tdq)
    rep.tensor("dcn", cd.grad, cb.grad, tdc)
    assert (float(lc) == 0.0) == (w[0] == 0.0) and (float(lq) == 0.0) == (w[1] == 0.0)
    rep.done()


def _latin_scores(nq, nv, step, seed):
    """[nq, nv] fp32-exact scores, DISTINCT within every row and every column: ((a*m + b*n) mod P) * step, P prime > nq."""
    P = next(p for p in range(max(nq, nv) + 1, 4 * max(nq, nv)) if all(p % d for d in range(2, int(p ** 0.5) + 1)))
    rng = np.random.RandomState(seed)
    a, b = int(rng.randint(1, P)), int(rng.randint(1, P))
    rows, cols = rng.permutation(nq)[:, None], rng.permutation(nv)[None, :]
    k = (a * rows + b * cols) % P
    return torch.from_numpy(((k - P // 2) * step).astype(np.float32))


def _rank_loss_abi(q2v, margin, lse, hard, pool, hard_w):
    from hero_amd import _lib as Lb
    nq, nv = q2v.shape
    s = q2v.cuda().contiguous()
    rows = torch.full((2, nq), 5.0, device="cuda")
    ds = torch.full((2, nq, nv), 5.0, device="cuda")
    r = Lb.RankLoss()
    r.s, r.loss_ctx_rows, r.loss_q_rows = Lb.ptr(s), Lb.ptr(rows[0]), Lb.ptr(rows[1])
    r.ds_ctx, r.ds_q, r.nq, r.nv = Lb.ptr(ds[0]), Lb.ptr(ds[1]), nq, nv
    r.margin, r.lse, r.hard, r.pool, r.hard_w, r.easy_w = margin, int(lse), int(hard), pool, hard_w, 0.1
    Lb.check(Lb.lib().hero_rank_loss(C.byref(r), Lb.stream()))
    torch.cuda.synchronize()
    return rows, ds


def _check_rank_loss(case, q2v, per, margin, lse, hard, pool, distinct=True):
    from tests.test_gpu_head import torch_rank_losses
    hard_w = 10.0
    nq, nv = q2v.shape
    if distinct:
        assert all(len(set(r.tolist())) == nv for r in q2v) and all(len(set(c.tolist())) == nq for c in q2v.t())
    b = R.leaf(q2v)
    rc, rq = R.rank_loss_rows(b, per, margin, lse, hard, pool, hard_w, EASY_W)
    g_ctx = torch.autograd.grad(rc.mean(), b, retain_graph=True)[0]
    g_q = torch.autograd.grad(rq.mean(), b)[0]
    if not lse:
        own = torch.arange(nq) // per
        pos = b.detach()[torch.arange(nq), own]
        is_pos = own[:, None] == torch.arange(nv)[None, :]
        assert float((margin + b.detach() - pos[:, None]).abs()[~is_pos].min()) > 1e-4
        assert float((margin + b.detach().t()[own] - pos[:, None]).abs()[~is_pos.t()[own]].min()) > 1e-4
    rows, ds = _rank_loss_abi(q2v, margin, lse, hard, pool, hard_w)
    t32 = [None] * 4
    if distinct:                                                           # (torch's sort is not stable: no fp32 figure on ties)
        t = q2v.cuda().requires_grad_(True)
        tc, tq = torch_rank_losses(t, per, margin, lse, hard, pool, hard_w)
        t32 = [tc.detach(), tq.detach(), torch.autograd.grad(tc, t, retain_graph=True)[0], torch.autograd.grad(tq, t)[0]]
    rep = Report("rank_loss", case)
    rep.tensor("rows_ctx", rows[0], rc)
    rep.tensor("rows_q", rows[1], rq)
    rep.scalar("mean_ctx", rows[0].double().mean(), rc.mean(), t32[0])
    rep.scalar("mean_q", rows[1].double().mean(), rq.mean(), t32[1])
    rep.tensor("ds_ctx", ds[0], g_ctx, t32[2])
    rep.tensor("ds_q", ds[1], g_q, t32[3])
    rep.done()


@pytest.mark.parametrize("nv,per,lse,hard,pool,step", [
    (260, 1, False, True, 20, 1 / 256),                                    # nv > 256: second trip of the candidate loop, both sides
    (60, 5, False, True, 3, 1 / 256),                                      # nq = 300, per = 5 (the pre-training mix)
    (60, 5, True, True, 20, 1 / 8),                                        # lse with gaps beyond +-15: both sides of the z > 15 branch
    (32, 5, True, False, 20, 1 / 8),
    (32, 1, False, True, 1, 1 / 256),
    (33, 1, False, True, 1000, 1 / 256),                                   # pool >= the number of negatives
    (7, 1, True, True, 3, 1 / 2),
    (9, 2, False, False, 20, 1 / 256),
])
def test_rank_loss_abi_parity(nv, per, lse, hard, pool, step):
    """hero_rank_loss through the C ABI on a given score matrix with distinct values in every row and column (the hard-negative
    ranks are then unambiguous); hinge: margin 0.1 against multiples of 1/256 keeps every argument 0.4/256 from zero."""
    q2v = _latin_scores(nv * per, nv, step, seed=nv + per)
    if lse and step >= 1 / 8 and nv >= 32:                                 # gaps z = neg - pos on both sides of +-15
        own = torch.arange(nv * per) // per
        z = (q2v - q2v[torch.arange(nv * per), own][:, None])[own[:, None] != torch.arange(nv)[None, :]]
        assert float(z.max()) > 15.5 and float(z.min()) < -15.5 and int(((z > 0) & (z < 15)).sum()) > 0
    _check_rank_loss("nv=%d per=%d %s%s" % (nv, per, "lse" if lse else "hinge", " hard%d" % pool if hard else ""), q2v, per, 0.1, lse, hard, pool)


@pytest.mark.parametrize("lse", [False, True], ids=["hinge", "lse"])
def test_rank_loss_equal_negatives_follow_the_stable_rule(lse):
    """Hand-made: equal negatives in rows and columns, pool = 1 and 2 - of equal values the one with the LOWER index is the
    harder (rank_loss_kernel counts v2 > neg || (v2 == neg && c2 < c))."""
    q2v = torch.tensor([[0.75, 0.50, 0.50, 0.25],
                        [0.25, 0.75, 0.25, 0.25],
                        [0.50, 0.50, 1.00, 0.50],
                        [0.25, 0.50, 0.50, 1.25]])
    for pool in (1, 2):
        _check_rank_loss("equal negatives pool=%d %s" % (pool, "lse" if lse else "hinge"), q2v, 1, 0.3, lse, True, pool, distinct=False)
    q2 = torch.tensor([[0.75, 0.50], [0.75, 0.50], [0.25, 1.00], [0.25, 1.00]])              # per = 2: equal rows
    _check_rank_loss("equal negatives per=2 %s" % ("lse" if lse else "hinge"), q2, 2, 0.3, lse, True, 1, distinct=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,L,D,K", [
    (32, 60, 768, 5),                                                      # bench
    (160, 60, 768, 5),                                                     # bench, five queries per video: three chunks of shares
    (32, 100, 768, 5),                                                     # ragged TVR
    (5, 256, 768, 15),                                                     # long video; L % 16 = 0
    (4, 300, 128, 5),                                                      # L > 256: second trips of the l += 256 loops
    (3, 100, 1536, 5),                                                     # D > 1024
    (130, 17, 128, 15),                                                    # B = 130; L % 16 = 1
    (65, 21, 128, 1),                                                      # B = 65; L % 16 = 5; K = 1
    (64, 31, 128, 5),                                                      # B = 64; L % 16 = 15
    (1, 2, 128, 5),                                                        # B = 1; L < 4, shorter than the filter
    (6, 3, 128, 15),
])
def test_st_ed_loss_parity(dtype, B, L, D, K):
    from hero_amd.head import StEdLossFn
    q2, ctx, mask, w_st, w_ed, tg = _sted_inputs(B, L, D, K, dtype)
    dev = [t.cuda() for t in (q2, ctx, mask, w_st, w_ed, tg)]
    for t in (dev[0], dev[1], dev[3], dev[4]):
        t.requires_grad_(True)
    loss = StEdLossFn.apply(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], 0.7)
    (2.5 * loss).backward()
    qr, cr, wsr, wer = R.leaf(q2), R.leaf(ctx), R.leaf(w_st), R.leaf(w_ed)
    ref, _ = R.st_ed_loss(qr, cr, mask.double(), wsr, wer, tg)
    (2.5 * 0.7 * ref).backward()
    qt, ct, wst, wet = [t.float().cuda().requires_grad_(True) for t in (q2, ctx, w_st, w_ed)]
    m = mask.cuda()
    sim = F.pad(torch.einsum("bd,bld->bl", qt, ct), (K // 2, K // 2)).unfold(-1, K, 1)          # model/pretrain.py _conv5
    st = (sim * wst.view(1, 1, K)).sum(-1) * m + (1 - m) * -1e4
    ed = (sim * wet.view(1, 1, K)).sum(-1) * m + (1 - m) * -1e4
    t32 = F.cross_entropy(st, dev[5][:, 0], ignore_index=-1) + F.cross_entropy(ed, dev[5][:, 1], ignore_index=-1)
    (2.5 * 0.7 * t32).backward()
    rep = Report("st_ed", "%s B=%d L=%d D=%d K=%d" % (str(dtype)[6:], B, L, D, K))
    rep.scalar("loss", loss.detach(), 0.7 * ref, 0.7 * t32.detach())
    rep.tensor("dq2", dev[0].grad, qr.grad, qt.grad)
    rep.tensor("dctx", dev[1].grad, cr.grad, ct.grad)
    rep.tensor("dw_st", dev[3].grad, wsr.grad, wst.grad)
    rep.tensor("dw_ed", dev[4].grad, wer.grad, wet.grad)
    rep.done()


def test_sums_scaled_parity_and_bit_reproducible():
    """hero_sums_scaled through the C ABI: 1-4 segments, seg_len on both sides of the 64-lane stride and at the long-video
    batch's 984, negative and zero scales, against a float64 sum; two calls give the same bits."""
    from hero_amd import _lib as Lb
    scales = [1.0 / 3, -2.5, 0.0, 8.0 / 984]
    rep = Report("sums_scaled", "")
    for n_segs in (1, 2, 3, 4):
        for seg_len in (1, 63, 64, 65, 984):
            src = gen(n_segs * seg_len + 3, seed=seg_len + n_segs).abs() + 0.25
            sd = src.cuda()
            sc = (C.c_float * n_segs)(*scales[:n_segs])
            outs = []
            for _ in range(2):
                out = torch.full((4,), 9.0, device="cuda")
                Lb.check(Lb.lib().hero_sums_scaled(Lb.ptr(sd), n_segs, seg_len, sc, Lb.ptr(out), Lb.stream()))
                torch.cuda.synchronize()
                outs.append(out)
            assert torch.equal(bits(outs[0]), bits(outs[1]))
            assert outs[0][n_segs:].tolist() == [9.0] * (4 - n_segs)       # nothing written past the last segment
            ref = R.sums_scaled(src, n_segs, seg_len, scales[:n_segs])
            t32 = sd[:n_segs * seg_len].view(n_segs, seg_len).sum(1) * torch.tensor(scales[:n_segs], device="cuda")
            rep.case = "n_segs=%d seg_len=%d" % (n_segs, seg_len)
            rep.tensor("out", outs[0][:n_segs], ref, t32)
            if n_segs >= 3:
                assert float(outs[0][2]) == 0.0
    rep.done()
