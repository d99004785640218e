"""The retrieval kernels of hero_amd/csrc/retrieval.hip through the C ABI: hero_topk_rows, hero_st_ed_probs, hero_moment_topk.

A. Exact tests, no tolerance.  Probabilities and weights are dyadic rationals with few significant bits (5 + 5 + 4 <= 24), so
   every product is exact in any order: the returned scores must be BITWISE the head of torch.sort over the materialised
   tensor, the indices those of a stable descending sort (equal scores: lower index first - the inputs are full of ties), two
   runs bit-identical.  hero_topk_rows against torch.topk values in the same way.
B. The order-robust index check, in EVERY case (check_indices): returned flat indices are unique, in band and in range, and
   the float64 score recomputed from the reference's probabilities at each returned index equals the returned score within the
   tolerance - near-ties may swap, a wrong selection cannot hide.  The reference's last kept score is asserted strictly
   positive before the kernel runs.
C. Parity with the float64 restatement tests/retrieval_reference.py, element-wise (tests.util.elem_rel_err).

Tolerances of B and C (none is taken from a kernel's output): the rule at the top of tests/test_gpu_head_kernels.py - the error
of the fp32 PyTorch formulation of the same step (on the GPU, same inputs) against the float64 reference, the worst over this
file's grid, times 4, floored at 16 * 2^-24 = 9.54e-7.  Every test prints the kernel's and PyTorch-fp32's figure (-s).

Measured on an AMD Instinct MI355X (gfx950), ROCm PyTorch, this file's inputs:

    step      worst PyTorch-fp32 elem_rel_err (case)                         x 4        TOL
    probs     5.288e-07  (st, Nq=80 Nv=2179 L=100 K=100 taps=5)                  2.12e-06   2.12e-06
    moments   8.320e-08  (Nq=80 K=100 L=100 band=[2,16) N=200)                   3.33e-07   9.54e-07 (floor)
    topk_exp  4.398e-07  (M=7 N=130 k=128)                                       1.76e-06   1.76e-06

The kernels' own worst figures in the same run, for the record (they are not where the constants come from): probs 7.64e-07
(st, L=33, 15 taps), moments 8.32e-08 (bitwise PyTorch-fp32's scores in every case of the grid), topk_exp 4.40e-07.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hero_amd import retrieval as HR
from tests import retrieval_reference as R
from tests.util import elem_rel_err

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
MEASURED = {"probs": 5.288e-7, "moments": 8.320e-8, "topk_exp": 4.398e-7}          # worst PyTorch-fp32 elem_rel_err, table above
TOL = {k: max(FLOOR, 4 * (v or 0.0)) for k, v in MEASURED.items()}
DEV = "cuda"


@pytest.fixture(autouse=True)
def reference_on_device():
    """The float64 reference runs on the device in this file (corpus-sized sorts); its results are taken back with .cpu()."""
    old, R.DEVICE = R.DEVICE, DEV
    yield
    R.DEVICE = old


def report(step, case, name, got, ref, t32=None):
    ek = elem_rel_err(got, ref)
    et = elem_rel_err(t32, ref) if t32 is not None else None
    ok = ek <= TOL[step]
    print("\n[retrieval-parity] %-9s %-40s %-6s kernel %.3e  torch-fp32 %s  tol %.3e %s"
          % (step, case, name, ek, "%.3e" % et if et is not None else "   -     ", TOL[step], "" if ok else "MISS"), end="")
    return [] if ok else [(step, case, name, ek, TOL[step])]


def dyadic_probs(nq, k, ln, seed):
    g = torch.Generator().manual_seed(seed)
    st = torch.randint(0, 32, (nq, k, ln), generator=g).float() / 32
    ed = torch.randint(0, 32, (nq, k, ln), generator=g).float() / 32
    w = torch.randint(1, 16, (nq, k), generator=g).float() / 8 * 2.0 ** torch.randint(-2, 6, (nq, k), generator=g).float()
    return st, ed, w


def soft_probs(nq, k, ln, seed, lens=None):
    """Softmax rows like the real ones: a few frames carry the mass; frames beyond a video's length are (almost) zero."""
    g = torch.Generator().manual_seed(seed)
    ls, le = torch.randn(nq, k, ln, generator=g) * 3, torch.randn(nq, k, ln, generator=g) * 3
    if lens is not None:
        dead = torch.arange(ln).view(1, 1, ln) >= lens.view(1, k, 1)
        ls, le = ls.masked_fill(dead, -10000.0), le.masked_fill(dead, -10000.0)
    w = torch.exp(20 * (torch.rand(nq, k, generator=g) * 0.6 - 0.1))
    return F.softmax(ls, -1), F.softmax(le, -1), w


def torch_moments(st, ed, w, min_l, max_l, top_n, stable):
    """The materialised formulation in fp32 on the device: (scores, flat) of the first top_n in-band entries, (0, -1) beyond."""
    nq, k, ln = st.shape
    outs = []
    for q0 in range(0, nq, 8):                                      # 8 queries at a time: the tensor is [8, K, L, L]
        s, e, ww = st[q0:q0 + 8], ed[q0:q0 + 8], w[q0:q0 + 8]
        prod = torch.einsum("qvm,qv,qvn->qvmn", s, ww, e)
        r = torch.arange(ln, device=st.device)
        band = HR.band_ok(r.view(ln, 1), r.view(1, ln), ln, min_l, max_l)
        flat_scores = torch.where(band.expand_as(prod), prod, torch.full_like(prod, -1.0)).reshape(len(s), -1)
        val, idx = torch.sort(flat_scores, dim=1, descending=True, stable=stable)
        val, idx = val[:, :top_n], idx[:, :top_n]
        if val.shape[1] < top_n:
            pad = top_n - val.shape[1]
            val, idx = F.pad(val, (0, pad), value=-1.0), F.pad(idx, (0, pad), value=-1)
        real = val >= 0
        outs.append((torch.where(real, val, torch.zeros_like(val)), torch.where(real, idx, torch.full_like(idx, -1))))
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]).to(torch.int32)


def reference_moments(st, ed, w, min_l, max_l, top_n):
    outs = [R.sorted_moments(st[q0:q0 + 8], ed[q0:q0 + 8], w[q0:q0 + 8], min_l, max_l, top_n) for q0 in range(0, st.shape[0], 8)]
    return torch.cat([o[0] for o in outs]).cpu(), torch.cat([o[1] for o in outs]).cpu()


def n_candidates(k, ln, min_l, max_l):
    return k * sum(1 for m in range(ln) for n in range(ln) if min_l <= n - m < max_l)


def check_indices(score, flat, st, ed, w, min_l, max_l, n_real, tol):
    """B of the module docstring.  score / flat: what the kernel returned; st, ed, w: the reference's (float64-able) inputs."""
    score, flat = score.cpu(), flat.cpu().long()
    nq, k, ln = st.shape
    assert flat.shape == score.shape
    assert bool((flat[:, n_real:] == -1).all()) and bool((score[:, n_real:] == 0).all())
    f = flat[:, :n_real]
    assert bool((f >= 0).all()) and bool((f < k * ln * ln).all())
    assert all(len(set(row.tolist())) == n_real for row in f), "a flat index is returned twice"
    m, n = (f // ln) % ln, f % ln
    assert bool(((n - m >= min_l) & (n - m < max_l)).all()), "a returned moment is out of band"
    again = R.scores_at(st, ed, w, f).cpu()
    got = score[:, :n_real].double()
    assert bool(((got - again).abs() <= tol * (again.abs() + again.pow(2).mean().sqrt())).all()), float(((got - again).abs() / (again.abs() + 1e-300)).max())
    assert bool((got[:, 1:] <= got[:, :-1]).all()), "scores are not sorted"


# ------------------------------------------------------------------------------------------------------------------------
# A. exact
# ------------------------------------------------------------------------------------------------------------------------
EXACT = [(3, 4, 12, 1, 4, 12), (2, 1, 30, 2, 16, 50), (2, 5, 100, 2, 16, 200), (2, 3, 7, 0, 3, 1024), (1, 128, 256, 2, 16, 1024),
         (2, 3, 1, 2, 16, 5), (2, 3, 2, 2, 16, 7), (2, 2, 6, 2, 16, 40), (3, 7, 33, 5, 6, 1)]


@pytest.mark.parametrize("nq,k,ln,min_l,max_l,top_n", EXACT)
def test_moment_topk_exact_with_ties(nq, k, ln, min_l, max_l, top_n):
    st, ed, w = (t.to(DEV) for t in dyadic_probs(nq, k, ln, seed=nq * 1000 + ln))
    want_s, want_f = torch_moments(st, ed, w, min_l, max_l, top_n, stable=True)
    n_real = min(top_n, n_candidates(k, ln, min_l, max_l))
    assert bool((want_f[:, :n_real] >= 0).all()) and bool((want_f[:, n_real:] == -1).all())
    score, flat = HR.k_moment_topk(st, ed, w, min_l, max_l, top_n)
    again = HR.k_moment_topk(st, ed, w, min_l, max_l, top_n)
    assert torch.equal(score, again[0]) and torch.equal(flat, again[1])                 # two runs, bit-identical
    assert torch.equal(score.view(torch.int32), want_s.view(torch.int32))               # bitwise the head of the full sort
    assert torch.equal(flat, want_f)                                                    # equal scores: lower flat index first
    if n_real:
        assert int((want_s[:, :n_real - 1] == want_s[:, 1:n_real]).sum()) > 0 or n_real == 1      # the case does have ties
    check_indices(score, flat, st.cpu(), ed.cpu(), w.cpu(), min_l, max_l, n_real, 0.0)


def test_moment_topk_all_equal_scores_take_the_lowest_indices():
    """Every candidate has the same score: the threshold is tied n_candidates ways and the index digits decide."""
    nq, k, ln, min_l, max_l, top_n = 2, 6, 40, 2, 16, 200
    st = torch.full((nq, k, ln), 0.25, device=DEV)
    ed = torch.full((nq, k, ln), 0.5, device=DEV)
    w = torch.full((nq, k), 2.0, device=DEV)
    score, flat = HR.k_moment_topk(st, ed, w, min_l, max_l, top_n)
    _, want_f = torch_moments(st, ed, w, min_l, max_l, top_n, stable=True)
    assert torch.equal(flat, want_f) and bool((score == 0.25).all())


@pytest.mark.parametrize("m,n,k,ld", [(5, 2179, 100, 2179), (3, 65536, 128, 65536), (4, 50, 128, 52), (2, 1, 1, 4), (80, 2179, 100, 2180)])
def test_topk_rows_exact(m, n, k, ld):
    g = torch.Generator().manual_seed(n + k)
    s = torch.randn(m, ld, generator=g).to(DEV)
    val, idx = HR.k_topk_rows(s, k, n=n)
    again = HR.k_topk_rows(s, k, n=n)
    assert torch.equal(val, again[0]) and torch.equal(idx, again[1])
    kk = min(k, n)
    want = torch.topk(s[:, :n], kk, dim=1)[0]
    assert torch.equal(val[:, :kk].view(torch.int32), want.view(torch.int32))
    assert torch.equal(torch.gather(s, 1, idx[:, :kk].long()), val[:, :kk])
    assert all(len(set(r.tolist())) == kk for r in idx[:, :kk].cpu()) and bool((idx[:, :kk] < n).all()) and bool((idx[:, :kk] >= 0).all())
    assert bool((idx[:, kk:] == -1).all()) and bool((val[:, kk:] == 0).all())           # k > N: (0, -1) in the remaining slots


def test_topk_rows_ties_go_to_the_lower_index():
    g = torch.Generator().manual_seed(3)
    s = torch.randint(-3, 4, (6, 500), generator=g).float().to(DEV)                     # seven distinct values (0 and -0 included below)
    s[0, 10], s[0, 20] = -0.0, 0.0
    val, idx = HR.k_topk_rows(s, 128)
    wv, wi = torch.sort(s, dim=1, descending=True, stable=True)
    assert torch.equal(val, wv[:, :128]) and torch.equal(idx.long(), wi[:, :128])


# ------------------------------------------------------------------------------------------------------------------------
# C. parity with the float64 reference
# ------------------------------------------------------------------------------------------------------------------------
def test_topk_rows_exp_alpha():
    bad = []
    g = torch.Generator().manual_seed(9)
    for (m, n, k) in [(80, 2179, 100), (7, 130, 128)]:
        s = (torch.rand(m, n, generator=g) * 1.4 - 0.6).to(DEV)                         # cosine-like scores
        val, idx = HR.k_topk_rows(s, k, alpha=20.0)
        rv, ri = (t.cpu() for t in R.vr_topk(s, 20.0, k))
        t32 = torch.topk(torch.exp(20.0 * s), k, dim=1)[0]
        assert torch.equal(idx.cpu().long(), ri)                                         # random fp32 scores: no ties
        bad += report("topk_exp", "M=%d N=%d k=%d" % (m, n, k), "val", val, rv, t32)
    assert not bad, bad


PROBS = [(3, 7, 12, 3, 5), (80, 2179, 100, 100, 5), (2, 3, 1, 2, 5), (4, 9, 33, 9, 15), (2, 5, 256, 5, 1), (3, 6, 50, 128, 3)]


@pytest.mark.parametrize("nq,nv,ln,k,taps", PROBS)
def test_st_ed_probs(nq, nv, ln, k, taps):
    """sim rows with a stride that is not Nv * L (hero_gemm's multiple-of-4 padding), videos of one valid frame, positions
    beyond a video's length that hold finite garbage (the convolution must see it), sel = -1."""
    g = torch.Generator().manual_seed(nq + nv + ln)
    ld = (nv * ln + 3) // 4 * 4 + 4
    sim = (torch.randn(nq, ld, generator=g) * 2).to(DEV)
    lens = torch.randint(1, ln + 1, (nv,), generator=g)
    lens[0] = 1                                                                       # a video with one valid frame
    mask = (torch.arange(ln).view(1, ln) < lens.view(nv, 1)).float().to(DEV)
    sel = torch.randint(0, nv, (nq, k), generator=g).to(torch.int32)
    sel[0, 0] = 0
    sel[-1, -1] = -1
    sel = sel.to(DEV)
    w_st, w_ed = (torch.randn(taps, generator=g) * 0.5).to(DEV), (torch.randn(taps, generator=g) * 0.5).to(DEV)
    st, ed = HR.k_st_ed_probs(sim, mask, sel, w_st, w_ed, ln)
    again = HR.k_st_ed_probs(sim, mask, sel, w_st, w_ed, ln)
    assert torch.equal(st, again[0]) and torch.equal(ed, again[1])
    sim3 = sim[:, :nv * ln].reshape(nq, nv, ln)
    rows = torch.arange(nq).unsqueeze(1)
    pair_sim = sim3[rows.to(DEV), sel.clamp(min=0).long()]                             # [Nq, K, L]: a pair is its own "video"
    pair_mask = mask[sel.clamp(min=0).long()]                                          # [Nq, K, L]
    live = (sel >= 0).cpu()
    bad = []
    ref, t32 = [], []
    for q in range(nq):                                                               # per query: K pairs as K videos of one query
        a, b = R.logits_from_similarities(pair_sim[q:q + 1], pair_mask[q], w_st, w_ed)
        ref.append((R.probs(a[0]).cpu(), R.probs(b[0]).cpu()))
        x = pair_sim[q].reshape(k, 1, ln)
        ta = F.conv1d(x, w_st.view(1, 1, -1), padding=taps // 2).view(k, ln)
        tb = F.conv1d(x, w_ed.view(1, 1, -1), padding=taps // 2).view(k, ln)
        pm32 = pair_mask[q]
        t32.append((F.softmax(ta * pm32 + (1 - pm32) * -10000.0, -1), F.softmax(tb * pm32 + (1 - pm32) * -10000.0, -1)))
    for i, (name, got) in enumerate((("st", st), ("ed", ed))):
        r = torch.stack([x[i] for x in ref]) * live.unsqueeze(-1).double()
        t = torch.stack([x[i] for x in t32]) * live.unsqueeze(-1).to(DEV).float()
        assert bool((got[~live.to(DEV)] == 0).all())                                   # sel = -1: a row of zeros
        bad += report("probs", "Nq=%d Nv=%d L=%d K=%d taps=%d" % (nq, nv, ln, k, taps), name, got, r, t)
    assert not bad, bad


MOMENTS = [(3, 4, 12, 1, 4, 12), (4, 1, 30, 2, 16, 50), (2, 3, 1, 2, 16, 5), (2, 3, 2, 2, 16, 7), (2, 2, 6, 2, 16, 40),
           (2, 128, 256, 2, 16, 1024), (80, 100, 100, 2, 16, 200), (5, 100, 37, 2, 16, 200)]


@pytest.mark.parametrize("nq,k,ln,min_l,max_l,top_n", MOMENTS)
def test_moment_topk_parity(nq, k, ln, min_l, max_l, top_n):
    g = torch.Generator().manual_seed(k + ln)
    lens = torch.randint(max(1, ln // 2), ln + 1, (k,), generator=g)
    n_real = min(top_n, n_candidates(k, ln, min_l, max_l))
    st, ed, w = soft_probs(nq, k, ln, seed=nq + ln, lens=lens if n_candidates(k, ln, min_l, max_l) > 2 * top_n else None)
    rs, rf = reference_moments(st, ed, w, min_l, max_l, top_n)
    if n_real:
        assert float(rs[:, n_real - 1].min()) > 0, "the reference's last kept score must be strictly positive"
    assert bool((rf[:, n_real:] == -1).all())
    std, edd, wd = st.to(DEV), ed.to(DEV), w.to(DEV)
    score, flat = HR.k_moment_topk(std, edd, wd, min_l, max_l, top_n)
    again = HR.k_moment_topk(std, edd, wd, min_l, max_l, top_n)
    assert torch.equal(score, again[0]) and torch.equal(flat, again[1])
    ts, _ = torch_moments(std, edd, wd, min_l, max_l, top_n, stable=False)
    case = "Nq=%d K=%d L=%d band=[%d,%d) N=%d" % (nq, k, ln, min_l, max_l, top_n)
    bad = report("moments", case, "score", score[:, :n_real], rs[:, :n_real], ts[:, :n_real]) if n_real else []
    check_indices(score, flat, st, ed, w, min_l, max_l, n_real, TOL["moments"])
    assert not bad, bad


def test_kernels_refuse_what_is_outside_the_envelope():
    z = torch.zeros(1, 1, 300, device=DEV)
    with pytest.raises(RuntimeError, match="hero_moment_topk"):
        HR.k_moment_topk(z, z, torch.ones(1, 1, device=DEV), 2, 16, 10)
    with pytest.raises(RuntimeError, match="hero_moment_topk"):
        HR.k_moment_topk(z[:, :, :10], z[:, :, :10], torch.ones(1, 1, device=DEV), 2, 16, 2000)
    with pytest.raises(RuntimeError, match="hero_topk_rows"):
        HR.k_topk_rows(torch.zeros(2, 8, device=DEV), 129)
    with pytest.raises(RuntimeError, match="hero_st_ed_probs"):
        HR.k_st_ed_probs(torch.zeros(1, 8, device=DEV), torch.ones(1, 8, device=DEV), torch.zeros(1, 1, dtype=torch.int32, device=DEV),
                         torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HR.k_topk_rows(torch.zeros(2, 8), 2)
