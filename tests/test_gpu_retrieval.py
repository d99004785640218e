"""hero_amd.retrieval end to end on the GPU: encode_corpus + CorpusIndex.search against the reference-made
tests/golden/case_retrieval.npz, against the float64 restatement tests/retrieval_reference.py (fp32 and bf16 corpora, the TVR-val
shape included), and against `search_torch` (same keys, shapes, dtypes; the out-of-envelope route).

Tolerances (none is taken from the fused path's output): the rule at the top of tests/test_gpu_head_kernels.py - the error of
`search_torch`'s fp32 formulation on the GPU against the float64 reference, per output, the worst over this file's grid, times 4,
floored at 16 * 2^-24 = 9.54e-7.  Both paths start from the same modularised queries (the encoder is not what is compared), the
reference gets them as float64.  Every test prints both figures (-s).

Measured on an AMD Instinct MI355X (gfx950), ROCm PyTorch, this file's inputs:

    output        worst search_torch elem_rel_err (case)                        x 4        TOL
    vr_scores     3.065e-06  (tvr: Nq=80 Nv=2179 L=100 D=768, fp32 corpus)          1.23e-05   1.23e-05
    vcmr_scores   5.809e-05  (tvr, bf16 corpus)                                      2.32e-04   2.32e-04
    svmr_scores   2.308e-05  (tvr, fp32 corpus)                                      9.23e-05   9.23e-05

The fused path's own worst figures in the same run, for the record (they are not where the constants come from): vr_scores
2.80e-06, vcmr_scores 4.87e-05, svmr_scores 3.32e-05 (all at the tvr shape; the fp32 GEMM over D = 768 and exp(20 s) carry them).

Indices: compared exactly where the reference's kept scores are further apart than the tolerance, and by the order-robust rule
everywhere (unique, in band, in range, the float64 score at the returned index equals the returned score within the tolerance).
"""
import os

import numpy as np
import pytest
import torch

import hero_amd
from hero_amd import retrieval as HR
from oracle import hero_oracle as O
from tests import retrieval_reference as R
from tests.util import GOLDEN, elem_rel_err, load_tiny, to_dev

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
MEASURED = {"vr_scores": 3.065e-6, "vcmr_scores": 5.809e-5, "svmr_scores": 2.308e-5}        # worst search_torch elem_rel_err, table above
TOL = {k: max(FLOOR, 4 * (v or 0.0)) for k, v in MEASURED.items()}
DEV = "cuda"


@pytest.fixture(autouse=True)
def reference_on_device():
    """The float64 reference runs on the device in this file (corpus-sized operands); results are taken back with .cpu()."""
    old, R.DEVICE = R.DEVICE, DEV
    yield
    R.DEVICE = old


KEYS = {"vr_scores": torch.float32, "vr_indices": torch.int32, "vcmr_scores": torch.float32, "vcmr_video": torch.int32,
        "vcmr_st": torch.int32, "vcmr_ed": torch.int32, "svmr_scores": torch.float32, "svmr_st": torch.int32, "svmr_ed": torch.int32}


@pytest.fixture()
def fp32_mode():
    old = hero_amd.compute_dtype()
    hero_amd.set_compute_dtype(torch.float32)
    yield
    hero_amd.set_compute_dtype(old)


def golden():
    z = np.load(os.path.join(GOLDEN, "case_retrieval.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def golden_batches(case):
    import json
    out = []
    for i in range(3):
        b = {}
        for k, a in case.items():
            if k.startswith("b%d.in." % i):
                b[k[len("b0.in."):]] = json.loads(str(a)) if a.dtype.kind == "U" else torch.from_numpy(a)
        out.append(to_dev(b, DEV))
    return out


def report(key, case, got, ref, t32):
    ek, et = elem_rel_err(got, ref), elem_rel_err(t32, ref)
    ok = ek <= TOL[key]
    print("\n[retrieval-search] %-12s %-44s fused %.3e  search_torch %.3e  tol %.3e %s" % (key, case, ek, et, TOL[key], "" if ok else "MISS"), end="")
    return [] if ok else [(key, case, ek, TOL[key])]


class FixedQueries:
    """The model's query side replaced by given modularised queries: both paths and the reference start from the same numbers."""

    def __init__(self, model, mod_q):
        self.model, self.mod_q = model, mod_q

    def __enter__(self):
        self.old = self.model.encode_txt_inputs
        self.model.encode_txt_inputs = lambda *a, **k: self.mod_q
        return self

    def __exit__(self, *exc):
        del self.model.encode_txt_inputs


def reference_search(model, index, mod_q, gt, alpha, k, min_l, max_l, top_n):
    """tests/retrieval_reference.py on the index's own (fp32-exact) corpus values; also the probabilities of every pair."""
    P = {n: p.detach() for n, p in model.named_parameters() if n.startswith("video_")}
    ctx, mask = index.frame_embeddings, index.masks
    st, ed = R.cross_logits(mod_q, P["video_query_linear.weight"], P["video_query_linear.bias"], ctx, mask,
                            P["video_st_predictor.weight"], P["video_ed_predictor.weight"])
    st, ed = R.probs(st), R.probs(ed)
    q2v = R.video_scores(mod_q, ctx, mask)
    vs, vi = R.vr_topk(q2v, alpha, k)
    cs, cf = [], []
    for q0 in range(0, mod_q.shape[0], 16):
        sl = slice(q0, q0 + 16)
        a, b = R.sorted_moments(R.gather_videos(st[sl], vi[sl]), R.gather_videos(ed[sl], vi[sl]), vs[sl], min_l, max_l, top_n)
        cs.append(a)
        cf.append(b)
    g = gt.long().reshape(-1, 1)
    ss, sf = R.sorted_moments(R.gather_videos(st, g), R.gather_videos(ed, g), torch.ones(len(g), 1, dtype=torch.float64), min_l, max_l, top_n)
    out = dict(vr_scores=vs, vr_indices=vi, vcmr_scores=torch.cat(cs), vcmr_flat=torch.cat(cf), svmr_scores=ss, svmr_flat=sf)
    return {k_: v.cpu() for k_, v in out.items()}, st, ed, q2v


def check_moments(score, st_i, ed_i, slot, ref_st, ref_ed, ref_w, ln, min_l, max_l, n_real, tol):
    """The order-robust rule: (slot, st, ed) unique, in band, in range; float64 score at the returned index == returned score."""
    score, st_i, ed_i, slot = score.cpu().double(), st_i.cpu().long(), ed_i.cpu().long(), slot.cpu().long()
    assert bool((st_i[:, n_real:] == -1).all()) and bool((ed_i[:, n_real:] == -1).all()) and bool((score[:, n_real:] == 0).all())
    m, n, j = st_i[:, :n_real], ed_i[:, :n_real], slot[:, :n_real]
    assert bool(((m >= 0) & (n < ln) & (n - m >= min_l) & (n - m < max_l) & (j >= 0) & (j < ref_st.shape[1])).all())
    flat = (j * ln + m) * ln + n
    assert all(len(set(r.tolist())) == n_real for r in flat)
    again = R.scores_at(ref_st, ref_ed, ref_w, flat).cpu()
    got = score[:, :n_real]
    assert bool(((got - again).abs() <= tol * (again.abs() + again.pow(2).mean().sqrt())).all())


def slots_of(video, vr_indices):
    """Corpus index of a moment's video -> its slot among the query's K best videos (vr_indices rows are duplicate-free)."""
    eq = video.unsqueeze(-1) == vr_indices.unsqueeze(1)
    assert bool((eq.sum(-1)[video >= 0] == 1).all())
    return torch.where(video >= 0, eq.float().argmax(-1), torch.full_like(video, -1).long())


def run_case(model, index, mod_q, gt, name, alpha=20, k=100, min_l=2, max_l=16, top_n=200, exact_indices=False):
    Nq = mod_q.shape[0]
    ids = torch.zeros(Nq, 4, dtype=torch.long, device=DEV)
    kw = dict(gt_vidx=gt, q2c_alpha=alpha, max_vcmr_video=k, min_pred_l=min_l, max_pred_l=max_l, max_before_nms=top_n)
    with FixedQueries(model, mod_q):
        ref, st_all, ed_all, q2v = reference_search(model, index, mod_q, gt, alpha, min(k, index.n_videos), min_l, max_l, top_n)
        n_vc = int((ref["vcmr_flat"][0] >= 0).sum())
        n_sv = int((ref["svmr_flat"] >= 0).sum(1).min())
        assert n_vc > 0 and float(ref["vcmr_scores"][:, n_vc - 1].min()) > 0, "the reference's last kept VCMR score must be > 0"
        assert n_sv > 0 and float(ref["svmr_scores"][:, n_sv - 1].min()) > 0
        fused = index.search(model, ids, None, torch.ones_like(ids), **kw)
        again = index.search(model, ids, None, torch.ones_like(ids), **kw)
        base = index.search_torch(model, ids, None, torch.ones_like(ids), **kw)
    assert set(fused) == set(base) == set(KEYS)
    for key, dt in KEYS.items():
        assert fused[key].dtype == base[key].dtype == dt and fused[key].shape == base[key].shape, key
        assert torch.equal(fused[key], again[key]), key                                # two runs, bit-identical
    bad = []
    for key in ("vr_scores", "vcmr_scores", "svmr_scores"):
        bad += report(key, name, fused[key], ref[key], base[key])
    ln = index.length
    assert torch.equal(fused["vr_indices"].cpu().long(), ref["vr_indices"]) or not exact_indices
    vr_i = fused["vr_indices"].cpu().long()
    assert all(len(set(r.tolist())) == len(r) for r in vr_i) and bool(((vr_i >= 0) & (vr_i < index.n_videos)).all())
    e = torch.exp(alpha * torch.gather(q2v.cpu(), 1, vr_i))
    assert bool(((fused["vr_scores"].cpu().double() - e).abs() <= TOL["vr_scores"] * (e.abs() + e.pow(2).mean().sqrt())).all())
    # VCMR: the float64 probabilities of the videos the FUSED path selected; the weight is the reference's exp(alpha * score)
    slot = slots_of(fused["vcmr_video"].cpu().long(), vr_i)
    check_moments(fused["vcmr_scores"], fused["vcmr_st"], fused["vcmr_ed"], slot, R.gather_videos(st_all, vr_i), R.gather_videos(ed_all, vr_i), e,
                  ln, min_l, max_l, n_vc, TOL["vcmr_scores"] + TOL["vr_scores"])
    g = gt.long().reshape(-1, 1)
    check_moments(fused["svmr_scores"], fused["svmr_st"], fused["svmr_ed"], torch.zeros_like(fused["svmr_st"]), R.gather_videos(st_all, g),
                  R.gather_videos(ed_all, g), torch.ones(len(g), 1, dtype=torch.float64), ln, min_l, max_l, n_sv, TOL["svmr_scores"])
    if exact_indices:
        f = ref["vcmr_flat"]
        assert torch.equal(fused["vcmr_st"].cpu().long(), torch.where(f >= 0, (f // ln) % ln, f))
        assert torch.equal(fused["vcmr_ed"].cpu().long(), torch.where(f >= 0, f % ln, f))
        want_v = torch.where(f >= 0, torch.gather(ref["vr_indices"], 1, (f // (ln * ln)).clamp(min=0)), f)
        assert torch.equal(fused["vcmr_video"].cpu().long(), want_v)
    assert not bad, bad
    return fused, base, ref


def synthetic(nq, nv, ln, d, seed, dtype, conv_taps=5):
    """A HERO head with seeded weights over a synthetic corpus (clips of different lengths; zeros beyond a clip's length, as the
    encoder batches leave them)."""
    g = torch.Generator().manual_seed(seed)
    model, _, _ = load_tiny("cpu")
    model.video_query_linear = torch.nn.Linear(d, d)
    model.video_st_predictor = torch.nn.Conv1d(1, 1, conv_taps, padding=conv_taps // 2, bias=False)
    model.video_ed_predictor = torch.nn.Conv1d(1, 1, conv_taps, padding=conv_taps // 2, bias=False)
    with torch.no_grad():
        model.video_query_linear.weight.copy_(torch.randn(d, d, generator=g) * d ** -0.5)
        model.video_query_linear.bias.copy_(torch.randn(d, generator=g) * 0.1)
        model.video_st_predictor.weight.copy_(torch.randn(1, 1, conv_taps, generator=g) * 0.5)
        model.video_ed_predictor.weight.copy_(torch.randn(1, 1, conv_taps, generator=g) * 0.5)
    model = model.to(DEV).eval()
    lens = torch.randint(max(1, (2 * ln) // 3), ln + 1, (nv,), generator=g)
    lens[0], lens[-1] = 1, ln
    mask = (torch.arange(ln).view(1, ln) < lens.view(nv, 1)).long()
    ctx = (torch.randn(nv, ln, d, generator=g) * mask.unsqueeze(-1)).to(dtype)
    index = HR.CorpusIndex(ctx.to(DEV), mask.to(DEV))
    mod_q = torch.randn(nq, d, generator=g).to(DEV)
    gt = torch.randint(1, nv, (nq,), generator=g).to(DEV)
    return model, index, mod_q, gt


def test_golden_end_to_end(fp32_mode):
    """encode_corpus + search with the tiny golden model in fp32 reproduce the reference's own arrays."""
    case = golden()
    alpha, k, min_l, max_l, top_n, max_clip_len, n_sv = (int(x) for x in case["cfg"])
    model, _, _ = load_tiny(DEV)
    index = hero_amd.encode_corpus(model, golden_batches(case), max_clip_len)
    assert index.frame_embeddings.shape == case["corpus"].shape and np.array_equal(index.masks.cpu().numpy(), case["corpus_masks"])
    valid = torch.from_numpy(case["corpus_masks"]).bool()
    assert elem_rel_err(index.frame_embeddings.cpu()[valid], torch.from_numpy(case["corpus"])[valid]) < 1e-3
    beyond = torch.from_numpy(case["corpus"]).abs().sum(-1) == 0            # beyond a BATCH's clip length: zeros, as the reference leaves them
    assert bool(beyond.any()) and float(index.frame_embeddings.cpu()[beyond].abs().max()) == 0
    q = [torch.from_numpy(case["in.query_" + n]).to(DEV) for n in ("input_ids", "pos_ids", "attn_masks")]
    gt = torch.from_numpy(case["in.gt_vidx"]).to(DEV)
    kw = dict(gt_vidx=gt, q2c_alpha=alpha, max_vcmr_video=k, min_pred_l=min_l, max_pred_l=max_l)
    out = index.search(model, *q, max_before_nms=top_n, **kw)
    base = index.search_torch(model, *q, max_before_nms=top_n, **kw)
    ln = index.length
    for o in (out, base):
        assert np.array_equal(o["vr_indices"].cpu().numpy(), case["vr_indices"])
        assert elem_rel_err(o["vr_scores"], torch.from_numpy(case["vr_scores"])) < 1e-3
        assert elem_rel_err(o["vcmr_scores"], torch.from_numpy(case["vcmr_scores"])) < 1e-3
        f = torch.from_numpy(case["vcmr_flat"])
        assert torch.equal(o["vcmr_st"].cpu().long(), (f // ln) % ln) and torch.equal(o["vcmr_ed"].cpu().long(), f % ln)
        assert torch.equal(o["vcmr_video"].cpu().long(), torch.gather(torch.from_numpy(case["vr_indices"]), 1, f // (ln * ln)))
    sv = index.search(model, *q, max_before_nms=n_sv, tasks=("SVMR",), **kw)
    assert set(sv) == {"svmr_scores", "svmr_st", "svmr_ed"}
    tri = case["svmr_triples"]
    assert np.array_equal(sv["svmr_st"].cpu().numpy(), tri[:, :, 0].astype(np.int32)) and np.array_equal(sv["svmr_ed"].cpu().numpy(), tri[:, :, 1].astype(np.int32))
    assert elem_rel_err(sv["svmr_scores"], torch.from_numpy(tri[:, :, 2])) < 1e-3
    # the corpus the REFERENCE encoded, through the fused path: only the head differs -> the oracle pin applies to the scores
    idx2 = HR.CorpusIndex(torch.from_numpy(case["corpus"]).to(DEV), torch.from_numpy(case["corpus_masks"]).to(DEV))
    with FixedQueries(model, torch.from_numpy(case["mod_q"]).to(DEV)):
        o2 = idx2.search(model, *q, max_before_nms=top_n, **kw)
    assert np.array_equal(o2["vr_indices"].cpu().numpy(), case["vr_indices"])
    assert elem_rel_err(o2["vcmr_scores"], torch.from_numpy(case["vcmr_scores"])) < 1e-5
    assert elem_rel_err(o2["vr_scores"], torch.from_numpy(case["vr_scores"])) < 1e-5


GRID = [("small", 5, 23, 13, 128, 7, 1, 4, 15), ("unpadded", 3, 7, 9, 64, 5, 2, 16, 8), ("tvr", 80, 2179, 100, 768, 100, 2, 16, 200)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name,nq,nv,ln,d,k,min_l,max_l,top_n", GRID)
def test_search_parity(name, nq, nv, ln, d, k, min_l, max_l, top_n, dtype, fp32_mode):
    """fp32 and bf16 corpora; Nv * L not a multiple of 4 (7 x 9 = 63, 23 x 13 = 299); a video with one valid frame; the TVR-val shape."""
    model, index, mod_q, gt = synthetic(nq, nv, ln, d, seed=nv + ln, dtype=dtype)
    assert index.dtype == dtype and (name == "tvr" or (nv * ln) % 4 != 0)
    run_case(model, index, mod_q, gt, "%s %s" % (name, str(dtype).split(".")[-1]), k=k, min_l=min_l, max_l=max_l, top_n=top_n)


def test_out_of_envelope_takes_search_torch(fp32_mode, monkeypatch):
    """max_before_nms beyond the kernels' 1024: `search` must route to `search_torch` (and only then), and still be right."""
    model, index, mod_q, gt = synthetic(3, 9, 20, 64, seed=5, dtype=torch.float32)
    calls = []
    real = HR.search_torch
    monkeypatch.setattr(HR, "search_torch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ids = torch.zeros(3, 4, dtype=torch.long, device=DEV)
    with FixedQueries(model, mod_q):
        inside = index.search(model, ids, None, torch.ones_like(ids), gt_vidx=gt, max_vcmr_video=4, max_before_nms=1024)
        assert not calls
        outside = index.search(model, ids, None, torch.ones_like(ids), gt_vidx=gt, max_vcmr_video=4, max_before_nms=1100)
        assert calls == [1]
    assert set(outside) == set(KEYS) and outside["vcmr_scores"].shape == (3, 1100)
    n_real = int((inside["vcmr_st"][0] >= 0).sum())                                   # 4 videos x in-band moments of L = 20 < 1024
    assert 0 < n_real < 1024 and bool((outside["vcmr_scores"][:, n_real:] == 0).all())
    # moments with a positive score (frames inside the video): the same list; zero-score slots are in no particular order in a full sort
    n_pos = int((inside["vcmr_scores"] > 0).sum(1).min())
    assert n_pos > 100 and elem_rel_err(outside["vcmr_scores"][:, :n_pos], inside["vcmr_scores"][:, :n_pos]) < 1e-4
    assert torch.equal(outside["vcmr_st"][:, :50], inside["vcmr_st"][:, :50]) and torch.equal(outside["vcmr_video"][:, :50], inside["vcmr_video"][:, :50])
    monkeypatch.setattr(model.video_st_predictor, "stride", (2,))
    assert not HR._fusable(index, model, 4, 100, 2, 16)
