"""CPU checks of the retrieval path: the float64 restatement (tests/retrieval_reference.py) reproduces every array the
reference wrote into tests/golden/case_retrieval.npz (integers and band masks exactly, floats to 1e-5 - the project's oracle
pin), the reference's band masks are the kernels' predicate, and `search` refuses CPU tensors."""
import os

import numpy as np
import pytest
import torch

from tests import retrieval_reference as R
from tests.util import GOLDEN

PIN = 1e-5


@pytest.fixture(scope="module")
def case():
    z = np.load(os.path.join(GOLDEN, "case_retrieval.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def weights():
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"), allow_pickle=False)
    return {k: torch.from_numpy(z[k]) for k in ("video_query_linear.weight", "video_query_linear.bias", "video_st_predictor.weight",
                                                "video_ed_predictor.weight")}


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-12)
    assert err < PIN, (what, err)


def logits(case, weights):
    return R.cross_logits(case["mod_q"], weights["video_query_linear.weight"], weights["video_query_linear.bias"], case["corpus"],
                          case["corpus_masks"], weights["video_st_predictor.weight"], weights["video_ed_predictor.weight"])


def test_reference_reproduces_logits_and_video_scores(case, weights):
    st, ed = logits(case, weights)
    valid = case["corpus_masks"].astype(bool)[None].repeat(st.shape[0], 0)
    close(st.numpy()[valid], case["st_logits"][valid], "st_logits")          # masked positions hold -10000 + a rounding of the
    close(ed.numpy()[valid], case["ed_logits"][valid], "ed_logits")          # logit in fp32: compared below, relative to 1e4
    close(st, case["st_logits"], "st_logits (all)")
    close(ed, case["ed_logits"], "ed_logits (all)")
    close(R.video_scores(case["mod_q"], case["corpus"], case["corpus_masks"]), case["q2video_scores"], "q2video_scores")


def test_reference_reproduces_topk_videos_and_moments(case, weights):
    alpha, k, min_l, max_l, top_n, _, n_sv = (int(x) for x in case["cfg"])
    st, ed = logits(case, weights)
    q2v = R.video_scores(case["mod_q"], case["corpus"], case["corpus_masks"])
    vs, vi = R.vr_topk(q2v, alpha, k)
    assert np.array_equal(vi.numpy(), case["vr_indices"])
    close(vs, case["vr_scores"], "vr_scores")
    score, flat = R.vcmr_moments(st, ed, vs, vi, min_l, max_l, top_n)
    assert np.array_equal(flat.numpy(), case["vcmr_flat"])
    close(score, case["vcmr_scores"], "vcmr_scores")
    ln = case["corpus"].shape[1]
    s2, f2 = R.svmr_moments(st, ed, case["in.gt_vidx"], min_l, max_l, n_sv)
    tri = case["svmr_triples"]                                       # [Nq, n, (st, ed, score)]
    assert np.array_equal((f2 // ln).numpy(), tri[:, :, 0].astype(np.int64)) and np.array_equal((f2 % ln).numpy(), tri[:, :, 1].astype(np.int64))
    close(s2, tri[:, :, 2], "svmr scores")
    # the order-robust check of the GPU tests, on the reference itself: the score recomputed at every returned index
    close(R.scores_at(R.gather_videos(R.probs(st), vi), R.gather_videos(R.probs(ed), vi), vs, flat), score, "scores_at")


def test_band_masks_equal_the_kernel_predicate(case):
    from hero_amd.retrieval import band_ok
    keys = [k for k in case if k.startswith("band.")]
    assert len(keys) >= 4
    for key in keys:
        ln, min_l, max_l = (int(x) for x in key.split(".")[1:])
        want = case[key]
        assert want.shape == (ln, ln)
        mine = np.array([[1.0 if (min_l <= n - m < max_l and n < ln) else 0.0 for n in range(ln)] for m in range(ln)], dtype=np.float32)
        assert np.array_equal(mine, want), key
        assert np.array_equal(R.band_mask(ln, min_l, max_l).numpy().astype(np.float32), want), key
        r = torch.arange(ln)
        assert np.array_equal(band_ok(r.view(ln, 1), r.view(1, ln), ln, min_l, max_l).float().numpy(), want), key


def test_search_raises_on_cpu_tensors(case):
    """No silent fallback: the index can be held on the CPU, a search on it is an error - and so is `search_torch`."""
    import hero_amd
    from hero_amd.retrieval import CorpusIndex
    from tests.util import load_tiny
    model, _, _ = load_tiny("cpu")
    index = CorpusIndex(torch.from_numpy(case["corpus"]), torch.from_numpy(case["corpus_masks"]))
    q = [torch.from_numpy(case["in.query_" + k]) for k in ("input_ids", "pos_ids", "attn_masks")]
    for fn in (index.search, index.search_torch, lambda *a: hero_amd.search(index, *a)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(model, *q)
