"""Float64 restatement of the reference's full-corpus retrieval (eval_vcmr.py:232-338), step by step with the reference's
file:line per step.  Pure torch, float64, CPU: the ground truth of tests/test_cpu_retrieval.py (against the reference-made
tests/golden/case_retrieval.npz) and of the GPU retrieval tests.  Ties are broken by the lower index (a stable sort).

DEVICE is where the float64 arithmetic runs: "cpu" by default; the GPU tests move it to the device for the corpus-sized cases
(float64 all the same) and take the results back with .cpu()."""
import torch
import torch.nn.functional as F

DEVICE = "cpu"


def _d(t):
    return torch.as_tensor(t).detach().to(device=DEVICE, dtype=torch.float64)


def mask_logits(x, m):
    """model/modeling_utils.py:42-43."""
    return x * m + (1.0 - m) * -10000.0


def similarities(mod_q, wq, bq, ctx):
    """model/pretrain.py:131-134 (cross): query = video_query_linear(modularized_query); sim = einsum("md,nld->mnl")."""
    q2 = _d(mod_q) @ _d(wq).t() + _d(bq)
    return torch.einsum("md,nld->mnl", q2, _d(ctx))


def logits_from_similarities(sim, mask, w_st, w_ed):
    """model/pretrain.py:135-149, 162-166: both Conv1d(1, 1, k, padding=k // 2, bias=False) over the whole padded row of every
    (query, video) pair, then mask_logits.  sim [Nq, Nv, L], mask [Nv, L]."""
    sim = _d(sim)
    nq, nv, ln = sim.shape
    flat = sim.reshape(nq * nv, 1, ln)
    out = []
    for w in (w_st, w_ed):
        w = _d(w).reshape(1, 1, -1)
        out.append(mask_logits(F.conv1d(flat, w, padding=w.shape[-1] // 2).view(nq, nv, ln), _d(mask).unsqueeze(0)))
    return out[0], out[1]


def cross_logits(mod_q, wq, bq, ctx, mask, w_st, w_ed):
    """eval_vcmr.py:232-235 -> model/vcmr.py get_pred_from_raw_query(cross=True): the start / end logits [Nq, Nv, L]."""
    return logits_from_similarities(similarities(mod_q, wq, bq, ctx), mask, w_st, w_ed)


def video_scores(mod_q, ctx, mask):
    """model/pretrain.py:364-413 at world size 1: F.normalize(eps=1e-5) of both sides, einsum("md,nld->mln"), mask_logits,
    max over the frames."""
    q = F.normalize(_d(mod_q), dim=-1, eps=1e-5)
    c = F.normalize(_d(ctx), dim=-1, eps=1e-5)
    s = torch.einsum("md,nld->mln", q, c)
    return mask_logits(s, _d(mask).t().unsqueeze(0)).max(dim=1)[0]


def probs(logits):
    """eval_vcmr.py:237-238."""
    return F.softmax(_d(logits), dim=-1)


def band_mask(length, min_l, max_l):
    """utils/tvr_eval_utils.py:237-260 generate_min_max_length_mask: triu(k=min_l) * (1 - triu(k=max_l)) of an L x L block of ones."""
    ones = torch.ones(length, length, dtype=torch.float64, device=DEVICE)
    return torch.triu(ones, diagonal=min_l) * (1.0 - torch.triu(ones, diagonal=max_l))


def vr_topk(q2v, alpha, k):
    """eval_vcmr.py:263-269: exp(q2c_alpha * scores), torch.topk.  Returns (scores [Nq, k], indices [Nq, k]); k > Nv pads with
    (0, -1)."""
    e = torch.exp(alpha * _d(q2v))
    val, idx = torch.sort(e, dim=1, descending=True, stable=True)
    val, idx = val[:, :k], idx[:, :k]
    if val.shape[1] < k:
        pad = k - val.shape[1]
        val, idx = F.pad(val, (0, pad)), F.pad(idx, (0, pad), value=-1)
    return val, idx


def gather_videos(p, idx):
    """eval_vcmr.py:284-288: probs[row, sorted_q2c_indices]; index -1 (no video) gives a row of zeros."""
    p = _d(p)
    idx = torch.as_tensor(idx).long().to(DEVICE)
    rows = torch.arange(p.shape[0], device=DEVICE).unsqueeze(1)
    out = p[rows, idx.clamp(min=0)]
    return out * (idx >= 0).unsqueeze(-1).double()


def sorted_moments(st_p, ed_p, w, min_l, max_l, top_n):
    """eval_vcmr.py:290-312: einsum("qvm,qv,qvn->qvmn"), band mask, flatten from the video dimension, sort descending, first
    top_n.  st_p, ed_p [Nq, K, L], w [Nq, K].  Returns (scores [Nq, top_n], flat [Nq, top_n]); only IN-BAND entries are moments:
    slots beyond them are (0, -1)."""
    st_p, ed_p, w = _d(st_p), _d(ed_p), _d(w)
    nq, k, ln = st_p.shape
    prod = torch.einsum("qvm,qv,qvn->qvmn", st_p, w, ed_p)
    band = band_mask(ln, min_l, max_l)
    flat_scores = torch.where(band.bool().expand_as(prod), prod, torch.full_like(prod, -1.0)).reshape(nq, -1)
    val, idx = torch.sort(flat_scores, dim=1, descending=True, stable=True)
    val, idx = val[:, :top_n], idx[:, :top_n]
    if val.shape[1] < top_n:
        pad = top_n - val.shape[1]
        val, idx = F.pad(val, (0, pad), value=-1.0), F.pad(idx, (0, pad), value=-1)
    real = val >= 0
    return torch.where(real, val, torch.zeros_like(val)), torch.where(real, idx, torch.full_like(idx, -1))


def vcmr_moments(st_logits, ed_logits, vr_scores, vr_indices, min_l, max_l, top_n):
    """eval_vcmr.py:237-238, 284-312 from the logits of every (query, video) pair."""
    return sorted_moments(gather_videos(probs(st_logits), vr_indices), gather_videos(probs(ed_logits), vr_indices), vr_scores,
                          min_l, max_l, top_n)


def svmr_moments(st_logits, ed_logits, gt_vidx, min_l, max_l, top_n):
    """eval_vcmr.py:241-258, 327-338: the ground-truth video's probabilities, einsum("bm,bn->bmn"), band mask,
    find_max_triples_from_upper_triangle_product (utils/tvr_eval_utils.py:95-129).  Returns (scores, flat = m L + n)."""
    g = torch.as_tensor(gt_vidx).long().reshape(-1, 1).to(DEVICE)
    st_p, ed_p = gather_videos(probs(st_logits), g), gather_videos(probs(ed_logits), g)
    return sorted_moments(st_p, ed_p, torch.ones(st_p.shape[0], 1, dtype=torch.float64, device=DEVICE), min_l, max_l, top_n)


def scores_at(st_p, ed_p, w, flat):
    """st * w * ed at flat = (j L + m) L + n, 0 where flat is -1 (the order-robust check of the GPU tests)."""
    st_p, ed_p, w = _d(st_p), _d(ed_p), _d(w)
    ln = st_p.shape[-1]
    f = torch.as_tensor(flat).long().to(DEVICE)
    ok = f >= 0
    f = f.clamp(min=0)
    j, m, n = f // (ln * ln), (f // ln) % ln, f % ln
    rows = torch.arange(st_p.shape[0], device=DEVICE).unsqueeze(1)
    return st_p[rows, j, m] * w[rows, j] * ed_p[rows, j, n] * ok.double()
