"""Float64 restatements of the VSM / VCMR loss-head operations, for the kernel tests of
tests/test_gpu_head_kernels.py (pinned to the project's PyTorch formulation by tests/test_cpu_head_reference.py).

Written from the formulas (model/modeling_utils.py:42-43, model/encoder.py:460-471, model/pretrain.py:96-110, 128-166,
203-264, 364-382), not from the kernels and not from the library: nothing here imports hero_amd.  Everything is torch on the
CPU in float64; gradients come from torch's float64 autograd.  Inputs of any float dtype are taken AS THEY ARE (`.double()`
of the very values the kernel reads), so input rounding is never part of a measured error.

Two places need a rule where the mathematics leaves a choice, and the kernels document theirs (include/hero_hip.h):

* max over the frames of a video: the FIRST frame that attains the maximum (numpy.argmax semantics); the gradient of the
  maximum flows to that frame alone.
* hard-negative rank of a negative inside its row / column: descending by value, equal values in index order (a STABLE
  descending sort): rank(c) = #{c2 : v[c2] > v[c] or (v[c2] == v[c] and c2 < c)}; the `pool` lowest ranks weigh `hard_w`,
  the rest `easy_w`.  The weights are constants of the loss (no gradient through the ranking).
"""
import numpy as np
import torch

NEG = -10000.0


def f64(t):
    return t.detach().to("cpu", torch.float64)


def leaf(t):
    return f64(t).clone().requires_grad_(True)


def mask_logits(x, m):
    return x * m + (1.0 - m) * NEG


def first_argmax(v):
    """Index of the first maximum along the last axis (int64 tensor)."""
    return torch.from_numpy(np.argmax(v.detach().numpy(), axis=-1))


def stable_desc_rank(v, valid):
    """v [R, C], valid [R, C] bool -> rank [R, C] of every valid entry among the valid entries of its row: descending by
    value, equal values in index order.  (Counted, not sorted: no library sort decides the ties.)"""
    v = v.detach()
    idx = torch.arange(v.shape[1])
    before = (v[:, None, :] > v[:, :, None]) | ((v[:, None, :] == v[:, :, None]) & (idx[None, None, :] < idx[None, :, None]))
    return (before & valid[:, None, :]).sum(-1)          # [R, C]: for entry c, the count over c2


# --- query pooling -------------------------------------------------------------------------------------------------------------
def query_pool(q, mask, w):
    """q [B, L, D], mask [B, L] 0/1, w [D] -> (pooled [B, D], att [B, L])."""
    sc = mask_logits(torch.einsum("bld,d->bl", q, w.reshape(-1)), mask)
    att = torch.softmax(sc, dim=1)
    return torch.einsum("bl,bld->bd", att, q), att


# --- F.normalize with the eps clamp ---------------------------------------------------------------------------------------------
def rownorm(x, eps):
    """y = x / max(||x||_2, eps) along the last axis.  Where the clamp is active the divisor is the constant eps."""
    ss = x.pow(2).sum(-1, keepdim=True)
    clamped = ss.detach().sqrt() < eps
    n = torch.where(clamped, torch.ones_like(ss), ss).sqrt()               # (no sqrt'(0) on the clamped rows)
    return x / torch.where(clamped, torch.full_like(n, eps), n)


# --- scores, mask_logits, max over frames ---------------------------------------------------------------------------------------
def score_max(s, mask):
    """s [M, N, L], mask [N, L] 0/1 -> (out [M, N], arg [M, N]): the masked maximum over the frames, FIRST maximum."""
    v = mask_logits(s, mask.unsqueeze(0))
    arg = first_argmax(v)
    return v.gather(-1, arg.unsqueeze(-1)).squeeze(-1), arg


def video_scores(qn, cn, mask):
    """qn [M, D], cn [N, L, D], mask [N, L] -> (q2v [M, N], arg [M, N], scores [M, N, L])."""
    s = torch.einsum("md,nld->mnl", qn, cn)
    out, arg = score_max(s, mask)
    return out, arg, s


# --- ranking loss over all in-batch negatives -----------------------------------------------------------------------------------
def _rl(pos, neg, margin, lse):
    if lse:
        return torch.logaddexp(torch.zeros_like(neg - pos), neg - pos)        # log(1 + exp(neg - pos))
    return torch.clamp(margin + neg - pos, min=0)


def rank_loss_rows(q2v, per, margin, lse, hard, pool, hard_w, easy_w=0.1):
    """q2v [nq, nv] with query m belonging to video m // per -> (l_ctx_rows [nq], l_q_rows [nq]):
    l_ctx_rows[m] = mean over the other videos n of w * rl(q2v[m, own], q2v[m, n]);
    l_q_rows[m]   = mean over the queries m2 of other videos of w * rl(q2v[m, own], q2v[m2, own])."""
    nq, nv = q2v.shape
    own = torch.arange(nq) // per
    is_pos = own[:, None] == torch.arange(nv)[None, :]                      # [nq, nv]
    pos = q2v[torch.arange(nq), own]                                        # [nq]
    neg_mask = ~is_pos
    w_ctx = torch.ones(nq, nv, dtype=torch.float64)
    w_q = torch.ones(nv, nq, dtype=torch.float64)
    if hard:
        r = stable_desc_rank(q2v, neg_mask)
        hw, ew = torch.tensor(hard_w, dtype=torch.float64), torch.tensor(easy_w, dtype=torch.float64)
        w_ctx = torch.where(r < pool, hw, ew)
        r = stable_desc_rank(q2v.t(), neg_mask.t())
        w_q = torch.where(r < pool, hw, ew)
    l_ctx = (w_ctx * _rl(pos[:, None], q2v, margin, lse) * neg_mask).sum(1) / (nv - 1)
    # the column of query m's own video: every query m2 of another video is a negative
    col = q2v.t()[own]                                                      # [nq, nq]: col[m, m2] = q2v[m2, own[m]]
    l_q = (w_q[own] * _rl(pos[:, None], col, margin, lse) * neg_mask.t()[own]).sum(1) / (nq - per)
    return l_ctx, l_q


def rank_losses(q2v, per, margin, lse, hard, pool, hard_w, easy_w=0.1):
    """The two scalars of get_video_level_loss(reduction='mean'): means over the queries of the rows above."""
    a, b = rank_loss_rows(q2v, per, margin, lse, hard, pool, hard_w, easy_w)
    return a.mean(), b.mean()


def video_rank_losses(qn, cn, mask, per, margin, lse, hard, pool, hard_w):
    q2v, arg, s = video_scores(qn, cn, mask)
    lc, lq = rank_losses(q2v, per, margin, lse, hard, pool, hard_w)
    return lc, lq, q2v, arg, s


# --- start / end localisation ---------------------------------------------------------------------------------------------------
def conv1d_same(x, w):
    """x [B, L], w [K] (K odd): out[b, l] = sum_k w[k] * x[b, l + k - K//2], zero outside (Conv1d(1, 1, K, padding=K//2))."""
    K = w.numel()
    L = x.shape[1]
    xp = torch.nn.functional.pad(x, (K // 2, K // 2))
    return sum(w.reshape(-1)[k] * xp[:, k:k + L] for k in range(K))


def masked_ce_mean(logits, target):
    """cross_entropy(logits, target, ignore_index=-1, reduction='mean'): mean over the rows whose target is not -1."""
    valid = target != -1
    assert bool(valid.any()), "every target of this column is -1: the mean divides by zero"
    t = torch.where(valid, target, torch.zeros_like(target))
    nll = torch.logsumexp(logits, dim=1) - logits.gather(1, t.unsqueeze(1)).squeeze(1)
    return (nll * valid).sum() / valid.sum()


def st_ed_loss(q2, ctx, mask, w_st, w_ed, targets):
    """q2 [B, D], ctx [B, L, D], mask [B, L], w_* [K], targets [B, 2] int64 -> (loss, sim [B, L])."""
    sim = torch.einsum("bd,bld->bl", q2, ctx)
    st = mask_logits(conv1d_same(sim, w_st), mask)
    ed = mask_logits(conv1d_same(sim, w_ed), mask)
    tg = targets.to("cpu", torch.int64)
    return masked_ce_mean(st, tg[:, 0]) + masked_ce_mean(ed, tg[:, 1]), sim


# --- final reductions -----------------------------------------------------------------------------------------------------------
def sums_scaled(src, n_segs, seg_len, scales):
    s = f64(src).reshape(-1)[:n_segs * seg_len].reshape(n_segs, seg_len).sum(1)
    return s * torch.tensor([float(np.float32(x)) for x in scales], dtype=torch.float64)
