"""tests/head_reference.py (the float64 references of the loss-head kernel tests) against what the project already trusts: the
PyTorch formulation kept in hero_amd/model/pretrain.py / encoder.py for the non-fused path, run in float64 on the CPU on
tie-free random inputs - forward values and gradients.  Both sides are the same mathematics in the same precision, so the
bound is rounding alone: 1e-12 under the element-wise relative error.  The two tie rules are pinned on a hand-written
example.  No GPU, no library call."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import head_reference as R
from tests.util import elem_rel_err

TOL = 1e-12


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def close(a, b):
    e = elem_rel_err(a, b)
    assert e < TOL, e


class _Head:
    """The loss methods of HeroForPretraining on a bare object (no encoder is built)."""

    def __init__(self, **kw):
        from hero_amd.model.pretrain import HeroForPretraining as H
        self.__dict__.update(kw)
        for name in ("get_video_level_loss", "get_ranking_loss", "_weight_hard", "get_video_level_scores", "_get_st_ed_prob"):
            setattr(self, name, getattr(H, name).__get__(self))
        self._conv5 = H._conv5


@pytest.mark.parametrize("B,L,D", [(3, 7, 32), (2, 70, 64)])
def test_query_pool_reference(B, L, D):
    from hero_amd.model.encoder import QueryFeatEncoder
    q, w, g = rnd(B, L, D, seed=1), rnd(1, D, seed=2, scale=0.3), rnd(B, D, seed=3)
    mask = torch.ones(B, L, dtype=torch.float64)
    mask[0, L - 3:] = 0
    mask[1, :] = 0                                                         # a fully masked query: uniform attention
    lin = nn.Linear(D, 1, bias=False).double()
    lin.weight.data.copy_(w)
    qa = q.clone().requires_grad_(True)
    ref = QueryFeatEncoder.get_modularized_queries(SimpleNamespace(modular_vector_mapping=lin), qa, mask)
    ref.backward(g)
    qb, wb = R.leaf(q), R.leaf(w)
    out, att = R.query_pool(qb, mask, wb)
    out.backward(g)
    close(out, ref)
    close(qb.grad, qa.grad)
    close(wb.grad, lin.weight.grad)
    assert torch.allclose(att[1], torch.full((L,), 1.0 / L, dtype=torch.float64), rtol=0, atol=1e-15)


def test_rownorm_reference():
    x = rnd(9, 48, seed=1)
    x[2] = 0                                                               # zero row
    x[4] = x[4] / x[4].norm() * 1e-7                                       # below eps, non-zero
    x[6] = x[6] / x[6].norm() * 1.5e-5                                     # just above eps
    g = rnd(9, 48, seed=2)
    xa, xb = x.clone().requires_grad_(True), R.leaf(x)
    ya = F.normalize(xa, dim=-1, eps=1e-5)
    ya.backward(g)
    yb = R.rownorm(xb, 1e-5)
    yb.backward(g)
    close(yb, ya)
    close(xb.grad, xa.grad)
    assert torch.equal(xb.grad[2], g[2] / 1e-5) and torch.equal(xb.grad[4], g[4] / 1e-5)     # dx = dy / eps under the clamp


@pytest.mark.parametrize("per,lse,hard,pool", [(1, False, False, 20), (1, False, True, 3), (2, True, False, 20), (3, False, True, 1),
                                               (5, True, True, 20), (2, False, True, 100)])
def test_video_rank_losses_reference(per, lse, hard, pool):
    N, L, D = 7, 13, 32
    M = N * per
    qn, cn = rnd(M, D, seed=1), rnd(N, L, D, seed=2)                      # get_video_level_scores normalises them itself
    mask = torch.ones(N, L, dtype=torch.float64)
    mask[1, 5:] = 0
    mask[4, 9:] = 0
    head = _Head(training=False, gather_gpus=False, use_all_neg=True, ranking_loss_type="lse" if lse else "hinge", margin=0.1,
                 use_hard_negative=hard, hard_pool_size=pool, hard_neg_weight=10.0)
    qa, ca = qn.clone().requires_grad_(True), cn.clone().requires_grad_(True)
    q2v_a = head.get_video_level_scores(qa, ca, mask, val_gather_gpus=False)
    la = head.get_video_level_loss(q2v_a, "mean")
    (1.7 * la[0] - 0.6 * la[1]).backward()
    qb, cb = R.leaf(qn), R.leaf(cn)
    lc, lq, q2v_b, arg, s = R.video_rank_losses(R.rownorm(qb, 1e-5), R.rownorm(cb, 1e-5), mask, per, 0.1, lse, hard, pool, 10.0)
    (1.7 * lc - 0.6 * lq).backward()
    # tie-free inputs: the two formulations cannot differ by a choice
    v = R.mask_logits(s.detach(), mask.unsqueeze(0))
    top2 = v.topk(2, dim=-1)[0]
    assert float((top2[..., 0] - top2[..., 1]).min()) > 0
    assert q2v_b.detach().unique().numel() == q2v_b.numel()
    close(q2v_b, q2v_a)
    close(lc, la[0])
    close(lq, la[1])
    close(qb.grad, qa.grad)
    close(cb.grad, ca.grad)


@pytest.mark.parametrize("per,lse,hard,pool", [(1, False, True, 3), (5, True, True, 2)])
def test_rank_losses_reference_against_the_sorted_formulation(per, lse, hard, pool):
    """...and against torch_rank_losses of tests/test_gpu_head.py (a sort; the reference counts), on a given score matrix."""
    from tests.test_gpu_head import torch_rank_losses
    nv = 9
    q2v = rnd(nv * per, nv, seed=5, scale=0.3)
    a = q2v.clone().requires_grad_(True)
    la = torch_rank_losses(a, per, 0.1, lse, hard, pool, 10.0)
    (la[0] + 2 * la[1]).backward()
    b = R.leaf(q2v)
    lb = R.rank_losses(b, per, 0.1, lse, hard, pool, 10.0)
    (lb[0] + 2 * lb[1]).backward()
    close(lb[0], la[0])
    close(lb[1], la[1])
    close(b.grad, a.grad)


@pytest.mark.parametrize("K", [1, 5, 15])
def test_st_ed_reference(K):
    B, L, D = 6, 23, 32
    q2, ctx = rnd(B, D, seed=1, scale=0.3), rnd(B, L, D, seed=2)
    w_st, w_ed = rnd(1, 1, K, seed=3, scale=0.5), rnd(1, 1, K, seed=4, scale=0.5)
    mask = torch.ones(B, L, dtype=torch.float64)
    mask[2, 15:] = 0
    tg = torch.tensor([[0, 3], [5, 9], [2, 20], [-1, 4], [22, 22], [7, -1]])         # [2, 20]: a masked frame as target
    st_conv, ed_conv = nn.Conv1d(1, 1, K, padding=K // 2, bias=False).double(), nn.Conv1d(1, 1, K, padding=K // 2, bias=False).double()
    st_conv.weight.data.copy_(w_st)
    ed_conv.weight.data.copy_(w_ed)
    head = _Head(video_query_linear=nn.Identity(), video_st_predictor=st_conv, video_ed_predictor=ed_conv)
    qa, ca = q2.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    st, ed = head._get_st_ed_prob(qa, ca, mask)
    ref = F.cross_entropy(st, tg[:, 0], ignore_index=-1) + F.cross_entropy(ed, tg[:, 1], ignore_index=-1)
    (2.5 * ref).backward()
    qb, cb, wsb, web = R.leaf(q2), R.leaf(ctx), R.leaf(w_st), R.leaf(w_ed)
    out, _ = R.st_ed_loss(qb, cb, mask, wsb, web, tg)
    (2.5 * out).backward()
    close(out, ref)
    close(qb.grad, qa.grad)
    close(cb.grad, ca.grad)
    close(wsb.grad, st_conv.weight.grad)
    close(web.grad, ed_conv.weight.grad)


def test_tie_rules_on_a_hand_written_example():
    # max over frames: 4 frames x 3 videos for one query; -10000 where masked
    s = torch.tensor([[[1.0, 3.0, 3.0, 2.0],                               # tie between frames 1 and 2 -> 1
                       [5.0, 5.0, 9.0, 9.0],                               # frames 2, 3 masked: tie between 0 and 1 -> 0
                       [7.0, 8.0, 9.0, 6.0]]], dtype=torch.float64)        # fully masked: all -10000 -> 0
    mask = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0]], dtype=torch.float64)
    sl = s.clone().requires_grad_(True)
    out, arg = R.score_max(sl, mask)
    assert arg.tolist() == [[1, 0, 0]] and out.tolist() == [[3.0, 5.0, -10000.0]]
    out.sum().backward()
    want = torch.zeros(1, 3, 4, dtype=torch.float64)
    want[0, 0, 1] = 1
    want[0, 1, 0] = 1                                                      # the fully masked video: gradient times mask = 0
    assert torch.equal(sl.grad, want)
    # hard-negative rank of the valid entries of each row of a 4 x 3 matrix
    v = torch.tensor([[0.5, 0.2, 0.5], [0.1, 0.1, 0.1], [0.3, 0.9, 0.3], [0.4, 0.4, 0.7]], dtype=torch.float64)
    valid = torch.tensor([[1, 1, 1], [1, 1, 1], [1, 0, 1], [0, 1, 1]], dtype=torch.bool)
    r = R.stable_desc_rank(v, valid)
    assert r[0].tolist() == [0, 2, 1] and r[1].tolist() == [0, 1, 2]
    assert (r[2, 0], r[2, 2]) == (0, 1) and (r[3, 1], r[3, 2]) == (1, 0)
    # numpy's stable sort of the negated values is the same rule
    assert np.argsort(-v[0].numpy(), kind="stable").tolist() == [0, 2, 1]
    # through the loss: equal negatives, pool = 1: the FIRST of them is the hard one
    q2v = torch.tensor([[0.9, 0.5, 0.5], [0.2, 0.8, 0.2], [0.1, 0.1, 0.7]], dtype=torch.float64)
    # row 0: negatives 0.5 (hard, x 10) and 0.5 (easy, x 0.5); margin 0.6 keeps both hinges active
    rows_c, rows_q = R.rank_loss_rows(q2v, 1, 0.6, False, True, 1, 10.0, 0.5)
    h = 0.6 + 0.5 - 0.9
    assert abs(float(rows_c[0]) - (10.0 * h + 0.5 * h) / 2) < 1e-15
    b = R.leaf(q2v)
    R.rank_loss_rows(b, 1, 0.6, False, True, 1, 10.0, 0.5)[0][0].backward()
    assert b.grad[0].tolist() == [-(10.0 + 0.5) / 2, 10.0 / 2, 0.5 / 2]
