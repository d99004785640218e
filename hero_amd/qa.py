"""Autograd node of the video-QA head on the libhero_hip.so kernels hero_qa_pool_fwd / hero_qa_pool_bwd
(include/hero_hip.h "Video-QA head"; reference: model/videoQA.py:36-59).  hero_amd.model.videoQA.HeroForVideoQA uses it
inside the kernels' envelope; outside it, and as the comparison side of the parity tests, that module keeps the PyTorch
formulation."""
import torch

from . import _lib as L
from . import functional as HF

MAX_A, MAX_L, MAX_LT, MAX_D = 8, 256, 512, 1024         # hero_amd/csrc/qa_pool.hip


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()       # no copy when it already is fp32 and contiguous


def in_envelope(A, Lf, Lt, D):
    return 1 <= A <= MAX_A and 1 <= Lf <= MAX_L and Lf <= Lt <= MAX_LT and D % 4 == 0 and 4 <= D <= MAX_D


class QaPoolFn(torch.autograd.Function):
    """(seq [Nv * A, Lt, D], mask [Nv * A, L], w_qa [1, D], w_se [1, D], A, L) -> (qa_pooled [Nv, A, D], se_pooled [Nv, L, D]),
    both fp32.  The first L rows of every sequence are the frames of one answer copy of one video; they are read in place.
        qa_pooled[v, a] = sum_l softmax_l(mask_logits(<x, w_qa>))[v, a, l] x[v, a, l]
        se_pooled[v, l] = sum_a softmax_a(mask_logits(<x, w_se>))[v, a, l] x[v, a, l]
    The gradient of `seq` covers the whole buffer (zero rows behind the frames)."""

    @staticmethod
    def forward(ctx, seq, mask, w_qa, w_se, A, Lf):
        S, Lt, D = seq.shape
        if S % A or not in_envelope(A, Lf, Lt, D) or tuple(mask.shape) != (S, Lf):
            raise ValueError("QaPoolFn: seq %s, mask %s, A=%d, L=%d is outside the kernels' envelope (1 <= A <= %d, 1 <= L <= %d, "
                             "L <= Lt <= %d, D %% 4 == 0, D <= %d)" % (tuple(seq.shape), tuple(mask.shape), A, Lf, MAX_A, MAX_L, MAX_LT, MAX_D))
        Nv = S // A
        seq = seq.contiguous()
        L.ptr(seq)                                                                # a CPU tensor raises here, before anything is allocated
        mask = _f32c(mask)
        wq, ws = w_qa.detach().reshape(-1).contiguous(), w_se.detach().reshape(-1).contiguous()
        dev = seq.device
        qa = torch.empty((Nv, A, D), dtype=torch.float32, device=dev)
        se = torch.empty((Nv, Lf, D), dtype=torch.float32, device=dev)
        att = torch.empty((2, Nv, A, Lf), dtype=torch.float32, device=dev)       # att_qa (over l), att_se (over a)
        L.check(L.lib().hero_qa_pool_fwd(L.ptr(seq), L.ptr(mask), L.ptr(wq), L.ptr(ws), L.ptr(qa), L.ptr(se), L.ptr(att[0]), L.ptr(att[1]),
                                         Nv, A, Lf, Lt, D, L.dt(seq), L.stream()))
        ctx.save_for_backward(seq, mask, att)
        ctx.ws = (w_qa, w_se)
        ctx.dims = (Nv, A, Lf)
        HF._use(w_qa, w_se)
        return qa, se

    @staticmethod
    def backward(ctx, dqa, dse):
        seq, mask, att = ctx.saved_tensors
        w_qa, w_se = ctx.ws
        Nv, A, Lf = ctx.dims
        _, Lt, D = seq.shape
        dev = seq.device
        dx = torch.empty_like(seq)                                                # written whole by the kernel
        part = torch.empty((2, Nv, D), dtype=torch.float32, device=dev)           # per-video shares of dw, folded in a fixed order
        L.check(L.lib().hero_qa_pool_bwd(L.ptr(seq), L.ptr(mask), L.ptr(w_qa.detach().reshape(-1).contiguous()),
                                         L.ptr(w_se.detach().reshape(-1).contiguous()), L.ptr(att[0]), L.ptr(att[1]),
                                         L.ptr(_f32c(dqa)), L.ptr(_f32c(dse)), L.ptr(dx), L.ptr(part[0]), L.ptr(part[1]),
                                         Nv, A, Lf, Lt, D, L.dt(seq), L.stream()))
        return dx, None, HF.fold_param_shares(part[0], w_qa), HF.fold_param_shares(part[1], w_se), None, None
