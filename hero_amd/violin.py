"""Autograd nodes, meter and validation loop of the VIOLIN head on the libhero_hip.so kernels hero_frame_pool_fwd / _bwd and
hero_bce_head_fwd / _bwd (include/hero_hip.h "VIOLIN head"; reference: model/violin.py:30-47, 73-81 and
eval_violin.py:118-164).  hero_amd.model.violin.HeroForViolin uses them inside the kernels' envelopes; outside them, and as
the comparison side of the parity tests, that module keeps the PyTorch formulation."""
import time

import torch
from torch.nn import functional as F

from . import _lib as L
from . import functional as HF

MAX_L, MAX_LT, MAX_D, MAX_K = 256, 512, 1024, 2048         # hero_amd/csrc/pool.hip (FP_MAX_*), hero_amd/csrc/violin.hip (BCE_MAX_K)


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()       # no copy when it already is fp32 and contiguous


def _flat(w):
    return w.detach().reshape(-1).contiguous()


def pool_in_envelope(Lf, Lt, D):
    return 1 <= Lf <= MAX_L and Lf <= Lt <= MAX_LT and D % 4 == 0 and 4 <= D <= MAX_D


def head_in_envelope(S, K):
    return S >= 1 and K % 4 == 0 and 4 <= K <= MAX_K


class FramePoolFn(torch.autograd.Function):
    """(seq [S, Lt, D], mask [S, L], w [1, D], L) -> pooled [S, D] fp32.  The first L rows of every sequence are the frames
    of one (video, statement) copy; they are read in place.
        pooled[s] = sum_l softmax_l(mask_logits(<x, w>))[s, l] x[s, l]
    The gradient of `seq` covers the whole buffer (zero rows behind the frames)."""

    in_envelope = staticmethod(pool_in_envelope)

    @staticmethod
    def forward(ctx, seq, mask, w, Lf):
        S, Lt, D = seq.shape
        if not pool_in_envelope(Lf, Lt, D) or tuple(mask.shape) != (S, Lf) or w.numel() != D:
            raise ValueError("FramePoolFn: seq %s, mask %s, L=%d is outside the kernels' envelope (1 <= L <= %d, L <= Lt <= %d, "
                             "D %% 4 == 0, 4 <= D <= %d)" % (tuple(seq.shape), tuple(mask.shape), Lf, MAX_L, MAX_LT, MAX_D))
        seq = seq.contiguous()
        L.ptr(seq)                                                                # a CPU tensor raises here, before anything is allocated
        mask = _f32c(mask)
        pooled = torch.empty((S, D), dtype=torch.float32, device=seq.device)
        att = torch.empty((S, Lf), dtype=torch.float32, device=seq.device)
        L.check(L.lib().hero_frame_pool_fwd(L.ptr(seq), L.ptr(mask), L.ptr(_flat(w)), L.ptr(pooled), L.ptr(att),
                                            S, Lf, Lt, D, L.dt(seq), L.stream()))
        ctx.save_for_backward(seq, mask, att)
        ctx.w = w
        ctx.Lf = Lf
        HF._use(w)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        seq, mask, att = ctx.saved_tensors
        w, Lf = ctx.w, ctx.Lf
        S, Lt, D = seq.shape
        dx = torch.empty_like(seq)                                                # written whole by the kernel
        part = torch.empty((S, D), dtype=torch.float32, device=seq.device)        # per-sequence shares of dw, folded in a fixed order
        L.check(L.lib().hero_frame_pool_bwd(L.ptr(seq), L.ptr(mask), L.ptr(_flat(w)), L.ptr(att), L.ptr(_f32c(dpooled)), L.ptr(dx),
                                            L.ptr(part), S, Lf, Lt, D, L.dt(seq), L.stream()))
        return dx, None, HF.fold_param_shares(part, w), None


class BceHeadFn(torch.autograd.Function):
    """(h [S, K], w2 [1, K], b2 [1], targets [S] int64 0/1) -> (loss [], logits [S]), both fp32:
        logits = h w2^T + b2,  loss = mean_s min(softplus(-+logits_s), 100)
    i.e. linear_2 -> sigmoid -> binary_cross_entropy of model/violin.py:73-81 in its stable form.  `logits` is the
    prediction output: no gradient flows through it, the gradient of `h`, `w2`, `b2` is the loss's."""

    in_envelope = staticmethod(head_in_envelope)

    @staticmethod
    def forward(ctx, h, w2, b2, targets):
        S, K = h.shape
        if not head_in_envelope(S, K) or w2.numel() != K or b2.numel() != 1 or tuple(targets.shape) != (S,):
            raise ValueError("BceHeadFn: h %s, w2 %s, b2 %s, targets %s is outside the kernels' envelope (S >= 1, K %% 4 == 0, "
                             "4 <= K <= %d)" % (tuple(h.shape), tuple(w2.shape), tuple(b2.shape), tuple(targets.shape), MAX_K))
        h = h.contiguous()
        L.ptr(h)                                                                  # a CPU tensor raises here, before anything is allocated
        targets = targets.to(torch.int64).contiguous()
        out = torch.empty((S + 1,), dtype=torch.float32, device=h.device)         # logits, loss
        logits, loss = out[:S], out[S:]
        L.check(L.lib().hero_bce_head_fwd(L.ptr(h), L.ptr(_flat(w2)), L.ptr(_flat(b2)), L.ptr(targets), L.ptr(logits), L.ptr(loss),
                                          None, S, K, L.dt(h), L.stream()))
        ctx.save_for_backward(h, logits, targets)
        ctx.wb = (w2, b2)
        ctx.mark_non_differentiable(logits)
        HF._use(w2, b2)
        return loss.view(()), logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        h, logits, targets = ctx.saved_tensors
        w2, b2 = ctx.wb
        S, K = h.shape
        dh = torch.empty_like(h)
        dwb = torch.empty((K + 4,), dtype=torch.float32, device=h.device)         # dw [K], db [1] (16-byte aligned behind it)
        dw, db = dwb[:K], dwb[K:K + 1]
        L.check(L.lib().hero_bce_head_bwd(L.ptr(h), L.ptr(_flat(w2)), L.ptr(logits), L.ptr(targets), L.ptr(_f32c(dloss).view(1)),
                                          L.ptr(dh), L.ptr(dw), L.ptr(db), S, K, L.dt(h), L.stream()))
        gw = HF.fold_param_shares(dw.view(1, K), w2)
        if HF._is_param(b2):                                                      # one float: hero_colsum takes widths that are multiples of 4
            HF.SINK.dst(b2).view(-1).add_(db)
            HF.SINK.done(b2)
            gb = None
        else:
            gb = db.view_as(b2) if b2.requires_grad else None
        return dh, gw, gb, None


class ViolinMeter:
    """Running loss and accuracy of eval_violin.py:validate_violin on the device: every update() adds
    (sum of the loss terms, number of right predictions, number of examples) into one float[3] through the `acc` argument of
    hero_bce_head_fwd; nothing is read back before compute()."""

    def __init__(self, device="cuda"):
        self.acc = torch.zeros(3, dtype=torch.float32, device=device)
        self._unit = None

    def update(self, *args):
        """update(logits [S] or [S, 1], targets)  or  update(h [S, K], w2, b2, targets): the classifier tail runs with `acc`."""
        if len(args) == 2:
            logits, targets = args
            L.ptr(logits)
            h = F.pad(_f32c(logits).reshape(-1, 1), (0, 3))                       # <(z, 0, 0, 0), (1, 0, 0, 0)> + 0 is z exactly
            if self._unit is None:
                self._unit = (torch.tensor([1.0, 0.0, 0.0, 0.0], device=h.device), torch.zeros(1, device=h.device))
            w2, b2 = self._unit
        else:
            h, w2, b2, targets = args
            L.ptr(h)
            h, w2, b2 = h.detach().contiguous(), _flat(w2), _flat(b2)
        S, K = h.shape
        if not head_in_envelope(S, K):
            raise ValueError("ViolinMeter.update: h %s is outside the kernel's envelope" % (tuple(h.shape),))
        targets = targets.reshape(-1).to(torch.int64).contiguous()
        out = torch.empty((S + 1,), dtype=torch.float32, device=h.device)
        L.check(L.lib().hero_bce_head_fwd(L.ptr(h), L.ptr(w2), L.ptr(b2), L.ptr(targets), L.ptr(out[:S]), L.ptr(out[S:]),
                                          L.ptr(self.acc), S, K, L.dt(h), L.stream()))
        return out[:S]

    def update_host(self, logits, targets):
        """The same sums in PyTorch ops, as eval_violin.py:136-150 computes them (sigmoid -> binary_cross_entropy(sum),
        sigmoid > 0.5): the route of CPU tensors, and the comparison side of the tests."""
        logits, targets = logits.detach().float().reshape(-1), targets.reshape(-1)
        scores = torch.sigmoid(logits)
        loss = F.binary_cross_entropy(scores, targets.to(scores.dtype), reduction="sum")
        right = ((scores > 0.5).long() == targets).sum()
        self.acc += torch.stack([loss, right.to(loss.dtype), loss.new_tensor(float(logits.numel()))]).to(self.acc.device)

    def compute(self):
        a = self.acc.tolist()                                                     # the one synchronisation
        n = max(a[2], 1.0)
        return {"loss": a[0] / n, "acc": a[1] / n}


@torch.no_grad()
def validate_violin(model, loader, split="val"):
    """eval_violin.py:118-164 without its per-batch `.item()`s: returns (val_log, results) with results[qid] = 0 | 1.  One
    device-to-host copy per batch - the predictions `results` is made of; loss and accuracy stay on the device until the end."""
    model.eval()
    meter, results, n_ex, st = None, {}, 0, time.time()
    for batch in loader:
        batch = dict(batch)
        qids = batch.pop("qids")
        logits = model(batch, "violin", compute_loss=False)                       # (S, 1)
        if meter is None:
            meter = ViolinMeter(logits.device)
        if logits.is_cuda:
            meter.update(logits, batch["targets"])
        else:
            meter.update_host(logits, batch["targets"])
        answers = (logits.reshape(-1) > 0).long().cpu().tolist()                  # sigmoid(z) > 0.5
        results.update((str(q), a) for q, a in zip(qids, answers))
        n_ex += len(qids)
    m = meter.compute() if meter is not None else {"loss": 0.0, "acc": 0.0}
    val_log = {"valid/%s_loss" % split: m["loss"], "valid/%s_acc" % split: m["acc"],
               "valid/%s_ex_per_s" % split: n_ex / max(time.time() - st, 1e-9)}
    return val_log, results
