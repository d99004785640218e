"""Float64 restatements of the captioning decoder's kernels (hero_amd/csrc/dec_attention.hip, the smoothed loss of
hero_amd/csrc/loss.hip), written from model/tvc.py's formulas and independent of the kernels' code: the two attentions with
ADDITIVE masks and optional dropout multipliers, the label-smoothed loss in both formulations, and their gradients (float64
autograd).  Also the counter-based dropout draw of hero_amd/csrc/common.h (DropCtx) in integer arithmetic, so that a run with
dropout can be restated exactly."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.dropout_hash import _M64, _mix32, _splitmix64

HEAD = 64
MASKED = -10000.0


def heads(x, N, L, H):
    """[N*L, H*64] or [N, L, H*64] -> [N, H, L, 64] float64 (cpu)."""
    return x.detach().double().cpu().reshape(N, L, H, HEAD).permute(0, 2, 1, 3)


def unheads(x):
    N, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(N * L, H * HEAD)


def attention(q, k, v, N, Lq, Lk, H, key_mask_add=None, causal=False, mult=None, dctx=None):
    """model/tvc.py:67-104 (and BertSelfAttention under tri_mask) in float64.  q [N*Lq, H*64], k / v [N*Lk, H*64],
    key_mask_add [N, Lk] additive, mult [N, H, Lq, Lk] dropout multipliers (0 or 1 / (1 - p)).
    -> {"ctx", "P"} and, with dctx [N*Lq, H*64], {"dq", "dk", "dv"} in the operands' row layout."""
    qh, kh, vh = (heads(t, N, L, H).requires_grad_(True) for t, L in ((q, Lq), (k, Lk), (v, Lk)))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(HEAD)
    if key_mask_add is not None:
        s = s + key_mask_add.detach().double().cpu().reshape(N, 1, 1, Lk)
    if causal:
        tri = torch.tril(torch.ones(Lq, Lk, dtype=torch.float64))
        s = s + ((1.0 - tri) * MASKED).reshape(1, 1, Lq, Lk)
    P = torch.softmax(s, dim=-1)
    Pd = P * mult.double().cpu() if mult is not None else P
    ctx = Pd @ vh
    out = {"ctx": unheads(ctx).detach(), "P": P.detach()}
    if dctx is not None:
        (ctx * heads(dctx, N, Lq, H)).sum().backward()
        out.update(dq=unheads(qh.grad), dk=unheads(kh.grad), dv=unheads(vh.grad))
    return out


def smooth_loss_closed(x, labels, eps, ignore_index=-1):
    """The closed form of include/hero_hip.h: per-row loss [rows] (0 for ignored rows), x [rows, C] float64."""
    x = x.double()
    C = x.shape[1]
    s, conf = eps / (C - 1), 1.0 - eps
    h0 = (conf * math.log(conf) if conf > 0 else 0.0) + (C - 1) * s * math.log(s)
    valid = labels != ignore_index
    lse = torch.logsumexp(x, dim=1)
    xt = x.gather(1, labels.clamp_min(0).unsqueeze(1)).squeeze(1)
    loss = h0 - (conf - s) * (xt - lse) - s * (x.sum(1) - C * lse)
    return torch.where(valid, loss, torch.zeros_like(loss))


def smooth_loss_kl(x, labels, eps, ignore_index=-1):
    """LabelSmoothingLoss.forward (model/tvc.py:42-64, reduction 'none') op for op, in x's dtype: the losses of the VALID rows."""
    C = x.shape[1]
    one_hot = torch.full((1, C), eps / (C - 1), dtype=x.dtype, device=x.device)
    valid = labels != ignore_index
    target = labels[valid]
    output = torch.log_softmax(x[valid], dim=-1)
    model_prob = one_hot.repeat(target.size(0), 1)
    model_prob.scatter_(1, target.unsqueeze(1), 1.0 - eps)
    return F.kl_div(output, model_prob, reduction="none").sum(dim=1)


def smooth_loss(x, labels, eps, ignore_index=-1, dloss_rows=None, mean=False, upstream=1.0):
    """Float64 losses and gradient of  upstream * sum_r dloss_rows[r] loss_r  (mean: / number of valid rows, 0 rows -> 0).
    -> {"loss" [rows], "sum", "count", "dx" [rows, C]}."""
    x = x.detach().double().cpu().requires_grad_(True)
    labels = labels.detach().cpu().long()
    loss = smooth_loss_closed(x, labels, eps, ignore_index)
    w = dloss_rows.detach().double().cpu() if dloss_rows is not None else torch.ones_like(loss)
    count = int((labels != ignore_index).sum())
    total = (loss * w).sum() * upstream
    if mean:
        total = total / max(count, 1)
    total.backward()
    return {"loss": loss.detach(), "sum": loss.detach().sum(), "count": count, "dx": x.grad}


# ---- the counter-based dropout draw (hero_amd/csrc/common.h: DropCtx::mask1; its two hashes are in tests/dropout_hash.py) ------
def dropout_multipliers(seed, site, threshold16, scale, N, H, Lq, Lk):
    """[N, H, Lq, Lk] multipliers of the dropout on P: element index ((n*H + h)*Lq + i) * round_up(Lk, 4) + j (< 2^34)."""
    base = _splitmix64((seed ^ ((site * 0xD6E8FEB86659FD93) & _M64)) & _M64)
    k0, k1 = base & 0xFFFFFFFF, base >> 32
    Lk4 = (Lk + 3) // 4 * 4
    rows = np.arange(N * H * Lq, dtype=np.uint64).reshape(-1, 1)
    elem = rows * np.uint64(Lk4) + np.arange(Lk, dtype=np.uint64).reshape(1, -1)
    assert int(elem.max()) < (1 << 34)
    key = np.where((elem & np.uint64(2)) != 0, np.uint64(k1), np.uint64(k0))
    r = _mix32(((elem >> np.uint64(2)) & np.uint64(0xFFFFFFFF)) ^ key)
    u = (r >> (np.uint64(16) * (elem & np.uint64(1)))) & np.uint64(0xFFFF)
    keep = u >= np.uint64(threshold16)
    return torch.from_numpy(np.where(keep, scale, 0.0)).reshape(N, H, Lq, Lk)


# ---- the decoder of model/tvc.py:107-266 from a dict of parameters, float64 ------------------------------------------------------
def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _lin(P, name, x):
    return x @ P[name + ".weight"].T + P[name + ".bias"]


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def decoder_scores(P, enc_out, enc_mask, caption_ids, pos_ids, n_layers, H, ln_eps=1e-5, layer_eps=1e-12):
    """prediction_scores (N, Lt, vocab) of HeroForTvc.decode from the parameters P (name -> tensor, any float dtype), the
    encoder outputs (N, Lv, D) and their 0/1 mask, through `attention` above."""
    P = {k: v.double() for k, v in P.items() if v.is_floating_point()}
    N, Lt = caption_ids.shape
    Lv = enc_out.shape[1]
    emb = "v_encoder.f_encoder.embeddings.word_embeddings.weight"
    x = _ln(P[emb][caption_ids] + P["position_embeddings.weight"][pos_ids], P["emb_LayerNorm.weight"], P["emb_LayerNorm.bias"], ln_eps)
    enc = enc_out.double().reshape(N * Lv, -1)
    mask_add = (1.0 - enc_mask.double()) * MASKED
    x = x.reshape(N * Lt, -1)
    for i in range(n_layers):
        pre = "decoder.layer.%d." % i
        q, k, v = (_lin(P, pre + "self_attention." + n, x) for n in ("query", "key", "value"))
        a = attention(q, k, v, N, Lt, Lt, H, causal=True)["ctx"]
        a = _ln(_lin(P, pre + "add_norm_1.dense", a) + x, P[pre + "add_norm_1.LayerNorm.weight"], P[pre + "add_norm_1.LayerNorm.bias"], layer_eps)
        q = _lin(P, pre + "dec_enc_attention.query", a)
        k, v = (_lin(P, pre + "dec_enc_attention." + n, enc) for n in ("key", "value"))
        c = attention(q, k, v, N, Lt, Lv, H, key_mask_add=mask_add)["ctx"]
        c = _ln(_lin(P, pre + "add_norm_2.dense", c) + a, P[pre + "add_norm_2.LayerNorm.weight"], P[pre + "add_norm_2.LayerNorm.bias"], layer_eps)
        h = _lin(P, pre + "add_norm_3.dense", _gelu(_lin(P, pre + "intermidiate.dense", c)))
        x = _ln(h + c, P[pre + "add_norm_3.LayerNorm.weight"], P[pre + "add_norm_3.LayerNorm.bias"], layer_eps)
    head = "v_encoder.f_encoder.lm_head."
    h = _ln(_gelu(_lin(P, head + "dense", x)), P[head + "LayerNorm.weight"], P[head + "LayerNorm.bias"], ln_eps)
    return (h @ P[emb].T + P[head + "bias"]).reshape(N, Lt, -1)
