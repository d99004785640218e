"""Autograd nodes of the captioning decoder (TVC) on the libhero_hip.so kernels hero_dec_attention_fwd / _bwd and
hero_smooth_ce_fwd / _bwd (include/hero_hip.h "Decoder attention", "Label-smoothed loss"; reference: model/tvc.py:19-154), and the
inference-only kernels of its incremental and beam-search decode.

    DecAttnCoreFn     the attention kernel on projected operands: a fused [N*L, 3*H*64] Q|K|V buffer (causal self-attention) or a
                      [N*Lq, H*64] query and a [N*Lk, 2*H*64] K|V buffer (decoder-encoder attention, key mask per caption)
    DecAttentionFn    the same with its projections: BertSelfAttention under tri_mask / BertDecEncAttention of a decoder layer
    SmoothCeFn        LabelSmoothingLoss in closed form: per-row losses plus the device pair (sum, number of valid rows)
    k_dec_attn_row / k_dec_attn_step   the one-query-row kernels of incremental decoding (no autograd: inference only) - attention
                      over the encoder keys, and causal self-attention against a key/value cache that the kernel extends;
                      `group=` / `anc=` are their beam-search forms (shared encoder keys, a cache read through an ancestry table)
    k_beam_select     the selection step of beam search over [N * B, vocab] scores (hero_beam_select), in place on device tables
    k_sample_select   the sampling step (temperature, top-k, top-p, Gumbel-max draw) over [N * S, vocab] scores
                      (hero_sample_select), in place on the same tables

There is no PyTorch route in here: outside the kernels' envelope the nodes raise."""
import ctypes as C
import math

import torch

from . import _lib as L
from . import functional as HF

MAX_LQ, MAX_LK, HEAD = 64, 128, 64                     # hero_amd/csrc/dec_attention.hip


def in_envelope(dtype, Lq, Lk):
    """The library's own answer (hero_dec_attention_in_envelope) for a torch dtype and the two sequence lengths."""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    return bool(L.lib().hero_dec_attention_in_envelope(L.F32 if dtype == torch.float32 else L.BF16, int(Lq), int(Lk)))


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def _operands(qbuf, kvbuf, H):
    """(q, k, v pointers, ldq, ldkv) of the two operand forms; kvbuf None = one fused Q|K|V buffer."""
    D, es = H * HEAD, qbuf.element_size()
    if kvbuf is None:
        if qbuf.shape[1] != 3 * D:
            raise ValueError("decoder attention: fused operand must be [rows, 3 * H * 64], got %s" % (tuple(qbuf.shape),))
        p = L.ptr(qbuf)
        return p, p + D * es, p + 2 * D * es, 3 * D, 3 * D
    if qbuf.shape[1] != D or kvbuf.shape[1] != 2 * D or kvbuf.dtype != qbuf.dtype:
        raise ValueError("decoder attention: operands must be [rows, H * 64] and [rows, 2 * H * 64] of one dtype, got %s %s"
                         % (tuple(qbuf.shape), tuple(kvbuf.shape)))
    p = L.ptr(kvbuf)
    return L.ptr(qbuf), p, p + D * es, D, 2 * D


def _drop_ref(drop):
    return C.byref(drop) if drop is not None else None


def k_dec_attn_fwd(qbuf, kvbuf, key_mask_add, N, Lq, Lk, H, causal, drop=None):
    """-> (ctx [N*Lq, H*64] in the operands' dtype, stats [N, H, Lq, 2] fp32)."""
    if not in_envelope(qbuf.dtype, Lq, Lk):
        raise ValueError("decoder attention: %s, Lq=%d, Lk=%d is outside the kernels' envelope (fp32 / bf16, 1 <= Lq <= %d, "
                         "1 <= Lk <= %d)" % (qbuf.dtype, Lq, Lk, MAX_LQ, MAX_LK))
    q, k, v, ldq, ldkv = _operands(qbuf, kvbuf, H)
    if qbuf.shape[0] != N * Lq or (kvbuf is not None and kvbuf.shape[0] != N * Lk) or (kvbuf is None and Lq != Lk):
        raise ValueError("decoder attention: operand rows do not match N=%d Lq=%d Lk=%d" % (N, Lq, Lk))
    if key_mask_add is not None and tuple(key_mask_add.shape) != (N, Lk):
        raise ValueError("decoder attention: key mask must be [N, Lk], got %s" % (tuple(key_mask_add.shape),))
    ctxt = torch.empty((N * Lq, H * HEAD), dtype=qbuf.dtype, device=qbuf.device)
    stats = torch.empty((N, H, Lq, 2), dtype=torch.float32, device=qbuf.device)
    L.check(L.lib().hero_dec_attention_fwd(q, k, v, L.ptr(key_mask_add), L.ptr(ctxt), L.ptr(stats), N, Lq, Lk, H, ldq, ldkv,
                                           1 if causal else 0, 1.0 / math.sqrt(HEAD), L.dt(qbuf), _drop_ref(drop), L.stream()))
    return ctxt, stats


def k_dec_attn_bwd(qbuf, kvbuf, key_mask_add, stats, dctx, N, Lq, Lk, H, causal, drop=None):
    """-> (dqbuf, dkvbuf) shaped like the operands (dkvbuf None in the fused form); every element is written by the kernel."""
    q, k, v, ldq, ldkv = _operands(qbuf, kvbuf, H)
    dqbuf = torch.empty_like(qbuf)
    dkvbuf = torch.empty_like(kvbuf) if kvbuf is not None else None
    dq, dk, dv, _, _ = _operands(dqbuf, dkvbuf, H)
    L.check(L.lib().hero_dec_attention_bwd(q, k, v, L.ptr(key_mask_add), L.ptr(stats), L.ptr(dctx), dq, dk, dv, N, Lq, Lk, H, ldq, ldkv,
                                           1 if causal else 0, 1.0 / math.sqrt(HEAD), L.dt(qbuf), _drop_ref(drop), L.stream()))
    return dqbuf, dkvbuf


def in_envelope_row(dtype, Lk):
    """The library's own answer (hero_dec_attention_row_in_envelope): the one-row kernels take 1 <= Lk (or cache rows) <= 128."""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    return bool(L.lib().hero_dec_attention_row_in_envelope(L.F32 if dtype == torch.float32 else L.BF16, int(Lk)))


def _row_operand(name, t, rows, cols, dtype=None):
    if t.dim() != 2 or tuple(t.shape) != (rows, cols) or (dtype is not None and t.dtype != dtype):
        raise ValueError("decoder attention: %s must be [%d, %d]%s, got %s %s"
                         % (name, rows, cols, " of %s" % dtype if dtype is not None else "", tuple(t.shape), t.dtype))


def k_dec_attn_row(q, kv, key_mask_add, N, Lk, H, group=1):
    """Decoder-encoder attention of ONE decoder position per caption (inference: no dropout, no stats):
    q [N, H*64], kv [N*Lk, 2*H*64] the packed K|V projection of the encoder rows, key_mask_add [N, Lk] fp32 | None
    -> ctx [N, H*64] in the operands' dtype.
    group > 1 (the beams of a caption): row r reads block r // group of kv [N//group * Lk, 2*H*64] and of the mask
    [N//group, Lk] - the encoder K|V are not replicated."""
    if N < 1 or not in_envelope_row(q.dtype, Lk):
        raise ValueError("decoder attention: %s, N=%d, Lk=%d is outside the one-row kernel's envelope (fp32 / bf16, N >= 1, "
                         "1 <= Lk <= %d)" % (q.dtype, N, Lk, MAX_LK))
    if group < 1 or N % group:
        raise ValueError("decoder attention: N=%d rows are no whole number of groups of %d" % (N, group))
    D, es, nb = H * HEAD, q.element_size(), N // group
    _row_operand("q", q, N, D)
    _row_operand("kv", kv, nb * Lk, 2 * D, q.dtype)
    if key_mask_add is not None and (tuple(key_mask_add.shape) != (nb, Lk) or key_mask_add.dtype != torch.float32):
        raise ValueError("decoder attention: key mask must be fp32 [%d, Lk], got %s %s" % (nb, tuple(key_mask_add.shape), key_mask_add.dtype))
    ctxt = torch.empty((N, D), dtype=q.dtype, device=q.device)
    p = L.ptr(kv)
    if group == 1:
        L.check(L.lib().hero_dec_attention_row(L.ptr(q), p, p + D * es, L.ptr(key_mask_add), L.ptr(ctxt), N, Lk, H, D, 2 * D,
                                               1.0 / math.sqrt(HEAD), L.dt(q), L.stream()))
    else:
        L.check(L.lib().hero_dec_attention_row_grouped(L.ptr(q), p, p + D * es, L.ptr(key_mask_add), L.ptr(ctxt), N, group, Lk, H, D,
                                                       2 * D, 1.0 / math.sqrt(HEAD), L.dt(q), L.stream()))
    return ctxt


def _pos_args(what, pos, pos_offset, Tcap, device):
    """The position of a step as the kernels take it, (pos_dev, pos_host): a 1-element int32 device tensor is read by the kernel
    and `pos_offset` added to it there; an int is checked here and passed with the offset already added."""
    if torch.is_tensor(pos):
        if pos.numel() != 1 or pos.dtype != torch.int32 or pos.device != device:
            raise ValueError("%s: a device position must be one int32 on %s, got %s %s on %s"
                             % (what, device, tuple(pos.shape), pos.dtype, pos.device))
        return L.ptr(pos), int(pos_offset)
    pos_host = int(pos) + int(pos_offset)
    if not 0 <= pos_host < Tcap:
        raise ValueError("%s: position %d outside [0, Tcap = %d)" % (what, pos_host, Tcap))
    return None, pos_host


def k_dec_attn_step(qkv, cache, pos, N, H, anc=None):
    """Causal self-attention of position `pos` against a key/value cache (inference):
    qkv [N, 3*H*64] this step's packed Q|K|V rows, cache [N, Tcap, 2*H*64] with K|V of the positions < pos; the kernel also
    writes this step's K|V into cache[:, pos].  pos: an int, or a 1-element int32 device tensor (read by the kernel, so that a
    captured launch serves every step; a value outside [0, Tcap) leaves the cache alone and gives zeros).
    anc [N, Tcap] int32 (beam search): key / value j < pos of row r come from cache row anc[r, j] - the cache is never reordered.
    -> ctx [N, H*64]."""
    D = H * HEAD
    if cache.dim() != 3:
        raise ValueError("decoder attention: the cache must be [N, Tcap, 2 * H * 64], got %s" % (tuple(cache.shape),))
    Tcap = cache.shape[1]
    if N < 1 or not in_envelope_row(qkv.dtype, Tcap):
        raise ValueError("decoder attention: %s, N=%d, Tcap=%d is outside the one-row kernel's envelope (fp32 / bf16, N >= 1, "
                         "1 <= Tcap <= %d)" % (qkv.dtype, N, Tcap, MAX_LK))
    _row_operand("qkv", qkv, N, 3 * D)
    if tuple(cache.shape) != (N, Tcap, 2 * D) or cache.dtype != qkv.dtype:
        raise ValueError("decoder attention: the cache must be [%d, Tcap, %d] of %s, got %s %s"
                         % (N, 2 * D, qkv.dtype, tuple(cache.shape), cache.dtype))
    pos_dev, pos_host = _pos_args("decoder attention", pos, 0, Tcap, qkv.device)
    ctxt = torch.empty((N, D), dtype=qkv.dtype, device=qkv.device)
    if anc is None:
        L.check(L.lib().hero_dec_attention_step(L.ptr(qkv), L.ptr(cache), L.ptr(ctxt), pos_dev, pos_host, N, Tcap, H,
                                                1.0 / math.sqrt(HEAD), L.dt(qkv), L.stream()))
        return ctxt
    _beam_table("anc", anc, (N, Tcap), torch.int32, qkv.device)
    L.check(L.lib().hero_dec_attention_step_beam(L.ptr(qkv), L.ptr(cache), L.ptr(anc), L.ptr(ctxt), pos_dev, pos_host, N, Tcap, H,
                                                 1.0 / math.sqrt(HEAD), L.dt(qkv), L.stream()))
    return ctxt


MAX_BEAM, MAX_BEAM_V = 8, 65536                        # hero_amd/csrc/beam.hip


def in_envelope_beam(dtype, V, B, Tcap):
    """The library's own answer (hero_beam_in_envelope): fp32 / bf16, 1 <= B <= 8, B <= V <= 65536, 1 <= Tcap <= 128."""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    return bool(L.lib().hero_beam_in_envelope(L.F32 if dtype == torch.float32 else L.BF16, int(V), int(B), int(Tcap)))


def _beam_table(name, t, shape, dtype, device):
    if tuple(t.shape) != shape or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError("beam search: %s must be a contiguous %s %s on %s, got %s %s on %s"
                         % (name, dtype, shape, device, tuple(t.shape), t.dtype, t.device))


def _score_rows(what, logits, R, ids):
    """The scores of a selection step, [R, >= V] with rows `ld` apart (they may be the first V columns of a wider buffer: the
    padded vocabulary) -> (ld, Tcap of the id table)."""
    if logits.dim() != 2 or logits.shape[0] != R or logits.stride(1) != 1:
        raise ValueError("%s: the scores must be [%d, >= V] with unit column stride, got %s" % (what, R, tuple(logits.shape)))
    return logits.stride(0), ids.shape[1] if ids.dim() == 2 else 0


def _cols_in_range(logits, ld, V, eos):
    """The vocabulary fits the score rows and holds `eos` (part of each kernel's envelope, refused in its words)."""
    return ld >= V and logits.shape[1] >= V and 0 <= eos < V


def _select_tables(R, Tcap, dev, cum, rows, mats):
    """The tables a selection step updates: cum [R] fp32, `rows` [R] and `mats` [R, Tcap] int32, as (name, tensor) pairs."""
    _beam_table("cum", cum, (R,), torch.float32, dev)
    for name, t in rows:
        _beam_table(name, t, (R,), torch.int32, dev)
    for name, t in mats:
        _beam_table(name, t, (R, Tcap), torch.int32, dev)


def k_beam_select(logits, cum, fin, length, ids, anc, last, workspace, pos, N, B, V, eos, pos_offset=0):
    """One selection step of beam search for N captions x B beams (row r = n*B + b), in place and on the device
    (include/hero_hip.h "Beam-search selection"): logits [R, ld >= V] fp32 / bf16; cum [R] fp32; fin, length, last [R] and
    ids, anc [R, Tcap] int32; workspace: at least R*B int64.  pos: the step's position as an int, or a 1-element int32 device
    tensor to which `pos_offset` is added (-1 when the counter has already advanced)."""
    R = N * B
    (ld, Tcap), dev = _score_rows("beam search", logits, R, ids), logits.device
    if not in_envelope_beam(logits.dtype, V, B, Tcap) or N < 1 or not _cols_in_range(logits, ld, V, eos):
        raise ValueError("beam search: %s, N=%d, B=%d, V=%d, ld=%d, Tcap=%d, eos=%d is outside the selection kernel's envelope (fp32 / "
                         "bf16, 1 <= B <= %d, B <= V <= %d, 1 <= Tcap <= %d, ld >= V, 0 <= eos < V)"
                         % (logits.dtype, N, B, V, ld, Tcap, eos, MAX_BEAM, MAX_BEAM_V, MAX_LK))
    _select_tables(R, Tcap, dev, cum, (("fin", fin), ("len", length), ("last", last)), (("ids", ids), ("anc", anc)))
    if workspace.dtype != torch.int64 or workspace.numel() < R * B or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("beam search: the workspace must be at least %d contiguous int64 on %s" % (R * B, dev))
    pos_dev, pos_host = _pos_args("beam search", pos, pos_offset, Tcap, dev)
    L.check(L.lib().hero_beam_select(logits.data_ptr(), L.ptr(cum), L.ptr(fin), L.ptr(length), L.ptr(ids), L.ptr(anc), L.ptr(last),
                                     L.ptr(workspace), pos_dev, pos_host, N, B, V, ld, Tcap, eos, L.dt(logits), L.stream()))


def in_envelope_sample(dtype, V, Tcap):
    """The library's own answer (hero_sample_in_envelope): fp32 / bf16, 1 <= V <= 65536, 1 <= Tcap <= 128."""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    return bool(L.lib().hero_sample_in_envelope(L.F32 if dtype == torch.float32 else L.BF16, int(V), int(Tcap)))


def inv_temperature(temperature):
    """The fp32 multiplier 1 / temperature that both routes of the sampling step apply to the logits."""
    return float(torch.tensor(1.0 / float(temperature), dtype=torch.float32))


def k_sample_select(logits, cum, fin, length, ids, last, kept, seed, pos, N, S, V, eos, temperature, top_k, top_p, pos_offset=0):
    """One sampling step for N captions x S samples (row r = n*S + s), in place and on the device (include/hero_hip.h "Sampled
    decoding"): logits [R, ld >= V] fp32 / bf16; cum [R] fp32; fin, length, last [R] and ids [R, Tcap] int32; kept [R] int32 or
    None (the size of every row's kept set); seed: a 1-element int64 device tensor whose 64 bits are the seed word.  pos: the
    step's position as an int, or a 1-element int32 device tensor to which `pos_offset` is added.  temperature > 0, top_k >= 0
    (0 = off), top_p > 0 (>= 1 = off)."""
    R = N * S
    (ld, Tcap), dev = _score_rows("sampling", logits, R, ids), logits.device
    if not temperature > 0 or not math.isfinite(temperature) or top_k < 0 or not top_p > 0:
        raise ValueError("sampling: temperature %r, top_k %r, top_p %r: temperature must be finite and > 0, top_k >= 0, top_p > 0"
                         % (temperature, top_k, top_p))
    if not in_envelope_sample(logits.dtype, V, Tcap) or N < 1 or S < 1 or not _cols_in_range(logits, ld, V, eos):
        raise ValueError("sampling: %s, N=%d, S=%d, V=%d, ld=%d, Tcap=%d, eos=%d is outside the sampling kernel's envelope (fp32 / "
                         "bf16, N, S >= 1, 1 <= V <= %d, 1 <= Tcap <= %d, ld >= V, 0 <= eos < V)"
                         % (logits.dtype, N, S, V, ld, Tcap, eos, MAX_BEAM_V, MAX_LK))
    _select_tables(R, Tcap, dev, cum, (("fin", fin), ("len", length), ("last", last)) + ((("kept", kept),) if kept is not None else ()),
                   (("ids", ids),))
    if not torch.is_tensor(seed) or seed.numel() != 1 or seed.dtype != torch.int64 or seed.device != dev:
        raise ValueError("sampling: the seed must be one int64 on %s" % (dev,))
    pos_dev, pos_host = _pos_args("sampling", pos, pos_offset, Tcap, dev)
    L.check(L.lib().hero_sample_select(logits.data_ptr(), L.ptr(cum), L.ptr(fin), L.ptr(length), L.ptr(ids), L.ptr(last), L.ptr(kept),
                                       L.ptr(seed), pos_dev, pos_host, N, S, V, ld, Tcap, eos, inv_temperature(temperature),
                                       int(top_k), float(top_p), L.dt(logits), L.stream()))


class DecAttnCoreFn(torch.autograd.Function):
    """(qbuf, kvbuf | None, key_mask_add [N, Lk] | None, N, Lq, Lk, H, causal, drop) -> ctx [N*Lq, H*64]."""

    @staticmethod
    def forward(ctx, qbuf, kvbuf, key_mask_add, N, Lq, Lk, H, causal, drop):
        qbuf = qbuf.contiguous()
        kvbuf = kvbuf.contiguous() if kvbuf is not None else None
        mask = _f32c(key_mask_add) if key_mask_add is not None else None
        out, stats = k_dec_attn_fwd(qbuf, kvbuf, mask, N, Lq, Lk, H, causal, drop)
        ctx.save_for_backward(qbuf, kvbuf, mask, stats)
        ctx.meta = (N, Lq, Lk, H, causal, drop)
        return out

    @staticmethod
    def backward(ctx, dctx):
        qbuf, kvbuf, mask, stats = ctx.saved_tensors
        N, Lq, Lk, H, causal, drop = ctx.meta
        dq, dkv = k_dec_attn_bwd(qbuf, kvbuf, mask, stats, dctx.contiguous().to(qbuf.dtype), N, Lq, Lk, H, causal, drop)
        return (dq, dkv) + (None,) * 7


class DecAttentionFn(torch.autograd.Function):
    """One attention of a decoder layer with its projections, ctx = MHA(x | enc):
        enc None   BertSelfAttention under the causal mask: one packed QKV GEMM on x [N, Lq, D], the kernel with causal = 1
        enc given  BertDecEncAttention: the Q GEMM on x, one packed K|V GEMM on enc [N, Lk, D], the kernel with the caption's
                   additive key mask [N, Lk]
    Weight and bias gradients go to the gradient sink, as in SelfAttentionFn."""

    @staticmethod
    def forward(ctx, x, enc, key_mask_add, H, drop, wq, bq, wk, bk, wv, bv):
        N, Lq, D = x.shape
        x2 = HF._as2d(x)
        cross = enc is not None
        if cross:
            Lk = enc.shape[1]
            e2 = HF._as2d(enc)
            qbuf = HF.k_linear(x2, HF.packed((wq,), x2.dtype), HF.packed((bq,), torch.float32))
            kvbuf = HF.k_linear(e2, HF.packed((wk, wv), e2.dtype), HF.packed((bk, bv), torch.float32))
            wt = (HF.packed_t((wq,), x2.dtype), HF.packed_t((wk, wv), x2.dtype))
            mask = _f32c(key_mask_add) if key_mask_add is not None else None
        else:
            Lk, e2, kvbuf, mask = Lq, None, None, None
            qbuf = HF.k_linear(x2, HF.packed((wq, wk, wv), x2.dtype), HF.packed((bq, bk, bv), torch.float32))
            wt = (HF.packed_t((wq, wk, wv), x2.dtype), None)
        out, stats = k_dec_attn_fwd(qbuf, kvbuf, mask, N, Lq, Lk, H, not cross, drop)
        ctx.meta = (N, Lq, Lk, H, D, cross, drop)
        ctx.params = (wq, bq, wk, bk, wv, bv)
        HF._use(*ctx.params)
        ctx.save_for_backward(x2, e2, qbuf, kvbuf, mask, stats, wt[0], wt[1])
        return out.view(N, Lq, D)

    @staticmethod
    def backward(ctx, dctx):
        x2, e2, qbuf, kvbuf, mask, stats, wt_q, wt_kv = ctx.saved_tensors
        N, Lq, Lk, H, D, cross, drop = ctx.meta
        wq, bq, wk, bk, wv, bv = ctx.params
        dq, dkv = k_dec_attn_bwd(qbuf, kvbuf, mask, stats, HF._as2d(dctx), N, Lq, Lk, H, not cross, drop)
        dx = HF.k_dgrad_t(dq, wt_q).view(N, Lq, D) if ctx.needs_input_grad[0] else None
        denc = None
        if cross:
            if ctx.needs_input_grad[1]:
                denc = HF.k_dgrad_t(dkv, wt_kv).view(N, Lk, D)
            HF.acc_linear_grads(dq, x2, wq, bq)
            HF.acc_linear_grads(dkv, e2, wk, bk, col0=0, ncols=D)
            HF.acc_linear_grads(dkv, e2, wv, bv, col0=D, ncols=D)
        else:
            HF._qkv_bwd(dq, x2, ctx.params, D)
        return (dx, denc) + (None,) * 9


class SmoothCeFn(torch.autograd.Function):
    """(logits [rows, ld], labels [rows], ncols, eps, ignore_index) -> (loss [rows] fp32, sum_cnt [2] fp32):
        loss_r   the KL divergence of softmax(logits[r, :ncols]) to the smoothed one-hot of labels[r] (0 for ignored rows)
        sum_cnt  (sum_r loss_r, number of valid rows), folded on the device in a fixed order
    The gradient of `sum_cnt[0]` and of `loss` reach the logits in ONE pass; both upstream gradients are read on the device."""

    @staticmethod
    def forward(ctx, logits, labels, ncols, eps, ignore_index):
        x2 = logits.contiguous()
        rows, ld = x2.shape
        lab = labels.contiguous().to(torch.int64)
        loss, lse = (torch.empty((rows,), dtype=torch.float32, device=x2.device) for _ in range(2))
        sum_cnt = torch.empty((2,), dtype=torch.float32, device=x2.device)
        L.check(L.lib().hero_smooth_ce_fwd(L.ptr(x2), L.ptr(lab), L.ptr(loss), L.ptr(lse), L.ptr(sum_cnt), rows, ncols, ld, L.dt(x2),
                                           float(eps), int(ignore_index), L.stream()))
        ctx.save_for_backward(x2, lab, lse)
        ctx.meta = (ncols, float(eps), int(ignore_index))
        return loss, sum_cnt

    @staticmethod
    def backward(ctx, dloss, dsum_cnt):
        x2, lab, lse = ctx.saved_tensors
        ncols, eps, ignore_index = ctx.meta
        rows, ld = x2.shape
        # d / d logits = (dloss[r] + dsum_cnt[0]) * d loss_r: one factor per row, the scalar upstream of the kernel is 1
        g = (_f32c(dloss) + _f32c(dsum_cnt)[0]).contiguous()
        one = torch.ones((1,), dtype=torch.float32, device=x2.device)
        dx = torch.empty_like(x2)
        L.check(L.lib().hero_smooth_ce_bwd(L.ptr(x2), L.ptr(lab), L.ptr(lse), L.ptr(one), L.ptr(g), None, L.ptr(dx), rows, ncols, ld,
                                           L.dt(x2), eps, ignore_index, L.stream()))
        return dx, None, None, None, None


class SmoothCeMeanFn(torch.autograd.Function):
    """(logits, labels, ncols, eps, ignore_index) -> the mean of the smoothed loss over the valid rows, a 0-d fp32 tensor (0 when
    no row is valid).  The valid count never leaves the device: forward divides by it there and backward reads it from the
    forward's pair, so the node can be captured into a hipGraph.  The gradient overwrites nothing the caller still owns: it is a
    new tensor unless `inplace`, which hands the logits' storage to the gradient (for logits nothing else reads)."""

    @staticmethod
    def forward(ctx, logits, labels, ncols, eps, ignore_index, inplace):
        x2 = logits.contiguous()
        rows, ld = x2.shape
        lab = labels.contiguous().to(torch.int64)
        loss, lse = (torch.empty((rows,), dtype=torch.float32, device=x2.device) for _ in range(2))
        sum_cnt = torch.empty((2,), dtype=torch.float32, device=x2.device)
        L.check(L.lib().hero_smooth_ce_fwd(L.ptr(x2), L.ptr(lab), L.ptr(loss), L.ptr(lse), L.ptr(sum_cnt), rows, ncols, ld, L.dt(x2),
                                           float(eps), int(ignore_index), L.stream()))
        ctx.save_for_backward(x2, lab, lse, sum_cnt)
        ctx.meta = (ncols, float(eps), int(ignore_index), bool(inplace))
        return sum_cnt[0] / sum_cnt[1].clamp_min(1.0)

    @staticmethod
    def backward(ctx, dmean):
        x2, lab, lse, sum_cnt = ctx.saved_tensors
        ncols, eps, ignore_index, inplace = ctx.meta
        rows, ld = x2.shape
        dx = x2 if inplace else torch.empty_like(x2)
        L.check(L.lib().hero_smooth_ce_bwd(L.ptr(x2), L.ptr(lab), L.ptr(lse), L.ptr(_f32c(dmean).view(1)), None, L.ptr(sum_cnt),
                                           L.ptr(dx), rows, ncols, ld, L.dt(x2), eps, ignore_index, L.stream()))
        return dx, None, None, None, None, None


def smooth_ce(logits, labels, eps, ncols=None, ignore_index=-1):
    """Per-row smoothed losses [rows] and the device pair (their sum, the number of valid rows)."""
    return SmoothCeFn.apply(logits, labels, logits.shape[1] if ncols is None else ncols, eps, ignore_index)


def smooth_ce_mean(logits, labels, eps, ncols=None, ignore_index=-1, inplace=False):
    return SmoothCeMeanFn.apply(logits, labels, logits.shape[1] if ncols is None else ncols, eps, ignore_index, inplace)
