"""HERO for video captioning, TVC (reference: model/tvc.py).

The hierarchical encoder produces the frame representations of every video; the frames of each caption's segment are
gathered into a zero-padded [Ncap, Lv, D] tensor, and a BERT decoder (causal self-attention, attention over the segment's
frames, feed-forward; the reference's module names, `intermidiate` included) predicts the caption's tokens through the
word-embedding table it shares with the encoder.  Both attentions run on one HIP kernel family
(hero_amd.tvc.DecAttentionFn) and the label-smoothed loss over the vocabulary is one kernel each way
(hero_amd.tvc.SmoothCeFn): no [rows, vocab] target matrix, no [N, H, Lq, Lk] probability tensor."""
import gc
import math

import torch
from torch import nn
from torch.nn import functional as F

from .. import functional as HF
from .. import tvc as T
from .layers import BertIntermediate, BertLayerNorm, BertOutput, BertSelfAttention, BertSelfOutput, _drop
from .model import HeroModel


class BertDecEncAttention(BertSelfAttention):
    """model/tvc.py:67-104: query from the decoder states, key / value from the encoder outputs (parameter holder; the
    decoder layer runs it through hero_amd.tvc.DecAttentionFn or the PyTorch formulation)."""


def _attention_torch(att, x, kv, mask_add, drop_p, training):
    """BertSelfAttention / BertDecEncAttention.forward of the reference, op for op.  mask_add broadcasts over the scores."""
    H = att.num_attention_heads

    def split(t):
        return t.view(t.shape[0], t.shape[1], H, att.attention_head_size).permute(0, 2, 1, 3)
    q, k, v = split(att.query(x)), split(att.key(kv)), split(att.value(kv))
    scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(att.attention_head_size)
    if mask_add is not None:
        scores = scores + mask_add
    probs = F.dropout(torch.softmax(scores, dim=-1), drop_p, training)
    ctx = torch.matmul(probs, v).permute(0, 2, 1, 3).contiguous()
    return ctx.view(ctx.shape[0], ctx.shape[1], att.all_head_size)


def _add_norm_torch(mod, hidden, residual):
    """BertSelfOutput / BertOutput.forward of the reference."""
    h = F.dropout(mod.dense(hidden), mod.dropout.p, mod.training)
    ln = mod.LayerNorm
    return F.layer_norm(h + residual, ln.normalized_shape, ln.weight, ln.bias, ln.eps)


def _attend_torch(att, q, k, v, mask_add):
    """The attention of `_attention_torch` on PROJECTED operands (q [N, Lq, D], k / v [N, Lk, D]) and without dropout: what an
    incremental decode step runs against the keys and values it has kept."""
    H = att.num_attention_heads

    def split(t):
        return t.view(t.shape[0], t.shape[1], H, att.attention_head_size).permute(0, 2, 1, 3)
    scores = torch.matmul(split(q), split(k).transpose(-1, -2)) / math.sqrt(att.attention_head_size)
    if mask_add is not None:
        scores = scores + mask_add
    ctx = torch.matmul(torch.softmax(scores, dim=-1), split(v)).permute(0, 2, 1, 3).contiguous()
    return ctx.view(ctx.shape[0], ctx.shape[1], att.all_head_size)


class TvcDecodeState(object):
    """What an incremental decode keeps between its steps (HeroForTvc.init_decode_state / decode_step), per decoder layer:
        fused    cross_kv [N*Lv, 2D] the packed K|V projection of the encoder rows, computed ONCE; cache [N, max_step, 2D] the
                 K|V of the decoded positions, extended by the step kernel; mask_add [N, Lv] fp32; pos (one device int32, the
                 position of the next step - the kernels and the embedding read it on the device) with pid = pos per caption and
                 wid, the int32 word ids of the step
        PyTorch  cross_k / cross_v [N, Lv, D], self_k / self_v [N, t, D] grown by concatenation, mask_add [N, 1, 1, Lv], t
    Every buffer keeps its address for the life of the state, so one captured step serves all steps and, after `refill`, all
    batches of the same shape.

    Beam search (beam > 1) decodes rows = N * beam rows, row n * beam + b = beam b of caption n.  The encoder side stays N
    blocks on both routes (cross_kv / cross_k / cross_v, mask_add): the rows of a caption share them.  Fused: cache
    [rows, max_step, 2D] is NEVER reordered - a row's K|V stay where the step kernel wrote them and the attention follows the
    beam's ancestry through `anc`; PyTorch: self_k / self_v [rows, t, D] are re-gathered by parent after every selection
    (HeroForTvc.reorder_decode_state).  `tables` (a BeamTables, when asked for) holds what hero_beam_select updates."""

    def __init__(self, fused, N, Lv, max_step, beam=1):
        self.fused, self.N, self.Lv, self.max_step, self.t = fused, N, Lv, max_step, 0
        self.beam, self.rows, self.tables = beam, N * beam, None
        self.cross_kv, self.cache, self.cross_k, self.cross_v, self.self_k, self.self_v = [], [], [], [], [], []
        self.mask_add = self.pos = self.pid = self.wid = None

    @property
    def anc(self):
        """The ancestry table the step kernel reads; None with one beam per caption (every row reads its own cache row)."""
        return self.tables.anc if self.beam > 1 else None


class BeamTables(object):
    """The tables of a beam search over rows = N * B decode rows (include/hero_hip.h "Beam-search selection"): cum [rows] fp32
    the summed log-probabilities, fin / len [rows] finished flag and token count, ids / anc [rows, max_step] the tokens and
    the cache row of every decoded position, ws the selection kernel's workspace, kept [rows] what a sampled decode reports.
    int32 on the kernels' route (the kernel's types), int64 indices in PyTorch ops."""
    DEAD = -1.0e30          # the initial score of the beams 1 .. B-1: below every real candidate of beam 0

    def __init__(self, N, B, max_step, device, fused):
        R, it = N * B, torch.int32 if fused else torch.long
        self.N, self.B = N, B
        self.cum = torch.empty((R,), dtype=torch.float32, device=device)
        self.fin, self.len = (torch.empty((R,), dtype=it, device=device) for _ in range(2))
        self.kept = torch.zeros((R,), dtype=it, device=device)      # sampling: the size of every row's kept set at the last step
        self.ids, self.anc = (torch.empty((R, max_step), dtype=it, device=device) for _ in range(2))
        self.ws = torch.empty((R * B,), dtype=torch.int64, device=device) if fused else None
        self._cum0 = torch.full((N, B), self.DEAD, dtype=torch.float32, device=device)
        self._cum0[:, 0] = 0.0
        self._anc0 = torch.arange(R, dtype=it, device=device).unsqueeze(1).expand(R, max_step).contiguous()

    def reset(self, sampling=False):
        """The start of a beam search, or of a SAMPLED decode (include/hero_hip.h "Sampled decoding"): there the rows of a caption
        are independent samples, so every row starts alive at cum = 0 and the ancestry stays the identity for the whole decode."""
        if sampling:
            self.cum.zero_()
        else:
            self.cum.copy_(self._cum0.view(-1))
        self.fin.zero_()
        self.len.zero_()
        self.ids.zero_()
        self.anc.copy_(self._anc0)
        return self

    def reset_sampling(self):
        return self.reset(sampling=True)


def beam_select_torch(scores, tb, t, eos):
    """hero_beam_select in PyTorch ops on a BeamTables of int64 indices: scores [rows, V] -> the parent ROW of every new beam
    (the tables are replaced, not updated in place).  fp32 throughout; a stable descending sort gives the tie rule (among
    equal scores the lower flat index b * V + v)."""
    N, B, V = tb.N, tb.B, scores.shape[1]
    x = scores.float()
    cand = tb.cum.unsqueeze(1) + (x - torch.logsumexp(x, dim=1, keepdim=True))
    done = tb.fin.bool().unsqueeze(1)
    only_eos = torch.full_like(cand, float("-inf"))
    only_eos[:, eos] = tb.cum
    cand = torch.where(done, only_eos, cand).view(N, B * V)
    val, idx = torch.sort(cand, dim=1, descending=True, stable=True)
    val, idx = val[:, :B].reshape(-1), idx[:, :B]
    rows = (torch.arange(N, device=x.device).unsqueeze(1) * B + idx // V).reshape(-1)
    v = (idx % V).reshape(-1)
    was_done = tb.fin[rows]
    tb.cum = val
    tb.fin = was_done | (v == eos).to(was_done.dtype)
    tb.len = tb.len[rows] + (1 - was_done)
    tb.ids, tb.anc = tb.ids[rows], tb.anc[rows]
    tb.ids[:, t] = v
    tb.anc[:, t] = rows
    return rows, v


_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _mul32(x, c):
    """(x * c) mod 2^32 for an int64 tensor of 32-bit values, without leaving 63 bits."""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & 0xFFFFFFFF


def gumbel_noise(seed, t, R, V, device):
    """g [R, V] fp32 of hero_sample_select at position t: the hashes of hero_amd/csrc/common.h in int64 arithmetic,
    u = (2h + 1) * 2^-24 exactly, g = -log(-log1p(-u)) in fp32."""
    keys = [_splitmix64((int(seed) & _M64) ^ (((t * R + r) * 0xD6E8FEB86659FD93) & _M64)) & 0xFFFFFFFF for r in range(R)]
    x = torch.arange(V, dtype=torch.long, device=device).unsqueeze(0) ^ torch.tensor(keys, dtype=torch.long, device=device).unsqueeze(1)
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    x = x ^ (x >> 16)
    u = (2 * (x >> 9) + 1).to(torch.float32) * (2.0 ** -24)
    return -torch.log(-torch.log1p(-u))


def sample_select_torch(scores, tb, t, eos, seed, temperature, top_k, top_p):
    """hero_sample_select in PyTorch ops on a BeamTables of int64 indices, updated in place: scores [rows, V] -> (the token of
    every row [rows], the size of every row's kept set [rows]).  Ordering, noise and the perturbed scores are fp32 as in the
    kernel - a stable descending sort gives the tie rule - and the nucleus masses are summed in float64; top_p counts as the
    fp32 value the kernel receives."""
    x = scores.float()
    R, V = x.shape
    dev = x.device
    z = x * T.inv_temperature(temperature)
    zs, order = torch.sort(z, dim=1, descending=True, stable=True)
    K = min(int(top_k), V) if top_k > 0 else V
    J = torch.full((R,), K, dtype=torch.long, device=dev)
    p32 = float(torch.tensor(float(top_p), dtype=torch.float32))
    if p32 < 1.0:
        csum = torch.cumsum(torch.exp(zs[:, :K].double() - zs[:, :1].double()), dim=1)
        J = ((csum < p32 * csum[:, -1:]).sum(dim=1) + 1).clamp(max=K)
    col = torch.arange(V, device=dev).unsqueeze(0)
    pert = zs + gumbel_noise(seed, t, R, V, dev).gather(1, order)
    pert = torch.where(col < J.unsqueeze(1), pert, torch.full_like(pert, float("-inf")))
    best = pert.max(dim=1, keepdim=True).values
    v = torch.where(pert == best, order, torch.full_like(order, V)).min(dim=1).values          # among equals the lower token
    live = tb.fin == 0
    logp = x.gather(1, v.unsqueeze(1)).squeeze(1) - torch.logsumexp(x, dim=1)
    tokens = torch.where(live, v, torch.full_like(v, eos))
    tb.cum = torch.where(live, tb.cum + logp, tb.cum)
    tb.len = tb.len + live.to(tb.len.dtype)
    tb.fin = torch.where(live, (v == eos).to(tb.fin.dtype), tb.fin)
    tb.ids[:, t] = tokens.to(tb.ids.dtype)
    tb.kept = torch.where(live, J, torch.zeros_like(J))
    return tokens, tb.kept


class BertDecoderLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.self_attention = BertSelfAttention(config)
        self.add_norm_1 = BertSelfOutput(config)
        self.dec_enc_attention = BertDecEncAttention(config)
        self.add_norm_2 = BertSelfOutput(config)
        self.intermidiate = BertIntermediate(config)
        self.add_norm_3 = BertOutput(config)

    def forward(self, dec_hidden_states, enc_outputs, enc_mask_add):
        """Fused: dec_hidden_states (N, Lt, D) and enc_outputs (N, Lv, D) in the compute dtype, enc_mask_add (N, Lv) fp32."""
        sa, ca, dev = self.self_attention, self.dec_enc_attention, dec_hidden_states.device
        a = T.DecAttentionFn.apply(dec_hidden_states, None, None, sa.num_attention_heads, _drop(sa.dropout, dev), *sa.qkv_params())
        a = self.add_norm_1(a, dec_hidden_states)
        c = T.DecAttentionFn.apply(a, enc_outputs, enc_mask_add, ca.num_attention_heads, _drop(ca.dropout, dev), *ca.qkv_params())
        c = self.add_norm_2(c, a)
        o = self.add_norm_3
        return HF.FfnBlockFn.apply(c, o.LayerNorm.eps, _drop(o.dropout, dev), self.intermidiate.dense.weight,
                                   self.intermidiate.dense.bias, o.dense.weight, o.dense.bias, o.LayerNorm.weight, o.LayerNorm.bias)

    def forward_torch(self, dec_hidden_states, enc_outputs, enc_mask, tri_mask):
        """model/tvc.py:118-154 in PyTorch ops; enc_mask (N, 1, 1, Lv) and tri_mask (1, 1, Lt, Lt) additive."""
        sa, ca = self.self_attention, self.dec_enc_attention
        a = _attention_torch(sa, dec_hidden_states, dec_hidden_states, tri_mask, sa.dropout.p, self.training)
        a = _add_norm_torch(self.add_norm_1, a, dec_hidden_states)
        c = _attention_torch(ca, a, enc_outputs, enc_mask, ca.dropout.p, self.training)
        c = _add_norm_torch(self.add_norm_2, c, a)
        h = F.gelu(self.intermidiate.dense(c))
        return _add_norm_torch(self.add_norm_3, h, c)

    def cross_kv(self, enc2):
        """The packed K|V projection [N*Lv, 2D] of the encoder rows: the same GEMM DecAttentionFn runs, once per decode."""
        ca = self.dec_enc_attention
        return HF.k_linear(enc2, HF.packed((ca.key.weight, ca.value.weight), enc2.dtype),
                           HF.packed((ca.key.bias, ca.value.bias), torch.float32))

    def step(self, x, state, li):
        """One decoded position per caption on the one-row kernels: x [N, D] in the compute dtype -> [N, D].  Inference only."""
        sa, ca = self.self_attention, self.dec_enc_attention
        wq, bq, wk, bk, wv, bv = sa.qkv_params()
        qkv = HF.k_linear(x, HF.packed((wq, wk, wv), x.dtype), HF.packed((bq, bk, bv), torch.float32))
        a = T.k_dec_attn_step(qkv, state.cache[li], state.pos, state.rows, sa.num_attention_heads, anc=state.anc)
        a = self.add_norm_1(a, x)
        q = HF.k_linear(a, HF.packed((ca.query.weight,), a.dtype), HF.packed((ca.query.bias,), torch.float32))
        c = T.k_dec_attn_row(q, state.cross_kv[li], state.mask_add, state.rows, state.Lv, ca.num_attention_heads, group=state.beam)
        c = self.add_norm_2(c, a)
        o = self.add_norm_3
        return HF.FfnBlockFn.apply(c, o.LayerNorm.eps, _drop(o.dropout, x.device), self.intermidiate.dense.weight,
                                   self.intermidiate.dense.bias, o.dense.weight, o.dense.bias, o.LayerNorm.weight, o.LayerNorm.bias)

    def step_torch(self, x, state, li):
        """The same step in PyTorch ops: x [N, 1, D]; the layer's keys / values grow by concatenation, so no tri_mask."""
        sa, ca = self.self_attention, self.dec_enc_attention
        k, v = sa.key(x), sa.value(x)
        if state.t:
            k, v = torch.cat([state.self_k[li], k], dim=1), torch.cat([state.self_v[li], v], dim=1)
        state.self_k[li], state.self_v[li] = k, v
        a = _add_norm_torch(self.add_norm_1, _attend_torch(sa, sa.query(x), k, v, None), x)
        # the beams of a caption are the query rows of ONE attention over the caption's encoder keys: [N, beam, D]
        q = ca.query(a).view(state.N, state.beam, -1)
        c = _attend_torch(ca, q, state.cross_k[li], state.cross_v[li], state.mask_add).view(state.rows, 1, -1)
        c = _add_norm_torch(self.add_norm_2, c, a)
        h = F.gelu(self.intermidiate.dense(c))
        return _add_norm_torch(self.add_norm_3, h, c)


class BertDecoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.layer = nn.ModuleList([BertDecoderLayer(config) for _ in range(config.num_hidden_layers)])
        tri_mask = torch.tril(torch.ones(1024, 1024), diagonal=0)
        self.register_buffer("tri_mask", (1.0 - tri_mask) * -10000.0)          # in the reference's state dict

    def forward(self, dec_hidden_states, enc_outputs, enc_mask_add):
        for layer in self.layer:
            dec_hidden_states = layer(dec_hidden_states, enc_outputs, enc_mask_add)
        return dec_hidden_states

    def forward_torch(self, dec_hidden_states, enc_outputs, enc_mask):
        len_ = dec_hidden_states.size(1)
        tri_mask = self.tri_mask[:len_, :len_].unsqueeze(0).unsqueeze(1).to(dec_hidden_states)
        enc_mask = (1.0 - enc_mask.unsqueeze(1).unsqueeze(2).to(dec_hidden_states)) * -10000.0
        for layer in self.layer:
            dec_hidden_states = layer.forward_torch(dec_hidden_states, enc_outputs, enc_mask, tri_mask)
        return dec_hidden_states


def smooth_loss_torch(output, target, eps, vocab_size, ignore_index=-1):
    """LabelSmoothingLoss.forward (model/tvc.py:42-64), reduction 'none': the losses of the valid rows."""
    valid = target != ignore_index
    target = target[valid]
    output = torch.log_softmax(output[valid], dim=-1)
    model_prob = torch.full((1, vocab_size), eps / (vocab_size - 1), dtype=output.dtype, device=output.device).repeat(target.size(0), 1)
    model_prob.scatter_(1, target.unsqueeze(1), 1.0 - eps)
    return F.kl_div(output, model_prob, reduction="none").sum(dim=1)


class LabelSmoothingLoss(nn.Module):
    """model/tvc.py:19-64.  Keeps the reference's `one_hot` buffer (1, vocab) because it is in the reference's state dict; the
    fused path never expands it to (rows, vocab) - hero_smooth_ce_* use the closed form."""

    def __init__(self, label_smoothing, tgt_vocab_size, ignore_index=-100, reduction="none"):
        assert 0.0 < label_smoothing <= 1.0
        super().__init__()
        self.ignore_index, self.reduction = ignore_index, reduction
        self.register_buffer("one_hot", torch.full((1, tgt_vocab_size), label_smoothing / (tgt_vocab_size - 1)))
        self.label_smoothing, self.confidence = label_smoothing, 1.0 - label_smoothing

    def forward(self, output, target):
        loss = smooth_loss_torch(output, target, self.label_smoothing, output.shape[-1], self.ignore_index)
        return loss.mean() if self.reduction == "mean" else loss.sum() if self.reduction == "sum" else loss


class HeroForTvc(HeroModel):
    def __init__(self, config, vfeat_dim, max_frm_seq_len, lsr=0.1):
        super().__init__(config, vfeat_dim, max_frm_seq_len)
        self.config = config
        d = config.d_config
        if d is None:
            raise ValueError("HeroForTvc: the model config has no d_config (config/hero_tvc.json)")
        if d.hidden_size != config.f_config.hidden_size:
            raise ValueError("HeroForTvc: the decoder shares the encoder's word embedding, hidden sizes must agree")
        self.position_embeddings = nn.Embedding(d.max_position_embeddings, d.hidden_size)
        self.emb_LayerNorm = BertLayerNorm(d.hidden_size, eps=1e-5)
        self.decoder = BertDecoder(d)
        if not 0.0 <= lsr <= 1.0:
            raise ValueError("HeroForTvc: label smoothing must be in [0, 1]")
        self.lsr = float(lsr)
        if lsr > 0:
            self.loss_func = LabelSmoothingLoss(lsr, config.f_config.vocab_size, ignore_index=-1, reduction="none")
        else:
            self.loss_func = nn.CrossEntropyLoss(ignore_index=-1, reduction="none")
        self._cap_index = {}
        self.v_encoder.initialize()

    fused_decoder = True    # decoder attentions and the smoothed loss on the HIP kernels (hero_dec_attention_*, hero_smooth_ce_*);
                            # False / shapes outside their envelope / CPU tensors: the PyTorch formulation below
    max_lq, max_lk = T.MAX_LQ, T.MAX_LK       # Python-side limits of the fused route (never above the kernels' envelope)

    # ---- encoder side --------------------------------------------------------------------------------------------------
    def _cap_frame_index(self, batch, n_frames, device):
        """Flat row of the (B * n_frames) frame representations behind every position of the padded segments, -1 = pad:
        the batch's own device tensor `cap_frame_index` (hero_amd.collate.tvc_collate) or built from `clip_ranges` once."""
        idx = batch.get("cap_frame_index") if hasattr(batch, "get") else None
        if idx is not None:
            return idx
        ranges = batch["clip_ranges"]
        key = (id(ranges), n_frames, str(device))
        hit = self._cap_index.get(key)
        if hit is None or hit[0] is not ranges:
            from ..collate import tvc_frame_index
            if len(self._cap_index) > 64:
                self._cap_index.clear()
            hit = (ranges, tvc_frame_index(ranges, n_frames).to(device))
            self._cap_index[key] = hit
        return hit[1]

    def encode(self, batch):
        """(Ncap, Lv, D): frame_embeddings[i, st:ed] of every caption, zero-padded (model/tvc.py:219-238)."""
        frame_embeddings = self.v_encoder(batch, "repr")
        B, NF, D = frame_embeddings.shape
        idx = self._cap_frame_index(batch, NF, frame_embeddings.device)
        n_cap, Lv = idx.shape
        if not frame_embeddings.is_cuda:
            flat = F.pad(frame_embeddings.reshape(B * NF, D), (0, 0, 0, 1))      # row -1: zeros
            return flat[idx.reshape(-1).long()].view(n_cap, Lv, D)
        return HF.ExpandRowsFn.apply(frame_embeddings.reshape(B * NF, D), idx).view(n_cap, Lv, D)

    # ---- decoder side --------------------------------------------------------------------------------------------------
    def _fused(self, encoder_outputs, caption_ids):
        f_enc = self.v_encoder.f_encoder
        if f_enc.vocab_pad:
            raise ValueError("HeroForTvc: the vocabulary (%d) is not a multiple of 8; the reference's own "
                             ".view(-1, vocab_size) of the padded prediction scores fails there too"
                             % self.config.f_config.vocab_size)
        Lt, Lv = caption_ids.shape[1], encoder_outputs.shape[1]
        return (self.fused_decoder and encoder_outputs.is_cuda and Lt <= self.max_lq and Lv <= self.max_lk and Lt <= self.max_lk
                and T.in_envelope(HF.compute_dtype(), Lt, Lv) and T.in_envelope(HF.compute_dtype(), Lt, Lt))

    def _decoder_states(self, encoder_outputs, encoder_masks, caption_ids, pos_ids, fused):
        emb = self.v_encoder.f_encoder.embeddings
        N, Lt = caption_ids.shape
        if fused:
            from .embed import _row_index
            wid, pid = _row_index(caption_ids, N, Lt), _row_index(pos_ids, N, Lt)
            x = HF.embed_ln(None, self.emb_LayerNorm.weight, self.emb_LayerNorm.bias, self.emb_LayerNorm.eps, None,
                            HF.compute_dtype(), tables=(emb.word_embeddings.weight, self.position_embeddings.weight),
                            idxs=(wid, pid), skip_idx=(emb.padding_idx, -1)).view(N, Lt, -1)
            enc = HF.cast(encoder_outputs, HF.compute_dtype())
            return self.decoder(x, enc, HF.as_mask_add(encoder_masks, N, encoder_outputs.shape[1]))
        x = emb.word_embeddings(caption_ids) + self.position_embeddings(pos_ids)
        ln = self.emb_LayerNorm
        x = F.layer_norm(x, ln.normalized_shape, ln.weight, ln.bias, ln.eps)
        return self.decoder.forward_torch(x, encoder_outputs.to(x.dtype), encoder_masks)

    def _scores_torch(self, states):
        """BertLMPredictionHead.forward of the reference in PyTorch ops (the tied projection)."""
        head = self.v_encoder.f_encoder.lm_head
        h = F.gelu(head.dense(states))
        h = F.layer_norm(h, head.LayerNorm.normalized_shape, head.LayerNorm.weight, head.LayerNorm.bias, head.LayerNorm.eps)
        return F.linear(h, head.decoder.weight, head.bias)

    def decode(self, encoder_outputs, encoder_masks, caption_ids, pos_ids, label_ids, compute_loss=True):
        """model/tvc.py:240-266.  With compute_loss the reference's loss VECTOR: the smoothed losses of the valid positions
        (boolean compaction: not capturable) or, with lsr == 0, plain cross-entropy over ALL positions with zeros at the ignored
        ones - the reference's `.mean()` therefore divides by different counts in the two modes."""
        fused = self._fused(encoder_outputs, caption_ids)
        states = self._decoder_states(encoder_outputs, encoder_masks, caption_ids, pos_ids, fused)
        V = self.config.f_config.vocab_size
        if not fused:
            scores = self._scores_torch(states)
            if not compute_loss:
                return scores
            flat, labels = scores.view(-1, V), label_ids.reshape(-1)
            return self.loss_func(flat, labels)
        head = self.v_encoder.f_encoder.lm_head
        if not compute_loss:
            return head(states).view(states.shape[0], states.shape[1], V)
        logits, labels = head(states.reshape(-1, states.shape[-1]), raw=True), label_ids.reshape(-1)
        if self.lsr > 0:
            rows, _ = T.smooth_ce(logits, labels, self.lsr, ncols=V, ignore_index=-1)
            return rows[labels != -1]
        return HF.cross_entropy(logits, labels, ncols=V, ignore_index=-1)

    # ---- incremental decoding ------------------------------------------------------------------------------------------
    max_cache = T.MAX_LK    # Python-side limit on max_step of the cached route (never above the one-row kernels' envelope)

    def _fused_step(self, encoder_outputs, max_step):
        if self.v_encoder.f_encoder.vocab_pad:
            raise ValueError("HeroForTvc: the vocabulary (%d) is not a multiple of 8" % self.config.f_config.vocab_size)
        Lv = encoder_outputs.shape[1]
        return (self.fused_decoder and encoder_outputs.is_cuda and max_step <= self.max_cache and Lv <= self.max_lk
                and T.in_envelope_row(HF.compute_dtype(), max_step) and T.in_envelope_row(HF.compute_dtype(), Lv))

    max_beam = T.MAX_BEAM   # Python-side limit on the beam size of the kernels' route (never above hero_beam_select's envelope)

    @torch.no_grad()
    def init_decode_state(self, encoder_outputs, encoder_masks, max_step, beam_size=1, beam_tables=False):
        """The state of an incremental decode of up to `max_step` positions over encoder_outputs [N, Lv, D] and their 0/1 mask:
        the cross-attention keys and values of every layer (they do not change during a decode), empty self-attention caches,
        position 0.  On the kernels inside their envelope, in PyTorch ops otherwise (CPU tensors, fused_decoder = False,
        max_step or Lv above 128 or above the Python-side limits).
        beam_size > 1: N * beam_size decode rows over the SAME N blocks of encoder keys, and the beam tables (also made for
        beam_size = 1 when `beam_tables` asks); the kernels' route then also needs beam size, vocabulary and max_step inside the
        selection kernel's envelope.  With beam_size = 1 state and kernels are those of the greedy decode."""
        N, Lv, D = encoder_outputs.shape
        if max_step < 1 or max_step > self.position_embeddings.num_embeddings:
            raise ValueError("HeroForTvc: max_step %d outside [1, %d]" % (max_step, self.position_embeddings.num_embeddings))
        if beam_size < 1:
            raise ValueError("HeroForTvc: beam size %d < 1" % beam_size)
        want_tables = beam_tables or beam_size > 1
        fused = self._fused_step(encoder_outputs, max_step)
        if fused and want_tables:
            fused = beam_size <= self.max_beam and T.in_envelope_beam(HF.compute_dtype(), self.config.f_config.vocab_size, beam_size, max_step)
        state = TvcDecodeState(fused, N, Lv, max_step, beam_size)
        dev, R = encoder_outputs.device, state.rows
        if state.fused:
            cd = HF.compute_dtype()
            for _ in self.decoder.layer:
                state.cross_kv.append(torch.empty((N * Lv, 2 * D), dtype=cd, device=dev))
                state.cache.append(torch.zeros((R, max_step, 2 * D), dtype=cd, device=dev))
            state.mask_add = torch.empty((N, Lv), dtype=torch.float32, device=dev)
            state.pos = torch.zeros((1,), dtype=torch.int32, device=dev)
            state.pid = torch.zeros((R,), dtype=torch.int32, device=dev)
            state.wid = torch.zeros((R,), dtype=torch.int32, device=dev)
        else:
            n = len(self.decoder.layer)
            state.self_k, state.self_v = [None] * n, [None] * n
        if want_tables:
            state.tables = BeamTables(N, beam_size, max_step, dev, state.fused)
        return self.refill_decode_state(state, encoder_outputs, encoder_masks)

    @torch.no_grad()
    def refill_decode_state(self, state, encoder_outputs, encoder_masks):
        """Another batch of the same shape into the SAME buffers, position back to 0 (a captured step holds their addresses)."""
        if tuple(encoder_outputs.shape[:2]) != (state.N, state.Lv):
            raise ValueError("HeroForTvc: the decode state was made for [%d, %d] encoder rows, got %s"
                             % (state.N, state.Lv, tuple(encoder_outputs.shape)))
        state.t = 0
        if state.tables is not None:
            state.tables.reset()
        if state.fused:
            enc2 = HF._as2d(HF.cast(encoder_outputs, HF.compute_dtype()))
            for li, layer in enumerate(self.decoder.layer):
                state.cross_kv[li].copy_(layer.cross_kv(enc2))
            state.mask_add.copy_((1.0 - encoder_masks.reshape(state.N, state.Lv).to(torch.float32)) * -10000.0)
            state.pos.zero_()
            state.pid.zero_()
            return state
        enc = encoder_outputs.to(self.emb_LayerNorm.weight.dtype)
        state.cross_k = [layer.dec_enc_attention.key(enc) for layer in self.decoder.layer]
        state.cross_v = [layer.dec_enc_attention.value(enc) for layer in self.decoder.layer]
        state.mask_add = (1.0 - encoder_masks.unsqueeze(1).unsqueeze(2).to(enc)) * -10000.0
        return state

    @torch.no_grad()
    def reorder_decode_state(self, state, parent_rows):
        """After a beam selection: row i continues row parent_rows[i].  The kernels' route keeps its caches where they are (the
        step kernel follows the tables' `anc`); the PyTorch route gathers the keys and values it has kept."""
        if state.fused:
            return
        state.self_k = [k.index_select(0, parent_rows) for k in state.self_k]
        state.self_v = [v.index_select(0, parent_rows) for v in state.self_v]

    @torch.no_grad()
    def decode_step(self, state, last_ids):
        """last_ids [rows] (rows = N, or N * beam): the token of every row at the state's position -> the prediction scores
        [rows, vocab] of the next one (in the compute dtype on the kernels); the position advances - on the device for the fused
        state, nothing here reads it on the host, so the call can be captured and replayed.  A fused state takes its own
        `wid` buffer as last_ids without a copy (hero_beam_select writes the next ids there)."""
        emb = self.v_encoder.f_encoder.embeddings
        V = self.config.f_config.vocab_size
        if state.fused:
            if last_ids is not state.wid:
                state.wid.copy_(last_ids)
            ln = self.emb_LayerNorm
            x = HF.embed_ln(None, ln.weight, ln.bias, ln.eps, None, HF.compute_dtype(),
                            tables=(emb.word_embeddings.weight, self.position_embeddings.weight), idxs=(state.wid, state.pid),
                            skip_idx=(emb.padding_idx, -1))
            for li, layer in enumerate(self.decoder.layer):
                x = layer.step(x, state, li)
            scores = self.v_encoder.f_encoder.lm_head(x, raw=True)
            state.pos.add_(1)
            state.pid.add_(1)
            return scores[:, :V]
        if state.t >= state.max_step:
            raise ValueError("HeroForTvc: decode step %d of a state made for %d" % (state.t, state.max_step))
        pos_ids = torch.full((state.rows, 1), state.t, dtype=torch.long, device=last_ids.device)
        x = emb.word_embeddings(last_ids.unsqueeze(1)) + self.position_embeddings(pos_ids)
        ln = self.emb_LayerNorm
        x = F.layer_norm(x, ln.normalized_shape, ln.weight, ln.bias, ln.eps)
        for li, layer in enumerate(self.decoder.layer):
            x = layer.step_torch(x, state, li)
        state.t += 1
        return self._scores_torch(x[:, 0])

    def forward(self, batch, mode="train", compute_loss=True, task=None):
        if task not in (None, "tvc"):
            raise ValueError(f"Unrecognized task: {task}")
        encoder_outputs = self.encode(batch)
        return self.decode(encoder_outputs, batch["cap_attn_mask"], batch["cap_input_ids"], batch["cap_pos_ids"],
                           batch.get("cap_tgt_ids"), compute_loss)

    def caption_loss(self, batch):
        """The scalar train_tvc.py:172-173 trains on - `forward(batch).mean()` - without the boolean compaction: the mean over
        the valid positions (lsr > 0) or over all positions (lsr == 0) is taken on the device, nothing synchronises."""
        encoder_outputs = self.encode(batch)
        caption_ids, label_ids = batch["cap_input_ids"], batch["cap_tgt_ids"]
        if not self._fused(encoder_outputs, caption_ids):
            return self.decode(encoder_outputs, batch["cap_attn_mask"], caption_ids, batch["cap_pos_ids"], label_ids, True).mean()
        states = self._decoder_states(encoder_outputs, batch["cap_attn_mask"], caption_ids, batch["cap_pos_ids"], True)
        V = self.config.f_config.vocab_size
        logits = self.v_encoder.f_encoder.lm_head(states.reshape(-1, states.shape[-1]), raw=True)
        labels = label_ids.reshape(-1)
        if self.lsr > 0:
            return T.smooth_ce_mean(logits, labels, self.lsr, ncols=V, ignore_index=-1, inplace=True)
        return HF.cross_entropy(logits, labels, ncols=V, ignore_index=-1).mean()


class TvcGenerator(object):
    """Greedy decoding (model/tvc.py:293-338) on a fixed [N, max_step] id buffer: the encoder runs once; every step runs the
    decoder over the whole buffer under the causal mask - positions past the current one cannot influence it - projects ONLY
    the current position through the vocabulary GEMM and takes the arg-max on the device.  One host transfer, at the end.

    kv_cache = True decodes incrementally instead (HeroForTvc.init_decode_state / decode_step): every step runs the decoder on
    ONE row per caption against the keys and values kept from the earlier steps, and the keys / values of the encoder rows are
    projected once per decode.  use_graph = True (needs kv_cache, and the kernels' route) captures that step - embedding, both
    layers, projection, arg-max, the id write at the device position, the position increment - once per (N, Lv, max_step) on one
    stream and replays it max_step times; between batches of one shape only the state's buffers are refilled.

    beam_decode(batch, beam_size) searches with beam_size beams per caption on the same incremental step (needs kv_cache; under
    use_graph the beam step is captured once per (N, beam, Lv, max_step) and shares MAX_GRAPHS and `counts` with the greedy
    graphs): the step runs N * beam rows, hero_beam_select takes the beam tables to the next step on the device, and neither
    the key/value cache nor the encoder keys are copied or replicated.

    sample_decode(batch, n_samples, temperature, top_k, top_p, seed) draws n_samples captions per clip on the same state (one
    hero_sample_select per step; the ancestry table stays at the identity) and keeps the best by model likelihood.
    stop_at_eos (beam_decode, sample_decode) ends a decode once every row has finished: after every `check_every` steps ONE
    word is read from the device, outside the captured step.  counts["steps"] counts the decode steps actually run."""

    MAX_GRAPHS = 8

    def __init__(self, model, max_step, bos, eos, kv_cache=False, use_graph=False, check_every=4):
        if use_graph and not kv_cache:
            raise ValueError("TvcGenerator: use_graph replays the incremental decode step, it needs kv_cache=True")
        if check_every < 1:
            raise ValueError("TvcGenerator: check_every %d < 1" % check_every)
        self.model, self.max_step, self.bos, self.eos = model, max_step, bos, eos
        self.kv_cache, self.use_graph, self.check_every = kv_cache, use_graph, int(check_every)
        self._graphs = {}          # (N, Lv, max_step, dtype, device, weight-copy generation) -> captured step and its buffers
        self.counts = {"captures": 0, "replayed": 0, "steps": 0}     # steps: decode steps actually run, on every cached route

    def _step(self, state, last, output_ids):
        """One incremental step on device buffers only: `last` [N] in, the arg-max ids out - into `last` and into column
        (position) of output_ids."""
        model = self.model
        scores = model.decode_step(state, last)
        nxt = scores.float().argmax(dim=-1)
        if state.fused:
            col = (state.pos - 1).long().view(1, 1).expand(state.N, 1)                 # the position this step decoded
            output_ids.scatter_(1, col, nxt.unsqueeze(1))
        else:
            output_ids[:, state.t - 1] = nxt
        last.copy_(nxt)

    def _weights_signature(self):
        return tuple(p._version for p in self.model.parameters()) + (HF.weight_epoch(),)

    def _all_finished(self, state):
        """ONE word from the device: every row of the state's tables has emitted `eos`.  Outside any captured step."""
        return int(state.tables.fin.min()) != 0

    def _run_steps(self, state, step, stop_at_eos):
        """step() up to max_step times; with stop_at_eos the finished flags are read after every `check_every` steps and the loop
        ends once every row has finished - a finished row only re-emits `eos` at an unchanged score, so nothing is lost."""
        done = 0
        while done < self.max_step:
            step()
            done += 1
            if stop_at_eos and done % self.check_every == 0 and done < self.max_step and self._all_finished(state):
                break
        self.counts["steps"] += done
        return done

    def _decode(self, kind, encoder_outputs, enc_mask, make, prepare=None, stop_at_eos=False):
        """One decode of `kind` (the kind's part of a graph key) over the batch -> its entry.  make() -> dict(state, last = the ids
        buffer the step embeds, filled with `bos`, step = one step on device buffers only that leaves the next ids in `last`, ...);
        prepare(entry) is what the kind adds to a filled state (sampling: its tables and seed).  Eager: a new entry per call.
        use_graph: the entry is made once per shape - the step runs once eagerly, so that every compute copy of a weight exists,
        and is then captured on one stream, a straight line - and from then on refilled with the batch and replayed."""
        model = self.model
        if not self.use_graph:
            hit = make()
            if prepare is not None:
                prepare(hit)
            self._run_steps(hit["state"], hit["step"], stop_at_eos)
            return hit
        N, Lv = encoder_outputs.shape[:2]
        key = kind + (N, Lv, self.max_step, HF.compute_dtype(), str(encoder_outputs.device), HF.weight_cache_generation())
        hit = self._graphs.get(key)
        if hit is None:
            hit = make()
            if not hit["state"].fused:
                raise ValueError("TvcGenerator: use_graph needs the kernels' route (CUDA tensors, fused_decoder, max_step and Lv "
                                 "inside the envelope; beam search: beam size and vocabulary, too)")
            hit["step"]()
            key = key[:-1] + (HF.weight_cache_generation(),)
            model.refill_decode_state(hit["state"], encoder_outputs, enc_mask)
            if prepare is not None:
                prepare(hit)
            torch.cuda.synchronize()
            # An entry and its generator refer to each other (the step closes over `self`), so a generator that was dropped
            # goes - with its graphs - only when the cycle collector runs.  Inside a capture that is an error (a graph and its
            # memory pool cannot be released while a stream captures): collect now, and let no collection start in there.
            gc.collect()
            hit["graph"] = torch.cuda.CUDAGraph()
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(hit["graph"]):
                    hit["step"]()
            finally:
                if gc_was_on:
                    gc.enable()
            if len(self._graphs) >= self.MAX_GRAPHS:
                self._graphs.clear()
            hit["wsig"] = self._weights_signature()
            self._graphs[key] = hit
            self.counts["captures"] += 1
        wsig = self._weights_signature()
        if wsig != hit["wsig"]:                                 # the replay calls no HF.packed: bring the compute copies up to date
            HF.refresh_weight_cache()
            hit["wsig"] = wsig
        model.refill_decode_state(hit["state"], encoder_outputs, enc_mask)
        if prepare is not None:
            prepare(hit)
        hit["last"].fill_(self.bos)
        self.counts["replayed"] += self._run_steps(hit["state"], hit["graph"].replay, stop_at_eos)
        return hit

    @torch.no_grad()
    def _decode_cached(self, encoder_outputs, enc_mask):
        def make():
            N, dev = encoder_outputs.shape[0], encoder_outputs.device
            state = self.model.init_decode_state(encoder_outputs, enc_mask, self.max_step)
            last = torch.full((N,), self.bos, dtype=torch.long, device=dev)
            out = torch.zeros((N, self.max_step), dtype=torch.long, device=dev)
            return dict(state=state, last=last, out=out, step=lambda: self._step(state, last, out))
        return self._decode((), encoder_outputs, enc_mask, make)["out"]

    @torch.no_grad()
    def greedy_decode(self, batch, encoder_outputs=None, as_tensor=False):
        """encoder_outputs: what model.encode(batch) returned, when the caller already has it.  as_tensor: the [N, max_step] id rows
        as a device tensor of their own, not cut at `eos`, without a host transfer (hero_amd.caption scores them there)."""
        model = self.model
        if encoder_outputs is None:
            encoder_outputs = model.encode(batch)
        enc_mask = batch["cap_attn_mask"]
        if self.kv_cache:
            out = self._decode_cached(encoder_outputs, enc_mask)
            return out.clone() if as_tensor else [self.cut_eos(ids) for ids in out.tolist()]
        N, dev = enc_mask.size(0), encoder_outputs.device
        # the buffer is padded with the pad id, whose embedding row and positions the causal mask hides from every earlier step
        input_ids = torch.full((N, self.max_step), model.v_encoder.f_encoder.embeddings.padding_idx, dtype=torch.long, device=dev)
        pos_ids = torch.arange(0, self.max_step, dtype=torch.long, device=dev).unsqueeze(0)
        output_ids = torch.empty((N, self.max_step), dtype=torch.long, device=dev)
        last_out = torch.full((N,), self.bos, dtype=torch.long, device=dev)
        fused = model._fused(encoder_outputs, input_ids)
        head = model.v_encoder.f_encoder.lm_head
        for step in range(self.max_step):
            input_ids[:, step] = last_out
            if fused:
                states = model._decoder_states(encoder_outputs, enc_mask, input_ids, pos_ids, True)
                scores = head(states[:, step].contiguous(), raw=True)
            else:                                    # the reference's growing prefix
                states = model._decoder_states(encoder_outputs, enc_mask, input_ids[:, :step + 1], pos_ids[:, :step + 1], False)
                scores = model._scores_torch(states[:, -1])
            last_out = scores[:, :model.config.f_config.vocab_size].float().argmax(dim=-1)
            output_ids[:, step] = last_out
        return output_ids if as_tensor else [self.cut_eos(ids) for ids in output_ids.tolist()]

    # ---- beam search --------------------------------------------------------------------------------------------------------
    def _beam_state(self, encoder_outputs, enc_mask, beam_size):
        state = self.model.init_decode_state(encoder_outputs, enc_mask, self.max_step, beam_size, beam_tables=True)
        if state.fused:
            state.wid.fill_(self.bos)
            return state, state.wid
        return state, torch.full((state.rows,), self.bos, dtype=torch.long, device=encoder_outputs.device)

    def _beam_step(self, state, last):
        """One beam step on device buffers only: decode_step over all rows, then the selection; the next ids go to `last`.  Fused:
        hero_beam_select updates the tables in place and leaves the ids in the state's `wid`, which is `last`; the position it
        reads has already advanced, hence the offset.  PyTorch route: the same algorithm in ops, and the kept keys / values
        follow their parents."""
        model, tb = self.model, state.tables
        scores = model.decode_step(state, last)
        if state.fused:
            T.k_beam_select(scores, tb.cum, tb.fin, tb.len, tb.ids, tb.anc, state.wid, tb.ws, state.pos, state.N, state.beam,
                            scores.shape[1], self.eos, pos_offset=-1)
            return
        rows, nxt = beam_select_torch(scores, tb, state.t - 1, self.eos)
        model.reorder_decode_state(state, rows)
        last.copy_(nxt)

    def _pick(self, tb, N, per, length_penalty, return_all, return_scores, as_tensor=False):
        """Of the `per` rows of each of the N captions the one with the largest  cum / max(len, 1) ** length_penalty  - a stable
        sort: the lower row wins a tie - or, with return_all, every row in row order; ids and the fp32 scores' bits come to the
        host in ONE int32 transfer.  -> list of id lists cut at `eos`[, list of their scores].  as_tensor: the same rows as a device
        tensor [rows, max_step], not cut (a finished row carries `eos` to the end)[, their scores as a device tensor]: no transfer."""
        norm = tb.cum.view(N, per) / tb.len.view(N, per).clamp(min=1).to(torch.float32) ** float(length_penalty)
        if return_all:
            rows, picked = torch.arange(N * per, device=norm.device), norm.reshape(-1, 1)
        else:
            best = torch.sort(norm, dim=1, descending=True, stable=True).indices[:, :1]
            rows, picked = torch.arange(N, device=best.device) * per + best[:, 0], norm.gather(1, best)
        if as_tensor:
            return (tb.ids[rows], picked.reshape(-1)) if return_scores else tb.ids[rows]
        packed = torch.cat([tb.ids[rows].to(torch.int32), picked.contiguous().view(torch.int32)], dim=1).cpu()
        ids = [self.cut_eos(r) for r in packed[:, :-1].tolist()]
        if return_scores:
            return ids, packed[:, -1:].contiguous().view(torch.float32).view(-1).tolist()
        return ids

    @torch.no_grad()
    def beam_decode(self, batch, beam_size, length_penalty=1.0, encoder_outputs=None, return_scores=False, stop_at_eos=False,
                    as_tensor=False):
        """Beam search over the incremental decode (needs kv_cache=True): max_step steps of decode_step + selection for
        N * beam_size rows, no early exit - a finished beam carries `eos` at an unchanged score - then per caption the beam with
        the largest  cum / max(len, 1) ** length_penalty  (the lower beam among equals), ONE host transfer, and the ids cut at
        `eos`.  On the kernels' route the selection is hero_beam_select and neither the cache nor the encoder keys are copied or
        replicated; use_graph replays the step, captured once per (N, beam, Lv, max_step) into the graph table it shares with the
        greedy steps.  stop_at_eos: leave the loop once every beam of every caption has finished
        (one word read from the device after every `check_every` steps, outside the captured step); the result is that of the
        full-length run.  -> list of id lists[, list of the picked beams' scores]; as_tensor: the picked rows [N, max_step] as a
        device tensor, not cut at `eos`, without the host transfer."""
        if not self.kv_cache:
            raise ValueError("TvcGenerator: beam_decode runs on the incremental decode step, it needs kv_cache=True")
        if beam_size < 1:
            raise ValueError("TvcGenerator: beam size %d < 1" % beam_size)
        if encoder_outputs is None:
            encoder_outputs = self.model.encode(batch)
        enc_mask = batch["cap_attn_mask"]

        def make():
            state, last = self._beam_state(encoder_outputs, enc_mask, beam_size)
            return dict(state=state, last=last, step=lambda: self._beam_step(state, last))
        state = self._decode(("beam", beam_size), encoder_outputs, enc_mask, make, stop_at_eos=stop_at_eos)["state"]
        return self._pick(state.tables, state.N, beam_size, length_penalty, False, return_scores, as_tensor)

    # ---- sampling -----------------------------------------------------------------------------------------------------------
    def _sample_step(self, state, last, seed, params):
        """One sampling step on device buffers only: decode_step over all rows, then the draw; the next ids go to `last`.  Fused:
        hero_sample_select updates the tables in place and leaves the ids in the state's `wid`, which is `last` (`seed` is a
        device word); PyTorch route: the same algorithm in ops (`seed` is an int)."""
        tb = state.tables
        temperature, top_k, top_p = params
        scores = self.model.decode_step(state, last)
        if state.fused:
            T.k_sample_select(scores, tb.cum, tb.fin, tb.len, tb.ids, state.wid, tb.kept, seed, state.pos, state.N, state.beam,
                              scores.shape[1], self.eos, temperature, top_k, top_p, pos_offset=-1)
            return
        last.copy_(sample_select_torch(scores, tb, state.t - 1, self.eos, seed, temperature, top_k, top_p)[0])

    @staticmethod
    def _seed_word(seed):
        s = int(seed) & _M64
        return s - (1 << 64) if s >= (1 << 63) else s              # the same 64 bits in an int64

    @torch.no_grad()
    def sample_decode(self, batch, n_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=0, length_penalty=1.0,
                      return_all=False, return_scores=False, stop_at_eos=False, encoder_outputs=None, as_tensor=False):
        """Sampled decoding over the incremental decode (needs kv_cache=True): n_samples independent captions per clip, drawn token
        by token from the step's scores under temperature, then top-k (0 = off), then top-p (>= 1 = off); the draw is a
        counter-based Gumbel-max, a function of (seed, position, row, token) alone.  The state is the beam state: N * n_samples
        rows over the caption's own N blocks of encoder keys, the ancestry table left at the identity, no cache copied.  cum is
        the model's own log-likelihood of the drawn tokens (temperature 1, no filter).  -> per caption the sample with the
        largest  cum / max(len, 1) ** length_penalty  (the lower sample among equals), or with return_all all N * n_samples
        captions in row order (caption-major); ONE host transfer, ids cut at `eos`[, the scores of the returned captions].
        On the kernels' route (n_samples within the beam envelope) the draw is hero_sample_select; use_graph replays the step,
        captured once per (N, samples, Lv, max_step, temperature, top_k, top_p) - the three are launch scalars of the captured
        kernel, the seed is a device word filled before the replays: a new seed does not recapture.  stop_at_eos as in
        beam_decode.  top_k = 1 is greedy decoding.  as_tensor: the returned rows as a device tensor [N or N * n_samples, max_step],
        not cut at `eos`, without the host transfer."""
        if not self.kv_cache:
            raise ValueError("TvcGenerator: sample_decode runs on the incremental decode step, it needs kv_cache=True")
        if n_samples < 1:
            raise ValueError("TvcGenerator: n_samples %d < 1" % n_samples)
        if not temperature > 0 or not math.isfinite(temperature):
            raise ValueError("TvcGenerator: temperature %r must be finite and > 0" % (temperature,))
        if top_k < 0:
            raise ValueError("TvcGenerator: top_k %r < 0" % (top_k,))
        if not top_p > 0:
            raise ValueError("TvcGenerator: top_p %r must be > 0" % (top_p,))
        params = (float(temperature), int(top_k), float(top_p))
        if encoder_outputs is None:
            encoder_outputs = self.model.encode(batch)
        enc_mask = batch["cap_attn_mask"]

        def make():
            state, last = self._beam_state(encoder_outputs, enc_mask, n_samples)
            hit = dict(state=state, last=last, seed=torch.zeros((1,), dtype=torch.long, device=last.device) if state.fused else 0)
            hit["step"] = lambda: self._sample_step(state, last, hit["seed"], params)
            return hit

        def prepare(hit):                                           # the seed: a device word on the kernels' route, the int in PyTorch ops
            hit["state"].tables.reset(sampling=True)
            if hit["state"].fused:
                hit["seed"].fill_(self._seed_word(seed))
            else:
                hit["seed"] = seed
        state = self._decode(("sample", n_samples) + params, encoder_outputs, enc_mask, make, prepare, stop_at_eos)["state"]
        return self._pick(state.tables, state.N, n_samples, length_penalty, return_all, return_scores, as_tensor)

    def cut_eos(self, ids):
        out_ids = []
        for i in ids:
            if i == self.eos:
                break
            out_ids.append(i)
        return out_ids
