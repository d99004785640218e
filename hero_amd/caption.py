"""Caption metrics and rewards for TVC on the device: BLEU-1..4, ROUGE-L and CIDEr-D of decoded id rows against reference
token sequences, as the reference's eval/pycocoevalcap computes them on words (BleuScorer(n=4) with the "closest" reference
length, Rouge(), CiderScorer(n=4, sigma=6.0)) - restated on integer tokens (include/hero_hip.h "Caption metrics").  Fed with
word ids they are the reference's numbers; fed with the model's BPE ids they are a training-time proxy and a reward.  METEOR,
detokenisation and the PTB tokeniser are not here.

    CaptionRefs            the reference tables, built once with PyTorch ops: per order the sorted n-gram keys (four 16-bit
                           tokens in one int64, exact) of every reference and clip with their counts, the idf table, the
                           reference norms and padded ids - one packed device buffer for the kernel
    k_caption_score        hero_caption_score: one launch over [M, ld] id rows -> BLEU's integers, ROUGE-L, CIDEr-D per row
    caption_score_torch    the same algorithm in PyTorch ops: CPU tensors and shapes outside the kernel's envelope
    CaptionMeter           per-clip results written by index into device buffers; compute() is the one synchronisation
    validate_tvc           the reference's validation loop (train_tvc.py:validate) without the strings
    caption_rewards        the per-row CIDEr-D on the device
    reward_weighted_loss   sum_rows w_row * sum_t CE(row, t) / (number of valid tokens) through HeroForTvc's teacher-forced decoder
    self_critical_loss     greedy baseline + sampled captions + CIDEr-D reward -> reward_weighted_loss (eager only)"""
import math

import torch

from . import _lib as L

ORDERS, MAX_REF_LEN, MAX_REFS, MAX_V, MAX_T, N_STATS = 4, 128, 32, 65536, 128, 10
_MAGIC, _HDR_WORDS = 0x4845524F43415031, 48


def in_envelope(V, Tcap):
    """The library's own answer (hero_caption_in_envelope): 1 <= V <= 65536, 1 <= Tcap <= 128."""
    return bool(L.lib().hero_caption_in_envelope(int(V), int(Tcap)))


def _pad_refs(refs, what):
    """Host validation and padding: list over clips of lists of token-id lists -> (ids [R, Lr] int64, len [R], clip [R], C)."""
    if not isinstance(refs, (list, tuple)) or len(refs) < 1:
        raise ValueError("CaptionRefs: %s must be a non-empty list over clips" % what)
    flat, clip = [], []
    for c, rs in enumerate(refs):
        if not isinstance(rs, (list, tuple)) or not 1 <= len(rs) <= MAX_REFS:
            raise ValueError("CaptionRefs: clip %d of %s has %s references, outside [1, %d]"
                             % (c, what, len(rs) if isinstance(rs, (list, tuple)) else "no list of", MAX_REFS))
        for r in rs:
            r = list(r)
            if not 1 <= len(r) <= MAX_REF_LEN:
                raise ValueError("CaptionRefs: a reference of clip %d of %s has %d tokens, outside [1, %d]" % (c, what, len(r), MAX_REF_LEN))
            if min(r) < 0 or max(r) >= MAX_V:
                raise ValueError("CaptionRefs: a reference of clip %d of %s holds an id outside [0, %d)" % (c, what, MAX_V))
            flat.append(r)
            clip.append(c)
    lens = torch.tensor([len(r) for r in flat], dtype=torch.long)
    ids = torch.zeros((len(flat), int(lens.max())), dtype=torch.long)
    for i, r in enumerate(flat):
        ids[i, :len(r)] = torch.tensor(r, dtype=torch.long)
    return ids, lens, torch.tensor(clip, dtype=torch.long), len(refs)


def pack_keys(win):
    """[..., n] int64 tokens below 65536 -> the n-gram's int64 key ((t0 << 16 | t1) << 16 | t2) << 16 | t3 (a 4-gram whose
    first token is >= 32768 wraps to a negative key: tables are sorted, and searched, as signed int64)."""
    key = win[..., 0]
    for k in range(1, win.shape[-1]):
        key = (key << 16) | win[..., k]
    return key


def _sorted_pairs(seg, key):
    """(seg, key) rows sorted by segment, then key; -> unique pairs, their multiplicities and the inverse map."""
    o = torch.sort(key, stable=True).indices
    seg, key = seg[o], key[o]
    o2 = torch.sort(seg, stable=True).indices
    pairs = torch.stack([seg[o2], key[o2]], dim=1)
    uniq, inv, cnt = torch.unique_consecutive(pairs, dim=0, return_inverse=True, return_counts=True)
    return uniq, cnt, inv, o[o2]


def _order_tables(ids, lens, clip, C, n):
    """The tables of order n over padded references: (rw_ref, rw_key, rw_cnt) per reference, (cm_clip, cm_key, cm_cnt) per clip
    with the largest count among the clip's references, (df_key, df) the number of clips that hold a key."""
    R, Lr = ids.shape
    e = torch.zeros((0,), dtype=torch.long)
    if Lr < n:
        return (e, e, e), (e, e, e), (e, e)
    key = pack_keys(ids.unfold(1, n, 1))
    valid = torch.arange(Lr - n + 1).unsqueeze(0) + n <= lens.unsqueeze(1)
    ref = torch.arange(R).unsqueeze(1).expand_as(key)[valid]
    rw, rw_cnt, _, _ = _sorted_pairs(ref, key[valid])
    cm, _, inv, order = _sorted_pairs(clip[rw[:, 0]], rw[:, 1])
    cm_cnt = torch.zeros((cm.shape[0],), dtype=torch.long).scatter_reduce(0, inv, rw_cnt[order], "amax", include_self=True)
    df_key, df = torch.unique_consecutive(torch.sort(cm[:, 1]).values, return_counts=True)
    return (rw[:, 0].clone(), rw[:, 1].clone(), rw_cnt), (cm[:, 0].clone(), cm[:, 1].clone(), cm_cnt), (df_key, df)


def _offsets(seg, n):
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(seg, minlength=n).cumsum(0)])


def _lookup(table, keys):
    """(position, found) of `keys` in a sorted 1-D int64 table."""
    if table.numel() == 0:
        return torch.zeros_like(keys), torch.zeros_like(keys, dtype=torch.bool)
    pos = torch.searchsorted(table, keys.contiguous()).clamp(max=table.numel() - 1)
    return pos, table[pos] == keys


class CaptionRefs(object):
    """The reference side of the caption metrics.  refs: list over clips of lists of token-id lists, without bos / eos (1..32
    references of 1..128 ids in [0, 65536) per clip).  clip_ids: the clips' names, for `rows()`; idf_refs: a second corpus in
    the same form that supplies the document frequencies and the clip count C of CIDEr's idf (a reward on a mini-batch's
    references with the training set's idf).  Everything is built once with PyTorch ops on the host and moved to `device`."""

    def __init__(self, refs, clip_ids=None, idf_refs=None, device=None):
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        ids, lens, clip, C = _pad_refs(refs, "refs")
        self.n_clips, self.n_refs, self.ld = C, ids.shape[0], ids.shape[1]
        if clip_ids is not None:
            clip_ids = list(clip_ids)
            if len(clip_ids) != C or len(set(clip_ids)) != C:
                raise ValueError("CaptionRefs: clip_ids must name every clip once (%d names for %d clips)" % (len(clip_ids), C))
        self.clip_ids = clip_ids
        self._index = {cid: i for i, cid in enumerate(clip_ids)} if clip_ids is not None else None
        own = [_order_tables(ids, lens, clip, C, n) for n in range(1, ORDERS + 1)]
        if idf_refs is None:
            c_idf, dfs = C, [t[2] for t in own]
        else:
            i_ids, i_lens, i_clip, c_idf = _pad_refs(idf_refs, "idf_refs")
            dfs = [_order_tables(i_ids, i_lens, i_clip, c_idf, n)[2] for n in range(1, ORDERS + 1)]
        log_c = torch.log(torch.tensor(float(c_idf), dtype=torch.float64))
        self.log_c = float(log_c)
        clip_ref = _offsets(clip, C)
        ref_norm = torch.zeros((self.n_refs, ORDERS), dtype=torch.float64)
        parts = [("clip_ref", clip_ref.to(torch.int32)), ("ref_len", lens.to(torch.int32)), ("ref_norm", ref_norm),
                 ("ref_ids", ids.to(torch.int32))]
        self.orders = []
        for n, ((rw_ref, rw_key, rw_cnt), (cm_clip, cm_key, cm_cnt), _) in enumerate(own):
            df_key, df = dfs[n]
            idf_val = log_c - torch.log(df.clamp(min=1).to(torch.float64))          # df == C gives exactly 0
            pos, found = _lookup(df_key, rw_key)
            w = rw_cnt.to(torch.float64) * (torch.where(found, idf_val[pos], log_c) if df_key.numel() else log_c.expand(rw_key.shape))
            ref_norm[:, n] = torch.sqrt(torch.zeros((self.n_refs,), dtype=torch.float64).index_add(0, rw_ref, w * w))
            parts += [("cm_off%d" % n, _offsets(cm_clip, C).to(torch.int32)), ("cm_key%d" % n, cm_key), ("cm_cnt%d" % n, cm_cnt.to(torch.int32)),
                      ("rw_off%d" % n, _offsets(rw_ref, self.n_refs).to(torch.int32)), ("rw_key%d" % n, rw_key),
                      ("rw_cnt%d" % n, rw_cnt.to(torch.int32)), ("idf_key%d" % n, df_key), ("idf_val%d" % n, idf_val)]
            # the PyTorch route searches one composite per table: segment * G + the key's rank among all reference keys
            uk = torch.unique(cm_key)
            G = max(int(uk.numel()), 1)
            self.orders.append(dict(
                G=G, uk=uk.to(self.device), cm_comp=(cm_clip * G + _lookup(uk, cm_key)[0]).to(self.device), cm_cnt=cm_cnt.to(self.device),
                rw_comp=(rw_ref * G + _lookup(uk, rw_key)[0]).to(self.device), rw_cnt=rw_cnt.to(self.device),
                idf_key=df_key.to(self.device), idf_val=idf_val.to(self.device)))
        self.clip_ref, self.ref_len = clip_ref.to(self.device), lens.to(self.device)
        self.ref_norm, self.ref_ids = ref_norm.to(self.device), ids.to(self.device)
        self.max_refs = int((clip_ref[1:] - clip_ref[:-1]).max())
        # one packed buffer: a header of 64-bit words (hero_amd/csrc/caption_metrics.hip), every part 8-byte aligned
        hdr = torch.zeros((_HDR_WORDS,), dtype=torch.long)
        hdr[0], hdr[1], hdr[2], hdr[3] = _MAGIC, C, self.n_refs, self.ld
        hdr[4] = log_c.reshape(1).view(torch.long)[0]
        slot = {"clip_ref": 5, "ref_len": 6, "ref_norm": 7, "ref_ids": 8}
        for n in range(ORDERS):
            for j, name in enumerate(("cm_off", "cm_key", "cm_cnt", "rw_off", "rw_key", "rw_cnt", "idf_key", "idf_val")):
                slot["%s%d" % (name, n)] = 10 + 8 * n + j
            hdr[42 + n] = dfs[n][0].numel()
        chunks, at = [], _HDR_WORDS * 8
        for name, t in parts:
            raw = torch.empty((t.numel(),), dtype=t.dtype).copy_(t.reshape(-1)).view(torch.uint8)     # fresh storage, unit stride
            raw = torch.cat([raw, torch.zeros(((-raw.numel()) % 8 + 8,), dtype=torch.uint8)])     # never empty, 8-byte steps
            hdr[slot[name]] = at
            chunks.append(raw)
            at += raw.numel()
        hdr[9] = at
        self.blob = torch.cat([hdr.view(torch.uint8)] + chunks).to(self.device)
        self.device = self.blob.device                    # with its index: what the rows' tensors report

    def rows(self, clip_ids):
        """The table rows of clip names (host): a list of ints."""
        if self._index is None:
            raise ValueError("CaptionRefs: built without clip_ids")
        return [self._index[c] for c in clip_ids]


def _check_rows(ids, clip, refs, eos, tcap):
    if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError("caption metrics: ids must be [M, ld] int32 or int64, got %s %s" % (tuple(ids.shape), ids.dtype))
    M, Tcap = ids.shape[0], ids.shape[1] if tcap is None else int(tcap)
    if tuple(clip.shape) != (M,) or clip.dtype not in (torch.int32, torch.int64):
        raise ValueError("caption metrics: clip must be [%d] int32 / int64, got %s %s" % (M, tuple(clip.shape), clip.dtype))
    if ids.device != refs.device or clip.device != refs.device:
        raise ValueError("caption metrics: ids on %s, clip on %s, reference tables on %s" % (ids.device, clip.device, refs.device))
    if not 1 <= Tcap <= ids.shape[1] or M < 1:
        raise ValueError("caption metrics: M=%d, Tcap=%d over rows of %d ids" % (M, Tcap, ids.shape[1]))
    return M, Tcap


def k_caption_score(ids, clip, refs, eos, tcap=None, vocab=MAX_V, out=None, want_lcs=False):
    """hero_caption_score: ids [M, ld] int32 / int64 device rows as the decoders leave them (unit column stride), clip [M] int32
    the rows' clips in `refs`; a row's caption is what stands before its first `eos` within tcap (default: ld) columns.
    -> (stats [M, 10] int32: correct[4], guess[4], testlen, reflen; rouge [M] fp32; cider [M] fp32[, lcs [M] int32]).
    out = (stats, rouge, cider[, lcs]): buffers to write into instead (stats [M, >= 10]: further columns are left alone).
    One launch, nothing read on the host.  Outside the kernel's envelope this raises (caption_score_torch serves it)."""
    M, Tcap = _check_rows(ids, clip, refs, eos, tcap)
    if not ids.is_cuda:
        raise RuntimeError("hero_amd: tensor is on %s; the HIP path needs CUDA/ROCm tensors and has no CPU fallback" % ids.device)
    if not in_envelope(vocab, Tcap) or not 0 <= eos < vocab:
        raise ValueError("caption metrics: V=%d, Tcap=%d, eos=%d is outside the kernel's envelope (1 <= V <= %d, 1 <= Tcap <= %d, "
                         "0 <= eos < V)" % (vocab, Tcap, eos, MAX_V, MAX_T))
    if ids.stride(1) != 1 or ids.stride(0) < Tcap:
        raise ValueError("caption metrics: id rows must have unit column stride")
    if clip.dtype != torch.int32:
        clip = clip.to(torch.int32)
    dev = ids.device
    if out is None:
        out = (torch.empty((M, N_STATS), dtype=torch.int32, device=dev), torch.empty((M,), dtype=torch.float32, device=dev),
               torch.empty((M,), dtype=torch.float32, device=dev)) + ((torch.empty((M,), dtype=torch.int32, device=dev),) if want_lcs else ())
    stats, rouge, cider = out[:3]
    lcs = out[3] if len(out) > 3 else None
    if stats.dim() != 2 or stats.shape[0] < M or stats.shape[1] < N_STATS or stats.dtype != torch.int32 or rouge.dtype != torch.float32 \
            or cider.dtype != torch.float32 or rouge.numel() < M or cider.numel() < M or (lcs is not None and (lcs.dtype != torch.int32 or lcs.numel() < M)):
        raise ValueError("caption metrics: outputs must be int32 [>= M, >= 10] and fp32 / fp32 / int32 [>= M]")
    L.check(L.lib().hero_caption_score(ids.data_ptr(), 1 if ids.dtype == torch.int64 else 0, L.ptr(clip), L.ptr(refs.blob), L.ptr(stats),
                                       L.ptr(rouge), L.ptr(cider), L.ptr(lcs), M, ids.stride(0), stats.stride(0), Tcap, int(eos), int(vocab),
                                       L.stream()))
    return out


def _score_rows_torch(ids, clip, refs, eos):
    """caption_score_torch on one block of rows: ids [M, T] int64 (already cut to Tcap columns), clip [M] int64."""
    dev, (M, T) = ids.device, ids.shape
    col = torch.arange(T, device=dev)
    Lh = torch.where(ids == eos, col.unsqueeze(0), torch.full_like(ids, T)).min(dim=1).values            # the caption's length
    r0, r1 = refs.clip_ref[clip], refs.clip_ref[clip + 1]
    ridx = r0.unsqueeze(1) + torch.arange(refs.max_refs, device=dev).unsqueeze(0)
    rvalid = ridx < r1.unsqueeze(1)
    ridx = torch.where(rvalid, ridx, torch.zeros_like(ridx))
    rlen = refs.ref_len[ridx]                                                                             # [M, Rm]
    stats = torch.zeros((M, N_STATS), dtype=torch.long, device=dev)
    stats[:, 8] = Lh
    big = torch.full_like(rlen, 1 << 30)
    stats[:, 9] = torch.where(rvalid, (rlen - Lh.unsqueeze(1)).abs() * 256 + rlen, big).min(dim=1).values % 256
    # LCS with every reference: row i of the table from row i - 1, L[i][j] = max(L[i-1][j], L[i][j-1], L[i-1][j-1] + match)
    rt = refs.ref_ids[ridx]                                                                               # [M, Rm, Lr]
    jvalid = torch.arange(refs.ld, device=dev).view(1, 1, -1) < rlen.unsqueeze(2)
    prev = torch.zeros((M, refs.max_refs, refs.ld + 1), dtype=torch.long, device=dev)
    for i in range(T):
        match = (rt == ids[:, i].view(M, 1, 1)) & jvalid & (Lh > i).view(M, 1, 1)
        cand = torch.maximum(prev[..., 1:], prev[..., :-1] + match.long())
        prev = torch.cat([prev[..., :1], torch.cummax(cand, dim=2).values], dim=2)
    lcs_r = torch.where(rvalid, prev[..., -1], torch.zeros_like(rlen))
    lcs = lcs_r.max(dim=1).values
    p = lcs.double() / Lh.clamp(min=1).double()
    q = (lcs_r.double() / rlen.double()).max(dim=1).values
    rouge = torch.where((p != 0) & (q != 0), (1.0 + 1.44) * p * q / (q + 1.44 * p).clamp(min=1e-300), torch.zeros_like(p))
    # n-gram counts, BLEU's clipped matches, CIDEr-D
    delta = ((Lh - 1).clamp(min=0).unsqueeze(1) - (rlen - 1).clamp(min=0)).double()
    penalty = torch.exp(-(delta * delta) / 72.0)
    score = torch.zeros((M,), dtype=torch.float64, device=dev)
    for n in range(1, ORDERS + 1):
        stats[:, 4 + n - 1] = (Lh - n + 1).clamp(min=0)
        P = T - n + 1
        if P < 1:
            continue
        t = refs.orders[n - 1]
        keys = pack_keys(ids.unfold(1, n, 1))                                                              # [M, P]
        kvalid = col[:P].unsqueeze(0) + n <= Lh.unsqueeze(1)
        eq = (keys.unsqueeze(2) == keys.unsqueeze(1)) & kvalid.unsqueeze(1) & kvalid.unsqueeze(2)
        cnt = eq.sum(dim=2)
        first = kvalid & ~(eq & torch.ones((P, P), dtype=torch.bool, device=dev).tril(-1)).any(dim=2)    # no earlier position holds it
        g, in_refs = _lookup(t["uk"], keys)
        at, found = _lookup(t["cm_comp"], clip.unsqueeze(1) * t["G"] + g)
        in_clip = first & in_refs & found
        top = t["cm_cnt"][at] if t["cm_cnt"].numel() else torch.zeros_like(cnt)
        stats[:, n - 1] = torch.where(in_clip, torch.minimum(cnt, top), torch.zeros_like(cnt)).sum(dim=1)
        ai, has_idf = _lookup(t["idf_key"], keys)
        idf = torch.where(has_idf, t["idf_val"][ai], torch.full_like(keys, refs.log_c, dtype=torch.float64)) if t["idf_key"].numel() \
            else torch.full_like(keys, refs.log_c, dtype=torch.float64)
        wh = torch.where(first, cnt.double() * idf, torch.zeros_like(idf))
        nh = torch.sqrt((wh * wh).sum(dim=1))
        if t["rw_cnt"].numel() == 0:
            continue
        ar, in_ref = _lookup(t["rw_comp"], ridx.unsqueeze(2) * t["G"] + g.unsqueeze(1))                  # [M, Rm, P]
        wr = t["rw_cnt"][ar].double() * idf.unsqueeze(1)
        live = in_clip.unsqueeze(1) & in_ref
        dot = torch.where(live, torch.minimum(wh.unsqueeze(1), wr) * wr, torch.zeros_like(wr)).sum(dim=2)
        nr = refs.ref_norm[ridx, n - 1]
        both = (nh.unsqueeze(1) != 0) & (nr != 0)
        val = torch.where(both, dot / torch.where(both, nh.unsqueeze(1) * nr, torch.ones_like(nr)), dot)
        score += torch.where(rvalid, val * penalty, torch.zeros_like(val)).sum(dim=1)
    cider = score / 4.0 / (r1 - r0).double() * 10.0
    return stats.to(torch.int32), rouge.float(), cider.float(), lcs.to(torch.int32)


def caption_score_torch(ids, clip, refs, eos, tcap=None, block=128):
    """k_caption_score's algorithm in PyTorch ops (float64 sums, fp32 results), on whatever device `refs` is: CPU tensors and
    shapes outside the kernel's envelope.  -> (stats [M, 10] int32, rouge [M] fp32, cider [M] fp32, lcs [M] int32)."""
    M, Tcap = _check_rows(ids, clip, refs, eos, tcap)
    ids, clip = ids[:, :Tcap].long(), clip.long()
    if bool(((clip < 0) | (clip >= refs.n_clips)).any()):
        raise ValueError("caption metrics: a clip index is outside [0, %d)" % refs.n_clips)
    outs = [_score_rows_torch(ids[i:i + block], clip[i:i + block], refs, int(eos)) for i in range(0, M, block)]
    return tuple(torch.cat([o[k] for o in outs]) for k in range(4))


def caption_score(ids, clip, refs, eos, tcap=None):
    """The kernel inside its envelope on CUDA rows, the PyTorch route otherwise -> (stats, rouge, cider)."""
    Tcap = ids.shape[1] if tcap is None else int(tcap)
    if ids.is_cuda and ids.stride(1) == 1 and in_envelope(MAX_V, Tcap) and 0 <= eos < MAX_V:
        return k_caption_score(ids, clip, refs, eos, tcap)[:3]
    return caption_score_torch(ids.contiguous(), clip, refs, eos, tcap)[:3]


def caption_rewards(ids, clip, refs, eos):
    """The per-row CIDEr-D [M] fp32 of decoded id rows, on the device: the reward of a sampled-caption objective."""
    return caption_score(ids, clip, refs, eos)[2]


class CaptionMeter(object):
    """Corpus BLEU-1..4, ROUGE-L and CIDEr over a reference table: update() scores a batch and writes the per-clip results by
    index into [C]-sized device buffers - nothing is read on the host; compute() is the one synchronisation."""

    def __init__(self, refs, eos=None):
        self.refs, self.eos = refs, eos
        C, dev = refs.n_clips, refs.device
        self.stats = torch.zeros((C, N_STATS), dtype=torch.int32, device=dev)
        self.rouge = torch.zeros((C,), dtype=torch.float32, device=dev)
        self.cider = torch.zeros((C,), dtype=torch.float32, device=dev)
        self.seen = torch.zeros((C,), dtype=torch.int32, device=dev)

    def update(self, ids, clip_index, eos=None, tcap=None):
        """ids [M, ld] id rows, clip_index [M] the rows' clips (a device tensor, or a host list of ints); eos: the id that ends a
        caption, when the meter was not given one."""
        eos = self.eos if eos is None else eos
        if eos is None:
            raise ValueError("CaptionMeter: no eos id (CaptionMeter(refs, eos=...) or update(..., eos=...))")
        if not torch.is_tensor(clip_index):
            clip_index = torch.tensor(list(clip_index), dtype=torch.int32, device=self.refs.device)
        stats, rouge, cider = caption_score(ids, clip_index, self.refs, eos, tcap)
        at = clip_index.long()
        self.stats.index_copy_(0, at, stats)
        self.rouge.index_copy_(0, at, rouge)
        self.cider.index_copy_(0, at, cider)
        self.seen.index_add_(0, at, torch.ones_like(at, dtype=torch.int32))
        return self

    def compute(self, partial=False):
        """{"Bleu_1".."Bleu_4", "ROUGE_L", "CIDEr"} times 100 (the keys and scale of eval/tvc.py): BLEU from the int64 sums of the
        statistics (bleu_scorer.py:252-261), ROUGE-L and CIDEr float64 means over the buffers in clip order - batch order does
        not matter.  Raises if a clip was scored twice or never; partial=True averages over the clips scored so far."""
        seen = self.seen.cpu()
        if int(seen.max()) > 1:
            raise ValueError("CaptionMeter: clip %d was scored %d times" % (int(seen.argmax()), int(seen.max())))
        if not partial and int(seen.min()) < 1:
            raise ValueError("CaptionMeter: %d of %d clips were never scored (first: %d)"
                             % (int((seen == 0).sum()), seen.numel(), int((seen == 0).long().argmax())))
        keep = seen > 0
        n = int(keep.sum())
        if n == 0:
            raise ValueError("CaptionMeter: nothing was scored")
        tot = self.stats.cpu()[keep].to(torch.int64).sum(dim=0).tolist()
        small, tiny = 1e-9, 1e-15
        out, bleu = {}, 1.0
        ratio = (tot[8] + tiny) / (tot[9] + small)
        brevity = math.exp(1 - 1 / ratio) if ratio < 1 else 1.0
        for k in range(ORDERS):
            bleu *= float(tot[k] + tiny) / (tot[4 + k] + small)
            out["Bleu_%d" % (k + 1)] = bleu ** (1.0 / (k + 1)) * brevity * 100
        out["ROUGE_L"] = float(self.rouge.cpu()[keep].double().sum() / n) * 100
        out["CIDEr"] = float(self.cider.cpu()[keep].double().sum() / n) * 100
        return out


@torch.no_grad()
def validate_tvc(generator, loader, refs, decode="greedy", partial=False, **decode_args):
    """The reference's validation loop (train_tvc.py:validate) without the strings: every batch is decoded with
    generator.greedy_decode / beam_decode / sample_decode (decode_args: beam_size, n_samples, temperature, ...), the id rows stay
    on the device and are scored there; batch["clip_ids"] are mapped to table rows on the host.  -> CaptionMeter.compute()."""
    calls = {"greedy": generator.greedy_decode, "beam": generator.beam_decode, "sample": generator.sample_decode}
    if decode not in calls:
        raise ValueError("validate_tvc: decode must be 'greedy', 'beam' or 'sample', got %r" % (decode,))
    if decode_args.get("return_all") or decode_args.get("return_scores"):
        raise ValueError("validate_tvc: one caption per clip is scored (no return_all / return_scores)")
    was_training = generator.model.training
    generator.model.eval()
    meter = CaptionMeter(refs, eos=generator.eos)
    try:
        for batch in loader:
            rows = calls[decode](batch, as_tensor=True, **decode_args)
            meter.update(rows.to(refs.device), refs.rows(batch["clip_ids"]))
    finally:
        generator.model.train(was_training)
    return meter.compute(partial=partial)


def teacher_forcing_rows(caption_ids, bos, eos, pad):
    """Device ops only: decoded id rows [R, T] -> (input ids [R, T] = bos + the caption shifted right, `pad` past its end;
    labels [R, T] = the caption through its first eos, -1 after; positions [1, T]).  A row without eos is all caption."""
    ids = caption_ids.long()
    R, T = ids.shape
    col = torch.arange(T, device=ids.device).unsqueeze(0)
    end = torch.where(ids == eos, col, torch.full_like(ids, T)).min(dim=1, keepdim=True).values            # the first eos, or T
    labels = torch.where(col <= end, ids, torch.full_like(ids, -1))
    shifted = torch.cat([torch.full((R, 1), bos, dtype=torch.long, device=ids.device), ids[:, :-1]], dim=1)
    inputs = torch.where(col <= end, shifted, torch.full_like(ids, pad))
    return inputs, labels, col


def reward_weighted_loss(model, batch, caption_ids, weights, eos, encoder_outputs=None, bos=0):
    """sum_rows w_row * sum_t CE(row, t) / (number of valid tokens) for caption rows [N * S, T] (row n * S + s belongs to
    caption n of the batch) through HeroForTvc's teacher-forced decoder over the encoder rows repeated per sample; the
    un-smoothed cross-entropy; gradients reach decoder and encoder.  weights [N * S] carry no gradient."""
    from . import functional as HF
    from torch.nn import functional as F
    if encoder_outputs is None:
        encoder_outputs = model.encode(batch)
    N, R = encoder_outputs.shape[0], caption_ids.shape[0]
    if R % N or tuple(weights.shape) != (R,):
        raise ValueError("reward_weighted_loss: %d caption rows and %s weights over %d captions" % (R, tuple(weights.shape), N))
    S = R // N
    pad = model.v_encoder.f_encoder.embeddings.padding_idx
    inputs, labels, col = teacher_forcing_rows(caption_ids, bos, eos, pad)
    enc = encoder_outputs.repeat_interleave(S, dim=0) if S > 1 else encoder_outputs
    mask = batch["cap_attn_mask"]
    mask = mask.repeat_interleave(S, dim=0) if S > 1 else mask
    fused = model._fused(enc, inputs)
    states = model._decoder_states(enc, mask, inputs, col, fused)
    V = model.config.f_config.vocab_size
    flat = labels.reshape(-1)
    if fused:
        logits = model.v_encoder.f_encoder.lm_head(states.reshape(-1, states.shape[-1]), raw=True)
        ce = HF.cross_entropy(logits, flat, ncols=V, ignore_index=-1)
    else:
        ce = F.cross_entropy(model._scores_torch(states).reshape(-1, V).float(), flat, ignore_index=-1, reduction="none")
    w = weights.detach().to(ce.dtype).unsqueeze(1)
    return (ce.view(R, -1) * w).sum() / (flat != -1).sum().clamp(min=1).to(ce.dtype)


def self_critical_loss(model, generator, batch, refs, clip_index, n_samples, seed=0, temperature=1.0, top_k=0, top_p=1.0):
    """Self-critical sequence training on a CIDEr-D reward: one encode; under no_grad a greedy decode and n_samples sampled
    captions per clip on the detached encoder rows, all id rows staying on the device; weights
    -(CIDEr(sample) - CIDEr(greedy caption of the same clip)); then reward_weighted_loss.  clip_index [N]: the captions' clips
    in `refs` (device int32 / int64, or a host list).  Eager only."""
    encoder_outputs = model.encode(batch)
    dev = encoder_outputs.device
    if not torch.is_tensor(clip_index):
        clip_index = torch.tensor(list(clip_index), dtype=torch.int32, device=dev)
    with torch.no_grad():
        was_training = model.training
        model.eval()
        try:
            enc = encoder_outputs.detach()
            greedy = generator.greedy_decode(batch, encoder_outputs=enc, as_tensor=True)
            sampled = generator.sample_decode(batch, n_samples=n_samples, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                              return_all=True, as_tensor=True, encoder_outputs=enc)
        finally:
            model.train(was_training)
        base = caption_rewards(greedy, clip_index, refs, generator.eos)
        reward = caption_rewards(sampled, clip_index.repeat_interleave(n_samples), refs, generator.eos)
        weights = -(reward - base.repeat_interleave(n_samples))
    return reward_weighted_loss(model, batch, sampled, weights, generator.eos, bos=generator.bos, encoder_outputs=encoder_outputs)
