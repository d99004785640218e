"""Full-corpus moment retrieval on the device: VR, SVMR and VCMR moments of a query batch against an encoded video corpus
(reference: eval_vcmr.py:143-323, validate_full_vcmr).

    index = encode_corpus(model, video_batches, max_clip_len)         # once per evaluation (eval_vcmr.py:165-203)
    out = index.search(model, query_input_ids, query_pos_ids, query_attn_masks, gt_vidx=...)   # per query batch (:209-323)

`search` runs on the hero_* kernels (hero_gemm x 2, hero_score_max_fwd, hero_topk_rows, hero_st_ed_probs, hero_moment_topk):
the reference's (Nq, K, L, L) product tensor, its host-built band mask and its full sort never exist.  `search_torch` is the
reference's formulation in PyTorch (get_pred_from_raw_query(cross=True), softmax, topk, einsum, band mask, sort) with the same
signature and result dictionary: it is what `search` takes outside the kernels' envelope, and the speed baseline.

The result dictionary (device tensors, no host synchronisation; K = min(max_vcmr_video, number of videos), N = max_before_nms):

    vr_scores    fp32  [Nq, K]   exp(q2c_alpha * score) of the K best videos, best first           (eval_vcmr.py:266-269)
    vr_indices   int32 [Nq, K]   their corpus indices
    vcmr_scores  fp32  [Nq, N]   st * video score * ed of the N best moments over those K videos     (:284-312)
    vcmr_video   int32 [Nq, N]   corpus index of each moment's video (already mapped through vr_indices)
    vcmr_st / vcmr_ed  int32 [Nq, N]   start / end FRAME index (the caller turns them into seconds, :396-400)
    svmr_scores  fp32  [Nq, N]   st * ed of the N best moments inside the ground-truth video        (:241-258, 327-338)
    svmr_st / svmr_ed  int32 [Nq, N]

Slots without a candidate (fewer than N in-band moments) hold score 0 and index -1.  Seconds, NMS, JSON and metrics stay with
the caller."""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib as L
from . import functional as HF

TASKS = ("VR", "SVMR", "VCMR")
MAX_L, MAX_K, MAX_N, MAX_NV, MAX_TAPS = 256, 128, 1024, 65536, 15          # the kernels' envelope (include/hero_hip.h)


def _need_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("hero_amd.retrieval: tensor is on %s; the retrieval path needs CUDA/ROCm tensors and has no CPU "
                               "fallback" % t.device)


def band_ok(m, n, length, min_l, max_l):
    """The kernels' candidate predicate: (start m, end n) is a moment iff min_l <= n - m < max_l and n < length - the ones of
    generate_min_max_length_mask (utils/tvr_eval_utils.py:237-260)."""
    return (n - m >= min_l) & (n - m < max_l) & (n < length) & (m >= 0)


# --------------------------------------------------------------------------------------------- #
# raw kernel wrappers
# --------------------------------------------------------------------------------------------- #
def k_topk_rows(scores, k, alpha=0.0, n=None):
    """(val [M, k] fp32, idx [M, k] int32) of the k largest of scores[:, :n] per row; alpha != 0: val = exp(alpha * score)."""
    _need_cuda(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32 or scores.stride(1) != 1:
        raise ValueError("k_topk_rows: scores must be a 2-D fp32 tensor with contiguous rows")
    M = scores.shape[0]
    n = scores.shape[1] if n is None else n
    val = torch.empty((M, k), dtype=torch.float32, device=scores.device)
    idx = torch.empty((M, k), dtype=torch.int32, device=scores.device)
    L.check(L.lib().hero_topk_rows(scores.data_ptr(), M, n, scores.stride(0) if M > 1 else scores.shape[1], k, float(alpha),
                                   L.ptr(val), L.ptr(idx), L.stream()))
    return val, idx


def k_st_ed_probs(sim, mask, sel, w_st, w_ed, length):
    """sim [Nq, >= Nv * length] fp32 (contiguous rows), mask [Nv, length] fp32, sel [Nq, K] int32 -> st_prob, ed_prob [Nq, K, length]."""
    _need_cuda(sim, mask, sel, w_st, w_ed)
    Nq, K = sel.shape
    Nv = mask.shape[0]
    if sim.stride(1) != 1 or sim.dtype != torch.float32 or sel.dtype != torch.int32:
        raise ValueError("k_st_ed_probs: sim must be fp32 with contiguous rows, sel int32")
    probs = torch.empty((2, Nq, K, length), dtype=torch.float32, device=sim.device)
    L.check(L.lib().hero_st_ed_probs(sim.data_ptr(), sim.stride(0), L.ptr(mask), L.ptr(sel), L.ptr(w_st), L.ptr(w_ed), Nq, Nv, K, length,
                                     w_st.numel(), L.ptr(probs[0]), L.ptr(probs[1]), L.stream()))
    return probs[0], probs[1]


def k_moment_topk(st_prob, ed_prob, w, min_l, max_l, top_n):
    """st_prob, ed_prob [Nq, K, L], w [Nq, K] fp32 -> (score [Nq, top_n] fp32, flat [Nq, top_n] int32 = (j L + m) L + n)."""
    _need_cuda(st_prob, ed_prob, w)
    Nq, K, Lc = st_prob.shape
    score = torch.empty((Nq, top_n), dtype=torch.float32, device=st_prob.device)
    flat = torch.empty((Nq, top_n), dtype=torch.int32, device=st_prob.device)
    L.check(L.lib().hero_moment_topk(L.ptr(st_prob), L.ptr(ed_prob), L.ptr(w), Nq, K, Lc, int(min_l), int(max_l), int(top_n),
                                     L.ptr(score), L.ptr(flat), L.stream()))
    return score, flat


def _unravel(flat, length):
    """flat = (j L + m) L + n (or -1) -> (j, m, n), -1 where flat is -1."""
    none = flat < 0
    f = flat.clamp(min=0)
    j = torch.div(f, length * length, rounding_mode="floor")
    m = torch.div(f, length, rounding_mode="floor") % length
    n = f % length
    minus = torch.full_like(flat, -1)
    return torch.where(none, minus, j), torch.where(none, minus, m), torch.where(none, minus, n)


# --------------------------------------------------------------------------------------------- #
# the index
# --------------------------------------------------------------------------------------------- #
class CorpusIndex:
    """Encoded corpus: frame_embeddings [Nv, L, D] (fp32 view of the GEMM operand), masks [Nv, L], and - on the device - the two
    fp32 GEMM operands of a search, built once: the frame rows and their row-normalised copy (F.normalize(eps=1e-5),
    model/pretrain.py:364-372), both padded to a multiple of 4 rows (hero_gemm's output width rule)."""

    def __init__(self, frame_embeddings, masks):
        if frame_embeddings.dim() != 3 or masks.shape != frame_embeddings.shape[:2]:
            raise ValueError("CorpusIndex: frame_embeddings [Nv, L, D] and masks [Nv, L] expected")
        self.n_videos, self.length, self.dim = frame_embeddings.shape
        self.dtype = frame_embeddings.dtype                     # what the encoder produced (bf16 values are exact in fp32)
        self.masks = masks.contiguous()
        rows = self.n_videos * self.length
        self.ld = (rows + 3) & ~3
        ctx = frame_embeddings.new_zeros((self.ld, self.dim), dtype=torch.float32)
        ctx[:rows] = frame_embeddings.reshape(rows, self.dim)
        self.ctx = ctx
        self.frame_embeddings = ctx[:rows].view(self.n_videos, self.length, self.dim)
        self.mask_f32 = self.masks.to(torch.float32).contiguous()
        self.ctx_norm = None
        if ctx.is_cuda:
            from .head import RowNormFn
            with torch.no_grad():
                self.ctx_norm = RowNormFn.apply(ctx, 1e-5)

    def search(self, model, query_input_ids, query_pos_ids, query_attn_masks, *, tasks=TASKS, gt_vidx=None, q2c_alpha=20,
               max_vcmr_video=100, min_pred_l=2, max_pred_l=16, max_before_nms=200):
        return search(self, model, query_input_ids, query_pos_ids, query_attn_masks, tasks=tasks, gt_vidx=gt_vidx,
                      q2c_alpha=q2c_alpha, max_vcmr_video=max_vcmr_video, min_pred_l=min_pred_l, max_pred_l=max_pred_l,
                      max_before_nms=max_before_nms)

    def search_torch(self, model, query_input_ids, query_pos_ids, query_attn_masks, **kw):
        return search_torch(self, model, query_input_ids, query_pos_ids, query_attn_masks, **kw)


@torch.no_grad()
def encode_corpus(model, video_batches, max_clip_len):
    """eval_vcmr.py:165-203: v_encoder(batch, 'repr') per video batch, rows written into a zero (Nv, max_clip_len, D) tensor and
    masks into (Nv, max_clip_len), both trimmed to the longest clip seen.  Videos are numbered in the order they come."""
    model.eval()
    video_batches = list(video_batches)
    n_videos = sum(int(b["c_attn_masks"].shape[0]) for b in video_batches)
    total = total_masks = None
    seen, at = 0, 0
    for batch in video_batches:
        emb = model.v_encoder(batch, "repr")
        cmask = batch["c_attn_masks"]
        n, clip_len = emb.shape[0], emb.shape[-2]
        if clip_len > max_clip_len:
            raise ValueError("encode_corpus: a batch has %d frames per clip, max_clip_len is %d" % (clip_len, max_clip_len))
        if total is None:
            total = emb.new_zeros((n_videos, max_clip_len, emb.shape[-1]))
            total_masks = cmask.new_zeros((n_videos, max_clip_len))
        total[at:at + n, :clip_len] = emb
        total_masks[at:at + n, :clip_len] = cmask
        seen = max(seen, clip_len)
        at += n
    if total is None:
        raise ValueError("encode_corpus: no video batch")
    return CorpusIndex(total[:, :seen], total_masks[:, :seen])


def _fusable(index, model, K, N, min_l, max_l):
    convs = (model.video_st_predictor, model.video_ed_predictor)
    return (all(c.stride[0] == 1 and c.kernel_size[0] % 2 == 1 and c.kernel_size[0] <= MAX_TAPS for c in convs)
            and index.length <= MAX_L and K <= MAX_K and N <= MAX_N and index.n_videos <= MAX_NV and index.dim % 4 == 0
            and 0 <= min_l < max_l)


def _check_tasks(tasks):
    tasks = tuple(tasks)
    bad = [t for t in tasks if t not in TASKS]
    if bad:
        raise ValueError("unknown retrieval tasks %s (of %s)" % (bad, TASKS))
    return tasks


@torch.no_grad()
def search(index, model, query_input_ids, query_pos_ids, query_attn_masks, *, tasks=TASKS, gt_vidx=None, q2c_alpha=20,
           max_vcmr_video=100, min_pred_l=2, max_pred_l=16, max_before_nms=200):
    """One query batch against the index on the HIP kernels (module docstring); raises on CPU tensors.  Configurations outside
    the kernels' envelope (conv stride != 1, even or > 15 taps, L > 256, K > 128, N > 1024) go to `search_torch`."""
    _need_cuda(index.ctx, query_input_ids, query_attn_masks, gt_vidx)
    tasks = _check_tasks(tasks)
    K, N = min(int(max_vcmr_video), index.n_videos), int(max_before_nms)
    if not _fusable(index, model, K, N, min_pred_l, max_pred_l):
        return search_torch(index, model, query_input_ids, query_pos_ids, query_attn_masks, tasks=tasks, gt_vidx=gt_vidx,
                            q2c_alpha=q2c_alpha, max_vcmr_video=max_vcmr_video, min_pred_l=min_pred_l, max_pred_l=max_pred_l,
                            max_before_nms=max_before_nms)
    from .head import RowNormFn
    model.eval()
    Nv, Lc, D, ld = index.n_videos, index.length, index.dim, index.ld
    dev = index.ctx.device
    mod_q = model.encode_txt_inputs(query_input_ids, query_pos_ids, query_attn_masks, attn_layer=model.q_feat_attn).float().contiguous()
    Nq = mod_q.shape[0]
    out = {}
    w_st = model.video_st_predictor.weight.detach().reshape(-1).float().contiguous()
    w_ed = model.video_ed_predictor.weight.detach().reshape(-1).float().contiguous()
    sim = None

    def similarities():
        q2 = HF.linear(mod_q, model.video_query_linear.weight, model.video_query_linear.bias).float().contiguous()
        s = torch.empty((Nq, ld), dtype=torch.float32, device=dev)
        HF.k_gemm(q2, index.ctx, s, Nq, ld, D, D, D, ld, L.LAYOUT_K, L.LAYOUT_K, L.F32)
        return s

    if "VR" in tasks or "VCMR" in tasks:
        qn = RowNormFn.apply(mod_q, 1e-5)
        s = torch.empty((Nq, ld), dtype=torch.float32, device=dev)
        HF.k_gemm(qn, index.ctx_norm, s, Nq, ld, D, D, D, ld, L.LAYOUT_K, L.LAYOUT_K, L.F32)
        q2v = torch.empty((Nq, Nv), dtype=torch.float32, device=dev)
        arg = torch.empty((Nq, Nv), dtype=torch.int32, device=dev)
        a = L.ScoreMax()
        a.s, a.mask, a.out, a.arg = L.ptr(s), L.ptr(index.mask_f32), L.ptr(q2v), L.ptr(arg)
        a.M, a.N, a.L, a.D, a.ld_s = Nq, Nv, Lc, D, ld
        L.check(L.lib().hero_score_max_fwd(C.byref(a), L.stream()))
        vr_scores, vr_indices = k_topk_rows(q2v, K, alpha=float(q2c_alpha))
        out["vr_scores"], out["vr_indices"] = vr_scores, vr_indices
        if "VCMR" in tasks:
            sim = similarities()
            st, ed = k_st_ed_probs(sim, index.mask_f32, vr_indices, w_st, w_ed, Lc)
            score, flat = k_moment_topk(st, ed, vr_scores, min_pred_l, max_pred_l, N)
            j, m, n = _unravel(flat, Lc)
            video = torch.gather(vr_indices, 1, j.clamp(min=0).long())
            out["vcmr_scores"] = score
            out["vcmr_video"] = torch.where(j < 0, j, video)
            out["vcmr_st"], out["vcmr_ed"] = m, n
    if "SVMR" in tasks and gt_vidx is not None:
        if sim is None:
            sim = similarities()
        sel = gt_vidx.reshape(Nq, 1).to(torch.int32).contiguous()
        st, ed = k_st_ed_probs(sim, index.mask_f32, sel, w_st, w_ed, Lc)
        score, flat = k_moment_topk(st, ed, torch.ones((Nq, 1), dtype=torch.float32, device=dev), min_pred_l, max_pred_l, N)
        _, m, n = _unravel(flat, Lc)
        out["svmr_scores"], out["svmr_st"], out["svmr_ed"] = score, m, n
    return out


def _sorted_moments(products, min_l, max_l, top_n):
    """products [Nq, K, L, L] (K may be 1) -> the reference's band mask, flatten, full sort, first top_n (eval_vcmr.py:292-312);
    slots that the sort filled with masked (out-of-band) entries become score 0, index -1."""
    Nq, K, Lc, _ = products.shape
    r = torch.arange(Lc, device=products.device)
    band = band_ok(r.view(Lc, 1), r.view(1, Lc), Lc, min_l, max_l).to(products.dtype)       # generate_min_max_length_mask
    products = products * band
    score, flat = torch.sort(products.reshape(Nq, -1), dim=1, descending=True)
    score, flat = score[:, :top_n], flat[:, :top_n]
    if score.shape[1] < top_n:
        pad = top_n - score.shape[1]
        score, flat = F.pad(score, (0, pad)), F.pad(flat, (0, pad), value=-1)
    m = torch.div(flat, Lc, rounding_mode="floor") % Lc
    n = flat % Lc
    real = band_ok(m, n, Lc, min_l, max_l) & (flat >= 0)
    return torch.where(real, score, torch.zeros_like(score)), torch.where(real, flat, torch.full_like(flat, -1)).to(torch.int32)


@torch.no_grad()
def search_torch(index, model, query_input_ids, query_pos_ids, query_attn_masks, *, tasks=TASKS, gt_vidx=None, q2c_alpha=20,
                 max_vcmr_video=100, min_pred_l=2, max_pred_l=16, max_before_nms=200):
    """The reference's formulation (eval_vcmr.py:232-323, 327-338) in PyTorch, same result dictionary as `search`."""
    _need_cuda(index.ctx, query_input_ids, query_attn_masks, gt_vidx)
    tasks = _check_tasks(tasks)
    model.eval()
    Lc = index.length
    K, N = min(int(max_vcmr_video), index.n_videos), int(max_before_nms)
    q2v, st, ed = model.get_pred_from_raw_query(index.frame_embeddings, index.masks, query_input_ids, query_pos_ids,
                                                query_attn_masks, cross=True, val_gather_gpus=False)
    st, ed = F.softmax(st.float(), dim=-1), F.softmax(ed.float(), dim=-1)
    Nq = st.shape[0]
    rows = torch.arange(Nq, device=st.device)
    out = {}
    if "VR" in tasks or "VCMR" in tasks:
        if q2v is None:                         # lw_neg_ctx == lw_neg_q == 0: get_pred_from_raw_query skipped the video scores
            mod_q = model.encode_txt_inputs(query_input_ids, query_pos_ids, query_attn_masks, attn_layer=model.q_feat_attn)
            q2v = model.get_video_level_scores(mod_q, index.frame_embeddings, index.masks, val_gather_gpus=False)
        vr_scores, vr_indices = torch.topk(torch.exp(q2c_alpha * q2v.float()), K, dim=1, largest=True)
        out["vr_scores"], out["vr_indices"] = vr_scores, vr_indices.to(torch.int32)
        if "VCMR" in tasks:
            st_k, ed_k = st[rows.unsqueeze(1), vr_indices], ed[rows.unsqueeze(1), vr_indices]
            score, flat = _sorted_moments(torch.einsum("qvm,qv,qvn->qvmn", st_k, vr_scores, ed_k), min_pred_l, max_pred_l, N)
            j, m, n = _unravel(flat, Lc)
            video = torch.gather(out["vr_indices"], 1, j.clamp(min=0).long())
            out["vcmr_scores"] = score
            out["vcmr_video"] = torch.where(j < 0, j, video)
            out["vcmr_st"], out["vcmr_ed"] = m, n
    if "SVMR" in tasks and gt_vidx is not None:
        g = gt_vidx.reshape(Nq).long()
        score, flat = _sorted_moments(torch.einsum("bm,bn->bmn", st[rows, g], ed[rows, g]).unsqueeze(1), min_pred_l, max_pred_l, N)
        _, m, n = _unravel(flat, Lc)
        out["svmr_scores"], out["svmr_st"], out["svmr_ed"] = score, m, n
    return out
