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

Slots without a candidate (fewer than N in-band moments) hold score 0 and index -1.

What follows a search is on the device too (hero_moment_nms, hero_first_hit; no host synchronisation before `compute`):

    post = postprocess(out, vfeat_interval=1.5, nms_thd=0.5, max_after_nms=100)    # seconds, temporal NMS, truncation (:345-348, 396-400, 458-478)
    meter.update(post, gt_vidx, gt_ts, desc_type)                                    # RecallMeter: hit counts of R@K at IoU thresholds
    metrics = meter.compute()                                                        # the dictionary of eval_retrieval, one synchronisation

Ground truth with several annotators per query (DiDeMo) goes through `pack_gt_ts` and `meter.update(post, gt_vidx, gt_ts, gt_n=gt_n)`
(hero_first_hit_multi); hero_amd/retrieval_eval.py holds the drivers that return the reference's val_log and submission.

`postprocess_host` is the reference's post-processing restated on the host (utils/tvr_eval_utils.py:35-92, 132-234): what
`postprocess` takes beyond N = 1024, and the speed baseline.  Writing the prediction JSON stays with the caller."""
import ctypes as C

import numpy as np
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


def k_moment_nms(video, st, ed, thd, per_video_cap=100, max_after=None):
    """video, st, ed int32 [Nq, N] (frame indices, ed inclusive, rows best first, -1 = vacant) -> (keep [Nq, max_after] int32:
    positions of the survivors of the greedy temporal NMS, ascending, -1 in unused slots; count [Nq] int32).  include/hero_hip.h."""
    _need_cuda(video, st, ed)
    for t in (video, st, ed):
        if t.dim() != 2 or t.dtype != torch.int32 or not t.is_contiguous() or t.shape != video.shape:
            raise ValueError("k_moment_nms: video, st and ed must be contiguous int32 [Nq, N] tensors of one shape")
    Nq, N = video.shape
    max_after = N if max_after is None else int(max_after)
    keep = torch.empty((Nq, max(max_after, 0)), dtype=torch.int32, device=video.device)
    count = torch.empty((Nq,), dtype=torch.int32, device=video.device)
    L.check(L.lib().hero_moment_nms(L.ptr(video), L.ptr(st), L.ptr(ed), Nq, N, float(thd), int(per_video_cap), max_after, L.ptr(keep),
                                    L.ptr(count), L.stream()))
    return keep, count


def k_first_hit(video, gt_video, st=None, ed=None, gt_ts=None, interval=1.5, thds=None, n_pred=None):
    """video (, st, ed) int32 [Nq, >= n_pred] with contiguous rows, gt_video int32 [Nq], gt_ts fp32 [Nq, 2] seconds, thds fp32 [T]
    on the device -> first [Nq, T + 1] int32: rank of the first prediction in the ground-truth video (column 0) and of the first
    one there with IoU >= thds[t] (column 1 + t) among the first n_pred columns; n_pred where there is none."""
    _need_cuda(video, gt_video, st, ed, gt_ts, thds)
    if (st is None) != (ed is None):
        raise ValueError("k_first_hit: st and ed are given together or not at all")
    for t in (video, st, ed):
        if t is not None and (t.dim() != 2 or t.dtype != torch.int32 or t.stride(1) != 1 or t.shape != video.shape or t.stride(0) != video.stride(0)):
            raise ValueError("k_first_hit: video, st and ed must be int32 [Nq, P] tensors of one shape and row stride, rows contiguous")
    Nq, cols = video.shape
    if gt_video.dtype != torch.int32 or gt_video.shape != (Nq,) or not gt_video.is_contiguous():
        raise ValueError("k_first_hit: gt_video must be a contiguous int32 [Nq] tensor")
    T = 0 if thds is None else int(thds.numel())
    if T:
        if thds.dtype != torch.float32 or not thds.is_contiguous():
            raise ValueError("k_first_hit: thds must be a contiguous fp32 tensor")
        if st is None or gt_ts is None or gt_ts.dtype != torch.float32 or gt_ts.shape != (Nq, 2) or not gt_ts.is_contiguous():
            raise ValueError("k_first_hit: IoU thresholds need st, ed and a contiguous fp32 gt_ts [Nq, 2]")
    n_pred = cols if n_pred is None else min(int(n_pred), cols)
    first = torch.empty((Nq, T + 1), dtype=torch.int32, device=video.device)
    ld = video.stride(0) if Nq > 1 else cols
    L.check(L.lib().hero_first_hit(video.data_ptr(), None if st is None else st.data_ptr(), None if ed is None else ed.data_ptr(), Nq, n_pred, ld,
                                   L.ptr(gt_video), L.ptr(gt_ts) if T else None, float(interval), L.ptr(thds) if T else None, T, L.ptr(first),
                                   L.stream()))
    return first


MAX_GT = 16          # annotators per query hero_first_hit_multi takes (include/hero_hip.h)


def k_first_hit_multi(video, gt_video, st, ed, gt_ts, gt_n, interval=1.5, thds=None, n_pred=None):
    """`k_first_hit` for ground truth with several annotators (DiDeMo): gt_ts fp32 [Nq, G, 2] seconds (padded, G <= 16), gt_n
    int32 [Nq] = the real timestamps of each query.  Column 1 + t of first [Nq, T + 1] is the rank of the first prediction in
    the ground-truth video at which at least `need` timestamps have IoU >= thds[t]; need = 2 from four timestamps on
    (utils/tvr_standalone_eval.py:159-170), else 1.  Slots at index >= gt_n[q] are never read."""
    _need_cuda(video, gt_video, st, ed, gt_ts, gt_n, thds)
    if (st is None) != (ed is None):
        raise ValueError("k_first_hit_multi: st and ed are given together or not at all")
    for t in (video, st, ed):
        if t is not None and (t.dim() != 2 or t.dtype != torch.int32 or t.stride(1) != 1 or t.shape != video.shape or t.stride(0) != video.stride(0)):
            raise ValueError("k_first_hit_multi: video, st and ed must be int32 [Nq, P] tensors of one shape and row stride, rows contiguous")
    Nq, cols = video.shape
    if gt_video.dtype != torch.int32 or gt_video.shape != (Nq,) or not gt_video.is_contiguous():
        raise ValueError("k_first_hit_multi: gt_video must be a contiguous int32 [Nq] tensor")
    T = 0 if thds is None else int(thds.numel())
    G = 1
    if gt_ts is not None or gt_n is not None:
        if (gt_ts is None or gt_n is None or gt_ts.dtype != torch.float32 or gt_ts.dim() != 3 or gt_ts.shape[0] != Nq or gt_ts.shape[2] != 2
                or not gt_ts.is_contiguous() or gt_n.dtype != torch.int32 or gt_n.shape != (Nq,) or not gt_n.is_contiguous()):
            raise ValueError("k_first_hit_multi: gt_ts must be a contiguous fp32 [Nq, G, 2] tensor and gt_n a contiguous int32 [Nq] tensor")
        G = int(gt_ts.shape[1])
    if T:
        if thds.dtype != torch.float32 or not thds.is_contiguous():
            raise ValueError("k_first_hit_multi: thds must be a contiguous fp32 tensor")
        if st is None or gt_ts is None:
            raise ValueError("k_first_hit_multi: IoU thresholds need st, ed, gt_ts and gt_n")
    n_pred = cols if n_pred is None else min(int(n_pred), cols)
    first = torch.empty((Nq, T + 1), dtype=torch.int32, device=video.device)
    ld = video.stride(0) if Nq > 1 else cols
    L.check(L.lib().hero_first_hit_multi(video.data_ptr(), None if st is None else st.data_ptr(), None if ed is None else ed.data_ptr(), Nq, n_pred,
                                         ld, L.ptr(gt_video), L.ptr(gt_ts) if T else None, L.ptr(gt_n) if T else None, G, float(interval),
                                         L.ptr(thds) if T else None, T, L.ptr(first), L.stream()))
    return first


def pack_gt_ts(ts_list):
    """Ground-truth timestamps as the reference's JSON holds them - per query either [st, ed] (TVR, How2R) or a list of at least
    four [st, ed] pairs (DiDeMo's annotators) - on the host -> (gt_ts fp32 [Nq, G, 2] zero-padded, gt_n int32 [Nq]): the inputs
    of `k_first_hit_multi` / `RecallMeter.update`.  Two or three pairs raise: eval_by_task_type takes `len(ts) >= 4` for the
    annotator list and everything shorter for ONE [st, ed], which a list of two or three pairs is not
    (utils/tvr_standalone_eval.py:159, 172-173).  More than 16 pairs raise: the kernel's envelope."""
    rows = []
    for q, ts in enumerate(ts_list):
        ts = list(ts)
        if len(ts) == 2 and not isinstance(ts[0], (list, tuple, np.ndarray)):
            rows.append([[float(ts[0]), float(ts[1])]])
            continue
        if not all(isinstance(p, (list, tuple, np.ndarray)) and len(p) == 2 for p in ts):
            raise ValueError("pack_gt_ts: query %d: expected [st, ed] or a list of [st, ed] pairs, got %r" % (q, ts))
        if len(ts) < 4:
            raise ValueError("pack_gt_ts: query %d has %d timestamps: the reference's rule is defined for one or for at least four" % (q, len(ts)))
        if len(ts) > MAX_GT:
            raise ValueError("pack_gt_ts: query %d has %d timestamps, at most %d are supported" % (q, len(ts), MAX_GT))
        rows.append([[float(p[0]), float(p[1])] for p in ts])
    if not rows:
        raise ValueError("pack_gt_ts: no query")
    G = max(len(r) for r in rows)
    gt_ts = np.zeros((len(rows), G, 2), dtype=np.float32)
    for q, r in enumerate(rows):
        gt_ts[q, :len(r)] = np.asarray(r, dtype=np.float32)
    return torch.from_numpy(gt_ts), torch.tensor([len(r) for r in rows], dtype=torch.int32)


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


# --------------------------------------------------------------------------------------------- #
# after the search: seconds, temporal NMS, truncation, recall
# --------------------------------------------------------------------------------------------- #
MOMENT_TASKS = ("vcmr", "svmr")


def _gather_survivors(out, task, keep, count, interval, A):
    """keep [Nq, <= A] positions (-1 = unused) -> the TASK_nms_* tensors, padded to A columns."""
    if keep.shape[1] < A:
        keep = F.pad(keep, (0, A - keep.shape[1]), value=-1)
    none = keep < 0
    at = keep.clamp(min=0).long()
    minus = torch.full_like(keep, -1)

    def take(x, empty):
        return torch.where(none, empty, torch.gather(x, 1, at))

    zero = torch.zeros((), dtype=torch.float32, device=keep.device)
    post = {task + "_nms_scores": take(out[task + "_scores"], zero)}
    if task == "vcmr":
        post["vcmr_nms_video"] = take(out["vcmr_video"], minus)
    st, ed = take(out[task + "_st"], minus), take(out[task + "_ed"], minus)
    post[task + "_nms_st"], post[task + "_nms_ed"] = st, ed
    post[task + "_nms_st_sec"] = torch.where(none, zero, st.to(torch.float32) * interval)                 # eval_vcmr.py:396-397
    post[task + "_nms_ed_sec"] = torch.where(none, zero, (ed + 1).to(torch.float32) * interval)           # :345-348, 398-400
    post[task + "_nms_count"] = count
    return post


def _first_columns(st, A):
    """No NMS (nms_thd == -1, eval_vcmr.py:458): the first A columns as they are."""
    N = st.shape[1]
    col = torch.arange(min(A, N), dtype=torch.int32, device=st.device).unsqueeze(0)
    keep = torch.where(st[:, :min(A, N)] >= 0, col, torch.full_like(col, -1))
    return keep, (keep >= 0).sum(1).to(torch.int32)


def _carry_video_lists(out, post):
    for k in ("vr_scores", "vr_indices"):               # the VR lists need no post-processing: RecallMeter finds them here
        if k in out:
            post[k] = out[k]
    return post


@torch.no_grad()
def postprocess(out, *, vfeat_interval=1.5, nms_thd=0.5, max_after_nms=100, per_video_cap=100):
    """Seconds, temporal NMS and truncation of a result dictionary of `search` / `search_torch`, on the device, without a host
    synchronisation.  For TASK in vcmr, svmr (whichever `out` holds), with A = max_after_nms:

        TASK_nms_scores  fp32  [Nq, A]   the survivors of the greedy NMS (hero_moment_nms; include/hero_hip.h), best first
        vcmr_nms_video   int32 [Nq, A]
        TASK_nms_st / TASK_nms_ed          int32 [Nq, A]   frame indices
        TASK_nms_st_sec / TASK_nms_ed_sec  fp32  [Nq, A]   st * vfeat_interval / (ed + 1) * vfeat_interval (eval_vcmr.py:345-348, 396-400)
        TASK_nms_count   int32 [Nq]

    Vacant slots hold score 0, index -1 and seconds 0.  nms_thd == -1: no NMS, the first A columns (eval_vcmr.py:458).
    per_video_cap = 100 is the reference's quirk: at most 100 survivors per video, whatever max_after_nms is (its inner
    function never gets max_after_nms, utils/tvr_eval_utils.py:159-160, 229-230).  vr_scores / vr_indices are carried over
    unchanged.  More than 1024 candidates per row go to `postprocess_host`."""
    A = int(max_after_nms)
    if A < 1:
        raise ValueError("postprocess: max_after_nms must be >= 1")
    tasks = [t for t in MOMENT_TASKS if t + "_scores" in out]
    if any(out[t + "_st"].shape[1] > MAX_N for t in tasks):
        return postprocess_host(out, vfeat_interval=vfeat_interval, nms_thd=nms_thd, max_after_nms=max_after_nms, per_video_cap=per_video_cap)
    post = {}
    for task in tasks:
        st, ed = out[task + "_st"], out[task + "_ed"]
        _need_cuda(st, ed, out[task + "_scores"])
        if nms_thd == -1:
            keep, count = _first_columns(st, A)
        else:
            video = out["vcmr_video"] if task == "vcmr" else st.clamp(min=-1, max=0)       # one video: group 0, -1 where vacant
            keep, count = k_moment_nms(video.contiguous(), st.contiguous(), ed.contiguous(), nms_thd, per_video_cap, min(A, st.shape[1]))
        post.update(_gather_survivors(out, task, keep, count, float(vfeat_interval), A))
    return _carry_video_lists(out, post)


def nms_rows_host(video, st, ed, thd, per_video_cap, max_after, interval=1.5):
    """The reference's NMS (utils/tvr_eval_utils.py:35-92 inside :132-175 / :214-234) restated per row in Python: video, st, ed
    integer arrays [Nq, N], rows best first, -1 = vacant.  A candidate falls iff an earlier SURVIVOR of its video overlaps it
    with IoU > thd (IoU of the spans in seconds, Python floats, "union" = the hull); a video keeps at most per_video_cap; the
    first max_after survivors of the row are the result.  -> (keep [Nq, max_after] int32, count [Nq] int32)."""
    video, st, ed = (np.asarray(x) for x in (video, st, ed))
    Nq, N = st.shape
    sec0 = (st.astype(np.float32) * np.float32(interval)).tolist()
    sec1 = ((ed + 1).astype(np.float32) * np.float32(interval)).tolist()
    vid, vacant = video.tolist(), ((video < 0) | (st < 0)).tolist()
    keep = np.full((Nq, max_after), -1, dtype=np.int32)
    count = np.zeros((Nq,), dtype=np.int32)
    for q in range(Nq):
        survivors = {}                      # video -> [(start, end)] of its survivors
        n = 0
        for i in range(N):
            if n >= max_after:
                break
            if vacant[q][i]:
                continue
            mine = survivors.setdefault(vid[q][i], [])
            if len(mine) >= per_video_cap:
                continue
            a0, a1 = sec0[q][i], sec1[q][i]
            for b0, b1 in mine:
                hull = max(a1, b1) - min(a0, b0)
                if (max(0.0, min(a1, b1) - max(a0, b0)) / hull if hull != 0 else 0.0) > thd:
                    break
            else:
                mine.append((a0, a1))
                keep[q, n] = i
                n += 1
        count[q] = n
    return keep, count


@torch.no_grad()
def postprocess_host(out, *, vfeat_interval=1.5, nms_thd=0.5, max_after_nms=100, per_video_cap=100):
    """`postprocess` on the host: the reference's algorithm in Python / numpy (`nms_rows_host`), any number of candidates, CPU or
    device tensors in (device tensors are copied: this synchronises), tensors on the input's device out.  The device path
    agrees with it bit for bit wherever frame index * vfeat_interval is exact in fp32 (1.5, 2, ...: then the IoU of seconds
    and the IoU of frame counts are the same rational number)."""
    A = int(max_after_nms)
    if A < 1:
        raise ValueError("postprocess_host: max_after_nms must be >= 1")
    post = {}
    for task in (t for t in MOMENT_TASKS if t + "_scores" in out):
        st, ed = out[task + "_st"], out[task + "_ed"]
        if nms_thd == -1:
            keep, count = _first_columns(st, A)
        else:
            st_h, ed_h = st.cpu().numpy(), ed.cpu().numpy()
            video = out["vcmr_video"].cpu().numpy() if task == "vcmr" else np.clip(st_h, -1, 0)
            keep, count = nms_rows_host(video, st_h, ed_h, float(nms_thd), int(per_video_cap), min(A, st.shape[1]), float(vfeat_interval))
            keep, count = torch.from_numpy(keep).to(st.device), torch.from_numpy(count).to(st.device)
        post.update(_gather_survivors(out, task, keep, count, float(vfeat_interval), A))
    return _carry_video_lists(out, post)


class RecallMeter:
    """R@K at IoU thresholds of VCMR and SVMR and R@K of VR, accumulated on the device over query batches: the metrics of
    eval_retrieval (utils/tvr_standalone_eval.py:86-283) without its per-query matrices.

        meter = RecallMeter()
        for each query batch:  meter.update(postprocess(index.search(...)), gt_vidx, gt_ts, desc_type)     # no host synchronisation
        meter.compute()  ->  {"VCMR": {"0.5-r1": ..}, "SVMR": {..}, "VR": {"r1": ..}, "VCMR_by_type": {"v-0.5-r1": .., "desc_type_ratio": ..}, ..}

    A query counts for R@K at a threshold when hero_first_hit's rank of its first correct prediction is below K.  In the
    reference's SVMR branch ranks are counted among the predictions in the ground-truth video; every SVMR prediction is in that
    video, so this is the plain rank.  Ground truth is one [st, ed] per query (TVR, How2R; hero_first_hit) or several
    annotators' timestamps (DiDeMo: from four on, two must reach the threshold; `pack_gt_ts`, hero_first_hit_multi).  Pass `device` to allocate the counters at construction
    (needed before capturing `update` in a graph); otherwise the first update allocates them."""

    TASKS = ("VCMR", "SVMR", "VR")
    TYPES = ("v", "t", "vt")

    def __init__(self, iou_thds=(0.5, 0.7), topks=(1, 5, 10, 100), max_pred_per_query=100, vfeat_interval=1.5, device=None):
        self.iou_thds, self.topks = tuple(float(t) for t in iou_thds), tuple(int(k) for k in topks)
        if len(self.iou_thds) > 8:
            raise ValueError("RecallMeter: at most 8 IoU thresholds")
        self.max_pred_per_query, self.vfeat_interval = int(max_pred_per_query), float(vfeat_interval)
        self.hits = self.n = None
        self.typed = False
        if device is not None:
            self._allocate(torch.device(device))

    def _allocate(self, device):
        T, K = len(self.iou_thds), len(self.topks)
        self.hits = torch.zeros((3, 4, T + 1, K), dtype=torch.int64, device=device)        # task, (all, v, t, vt), column of first_hit, K
        self.n = torch.zeros((3, 4), dtype=torch.int64, device=device)
        self._thds = torch.tensor(self.iou_thds, dtype=torch.float32, device=device)
        self._topks = torch.tensor(self.topks, dtype=torch.int32, device=device)
        self._types = torch.arange(3, device=device).view(1, 3)

    def reset(self):
        if self.hits is not None:
            self.hits.zero_()
            self.n.zero_()
        self.typed = False

    def add_first(self, task, first, n_pred, desc_type=None):
        """Accumulate first-hit ranks [Nq, T + 1] (hero_first_hit's output; `n_pred` = none) of one task; any device."""
        if self.hits is None:
            self._allocate(first.device)
        ti = self.TASKS.index(task)
        hit = first.unsqueeze(-1) < self._topks.clamp(max=int(n_pred)).view(1, 1, -1)                  # [Nq, T + 1, K]; rank n_pred = no hit
        self.hits[ti, 0] += hit.sum(0)
        self.n[ti, 0] += first.shape[0]
        if desc_type is not None:
            of_type = desc_type.view(-1, 1).to(self._types.dtype) == self._types                             # [Nq, 3]
            self.hits[ti, 1:] += (of_type.view(-1, 3, 1, 1) & hit.unsqueeze(1)).sum(0)
            self.n[ti, 1:] += of_type.sum(0)
            self.typed = True

    @torch.no_grad()
    def update(self, out_or_post, gt_vidx, gt_ts=None, desc_type=None, gt_n=None):
        """One query batch.  out_or_post: a dictionary of `postprocess` (TASK_nms_* keys, preferred) and / or of `search`; VR is read
        from vr_indices.  gt_vidx int [Nq]; gt_ts fp32 [Nq, 2] seconds (without it only VR is counted), or fp32 [Nq, G, 2] with
        gt_n int [Nq] (`pack_gt_ts`: several annotators per query); desc_type optional int [Nq], 0 / 1 / 2 = v / t / vt.  Only the
        first max_pred_per_query predictions count.  Enqueues kernels, never waits for them."""
        d = out_or_post
        gt = gt_vidx.reshape(-1).to(torch.int32).contiguous()
        _need_cuda(gt, gt_ts, desc_type, gt_n)
        if self.hits is None:
            self._allocate(gt.device)
        multi = gt_ts is not None and gt_ts.dim() == 3
        if multi:
            if gt_n is None:
                raise ValueError("RecallMeter.update: gt_ts [Nq, G, 2] needs gt_n [Nq] (pack_gt_ts gives both)")
            ts, n = gt_ts.to(torch.float32).contiguous(), gt_n.reshape(-1).to(torch.int32).contiguous()
        else:
            if gt_n is not None:
                raise ValueError("RecallMeter.update: gt_n goes with a 3-D gt_ts [Nq, G, 2]")
            ts = None if gt_ts is None else gt_ts.to(torch.float32).reshape(-1, 2).contiguous()
        for task in MOMENT_TASKS:
            pre = task + "_nms_" if task + "_nms_st" in d else task + "_"
            if pre + "st" not in d or ts is None:
                continue
            st, ed = d[pre + "st"], d[pre + "ed"]
            video = d[pre + "video"] if task == "vcmr" else torch.where(st >= 0, gt.view(-1, 1), torch.full_like(st, -1))
            thds = self._thds if self.iou_thds else None
            if multi:
                first = k_first_hit_multi(video, gt, st, ed, ts, n, self.vfeat_interval, thds, self.max_pred_per_query)
            else:
                first = k_first_hit(video, gt, st, ed, ts, self.vfeat_interval, thds, self.max_pred_per_query)
            self.add_first(task.upper(), first, min(self.max_pred_per_query, st.shape[1]), desc_type)
        if "vr_indices" in d:
            vi = d["vr_indices"]
            first = k_first_hit(vi, gt, n_pred=self.max_pred_per_query)
            first = first.expand(-1, len(self.iou_thds) + 1)                      # VR has one column; the counters are one shape
            self.add_first("VR", first, min(self.max_pred_per_query, vi.shape[1]), desc_type)

    def compute(self):
        """The one synchronisation: the nested dictionary of eval_retrieval with its keys and its rounding, round(100 * x, 2)."""
        if self.hits is None:
            return {}
        hits, n = self.hits.cpu().numpy(), self.n.cpu().numpy()

        def pct(a, b):
            with np.errstate(divide="ignore", invalid="ignore"):
                return float(round(np.float64(a) / np.float64(b) * 100, 2))         # numpy's rounding, as get_rounded_percentage applies it

        def table(ti, row, prefix):
            if self.TASKS[ti] == "VR":
                return {"%sr%d" % (prefix, k): pct(hits[ti, row, 0, j], n[ti, row]) for j, k in enumerate(self.topks)}
            return {"%s%s-r%d" % (prefix, thd, k): pct(hits[ti, row, 1 + t, j], n[ti, row])
                    for t, thd in enumerate(self.iou_thds) for j, k in enumerate(self.topks)}

        present = [ti for ti in range(3) if n[ti, 0] > 0]
        res = {self.TASKS[ti]: table(ti, 0, "") for ti in present}
        if self.typed:
            for ti in present:
                by = {}
                for c, name in enumerate(self.TYPES):
                    by.update(table(ti, 1 + c, name + "-"))
                by["desc_type_ratio"] = "v {} t {} vt {}".format(*[pct(n[ti, 1 + c], n[ti, 0]) for c in range(3)])
                res[self.TASKS[ti] + "_by_type"] = by
        return res
