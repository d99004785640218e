"""The batch boundary: HERO's collate functions (host half) and their device half.

Host half - same names, inputs and outputs as the reference, so a reference DataLoader can take these as
`collate_fn` unchanged (pinned by tests/golden/case_collate.npz, which the reference's own code produced):
    video_item      VideoFeatSubTokDataset.__getitem__   data/data.py:345-403
    video_collate   video_collate + get_gather_index     data/data.py:406-471, 504-512
    query_collate   query_collate                        data/vcmr.py:120-137
    vcmr_collate    vcmr_collate                         data/vcmr.py:140-159
    video_only_item VideoFeatDataset.__getitem__         data/vr_video_only.py:29-49 (a corpus without subtitles: [CLS] + every frame)
    vr_item, vr_collate, vr_eval_collate, vr_full_eval_item, vr_full_eval_collate       data/vr.py:98-200
    vcmr_eval_collate, vcmr_full_eval_item, vcmr_full_eval_collate                      data/vcmr.py:171-253
        (pinned by tests/golden/case_vr.npz)
    videoqa_item    VideoQaDataset.__getitem__          data/videoQA.py:62-121 (one question)
    video_qa_collate  video_qa_collate                   data/videoQA.py:155-182 (pinned by tests/golden/case_videoqa.npz)
    violin_item     ViolinDataset.__getitem__            data/violin.py:66-110
    violin_collate / violin_eval_collate                 data/violin.py:118-141, 163-170 (pinned by tests/golden/case_violin.npz)
    tvc_st_ed_label, tvc_item, tvc_val_item              data/tvc.py:39-49, 100-138, 170-190, 246-265
    tvc_collate / tvc_val_collate / tvc_eval_collate     data/tvc.py:140-161, 192-218, 267-291 (+ `cap_frame_index`)
    random_word, mlm_item, mlm_collate                   data/mlm.py:21-75, 93-131, 134-176
    frame_mask, mfm_item, mfm_collate                    data/mfm.py:19-39, 55-97
    random_reorder, fom_item, fom_collate / fom_eval_collate   data/fom.py:31-133
    vsm_item, vsm_collate                                data/vsm.py:35-145
        (the four pre-training tasks; their draws come from Python's `random` in the reference's order, so after
        random.seed(s) a batch is the reference's bit for bit: tests/golden/case_pretrain_collate.npz.  The device half of the
        MLM / MFM / FOM draws is hero_amd.pretrain_data.PretrainMasker.)
They are written over LENGTH arrays (one allocation per output, no pad_sequence / per-row python tensors) and also
return the handful of int32 length arrays (`batch["lengths"]`) from which the device half rebuilds every index tensor.

Device half - the reference builds every index tensor of a batch on the host in the DataLoader workers and
`collect_frame_outputs` (model/model.py:156-187) walks python lists per forward.  `DeviceCollate` takes the length
arrays and derives, with kernels, in place, into buffers of fixed capacity:

    f_gather_index, f_attn_masks  [T, out_size]          int64   out_size = max_i(frames_i + tokens_i), data.py:433
    c_attn_masks                  [B, NF]                int64
    f_v_feats                     [T, max_vl, D]         gathered from c_v_feats (optional: halves the PCIe bytes)
    frame_map = (offsets [B*NF + 1], entries [capacity], inverse [T * out_size])   int32, the CSR that
                hero_csr_gather_sum consumes (== hero_amd.model.model.build_frame_map, bit for bit)

Because the outputs keep their addresses, a hipGraph captured on one batch replays on the next batch of
the same SHAPE after `update()` + `hero_amd.functional.refresh_memo()` (tests/test_gpu_collate.py).
The packed (variable-length) formulation of ragged batches replays too when the batch's feeder owns a pack plan
of fixed row capacity (hero_amd.loader.StaticBatchFeeder(packed_rows=...), BertEncoder.register_static_plan).
"""
import numpy as np
import torch

from . import _lib as L


PAD_ID = 1          # RoBERTa <pad>, hard-coded in the reference's collates (data/data.py:423, data/vcmr.py:122)
MAX_POS = 511       # position ids are clamped here (data/data.py:429)


def video_item(v_feat, sub2frames, sub_tokens, sep=2, sub_ctx_len=0):
    """One video -> the 7-tuple of VideoFeatSubTokDataset.__getitem__ (data/data.py:345-403).
    v_feat [n_frames, D] float; sub2frames [(sub_idx, [frame_idx])]; sub_tokens[sub_idx] = token id list."""
    n_total, nf = len(sub2frames), v_feat.shape[0]
    ids, feats, masks = [], [], []
    for sub_idx, frames in sub2frames:
        toks = [sep]
        for j in range(sub_idx - sub_ctx_len, sub_idx + 1):      # the subtitle and its `sub_ctx_len` predecessors
            if 0 <= j < n_total:
                toks.extend(sub_tokens[j])
        keep = [f for f in frames if 0 <= f < nf]                 # frames past the (clipped) video are dropped
        if keep:
            feats.append(v_feat[torch.as_tensor(keep)])
            masks.append(torch.ones(len(keep) + len(toks), dtype=torch.long))
        else:                                                     # no frame: ONE zero frame slot, masked (data.py:380-382)
            feats.append(v_feat.new_zeros(1, v_feat.shape[1]))
            m = torch.ones(1 + len(toks), dtype=torch.long)
            m[0] = 0
            masks.append(m)
        ids.append(torch.tensor(toks, dtype=torch.long))
    return (ids, feats, masks, v_feat, torch.ones(nf, dtype=torch.long), n_total, sub2frames)


def st_ed_label(ts, max_idx, frame_interval=1.5):
    """[start s, end s] -> (first, last) frame index, VcmrDataset.get_st_ed_label (data/vcmr.py:103-117)."""
    import math
    st = min(math.floor(ts[0] / frame_interval), max_idx)
    return st, min(max(math.ceil(ts[1] / frame_interval) - 1, st + 1), max_idx)


def vcmr_item(video, vid, queries, cls_=0, frame_interval=1.5):
    """video: a video_item tuple; queries: [(token id list, [start s, end s])] -> VcmrDataset.__getitem__'s
    (video, vid, ((ids, mask, vid, target), ...)) (data/vcmr.py:73-98)."""
    last = video[3].shape[0] - 1
    out = []
    for toks, ts in queries:
        ids = torch.tensor([cls_] + list(toks), dtype=torch.long)
        out.append((ids, torch.ones_like(ids), vid, torch.tensor(st_ed_label(ts, last, frame_interval), dtype=torch.long)))
    return (video, vid, tuple(out))


def _pad_rows(rows, width, fill, dtype):
    out = torch.full((len(rows), width), fill, dtype=dtype)
    for r, t in enumerate(rows):
        out[r, :t.shape[0]] = t
    return out


def _pad_feats(rows, width):
    out = rows[0].new_zeros(len(rows), width, rows[0].shape[-1])
    for r, t in enumerate(rows):
        out[r, :t.shape[0]] = t
    return out


def video_collate(inputs):
    """list of video_item tuples -> the reference's batch dict (data/data.py:406-471), same keys / shapes / dtypes,
    plus `lengths` (int32 arrays, DeviceCollate's input).  Widths: f_attn_masks / f_gather_index have
    out_size = max_i(len(mask_i)) = max_i(frame slots_i + tokens_i) columns - NOT max_vl + max_sl."""
    ids = [t for it in inputs for t in it[0]]
    feats = [t for it in inputs for t in it[1]]
    masks = [t for it in inputs for t in it[2]]
    clips = [it[3] for it in inputs]
    num_subs = [it[5] for it in inputs]
    sub2frm = [it[6] for it in inputs]
    ntok = np.array([t.shape[0] for t in ids], dtype=np.int32)
    vlen = np.array([t.shape[0] for t in feats], dtype=np.int32)              # frame SLOTS (>= 1)
    max_sl, max_vl = int(ntok.max()), int(vlen.max())
    out_size = max(int(m.shape[0]) for m in masks)
    T = len(ids)
    gidx = torch.arange(out_size, dtype=torch.long).repeat(T, 1)              # get_gather_index, data.py:504-512
    for r in range(T):
        gidx[r, vlen[r]:vlen[r] + ntok[r]] = torch.arange(max_vl, max_vl + int(ntok[r]))
    nfr = np.array([c.shape[0] for c in clips], dtype=np.int32)
    NF = int(nfr.max())
    c_feats = _pad_feats(clips, NF)
    batch = {
        "f_sub_input_ids": _pad_rows(ids, max_sl, PAD_ID, torch.long),
        "f_sub_pos_ids": torch.arange(max_sl, dtype=torch.long).clamp_(max=MAX_POS).unsqueeze(0),
        "f_v_feats": _pad_feats(feats, max_vl),
        "f_v_pos_ids": torch.arange(max_vl, dtype=torch.long).unsqueeze(0),
        "f_attn_masks": _pad_rows(masks, out_size, 0, torch.long),
        "f_gather_index": gidx,
        "f_sub_input_attn_masks": (torch.arange(max_sl).unsqueeze(0) < torch.from_numpy(ntok).unsqueeze(1)).long(),
        "c_v_feats": c_feats,
        "c_pos_ids": torch.arange(NF, dtype=torch.long).repeat(len(clips), 1),
        "c_attn_masks": _pad_rows([it[4] for it in inputs], NF, 0, torch.long),
        "num_subs": num_subs,
        "sub_idx2frame_idx": sub2frm,
    }
    # frames per row as the MASK sees them (0 for the zero-slot rows): what DeviceCollate consumes
    nfrm_eff = np.array([int(m[0]) * int(v) for m, v in zip(masks, vlen)], dtype=np.int32)
    batch["lengths"] = _lengths(num_subs, sub2frm, nfrm_eff, ntok, nfr)
    return batch


def query_collate(query_input_ids, query_attn_mask, targets):
    """data/vcmr.py:120-137."""
    Lq = max(t.shape[0] for t in query_input_ids)
    return {"query_input_ids": _pad_rows(query_input_ids, Lq, PAD_ID, torch.long),
            "query_pos_ids": torch.arange(Lq, dtype=torch.long).unsqueeze(0),
            "query_attn_masks": _pad_rows(query_attn_mask, Lq, 0, torch.long),
            "targets": torch.stack(list(targets))}


def vcmr_collate(inputs):
    """list of (video_item tuple, vid, ((query ids, query mask, vid, target), ...)) -> batch (data/vcmr.py:140-159)."""
    vids = [it[1] for it in inputs]
    qs = [q for it in inputs for q in it[2]]
    batch = query_collate([q[0] for q in qs], [q[1] for q in qs], [q[3] for q in qs])
    batch.update(video_collate([it[0] for it in inputs]))
    batch["vids"] = vids
    where = {v: i for i, v in enumerate(vids)}
    batch["q_vidx"] = torch.tensor([where[q[2]] for q in qs], dtype=torch.long)
    return batch


def video_only_item(v_feat, cls_=0):
    """One video of a corpus without subtitles -> the 7-tuple of VideoFeatDataset.__getitem__ (data/vr_video_only.py:29-49, which
    data/vcmr_video_only.py shares): ONE fake subtitle holding the single token `cls_` (CLS, not SEP) and every frame of the video,
    so its row is 1 + n_frames positions long."""
    n = v_feat.shape[0]
    return ([torch.tensor([cls_])], [v_feat], [torch.ones(1 + n, dtype=torch.long)], v_feat, torch.ones(n, dtype=torch.long), 1,
            [(0, list(range(n)))])


def _query_row(toks, vid, target, cls_):
    ids = torch.tensor([cls_] + list(toks), dtype=torch.long)
    return (ids, torch.ones_like(ids), vid, torch.tensor(target, dtype=torch.long))


def vr_item(video, vid, queries, cls_=0):
    """video: a video_item / video_only_item tuple; queries: token id lists -> VrDataset.__getitem__'s (video, vid, ((ids, mask,
    vid, [-1, -1]), ...)) (data/vr.py:98-120): video retrieval has no moment to point at."""
    return (video, vid, tuple(_query_row(toks, vid, [-1, -1], cls_) for toks in queries))


def vr_collate(inputs):
    """data/vr.py:123-124."""
    return vcmr_collate(inputs)


def vcmr_eval_collate(inputs):
    """list of (qids, vcmr_item tuple) -> vcmr_collate's batch plus `qids` (data/vcmr.py:171-178)."""
    batch = vcmr_collate([item for _, item in inputs])
    batch["qids"] = [q for ids, _ in inputs for q in ids]
    return batch


def vr_eval_collate(inputs):
    """data/vr.py:134-141."""
    return vcmr_eval_collate(inputs)


def vcmr_full_eval_item(qid, toks, vid, ts=None, n_frames=None, cls_=0, frame_interval=1.5):
    """One query of a full-corpus evaluation -> VcmrFullEvalDataset.__getitem__'s (qid, [(ids, mask, vid, target)])
    (data/vcmr.py:215-242): the target is st_ed_label(ts) in the `n_frames` frames of its video when the query carries a
    timestamp, [-1, -1] otherwise."""
    if ts is None:
        target = [-1, -1]
    else:
        if n_frames is None:
            raise ValueError("vcmr_full_eval_item: a query with a timestamp needs n_frames of its video")
        target = st_ed_label(ts, n_frames - 1, frame_interval)
    return (qid, [_query_row(toks, vid, target, cls_)])


def vr_full_eval_item(qid, toks, vid, cls_=0):
    """VrFullEvalDataset.__getitem__ (data/vr.py:175-196): the target is always [-1, -1]."""
    return vcmr_full_eval_item(qid, toks, vid, cls_=cls_)


def vcmr_full_eval_collate(inputs):
    """list of full-eval items -> the query-only batch of data/vcmr.py:245-253: query_input_ids / query_pos_ids / query_attn_masks,
    targets, `vids` (one per query) and `qids`."""
    qs = [q for _, rows in inputs for q in rows]
    batch = query_collate([q[0] for q in qs], [q[1] for q in qs], [q[3] for q in qs])
    batch["vids"] = [q[2] for q in qs]
    batch["qids"] = [qid for qid, _ in inputs]
    return batch


def vr_full_eval_collate(inputs):
    """data/vr.py:199-200."""
    return vcmr_full_eval_collate(inputs)


def videoqa_item(video, question, answers, target, ts, sep=2, frame_interval=1.5, vid=None):
    """One question about one video -> VideoQaDataset.__getitem__'s 6-tuple (data/videoQA.py:62-121).
    video: a video_item tuple; question / answers: token id lists (5 answers for TVQA, 4 for How2QA); target: index of the
    right answer or None; ts: [start s, end s], the reference's "start-end" string, or None.  Every answer gets its own copy
    of the video whose subtitles carry `[sep] question [sep] answer` behind their tokens (mask extended by ones)."""
    ids, feats, masks, clip, clip_mask, n_subs, sub2frames = video
    last = clip.shape[0] - 1
    if ts is None:
        ts_target = torch.tensor([-1, -1], dtype=torch.long)
    else:
        try:
            if isinstance(ts, str):
                ts = [float(t) for t in ts.split("-")[:2]]
            ts_target = torch.tensor(st_ed_label(ts, last, frame_interval), dtype=torch.long)
        except Exception:                                         # data/videoQA.py:149-150: an unreadable stamp is a missing label
            ts_target = torch.tensor([-1, -1], dtype=torch.long)
    copies, qa_ids, qa_masks = [], [], []
    for ans in answers:
        qa = torch.tensor([sep] + list(question) + [sep] + list(ans), dtype=torch.long)
        ones = torch.ones_like(qa)
        qa_ids.append(qa)
        qa_masks.append(ones)
        copies.append(([torch.cat((t, qa)) for t in ids], feats, [torch.cat((m, ones)) for m in masks],
                       clip, clip_mask, n_subs, sub2frames))
    return (copies, qa_ids, qa_masks, [vid], [torch.tensor([-1 if target is None else target], dtype=torch.long)], [ts_target])


def video_qa_collate(inputs):
    """list of videoqa_item tuples -> the reference's batch (data/videoQA.py:155-182): video_collate over every answer copy
    (question-major, A copies each), `targets` (Nv, 1), `ts_targets` (Nv, 2) with -1 for a missing label, and the padded
    `[sep] q [sep] a` rows qa_input_ids / qa_pos_ids / qa_attn_masks (txt_input_collate, data/data.py:474-484)."""
    copies = [c for it in inputs for c in it[0]]
    qa_ids = [t for it in inputs for t in it[1]]
    qa_masks = [t for it in inputs for t in it[2]]
    batch = video_collate(copies)
    Lqa = max(t.shape[0] for t in qa_ids)
    batch["targets"] = torch.stack([t for it in inputs for t in it[4]])
    batch["ts_targets"] = torch.stack([t for it in inputs for t in it[5]])
    batch["qa_input_ids"] = _pad_rows(qa_ids, Lqa, PAD_ID, torch.long)
    batch["qa_pos_ids"] = torch.arange(Lqa, dtype=torch.long).clamp_(max=MAX_POS).unsqueeze(0)
    batch["qa_attn_masks"] = _pad_rows(qa_masks, Lqa, 0, torch.long)
    return batch


def violin_item(video, statements, targets, sep=2, vid=None):
    """The statements about one video -> ViolinDataset.__getitem__'s 5-tuple (data/violin.py:66-110).
    video: a video_item tuple; statements: token id lists (a statement and its paired one when sampled by statement);
    targets: one truth value per statement.  Every statement gets its own copy of the video whose subtitles carry
    `[sep] statement` behind their tokens (mask extended by ones)."""
    ids, feats, masks, clip, clip_mask, n_subs, sub2frames = video
    copies, q_ids, q_masks, labels = [], [], [], []
    for toks, target in zip(statements, targets):
        q = torch.tensor([sep] + list(toks), dtype=torch.long)
        ones = torch.ones_like(q)
        q_ids.append(q)
        q_masks.append(ones)
        copies.append(([torch.cat((t, q)) for t in ids], feats, [torch.cat((m, ones)) for m in masks],
                       clip, clip_mask, n_subs, sub2frames))
        labels.append(torch.tensor([1 if target else 0], dtype=torch.long))
    return (copies, q_ids, q_masks, [vid] * len(copies), labels)


def violin_collate(inputs):
    """list of violin_item tuples -> the reference's batch (data/violin.py:118-141): video_collate over every statement's copy
    (item-major), `targets` (S, 1), and the padded `[sep] statement` rows q_input_ids / q_pos_ids / q_attn_masks
    (txt_input_collate, data/data.py:474-484)."""
    copies = [c for it in inputs for c in it[0]]
    q_ids = [t for it in inputs for t in it[1]]
    q_masks = [t for it in inputs for t in it[2]]
    batch = video_collate(copies)
    Lq = max(t.shape[0] for t in q_ids)
    batch["targets"] = torch.stack([t for it in inputs for t in it[4]])      # pad_sequence of one-element rows
    batch["q_input_ids"] = _pad_rows(q_ids, Lq, PAD_ID, torch.long)
    batch["q_pos_ids"] = torch.arange(Lq, dtype=torch.long).clamp_(max=MAX_POS).unsqueeze(0)
    batch["q_attn_masks"] = _pad_rows(q_masks, Lq, 0, torch.long)
    return batch


def violin_eval_collate(inputs):
    """list of (qids, violin_item tuple) -> violin_collate's batch plus `qids` (data/violin.py:163-170)."""
    batch = violin_collate([item for _, item in inputs])
    batch["qids"] = [q for ids, _ in inputs for q in ids]
    return batch


def tvc_st_ed_label(ts, nframes, frame_interval=1.5):
    """[start s, end s] -> the frames [st, ed) of a caption's segment, TvcTrainDataset.get_st_ed_label (data/tvc.py:119-138):
    Python `round` (half to even) on the end, at least one frame, both clamped at the video's end - so a caption that starts
    at or past the end gets the EMPTY segment (nframes, nframes)."""
    import math
    st = min(math.floor(ts[0] / frame_interval), nframes)
    return st, min(max(round(ts[1] / frame_interval), st + 1), nframes)


def tvc_frame_index(clip_ranges, n_frames):
    """clip_ranges: per video the (st, ed) of its captions -> int32 [Ncap, Lv], Lv = the longest segment (at least 1): the
    flat row video * n_frames + frame behind every position of the zero-padded segments of model/tvc.py:219-238, -1 = pad."""
    segs = [(v, st, ed) for v, rs in enumerate(clip_ranges) for st, ed in rs]
    Lv = max([ed - st for _, st, ed in segs] + [1])
    idx = torch.full((len(segs), Lv), -1, dtype=torch.int32)
    for r, (v, st, ed) in enumerate(segs):
        if not 0 <= st <= ed <= n_frames:
            raise IndexError("tvc_frame_index: segment [%d, %d) outside a video of %d frames" % (st, ed, n_frames))
        idx[r, :ed - st] = torch.arange(v * n_frames + st, v * n_frames + ed, dtype=torch.int32)
    return idx


def tvc_item(video, captions, bos=0, eos=2, max_txt_len=-1, frame_interval=1.5):
    """One video and its captions -> TvcTrainDataset.__getitem__'s (video, clip_ranges, cap_inputs) (data/tvc.py:100-114 with
    CaptionTokLmdb.get_caption, data/tvc.py:39-49).  video: a video_item tuple; captions: [(token id list, [start s, end s])]."""
    nframes = len(video[4])
    clip_ranges, cap_inputs = [], []
    for toks, ts in captions:
        input_ids, tgt_ids = [bos] + list(toks), list(toks) + [eos]
        if max_txt_len != -1:
            input_ids, tgt_ids = input_ids[:max_txt_len], tgt_ids[:max_txt_len]
        st, ed = tvc_st_ed_label(ts, nframes, frame_interval)
        clip_ranges.append((st, ed))
        cap_inputs.append((torch.tensor(input_ids, dtype=torch.long), torch.tensor(tgt_ids, dtype=torch.long),
                           torch.ones(ed - st, dtype=torch.long)))
    return (video, clip_ranges, cap_inputs)


def tvc_val_item(video, clips, vid, frame_interval=1.5, with_gts=True):
    """One video and its clips -> TvcValDataset / TvcEvalDataset.__getitem__ (data/tvc.py:170-190, 246-265).
    clips: [(clip id, [start s, end s], ground-truth text)] (the text is ignored without with_gts)."""
    nframes = len(video[4])
    ranges = [tvc_st_ed_label(c[1], nframes, frame_interval) for c in clips]
    masks = [torch.ones(ed - st, dtype=torch.long) for st, ed in ranges]
    meta = (vid, [c[0] for c in clips], [c[1] for c in clips]) + (([c[2] for c in clips],) if with_gts else ())
    return (video, ranges, masks, meta)


def _tvc_video_part(batch, inputs):
    batch["clip_ranges"] = tuple(tuple(it[1]) for it in inputs)
    batch.update(video_collate([it[0] for it in inputs]))
    # hero_amd only: the segments' rows as a tensor, so that a captured step reads them from the device
    batch["cap_frame_index"] = tvc_frame_index(batch["clip_ranges"], batch["c_v_feats"].shape[1])
    return batch


def tvc_collate(inputs):
    """list of tvc_item tuples -> the reference's training batch (TvcTrainDataset.collate, data/tvc.py:140-161): cap_input_ids
    padded with 1, cap_tgt_ids padded with -1, cap_pos_ids (1, Lt), cap_attn_mask over the segment frames, clip_ranges as
    tuples, the video_collate keys - plus the one extra key `cap_frame_index` (tvc_frame_index)."""
    caps = [c for it in inputs for c in it[2]]
    Lt = max(c[0].shape[0] for c in caps)
    Lv = max(c[2].shape[0] for c in caps)
    batch = {"cap_input_ids": _pad_rows([c[0] for c in caps], Lt, PAD_ID, torch.long),
             "cap_pos_ids": torch.arange(0, Lt, dtype=torch.long).unsqueeze(0),
             "cap_tgt_ids": _pad_rows([c[1] for c in caps], Lt, -1, torch.long),
             "cap_attn_mask": _pad_rows([c[2] for c in caps], Lv, 0, torch.long)}
    return _tvc_video_part(batch, inputs)


def tvc_val_collate(inputs, with_gts=True):
    """list of tvc_val_item tuples -> TvcValDataset.collate's batch (data/tvc.py:192-218): cap_attn_mask, clip_ranges, the
    video keys and the meta lists vid_names / clip_ids / all_ts / gts - plus `cap_frame_index`."""
    masks = [m for it in inputs for m in it[2]]
    Lv = max(m.shape[0] for m in masks)
    batch = _tvc_video_part({"cap_attn_mask": _pad_rows(masks, Lv, 0, torch.long)}, inputs)
    vids, clip_ids, all_ts, all_gts = [], [], [], []
    for it in inputs:
        meta = it[3]
        for j, (cid, ts) in enumerate(zip(meta[1], meta[2])):
            vids.append(meta[0])
            clip_ids.append(int(cid))
            all_ts.append(ts)
            if with_gts:
                all_gts.append(meta[3][j])
    batch.update(vid_names=vids, clip_ids=clip_ids, all_ts=all_ts)
    if with_gts:
        batch["gts"] = all_gts
    return batch


def tvc_eval_collate(inputs):
    """TvcEvalDataset.collate (data/tvc.py:267-291): tvc_val_collate without the ground-truth texts."""
    return tvc_val_collate(inputs, with_gts=False)


# ---- the four pre-training tasks (host half; device half: hero_amd/pretrain_data.py) -----------------------------------------
def random_word(tokens, v_range, mask, mask_prob=0.15):
    """BERT's token masking, data/mlm.py:21-58: one random.random() per token; a drawn token becomes `mask` (80 %), a token
    of range(*v_range) (10 %, one random.choice) or stays (10 %); a sentence with no drawn token masks its first one.
    `tokens` is changed in place.  Returns (tokens, labels) with -1 for the tokens that were not drawn.  (An empty token list
    comes back empty; the reference raises on it.)"""
    import random
    labels = []
    for i, tok in enumerate(tokens):
        prob = random.random()
        if prob < mask_prob:
            prob /= mask_prob
            if prob < 0.8:
                tokens[i] = mask
            elif prob < 0.9:
                tokens[i] = random.choice(range(*v_range))
            labels.append(tok)
        else:
            labels.append(-1)
    if tokens and all(lab == -1 for lab in labels):
        labels[0] = tokens[0]
        tokens[0] = mask
    return tokens, labels


def _sub_context(sub_tokens, sub_idx, sub_ctx_len, n_subs, max_txt_len, skip=()):
    """The tokens of subtitle `sub_idx` behind those of its `sub_ctx_len` predecessors, each cut at max_txt_len (-1: whole)."""
    toks = []
    for j in range(sub_idx - sub_ctx_len, sub_idx + 1):
        if 0 <= j < n_subs and j not in skip:
            toks.extend(sub_tokens[j] if max_txt_len == -1 else sub_tokens[j][:max_txt_len])
    return toks


def mlm_item(v_feat, sub2frames, sub_tokens, mask, v_range, cls_=0, mask_prob=0.15, sub_ctx_len=0, max_txt_len=-1):
    """One video -> VideoMlmDataset.__getitem__'s list of (input_ids, frame feats, attn mask, txt_mask_tgt, txt_labels), one per
    subtitle (data/mlm.py:93-131 with create_mlm_io, :67-75): rows start with CLS, the token mask is shifted right by the row's
    frame slots, and a subtitle without frames gets one zero slot whose attention mask is 0.  The frame lists are used as
    they are (the reference does not filter them here)."""
    n_subs, out = len(sub2frames), []
    for sub_idx, frames in sub2frames:
        toks, labels = random_word(_sub_context(sub_tokens, sub_idx, sub_ctx_len, n_subs, max_txt_len), v_range, mask, mask_prob)
        ids = torch.tensor([cls_] + toks, dtype=torch.long)
        labels = torch.tensor([-1] + labels, dtype=torch.long)
        slots = max(len(frames), 1)
        attn = torch.ones(slots + ids.shape[0], dtype=torch.long)
        if frames:
            feats = v_feat[torch.as_tensor(frames)]
        else:
            feats = v_feat.new_zeros(1, v_feat.shape[1])
            attn[0] = 0
        tgt = torch.zeros(slots + ids.shape[0], dtype=torch.bool)
        tgt[slots:] = labels != -1
        out.append((ids, feats, attn, tgt, labels))
    return out


def mlm_collate(inputs):
    """list of mlm_item lists -> the reference's batch (data/mlm.py:134-176): input_ids padded with 1, position_ids (1, L),
    v_feat, attn_masks, gather_index, txt_mask_tgt [T, out_size] and the compact txt_labels in row-major order."""
    rows = [r for it in inputs for r in it]
    ntok = np.array([r[0].shape[0] for r in rows], dtype=np.int32)
    vlen = np.array([r[1].shape[0] for r in rows], dtype=np.int32)
    max_sl, max_vl, T = int(ntok.max()), int(vlen.max()), len(rows)
    out_size = max(int(r[2].shape[0]) for r in rows)
    gidx = torch.arange(out_size, dtype=torch.long).repeat(T, 1)
    for r in range(T):
        gidx[r, vlen[r]:vlen[r] + ntok[r]] = torch.arange(max_vl, max_vl + int(ntok[r]))
    labels = _pad_rows([r[4] for r in rows], max_sl, -1, torch.long)
    return {"input_ids": _pad_rows([r[0] for r in rows], max_sl, PAD_ID, torch.long),
            "position_ids": torch.arange(max_sl, dtype=torch.long).unsqueeze(0),
            "v_feat": _pad_feats([r[1] for r in rows], max_vl),
            "attn_masks": _pad_rows([r[2] for r in rows], out_size, 0, torch.long),
            "gather_index": gidx,
            "txt_mask_tgt": _pad_rows([r[3] for r in rows], max(int(r[3].shape[0]) for r in rows), False, torch.bool),
            "txt_labels": labels[labels != -1]}


def frame_mask(mask_prob, n):
    """_get_img_mask, data/mfm.py:19-25: one random.random() per frame, at least one frame (one random.choice)."""
    import random
    m = [random.random() < mask_prob for _ in range(n)]
    if not any(m):
        m[random.choice(range(n))] = True
    return torch.tensor(m)


def mfm_item(video, mask_prob=0.15):
    """video: a video_item tuple -> MfmDataset.__getitem__'s (video, per-subtitle frame masks, clip mask) (data/mfm.py:55-74):
    the subtitle masks are the clip mask at the subtitle's frames, [False] for a subtitle without frames."""
    c_mask = frame_mask(mask_prob, video[3].shape[0])
    masks = [c_mask[torch.as_tensor(frames)] if len(frames) else torch.zeros(1, dtype=torch.bool) for _, frames in video[6]]
    return (video, masks, c_mask)


def mfm_collate(inputs):
    """list of mfm_item tuples -> the reference's batch (data/mfm.py:77-97): video_collate's keys with f_v_feats / c_v_feats
    zeroed at the masked frames, f_v_masks [T, max_vl], c_v_masks [B, NF] and feat_targets (taken before the zeroing)."""
    batch = video_collate([it[0] for it in inputs])
    f_masks = [m for it in inputs for m in it[1]]
    f_mask = _pad_rows(f_masks, max(int(m.shape[0]) for m in f_masks), False, torch.bool)
    c_mask = _pad_rows([it[2] for it in inputs], batch["c_v_feats"].shape[1], False, torch.bool)
    batch["feat_targets"] = batch["c_v_feats"][c_mask]
    batch["f_v_feats"] = batch["f_v_feats"].masked_fill(f_mask.unsqueeze(-1), 0)
    batch["c_v_feats"] = batch["c_v_feats"].masked_fill(c_mask.unsqueeze(-1), 0)
    batch["f_v_masks"], batch["c_v_masks"] = f_mask, c_mask
    return batch


def random_reorder(pos_ids, p=0.15):
    """data/fom.py:96-115: one random.random() per position, the drawn positions are permuted among themselves by one
    random.shuffle.  Returns (order, target): order[pos] = the position shown there, target[shown position] = pos, -1 elsewhere."""
    import random
    selected = [i for i in range(len(pos_ids)) if random.random() < p]
    shuffled = [pos_ids[i] for i in selected]
    random.shuffle(shuffled)
    order, target = list(pos_ids), [-1] * len(pos_ids)
    for pos, shown in zip(selected, shuffled):
        order[pos] = shown
        target[shown] = pos
    return order, target


def fom_item(video, p=0.15):
    """video: a video_item tuple -> FomDataset.__getitem__'s (video, orders, targets) (data/fom.py:31-47)."""
    order, target = random_reorder(list(range(video[3].shape[0])), p)
    return (video, torch.tensor(order, dtype=torch.long), torch.tensor(target, dtype=torch.long))


def fom_collate(inputs):
    """list of fom_item tuples -> the reference's batch (data/fom.py:50-93): video_collate's keys, shuffled_orders (identity
    in the padding) and targets (-1 there) [B, NF], and for every pair i < j of reordered frames of a clip the flat rows
    (i, j, j, i) in reordered_frame_idx with binary_targets (0 where the first of a pair has the larger target) - built
    per clip from index arrays, not pair by pair."""
    batch = video_collate([it[0] for it in inputs])
    B, NF = batch["c_v_feats"].shape[:2]
    orders = torch.arange(NF, dtype=torch.long).repeat(B, 1)
    targets = torch.full((B, NF), -1, dtype=torch.long)
    idx, binary = [], []
    for b, (_, o, t) in enumerate(inputs):
        orders[b, :o.shape[0]] = o
        targets[b, :t.shape[0]] = t
        tn = t.numpy()
        pos = np.nonzero(tn != -1)[0]
        i, j = np.triu_indices(pos.shape[0], 1)                  # pairs in (i, j) row-major order, the reference's loop order
        pi, pj = b * NF + pos[i], b * NF + pos[j]
        idx.append(np.stack([pi, pj, pj, pi], 1).reshape(-1))
        ti, tj = tn[pos[i]], tn[pos[j]]
        binary.append(np.stack([ti <= tj, tj <= ti], 1).reshape(-1))
    batch["shuffled_orders"], batch["targets"] = orders, targets
    batch["reordered_frame_idx"] = torch.from_numpy(np.concatenate(idx).astype(np.int64))
    batch["binary_targets"] = torch.from_numpy(np.concatenate(binary).astype(np.int64))
    return batch


def fom_eval_collate(inputs):
    """list of (vid, *fom_item tuple) -> fom_collate's batch plus `vids` (data/fom.py:125-132)."""
    batch = fom_collate([tuple(it[1:]) for it in inputs])
    batch["vids"] = [it[0] for it in inputs]
    return batch


def vsm_item(v_feat, sub2frames, sub_tokens, vid, query_per_video=5, sep=2, cls_=0, sub_ctx_len=0, max_txt_len=-1):
    """One video -> VsmDataset.__getitem__'s (video, vid, ((query ids, query mask, vid, target), ...)) (data/vsm.py:35-117):
    up to `query_per_video` subtitles with frames are drawn (one random.sample), leave every subtitle context and become
    the queries `[cls] tokens` with target (st, ed) = (first frame, min(max(first + 1, last frame), nframes - 1)); the last
    query is repeated up to query_per_video.  The frame lists are used as they are."""
    import random
    n_subs, nframes = len(sub2frames), v_feat.shape[0]
    matched = [sub_idx for sub_idx, frames in sub2frames if frames]
    picked = set(random.sample(matched, min(len(matched), query_per_video)))
    ids, feats, masks, queries = [], [], [], []
    for sub_idx, frames in sub2frames:
        toks = [sep] + _sub_context(sub_tokens, sub_idx, sub_ctx_len, n_subs, max_txt_len, skip=picked)
        if frames:
            feats.append(v_feat[torch.as_tensor(frames)])
            masks.append(torch.ones(len(frames) + len(toks), dtype=torch.long))
            if sub_idx in picked:
                q = sub_tokens[sub_idx] if max_txt_len == -1 else sub_tokens[sub_idx][:max_txt_len]
                q = torch.tensor([cls_] + list(q), dtype=torch.long)
                st, ed = frames[0], min(max(frames[0] + 1, frames[-1]), nframes - 1)
                assert 0 <= st <= ed < nframes, "vsm_item: target frames (%d, %d) outside a video of %d frames" % (st, ed, nframes)
                queries.append((q, torch.ones_like(q), vid, torch.tensor([st, ed], dtype=torch.long)))
        else:
            feats.append(v_feat.new_zeros(1, v_feat.shape[1]))
            m = torch.ones(1 + len(toks), dtype=torch.long)
            m[0] = 0
            masks.append(m)
        ids.append(torch.tensor(toks, dtype=torch.long))
    while len(queries) < query_per_video:
        queries.append(queries[-1])
    return ((ids, feats, masks, v_feat, torch.ones(nframes, dtype=torch.long), n_subs, sub2frames), vid, tuple(queries))


def vsm_collate(inputs):
    """list of vsm_item tuples -> the reference's batch (data/vsm.py:120-145): video_collate's keys, q_vidx, the padded
    queries query_input_ids / query_pos_ids (not clamped) / query_attn_masks, targets (Nq, 2) and vids."""
    vids = [it[1] for it in inputs]
    qs = [q for it in inputs for q in it[2]]
    batch = video_collate([it[0] for it in inputs])
    where = {v: i for i, v in enumerate(vids)}
    batch["q_vidx"] = torch.tensor([where[q[2]] for q in qs], dtype=torch.long)
    Lq = max(q[0].shape[0] for q in qs)
    batch.update({"query_input_ids": _pad_rows([q[0] for q in qs], Lq, PAD_ID, torch.long),
                  "query_pos_ids": torch.arange(Lq, dtype=torch.long).unsqueeze(0),
                  "query_attn_masks": _pad_rows([q[1] for q in qs], Lq, 0, torch.long),
                  "targets": torch.stack([q[3] for q in qs]),
                  "vids": vids})
    return batch


def _lengths(num_subs, sub2frm, sub_nfrm, sub_ntok, n_frames):
    """Flat int32 description of a batch (host, ~1 KB).  sub_frm lists the frames as collect_frame_outputs will use
    them (the UNFILTERED lists of sub_idx2frame_idx, model/model.py:174-184); sub_nfrm the mask's frame counts."""
    frm, off = [], [0]
    for v, n in enumerate(num_subs):
        rows = sorted(sub2frm[v], key=lambda t: t[0])
        assert [sid for sid, _ in rows] == list(range(n)), "subtitle ids must be their row offsets inside the video"
        for _, frames in rows:
            frm.extend(frames)
            off.append(len(frm))
    i32 = lambda a: np.asarray(a, dtype=np.int32)      # noqa: E731
    return {"sub_nfrm": i32(sub_nfrm), "sub_ntok": i32(sub_ntok), "sub_frm_off": i32(off), "sub_frm": i32(frm if frm else [0]),
            "vid_sub_off": i32(np.concatenate([[0], np.cumsum(num_subs)])), "vid_nfrm": i32(n_frames)}


def lengths_from_lists(num_subs, sub_idx2frame_idx, sub_ntok, n_frames, sub_nfrm=None):
    """Length arrays from the host lists of an existing batch dict.  sub_ntok: tokens (incl. SEP) per subtitle
    row; sub_nfrm: frames per row as f_attn_masks sees them (default: the list lengths)."""
    if sub_nfrm is None:
        sub_nfrm = [len(fr) for v, n in enumerate(num_subs) for _, fr in sorted(sub_idx2frame_idx[v], key=lambda t: t[0])]
    return _lengths(num_subs, sub_idx2frame_idx, sub_nfrm, sub_ntok, n_frames)


class DeviceCollate:
    def __init__(self, T, max_vl, max_sl, B, NF, device, entry_capacity=None, out_size=None, vfeat_dim=None):
        """out_size: width of f_attn_masks / f_gather_index (the reference's: max over rows of frame slots +
        tokens; default max_vl + max_sl, its upper bound).  vfeat_dim: also own f_v_feats [T, max_vl, vfeat_dim]
        and fill it from c_v_feats in update() (hero_collate_gather_feats)."""
        self.T, self.max_vl, self.max_sl, self.B, self.NF = T, max_vl, max_sl, B, NF
        self.Lf = out_size or (max_vl + max_sl)
        if not 0 < self.Lf <= max_vl + max_sl:
            raise ValueError("DeviceCollate: out_size %d outside (0, max_vl + max_sl = %d]" % (self.Lf, max_vl + max_sl))
        self.device = torch.device(device)
        cap = entry_capacity or T * max_vl
        z = lambda *shape, dt=torch.int32: torch.zeros(*shape, dtype=dt, device=self.device)      # noqa: E731
        self.f_gather_index = z(T, self.Lf, dt=torch.int64)
        self.f_attn_masks = z(T, self.Lf, dt=torch.int64)
        self.c_attn_masks = z(B, NF, dt=torch.int64)
        self.f_v_feats = z(T, max_vl, vfeat_dim, dt=torch.float32) if vfeat_dim else None
        self.offsets = z(B * NF + 1)
        self.entries = z(max(cap, 1))
        self.inverse = z(T * self.Lf)
        self._counts = z(B * NF)
        self._row_vid = z(T)
        # the six length arrays live in ONE int32 buffer (slots padded to 4 elements): a feeder refreshes them with one copy
        sizes = {"sub_nfrm": T, "sub_ntok": T, "sub_frm_off": T + 1, "sub_frm": max(cap, 1), "vid_sub_off": B + 1, "vid_nfrm": B}
        self._in_off, off = {}, 0
        for k, n in sizes.items():
            self._in_off[k] = (off, n)
            off += (n + 3) & ~3
        self._in_flat = z(off)
        self._in = {k: self._in_flat[o:o + n] for k, (o, n) in self._in_off.items()}

    @classmethod
    def for_batch(cls, batch, device, entry_capacity=None, **kw):
        """Buffers sized for a (host) batch of video_collate.  entry_capacity: at least that much room for the frame lists."""
        T, max_vl = batch["f_v_feats"].shape[:2]
        B, NF = batch["c_attn_masks"].shape
        cap = max(int(batch["lengths"]["sub_frm"].shape[0]), T * max_vl) if "lengths" in batch else None
        if entry_capacity:
            cap = max(cap or 0, int(entry_capacity))
        return cls(T, max_vl, batch["f_sub_input_ids"].shape[1], B, NF, device, out_size=batch["f_attn_masks"].shape[1],
                   entry_capacity=cap, **kw)

    @property
    def frame_map(self):
        return self.offsets, self.entries, self.inverse

    def load_lengths(self, lengths, src_device=None):
        """Copy the length arrays into the device-side input slots (a few hundred bytes, stream-ordered).
        lengths: host arrays (video_collate's batch["lengths"]) or, with src_device=True, a dict of int32 DEVICE
        tensors of exactly the slot sizes (a staging copy made on another stream: StaticBatchFeeder)."""
        if src_device and torch.is_tensor(lengths):          # a flat staging copy of the whole input buffer (same layout)
            if lengths.shape != self._in_flat.shape:
                raise ValueError("DeviceCollate: flat length buffer of %d entries, expected %d" % (lengths.numel(), self._in_flat.numel()))
            self._in_flat.copy_(lengths, non_blocking=True)
            return self
        for k, dst in self._in.items():
            src = lengths[k] if src_device else torch.as_tensor(lengths[k], dtype=torch.int32)
            if src.numel() > dst.numel() or (k in ("sub_nfrm", "sub_ntok", "vid_nfrm") and src.numel() != dst.numel()):
                raise ValueError("DeviceCollate: %s has %d entries, the buffers were sized for %d" % (k, src.numel(), dst.numel()))
            dst[:src.numel()].copy_(src, non_blocking=True)
        return self

    def rebuild(self, c_v_feats=None):
        """Rebuild every index tensor in place from the loaded lengths: kernels only, no host data, no synchronisation
        (capturable in a hipGraph).  c_v_feats (device, [B, NF, vfeat_dim] fp32): also rebuild f_v_feats from it."""
        i, s, lib = self._in, L.stream(), L.lib()
        L.check(lib.hero_collate_subs(L.ptr(i["sub_nfrm"]), L.ptr(i["sub_ntok"]), L.ptr(self.f_gather_index),
                                      L.ptr(self.f_attn_masks), self.T, self.max_vl, self.Lf, s))
        if c_v_feats is not None:
            if self.f_v_feats is None or tuple(c_v_feats.shape) != (self.B, self.NF, self.f_v_feats.shape[2]) or c_v_feats.dtype != torch.float32:
                raise ValueError("DeviceCollate: c_v_feats must be fp32 [B, NF, vfeat_dim] and the collate built with vfeat_dim")
            L.check(lib.hero_collate_gather_feats(L.ptr(c_v_feats.contiguous()), L.ptr(self.f_v_feats), L.ptr(i["vid_sub_off"]),
                                                  L.ptr(i["vid_nfrm"]), L.ptr(i["sub_frm_off"]), L.ptr(i["sub_frm"]),
                                                  L.ptr(self._row_vid), self.T, self.max_vl, self.B, self.NF, self.f_v_feats.shape[2], s))
            torch._C._increment_version([self.f_v_feats])
        L.check(lib.hero_collate_clip_mask(L.ptr(i["vid_nfrm"]), L.ptr(self.c_attn_masks), self.B, self.NF, s))
        L.check(lib.hero_collate_frame_map(L.ptr(i["vid_sub_off"]), L.ptr(i["sub_frm_off"]), L.ptr(i["sub_frm"]), None,
                                           L.ptr(self._counts), None, None, self.B, self.NF, self.Lf, 0, s))
        self.offsets[:1].zero_()
        torch.cumsum(self._counts, 0, out=self.offsets[1:])          # exclusive scan of the counts (device op)
        self.inverse.fill_(-1)
        L.check(lib.hero_collate_frame_map(L.ptr(i["vid_sub_off"]), L.ptr(i["sub_frm_off"]), L.ptr(i["sub_frm"]),
                                           L.ptr(self.offsets), None, L.ptr(self.entries), L.ptr(self.inverse),
                                           self.B, self.NF, self.Lf, 1, s))
        # raw kernels wrote them: caches keyed on (address, version) must miss (the call takes an ITERABLE of tensors)
        torch._C._increment_version([self.f_gather_index, self.f_attn_masks, self.c_attn_masks])
        return self

    def update(self, lengths, c_v_feats=None):
        """load_lengths + rebuild: lengths are host arrays (video_collate's batch["lengths"] / lengths_from_lists)."""
        return self.load_lengths(lengths).rebuild(c_v_feats)

    def batch_entries(self):
        """The keys of the reference batch dict this object owns (+ `frame_map`, which replaces the host
        lists num_subs / sub_idx2frame_idx inside HierarchicalVlModel.collect_frame_outputs)."""
        out = {"f_gather_index": self.f_gather_index, "f_attn_masks": self.f_attn_masks,
               "c_attn_masks": self.c_attn_masks, "frame_map": self.frame_map}
        if self.f_v_feats is not None:
            out["f_v_feats"] = self.f_v_feats
        return out
