"""Validation of the retrieval tasks (reference: train_vcmr.py:339-394 `validate_vcmr`, train_vr.py:335-382 `validate_vr`,
eval_vr.py:137-305 `validate_full_vr`, eval_vcmr.py:143-515 `validate_full_vcmr`).

The two in-training validators run the model's own eval path and keep the loss sums on the device: one host read after the
loader is exhausted (the reference reads two or three `.item()`s per batch), summed over the ranks like its all_gather_list.

The two full drivers close the loop of hero_amd.retrieval: `encode_corpus` once, `CorpusIndex.search` per query batch,
`postprocess` (moments only) and `RecallMeter`; they return the reference's `(val_log, submission)`.  Everything a query batch
produces stays on the device until the loader is exhausted; the lists of the submission are then copied to the host once.
Ground truth comes per query from `opts.query_data[qid]` (the reference's query_data: "ts" = [st, ed] or a list of at least four
[st, ed] pairs - DiDeMo - and optionally "type") and is packed with `pack_gt_ts`.

`video_items`: {video name: item tuple of hero_amd.collate.video_item / video_only_item}; videos are numbered in sorted name
order as the reference numbers them, and `opts.video2idx` (default: that numbering) gives the indices the submission carries.
"""
from time import time

import torch

from . import retrieval as R
from .collate import video_collate
from .pretrain_eval import _Eval, _read
from .utils import distributed as dist_utils

TYPES = {"v": 0, "t": 1, "vt": 2}


def _opt(opts, name, default):
    return getattr(opts, name, default)


def _model_batch(batch):
    return {k: v for k, v in batch.items() if k != "qids"}            # train_vcmr.py:352-354


def _normalise(sums, n_ex_pos, opts):
    val_loss_neg_ctx, val_loss_neg_q = sums
    if n_ex_pos > 0 and opts.lw_neg_q > 0 and opts.lw_neg_ctx > 0:
        val_loss_neg_ctx /= n_ex_pos
        val_loss_neg_q /= n_ex_pos
        val_loss_neg_ctx /= opts.lw_neg_ctx
        val_loss_neg_q /= opts.lw_neg_q
    return val_loss_neg_ctx, val_loss_neg_q


def _validate(model, val_loader, opts, n_terms):
    """The loop of both validators: n_terms loss tensors per batch, their float64 sums accumulated on the device."""
    sums, n_ex, n_ex_pos, st = None, 0, 0, time()
    ranked = opts.lw_neg_ctx != 0 or opts.lw_neg_q != 0
    with _Eval(model):
        for batch in val_loader:
            n_ex += len(batch["q_vidx"])
            out = model(_model_batch(batch), opts.task, compute_loss=True)
            loss_neg_ctx = out[-2]
            z = loss_neg_ctx.new_zeros((), dtype=torch.float64)
            cur = torch.stack([t.double().sum() if ranked or i < n_terms - 2 else z for i, t in enumerate(out)])
            sums = cur if sums is None else sums + cur
            if ranked:
                n_ex_pos += len(loss_neg_ctx) if loss_neg_ctx.ndim > 0 else 1
    vals = _read(sums if sums is not None else [0.0] * n_terms, n_ex, n_ex_pos)
    return vals[:n_terms], vals[n_terms], vals[n_terms + 1], time() - st


def validate_vcmr(model, val_loader, opts):
    """train_vcmr.py:339-394; opts: task, lw_st_ed, lw_neg_ctx, lw_neg_q."""
    (val_loss_st_ed, *ranks), n_ex, n_ex_pos, tot_time = _validate(model, val_loader, opts, 3)
    if opts.lw_st_ed:
        val_loss_st_ed /= n_ex
        val_loss_st_ed /= opts.lw_st_ed
    val_loss_neg_ctx, val_loss_neg_q = _normalise(ranks, n_ex_pos, opts)
    val_loss = opts.lw_st_ed * val_loss_st_ed + opts.lw_neg_ctx * val_loss_neg_ctx + opts.lw_neg_q * val_loss_neg_q
    return {"valid/loss_overall": val_loss, "valid/loss_st_ed": val_loss_st_ed, "valid/loss_neg_ctx": val_loss_neg_ctx,
            "valid/loss_neg_q": val_loss_neg_q, "valid/ex_per_s": n_ex / tot_time}


def validate_vr(model, val_loader, opts):
    """train_vr.py:335-382; opts: task, lw_neg_ctx, lw_neg_q."""
    ranks, n_ex, n_ex_pos, tot_time = _validate(model, val_loader, opts, 2)
    val_loss_neg_ctx, val_loss_neg_q = _normalise(ranks, n_ex_pos, opts)
    val_loss = opts.lw_neg_ctx * val_loss_neg_ctx + opts.lw_neg_q * val_loss_neg_q
    return {"valid/loss_overall": val_loss, "valid/loss_neg_ctx": val_loss_neg_ctx, "valid/loss_neg_q": val_loss_neg_q,
            "valid/ex_per_s": n_ex / tot_time}


# --------------------------------------------------------------------------------------------- #
# full-corpus drivers
# --------------------------------------------------------------------------------------------- #
def _to(batch, device):
    return {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _corpus(model, video_items, opts, batch_size):
    """(index, sorted video names, local numbering, the submission's numbering)."""
    names = sorted(video_items)
    local = {v: i for i, v in enumerate(names)}
    device = next(model.parameters()).device
    batches = (_to(video_collate([video_items[v] for v in names[i:i + batch_size]]), device) for i in range(0, len(names), batch_size))
    index = R.encode_corpus(model, batches, int(opts.max_clip_len))
    return index, names, local, dict(_opt(opts, "video2idx", None) or local)


def _gathered(metrics, n_ex, opts):
    """eval_vcmr.py:430-448: the ranks' metrics weighted by their query counts."""
    if _opt(opts, "distributed_eval", False) and dist_utils.world_size() > 1:
        n_per_rank, m_per_rank = dist_utils.all_gather_list(n_ex), dist_utils.all_gather_list(metrics)
    else:
        n_per_rank, m_per_rank = [n_ex], [metrics]
    total = sum(n_per_rank)
    out = {}
    for task_type, task_metric in metrics.items():
        out[task_type] = {k: sum(n * m[task_type][k] for n, m in zip(n_per_rank, m_per_rank)) / total
                          for k in task_metric if k != "desc_type_ratio"}
    return out, total


def _vr_lists(qids, scores, indices, names, video2idx, top_n):
    """eval_vr.py:245-266 / eval_vcmr.py:356-372 on host arrays: the first 100 of every row, cut to top_n."""
    return [dict(desc_id=qid, desc="", predictions=[[video2idx[names[int(v)]], 0, 0, float(s)] for s, v in zip(srow[:100], vrow[:100])][:top_n])
            for qid, srow, vrow in zip(qids, scores.tolist(), indices.tolist())]


@torch.no_grad()
def validate_full_vr(model, video_items, query_loader, split, opts):
    """eval_vr.py:137-305.  opts: max_clip_len, max_vr_video, vr_eval_video_batch_size (50); optional video2idx, distributed_eval.
    query_loader yields vr_full_eval_collate batches.  -> (val_log, submission)."""
    st = time()
    with _Eval(model):
        index, names, local, video2idx = _corpus(model, video_items, opts, int(_opt(opts, "vr_eval_video_batch_size", 50)))
        device = index.ctx.device
        meter = R.RecallMeter(iou_thds=(), device=device)
        qids, scores, indices = [], [], []
        for batch in query_loader:
            gt = torch.tensor([local.get(v, -1) for v in batch["vids"]], dtype=torch.int32, device=device)
            b = _to(batch, device)
            out = index.search(model, b["query_input_ids"], b["query_pos_ids"], b["query_attn_masks"], tasks=("VR",), q2c_alpha=0,
                               max_vcmr_video=int(opts.max_vr_video))      # alpha 0: the scores themselves (eval_vr.py:228-233)
            meter.update(out, gt)
            qids.extend(batch["qids"])
            scores.append(out["vr_scores"])
            indices.append(out["vr_indices"])
        metrics = meter.compute()
        scores, indices = torch.cat(scores).cpu(), torch.cat(indices).cpu()                  # the one copy of the lists
    submission = {"VR": _vr_lists(qids, scores, indices, names, video2idx, int(opts.max_vr_video)), "video2idx": video2idx}
    gathered, n_ex = _gathered({"VR": metrics["VR"]}, len(qids), opts)
    val_log = {f"valid_{split}_{t}/{t}_{k}": v for t, m in gathered.items() for k, v in m.items()}
    val_log[f"valid/vr_{split}_ex_per_s"] = n_ex / (time() - st)
    return val_log, submission


def _ground_truth(qids, vids, local, query_data, device):
    """(gt_vidx, gt_ts, gt_n, desc_type) of one query batch; gt_ts is None when no query of the run carries a timestamp."""
    gt = torch.tensor([local.get(v, -1) for v in vids], dtype=torch.int32, device=device)
    rows = [query_data[q] for q in qids] if query_data is not None else []
    if not rows or any("ts" not in r or r["ts"] is None for r in rows):
        return gt, None, None, None
    gt_ts, gt_n = R.pack_gt_ts([r["ts"] for r in rows])
    types = None
    if all("type" in r for r in rows):
        types = torch.tensor([TYPES[r["type"]] for r in rows], dtype=torch.int32, device=device)
    return gt, gt_ts.to(device), gt_n.to(device), types


def _moment_lists(qids, post, task, gt, names, video2idx):
    """eval_vcmr.py:339-354, 396-414 on host copies of a `postprocess` dictionary."""
    st, ed, sc = (post[task + k].cpu() for k in ("_nms_st_sec", "_nms_ed_sec", "_nms_scores"))
    live = (post[task + "_nms_st"] >= 0).cpu()
    video = post["vcmr_nms_video"].cpu() if task == "vcmr" else gt.cpu().view(-1, 1).expand_as(st)
    res = []
    for q, qid in enumerate(qids):
        keep = live[q].nonzero().reshape(-1).tolist()
        res.append(dict(desc_id=qid, desc="", predictions=[[video2idx[names[int(video[q, i])]], float(st[q, i]), float(ed[q, i]), float(sc[q, i])]
                                                             for i in keep]))
    return res


@torch.no_grad()
def validate_full_vcmr(model, video_items, query_loader, split, opts):
    """eval_vcmr.py:143-515.  opts: max_clip_len, full_eval_tasks, q2c_alpha, max_vcmr_video, min_pred_l, max_pred_l, max_before_nms,
    max_after_nms, nms_thd, vfeat_interval, vcmr_eval_video_batch_size (50); query_data {qid: {"ts", ["type"]}}; optional
    video2idx, distributed_eval.  query_loader yields vcmr_full_eval_collate batches.  The metrics before NMS go under
    valid_{split}_{TASK}/{TASK}_{k}, those after NMS (nms_thd != -1) under valid_{split}_{TASK}_nms_{nms_thd}/{TASK}_{k}."""
    st = time()
    tasks = tuple(opts.full_eval_tasks)
    interval, A, nms_thd = float(_opt(opts, "vfeat_interval", 1.5)), int(_opt(opts, "max_after_nms", 100)), _opt(opts, "nms_thd", -1)
    query_data = _opt(opts, "query_data", None)
    if query_data is None:
        query_data = getattr(getattr(query_loader, "dataset", None), "query_data", None)
    with _Eval(model):
        index, names, local, video2idx = _corpus(model, video_items, opts, int(_opt(opts, "vcmr_eval_video_batch_size", 50)))
        device = index.ctx.device
        plain, after = R.RecallMeter(vfeat_interval=interval, device=device), R.RecallMeter(vfeat_interval=interval, device=device)
        qids, kept = [], []
        for batch in query_loader:
            if "SVMR" in tasks and any(v not in local for v in batch["vids"]):      # its kernels index the corpus with the ground-truth video
                raise ValueError("validate_full_vcmr: SVMR needs every query's video in the corpus")
            gt, gt_ts, gt_n, types = _ground_truth(batch["qids"], batch["vids"], local, query_data, device)
            b = _to(batch, device)
            out = index.search(model, b["query_input_ids"], b["query_pos_ids"], b["query_attn_masks"], tasks=tasks, gt_vidx=gt,
                               q2c_alpha=_opt(opts, "q2c_alpha", 20), max_vcmr_video=int(_opt(opts, "max_vcmr_video", 100)),
                               min_pred_l=int(_opt(opts, "min_pred_l", 2)), max_pred_l=int(_opt(opts, "max_pred_l", 16)),
                               max_before_nms=int(_opt(opts, "max_before_nms", 200)))
            if "VR" not in tasks:                           # the video lists behind VCMR are not a result of their own
                out = {k: v for k, v in out.items() if not k.startswith("vr_")}
            post = R.postprocess(out, vfeat_interval=interval, nms_thd=-1, max_after_nms=A)
            two_d = gt_ts is not None and gt_ts.shape[1] == 1
            ts, n = (gt_ts[:, 0], None) if two_d else (gt_ts, gt_n)
            plain.update(post, gt, ts, types, gt_n=n)
            if nms_thd != -1:
                nms = R.postprocess(out, vfeat_interval=interval, nms_thd=nms_thd, max_after_nms=A)
                after.update({k: v for k, v in nms.items() if not k.startswith("vr_")}, gt, ts, types, gt_n=n)
            qids.extend(batch["qids"])
            kept.append((batch["qids"], post, gt))
        metrics, metrics_nms = plain.compute(), after.compute() if nms_thd != -1 else {}
    submission = {}
    for task in ("svmr", "vcmr"):
        if kept and task + "_nms_st" in kept[0][1]:
            submission[task.upper()] = [e for q, post, gt in kept for e in _moment_lists(q, post, task, gt, names, video2idx)]
    if kept and "vr_indices" in kept[0][1]:
        scores, indices = torch.cat([p["vr_scores"] for _, p, _ in kept]).cpu(), torch.cat([p["vr_indices"] for _, p, _ in kept]).cpu()
        submission["VR"] = _vr_lists(qids, scores, indices, names, video2idx, A)
    submission["video2idx"] = video2idx
    val_log = {}
    gathered, n_ex = _gathered(metrics, len(qids), opts)
    for t, m in gathered.items():
        val_log.update({f"valid_{split}_{t}/{t}_{k}": v for k, v in m.items()})
    if nms_thd != -1:
        for t, m in _gathered(metrics_nms, len(qids), opts)[0].items():
            val_log.update({f"valid_{split}_{t}_nms_{nms_thd}/{t}_{k}": v for k, v in m.items()})
    val_log[f"valid/vcmr_{split}_ex_per_s"] = n_ex / (time() - st)
    return val_log, submission
