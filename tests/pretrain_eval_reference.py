"""Float64 / integer statement of hero_ce_eval and hero_feat_eval (hero_amd/csrc/loss.hip, include/hero_hip.h "Validation
counters") and of the bookkeeping of the five pre-training validators (hero_amd/pretrain_eval.py; reference: pretrain.py:409-608),
in numpy.  Shared by tests/test_cpu_pretrain_eval.py, tests/test_gpu_pretrain_eval_kernels.py and tests/test_gpu_pretrain_eval.py.
"""
import numpy as np

# ---- hero_ce_eval --------------------------------------------------------------------------------------------------------


def ce_eval_rows(logits, labels, cols, inv_temp=1.0, ignore_index=-100):
    """logits: [rows, ld] array of the STORED values (any float dtype).  Returns (loss [rows] float64, 0 on invalid rows;
    pred [rows] int64; valid [rows] bool)."""
    raw = np.asarray(logits, dtype=np.float64)[:, :cols]
    y = np.asarray(labels, dtype=np.int64).reshape(-1)
    rows = raw.shape[0]
    if rows == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    valid = (y != ignore_index) & (y >= 0) & (y < cols)
    x = raw * float(inv_temp)
    m = x.max(axis=1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
    loss = np.where(valid, lse - x[np.arange(rows), np.clip(y, 0, cols - 1)], 0.0)
    pred = np.argmax(raw == raw.max(axis=1, keepdims=True), axis=1)          # first True: the lowest column among the maxima
    return loss, pred.astype(np.int64), valid


def ce_eval(logits, labels, cols, inv_temp=1.0, ignore_index=-100):
    """(acc [3] float64 = (loss sum, rows correct, rows valid), pred [rows])."""
    loss, pred, valid = ce_eval_rows(logits, labels, cols, inv_temp, ignore_index)
    y = np.asarray(labels, dtype=np.int64).reshape(-1)
    return np.array([loss.sum(), float((valid & (pred == y)).sum()), float(valid.sum())]), pred


def ce_loss_tolerance(logits, labels, cols, inv_temp=1.0, ignore_index=-100):
    """sum over the valid rows of (1e-4 + 1e-4 |loss_r|): the per-row tolerance test_cross_entropy_matches_torch carries for
    the arithmetic of ce_fwd_kernel, which hero_ce_eval repeats."""
    loss, _, valid = ce_eval_rows(logits, labels, cols, inv_temp, ignore_index)
    return float((1e-4 + 1e-4 * np.abs(loss[valid])).sum())


# ---- hero_feat_eval ------------------------------------------------------------------------------------------------------
COS_EPS = 1e-8       # F.cosine_similarity: x.y / (max(|x|, eps) * max(|y|, eps))


def feat_eval_rows(pred, target):
    """(l2 [rows], cos [rows]) in float64."""
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    l2 = np.sqrt(((p - t) ** 2).sum(axis=1))
    cos = (p * t).sum(axis=1) / (np.maximum(np.sqrt((p * p).sum(axis=1)), COS_EPS) * np.maximum(np.sqrt((t * t).sum(axis=1)), COS_EPS))
    return l2, cos


def feat_eval(pred, target):
    l2, cos = feat_eval_rows(pred, target)
    return np.array([l2.sum(), cos.sum(), float(len(l2))])


def _pairwise(x):
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def feat_eval_rows_f32(pred, target, vector=True):
    """The kernel's own evaluation order in float32 (no fused multiply-add: the library is built with -ffp-contract=off): 256
    threads per row; thread i adds the columns 8 i .. 8 i + 7 (+ 2048 per trip) below `cols & ~7` in ascending order, then the
    columns (cols & ~7) + i (+ 256 per trip); the 256 partial sums are added pairwise (neighbours, then neighbouring pairs, ...).
    vector=False: a leading dimension that is no multiple of 8 - every column takes the second form."""
    p, t = np.asarray(pred, dtype=np.float32), np.asarray(target, dtype=np.float32)
    rows, cols = p.shape
    acc = np.zeros((4, rows, 256), dtype=np.float32)
    tid = np.arange(256)

    def add(idx, ok):
        a, b = p[:, idx[ok]], t[:, idx[ok]]
        d = a - b
        acc[0][:, ok] += d * d
        acc[1][:, ok] += a * b
        acc[2][:, ok] += a * a
        acc[3][:, ok] += b * b

    vec_end = (cols & ~7) if vector else 0
    for c0 in range(0, vec_end, 2048):
        ok = c0 + tid * 8 < vec_end
        for k in range(8):
            add(c0 + tid * 8 + k, ok)
    for c0 in range(vec_end, cols, 256):
        add(c0 + tid, c0 + tid < cols)
    dd, pg, pp, gg = (_pairwise(acc[k]) for k in range(4))
    eps = np.float32(COS_EPS)
    return np.sqrt(dd), pg / (np.maximum(np.sqrt(pp), eps) * np.maximum(np.sqrt(gg), eps))


FEAT_ROWS = (1, 5, 300)
FEAT_COLS = (7, 132, 2056, 4352)


def feat_case(rows, cols, seed=0):
    """(pred, target) float32 [rows, cols] whose values bf16 holds exactly (one case serves both dtypes): unit-variance
    features, the LAST row's target all zero (cosine 0 by the eps rule), row 0 with pred == target (l2 exactly 0) when
    rows > 1."""
    g = np.random.default_rng(1000 * rows + cols + seed)

    def bf16(x):
        b = x.astype(np.float32).view(np.uint32)
        b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000          # round to nearest even
        return b.astype(np.uint32).view(np.float32)

    p = bf16(g.standard_normal((rows, cols)))
    t = bf16(p + 0.5 * g.standard_normal((rows, cols)))
    if rows > 1:
        t[0] = p[0]
    t[rows - 1] = 0.0
    return p, t


# Per-row error bounds of the fp32 evaluation above against float64, over feat_case(rows, cols) for every FEAT_ROWS x
# FEAT_COLS, both column forms: 4 x the largest error tests/test_cpu_pretrain_eval.py::test_feat_eval_bound_is_4x_the_fp32_error
# measures (largest measured: l2 1.227e-7 relative, cosine 2.239e-7 absolute), rounded up.  The GPU sums must lie within
# sum_r FEAT_L2_REL * l2_r and rows * FEAT_COS_ABS of the float64 statement.
FEAT_L2_REL = 5.0e-7
FEAT_COS_ABS = 9.0e-7


# ---- validators (pretrain.py:409-608) ------------------------------------------------------------------------------------
def mlm_log(batches):
    """batches: [(logits [n, ld], ncols, labels [n])]; labels of -1 are no words."""
    acc = sum(ce_eval(x, y, c, ignore_index=-1)[0] for x, c, y in batches)
    return {"loss": acc[0] / acc[2], "acc": acc[1] / acc[2]}


def mffr_log(batches):
    """batches: [(pred [n, D], targets [n, D], c_v_masks.sum())]."""
    acc = sum(feat_eval(p, t) for p, t, _ in batches)
    n_feat = float(sum(int(n) for _, _, n in batches))
    return {"loss": acc[0] / n_feat, "cosine": acc[1] / n_feat}


def mfm_nce_log(batches):
    """batches: [(feats [n, D], pos_feats [n, D], logits [n, ld], ncols)]; the label of row r is r, no temperature."""
    acc = sum(ce_eval(x, np.arange(x.shape[0]), c)[0] for _, _, x, c in batches)
    facc = sum(feat_eval(f, p) for f, p, _, _ in batches)
    n_feat = facc[2]
    return {"loss": acc[0] / n_feat, "acc": acc[1] / n_feat, "l2": facc[0] / n_feat, "cosine": facc[1] / n_feat}


def fom_log(batches):
    """batches: [(logits [B * L, C], targets [B, L])]; targets of -1 are not scored."""
    acc = sum(ce_eval(x, y, x.shape[1], ignore_index=-1)[0] for x, y in batches)
    return {"valid/loss": acc[0] / acc[2], "valid/acc": acc[1] / acc[2]}


def vsm_log(batches, lw_st_ed, lw_neg_ctx, lw_neg_q):
    """batches: [(n_queries, loss_st_ed (scalar), loss_neg_ctx [n], loss_neg_q [n])] as the eval path returns them."""
    st_ed = sum(float(np.asarray(b[1], dtype=np.float64).sum()) for b in batches)
    ctx = q = 0.0
    n_ex = sum(int(b[0]) for b in batches)
    n_pos = 0
    if lw_neg_ctx != 0 or lw_neg_q != 0:
        ctx = sum(float(np.asarray(b[2], dtype=np.float64).sum()) for b in batches)
        q = sum(float(np.asarray(b[3], dtype=np.float64).sum()) for b in batches)
        n_pos = sum(np.asarray(b[2]).size if np.asarray(b[2]).ndim > 0 else 1 for b in batches)
    if lw_st_ed:
        st_ed = st_ed / n_ex / lw_st_ed
    if n_pos > 0 and lw_neg_q > 0 and lw_neg_ctx > 0:
        ctx, q = ctx / n_pos / lw_neg_ctx, q / n_pos / lw_neg_q
    return {"valid/loss_overall": lw_st_ed * st_ed + lw_neg_ctx * ctx + lw_neg_q * q, "valid/loss_st_ed": st_ed,
            "valid/loss_neg_ctx": ctx, "valid/loss_neg_q": q}


# ---- tests/golden/case_pretrain_eval.npz (tests/golden/make_golden_pretrain_eval.py) ----------------------------------------
VSM_OPTS = dict(lw_st_ed=0.01, lw_neg_ctx=8.0, lw_neg_q=8.0)          # the maker's OPTS
TASKS = ("mlm", "mffr", "mfm-nce", "fom", "vsm")


def load_golden(path):
    """(loaders, outs): loaders[task] = list of batch dicts (torch tensors / host lists) assembled as the maker's `loaders()`;
    outs = every other array of the file ('mlm.0.scores', ..., 'log.mlm.loss')."""
    import json
    import torch
    z = np.load(path)
    raw, outs = {}, {}
    for k in z.files:
        a = z[k]
        if k.startswith("in."):
            i, name = k[3:].split(".", 1)
            raw.setdefault(int(i), {})[name] = json.loads(str(a)) if a.dtype.kind == "U" else torch.from_numpy(a)
        else:
            outs[k] = a
    loaders = {t: [] for t in TASKS}
    extra = ("txt_mask_tgt", "txt_labels", "c_v_masks", "f_v_masks", "feat_targets", "shuffled_orders", "fom_targets")
    for i in sorted(raw):
        k = raw[i]
        vb = {n: v for n, v in k.items() if n not in extra and not n.startswith("vsm.")}
        loaders["mlm"].append({"input_ids": vb["f_sub_input_ids"], "position_ids": vb["f_sub_pos_ids"], "v_feat": vb["f_v_feats"],
                               "f_pos_ids": vb["f_v_pos_ids"], "attn_masks": vb["f_attn_masks"], "gather_index": vb["f_gather_index"],
                               "txt_mask_tgt": k["txt_mask_tgt"], "txt_labels": k["txt_labels"]})
        for task in ("mffr", "mfm-nce"):
            b = dict(vb)
            b["c_v_feats"] = vb["c_v_feats"].clone()                  # forward_mfm mutates it
            b["f_v_feats"] = vb["f_v_feats"].masked_fill(k["f_v_masks"].unsqueeze(-1), 0)
            b.update({"c_v_masks": k["c_v_masks"], "f_v_masks": k["f_v_masks"], "feat_targets": k["feat_targets"]})
            loaders[task].append(b)
        fb = dict(vb)
        fb.update({"shuffled_orders": k["shuffled_orders"], "targets": k["fom_targets"],
                   "vids": ["v%d" % j for j in range(vb["c_attn_masks"].shape[0])]})
        loaders["fom"].append(fb)
        sb = dict(vb)
        sb.update({n[4:]: v for n, v in k.items() if n.startswith("vsm.")})
        loaders["vsm"].append(sb)
    return loaders, outs


def golden_logs(outs):
    """{task: {key: value}} of the reference's returned dictionaries."""
    logs = {}
    for k, v in outs.items():
        if k.startswith("log."):
            _, task, key = k.split(".", 2)
            logs.setdefault(task, {})[key] = float(v)
    return logs


# ---- cases of hero_ce_eval shared by the CPU (fallback) and GPU (kernel) tests ---------------------------------------------
CE_SHAPES = ((3, 7, 7),              # fewer columns than lanes
             (5, 100, 100),          # ld % 8 != 0: every column on the scalar path
             (64, 1931, 1936),       # vector body plus scalar tail
             (37, 50265, 50272),     # vocabulary: 25 trips, padding columns
             (300, 24, 24))          # fold past one workgroup's width
CE_IGNORE = -1


def ce_case(rows, cols, ld, seed=0):
    """(logits float32 [rows, ld], labels int64 [rows]).  Logits lie on the grid k / 8, |k| <= 32 (exact in bf16; every row
    holds its maximum many times once cols >> 65, so the lowest-column rule is exercised throughout), with planted rows:
      row 0   the only maxima (5.0) at two columns one thread meets in neighbouring trips (2047 / 2048) when cols allows, else
              at columns 1 and cols - 1; the label is the FIRST of them (correct)
      row 1   maxima at 5 and 2053 (else 1 and cols - 1); the label is the SECOND (incorrect)
      row 2   maxima at column 8 of the vector body and at cols - 1 (the scalar tail when cols % 8 != 0); label 8 (correct)
    Every padding column holds 6.0, above every valid column.  Labels: uniform in [0, cols), every third row from 3 on the
    statement's own prediction, and from the end backwards the invalid values -1 (= CE_IGNORE), cols and ld - 1 (when that
    is a padding column)."""
    g = np.random.default_rng(7919 * rows + 31 * cols + ld + seed)
    x = (g.integers(-32, 33, size=(rows, ld)) / 8.0).astype(np.float32)
    y = g.integers(0, cols, size=rows).astype(np.int64)
    first = (2047, 2048) if cols > 2048 else (1, cols - 1)
    second = (5, 2053) if cols > 2053 else (1, cols - 1)
    third = (8, cols - 1) if cols > 9 else (0, cols - 1)
    x[0, list(first)] = 5.0
    y[0] = first[0]
    x[1, list(second)] = 5.0
    y[1] = second[1]
    x[2, list(third)] = 5.0
    y[2] = third[0]
    x[:, cols:] = 6.0
    pred = ce_eval_rows(x, y, cols)[1]
    y[3::3] = pred[3::3]
    bad = [-1, cols] + ([ld - 1] if ld - 1 >= cols else [])
    if rows >= 3 + len(bad):
        y[rows - len(bad):] = bad
    return x, y
