"""Validation of the four pre-training tasks (reference: pretrain.py:387-608 `validate`, `validate_mlm`, `validate_mffr`,
`validate_mfm_nce`, `validate_fom`, `validate_vsm`) with the counters kept on the device.

The reference scores every batch with F.cross_entropy(reduction='sum') on an fp32 copy of the logits, `scores.max(-1)` and
two `.item()` reads.  Here `ce_eval` (hero_ce_eval, hero_amd/csrc/loss.hip) reads the head's own GEMM output once and adds
(loss sum, rows correct, rows valid) to a float64 device triple; `feat_eval` (hero_feat_eval) does the same for the l2 /
cosine terms of MFFR and MFM-NCE.  A validator reads its counters once, after the loader is exhausted, sums them across
ranks and returns the reference's dictionary.

CPU tensors, and anything the kernels refuse (other dtypes, strided views), take the same statement in float64 PyTorch ops,
with the same lowest-column rule among equal maxima (`KERNELS[0] = False` forces that path: the tests compare the two).

The validation batches come from the host collates (hero_amd.collate with the reference's random stream) or from
`PretrainMasker`; with `ignore_index = -1` the fixed-capacity `txt_labels` of `PretrainMasker.static_entries()` is served as
it stands.
"""
from time import time

import torch
from torch.nn import functional as F

from . import _lib as L
from .utils import distributed as dist_utils

KERNELS = [True]


def _kernel_ok(*ts):
    return KERNELS[0] and all(t.is_cuda and t.dim() == 2 and t.dtype in (torch.float32, torch.bfloat16) and t.is_contiguous()
                              and t.data_ptr() % 16 == 0 for t in ts) and len({t.dtype for t in ts}) == 1


def _acc(acc, device):
    if acc is None:
        return torch.zeros(3, dtype=torch.float64, device=device)
    if acc.dtype != torch.float64 or acc.shape != (3,) or acc.device != device or not acc.is_contiguous():
        raise ValueError("pretrain_eval: acc must be a contiguous float64 [3] tensor on the logits' device")
    return acc


def first_argmax(x):
    """Lowest column among those equal to the row maximum (torch.argmax leaves the choice among ties open)."""
    cols = torch.arange(x.shape[1], device=x.device).expand_as(x)
    return torch.where(x == x.max(dim=1, keepdim=True).values, cols, x.shape[1]).min(dim=1).values


def ce_eval_torch(logits, labels, ncols=None, ignore_index=-100, inv_temp=1.0, acc=None, want_pred=False):
    """The statement of hero_ce_eval in float64 PyTorch ops."""
    ncols = logits.shape[1] if ncols is None else int(ncols)
    acc = _acc(acc, logits.device)
    rows = logits.shape[0]
    pred = torch.zeros(rows, dtype=torch.int32, device=logits.device)
    if rows:
        raw = logits[:, :ncols].double()
        y = labels.reshape(-1).to(torch.int64)
        live = (y != ignore_index) & (y >= 0) & (y < ncols)
        x = raw * float(inv_temp)
        loss = torch.logsumexp(x, dim=1) - x.gather(1, y.clamp(0, ncols - 1).unsqueeze(1)).squeeze(1)
        pred = first_argmax(raw).to(torch.int32)
        acc += torch.stack([torch.where(live, loss, torch.zeros_like(loss)).sum(), (live & (pred == y)).sum().double(), live.sum().double()])
    return (acc, pred) if want_pred else acc


def ce_eval(logits, labels, ncols=None, ignore_index=-100, inv_temp=1.0, acc=None, want_pred=False):
    """acc[0..2] += (sum of the valid rows' losses, rows whose arg-max is the label, valid rows) for [rows, ld] logits over
    their first `ncols` columns; returns acc (float64 [3], allocated when None), with want_pred also the int32 [rows]
    predictions.  Nothing is read on the host."""
    if not _kernel_ok(logits):
        return ce_eval_torch(logits, labels, ncols, ignore_index, inv_temp, acc, want_pred)
    rows, ld = logits.shape
    ncols = ld if ncols is None else int(ncols)
    acc = _acc(acc, logits.device)
    lab = labels.reshape(-1).to(torch.int64).contiguous()
    if lab.numel() != rows:
        raise ValueError("ce_eval: %d labels for %d rows" % (lab.numel(), rows))
    pred = torch.empty(rows, dtype=torch.int32, device=logits.device) if want_pred else None
    ws = torch.empty(3 * max(rows, 1), dtype=torch.float32, device=logits.device)
    L.check(L.lib().hero_ce_eval(L.ptr(logits), L.ptr(lab), rows, ncols, ld, L.dt(logits), float(inv_temp), int(ignore_index),
                                 L.ptr(acc), L.ptr(pred), L.ptr(ws), L.stream()))
    return (acc, pred) if want_pred else acc


def feat_eval_torch(pred, target, acc=None):
    """The statement of hero_feat_eval in float64 PyTorch ops."""
    acc = _acc(acc, pred.device)
    if pred.shape[0]:
        p, t = pred.double(), target.double()
        acc += torch.stack([(p - t).pow(2).sum(dim=1).sqrt().sum(), F.cosine_similarity(p, t, dim=-1).sum(),
                            torch.tensor(float(p.shape[0]), dtype=torch.float64, device=p.device)])
    return acc


def feat_eval(pred, target, acc=None):
    """acc[0..2] += (sum of |p - t|, sum of cosine_similarity(p, t), rows) over the rows of two [rows, cols] tensors."""
    if pred.shape != target.shape:
        raise ValueError("feat_eval: shapes differ: %s / %s" % (tuple(pred.shape), tuple(target.shape)))
    if not _kernel_ok(pred, target):
        return feat_eval_torch(pred, target, acc)
    rows, cols = pred.shape
    acc = _acc(acc, pred.device)
    ws = torch.empty(2 * max(rows, 1), dtype=torch.float32, device=pred.device)
    L.check(L.lib().hero_feat_eval(L.ptr(pred), L.ptr(target), rows, cols, cols, cols, L.dt(pred), L.ptr(acc), L.ptr(ws), L.stream()))
    return acc


# ---- validators ------------------------------------------------------------------------------------------------------
class _Eval:
    """eval() + no_grad for the loop, the earlier mode afterwards."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.was_training = self.model.training
        self.model.eval()
        self.grad = torch.no_grad()
        self.grad.__enter__()

    def __exit__(self, *exc):
        self.grad.__exit__(*exc)
        self.model.train(self.was_training)


def _read(*counters):
    """ONE host read of the device counters (and host counts), summed over the ranks like the reference's all_gather_list."""
    vals = []
    for c in counters:
        vals += c.tolist() if torch.is_tensor(c) else list(c) if isinstance(c, (list, tuple)) else [c]
    if dist_utils.world_size() > 1:
        vals = [sum(v) for v in zip(*dist_utils.all_gather_list(vals))]
    return vals


def validate_mlm(model, val_loader):
    """pretrain.py:462-487.  A label of -1 (the slack of a fixed-capacity `txt_labels`) is no word."""
    acc, st = None, time()
    with _Eval(model):
        for batch in val_loader:
            logits, ncols = model.v_encoder.mlm_logits(batch)
            acc = ce_eval(logits, batch["txt_labels"][:logits.shape[0]], ncols=ncols, ignore_index=-1, acc=acc)
    val_loss, n_correct, n_word = _read(acc) if acc is not None else _read(0.0, 0, 0)
    tot_time = time() - st
    return {"loss": val_loss / n_word, "acc": n_correct / n_word, "tok_per_s": n_word / tot_time}


def validate_mffr(model, val_loader):
    """pretrain.py:490-515; divided by c_v_masks.sum() as there."""
    acc, n_feat, st = None, None, time()
    with _Eval(model):
        for batch in val_loader:
            pred = model.v_encoder(batch, "mffr", compute_loss=False)
            acc = feat_eval(pred, batch["feat_targets"][:pred.shape[0]].to(pred.dtype), acc=acc)
            n = batch["c_v_masks"].sum().double().reshape(1)
            n_feat = n if n_feat is None else n_feat + n
    if acc is None:
        val_loss, cosine, _, n_feat = _read(0.0, 0.0, 0, 0)
    else:
        val_loss, cosine, _, n_feat = _read(acc, n_feat)
    tot_time = time() - st
    return {"loss": val_loss / n_feat, "cosine": cosine / n_feat, "feat_per_s": n_feat / tot_time}


def validate_mfm_nce(model, val_loader):
    """pretrain.py:518-561.  The logits are scored WITHOUT the NCE temperature: mfm_nce(compute_loss=False) returns them
    undivided (model/model.py:281-289)."""
    acc, facc, n_neg, st = None, None, 0, time()
    with _Eval(model):
        enc = model.v_encoder
        for batch in val_loader:
            feats, neg_feats = enc(batch, "mfm-nce", compute_loss=False)
            pos_feats = batch["feat_targets"][:feats.shape[0]]
            logits, ncols = enc.mfm_nce_logits(feats, pos_feats, neg_feats)
            targets = torch.arange(logits.shape[0], dtype=torch.long, device=logits.device)
            acc = ce_eval(logits, targets, ncols=ncols, acc=acc)
            facc = feat_eval(feats, pos_feats.to(feats.dtype), acc=facc)
            n_neg += neg_feats.shape[0] * feats.shape[0]
    if acc is None:
        val_loss, n_correct, _, val_l2, cosine, n_feat, n_neg = _read(0.0, 0, 0, 0.0, 0.0, 0, 0)
    else:
        val_loss, n_correct, _, val_l2, cosine, n_feat, n_neg = _read(acc, facc, n_neg)
    tot_time = time() - st
    return {"loss": val_loss / n_feat, "acc": n_correct / n_feat, "l2": val_l2 / n_feat, "cosine": cosine / n_feat,
            "feat_per_s": n_feat / tot_time}


def validate_fom(model, val_loader):
    """pretrain.py:564-608; divided by the number of targets that are not -1.  The batch is left as it came (the reference
    deletes 'targets' and 'vids' from it)."""
    acc, n_ex, st = None, 0, time()
    with _Eval(model):
        for batch in val_loader:
            logits = model.v_encoder.fom_logits(batch)
            acc = ce_eval(logits, batch["targets"].reshape(-1), ignore_index=-1, acc=acc)
            n_ex += len(batch["vids"]) if "vids" in batch else batch["targets"].shape[0]
    val_loss, tot_score, n_valid_ex, n_ex = _read(acc, n_ex) if acc is not None else _read(0.0, 0, 0, 0)
    tot_time = time() - st
    return {"valid/loss": val_loss / n_valid_ex, "valid/acc": tot_score / n_valid_ex, "valid/ex_per_s": n_ex / tot_time}


def validate_vsm(model, val_loader, opts):
    """pretrain.py:409-459: the model's own eval path ('sum' reduction), the three loss tensors accumulated on the device."""
    sums, n_ex, n_ex_pos, st = None, 0, 0, time()
    ranked = opts.lw_neg_ctx != 0 or opts.lw_neg_q != 0
    with _Eval(model):
        for batch in val_loader:
            n_ex += len(batch["q_vidx"])
            loss_st_ed, loss_neg_ctx, loss_neg_q = model(batch, "vsm", compute_loss=True)
            z = loss_st_ed.new_zeros((), dtype=torch.float64)
            cur = torch.stack([loss_st_ed.double().sum(), loss_neg_ctx.double().sum() if ranked else z,
                               loss_neg_q.double().sum() if ranked else z])
            sums = cur if sums is None else sums + cur
            if ranked:
                n_ex_pos += len(loss_neg_ctx) if loss_neg_ctx.ndim > 0 else 1
    if sums is None:
        sums = [0.0, 0.0, 0.0]
    val_loss_st_ed, val_loss_neg_ctx, val_loss_neg_q, n_ex, n_ex_pos = _read(sums, n_ex, n_ex_pos)
    tot_time = time() - st
    if opts.lw_st_ed:
        val_loss_st_ed /= n_ex
        val_loss_st_ed /= opts.lw_st_ed
    if n_ex_pos > 0 and opts.lw_neg_q > 0 and opts.lw_neg_ctx > 0:
        val_loss_neg_ctx /= n_ex_pos
        val_loss_neg_q /= n_ex_pos
        val_loss_neg_ctx /= opts.lw_neg_ctx
        val_loss_neg_q /= opts.lw_neg_q
    val_loss = opts.lw_st_ed * val_loss_st_ed + opts.lw_neg_ctx * val_loss_neg_ctx + opts.lw_neg_q * val_loss_neg_q
    return {"valid/loss_overall": val_loss, "valid/loss_st_ed": val_loss_st_ed, "valid/loss_neg_ctx": val_loss_neg_ctx,
            "valid/loss_neg_q": val_loss_neg_q, "valid/ex_per_s": n_ex / tot_time}


def validate(model, val_dataloaders, opts):
    """pretrain.py:387-406: every loader by its task-name prefix; returns the merged dictionary with the reference's
    f'{task}_{k}' keys (the reference only logs it, under 'valid_{task}/{k}')."""
    out = {}
    was_training = model.training
    model.eval()
    try:
        for task, loader in val_dataloaders.items():
            if task.startswith("mlm"):
                val_log = validate_mlm(model, loader)
            elif task.startswith("mffr"):
                val_log = validate_mffr(model, loader)
            elif task.startswith("mfm-nce"):
                val_log = validate_mfm_nce(model, loader)
            elif task.startswith("fom"):
                val_log = validate_fom(model, loader)
            elif task.startswith("vsm"):
                val_log = validate_vsm(model, loader, opts)
            else:
                raise ValueError(f"Undefined task {task}")
            out.update({f"{task}_{k}": v for k, v in val_log.items()})
    finally:
        model.train(was_training)
    return out
