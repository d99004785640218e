"""What the tests of the fixed-capacity pre-training forms share: the ragged two-video batch, the seeds and probabilities of
every draw the GPU tests make WITHOUT expecting overflow, and the statement's counts for them (numpy integers,
tests/pretrain_mask_reference.py).  tests/test_cpu_pretrain_fixed.py asserts that those counts fit the default capacities;
the GPU tests rely on that - checked there, not assumed."""
import numpy as np
import torch

from tests import pretrain_mask_reference as R
from tests.test_gpu_pretrain_mask import CLS, MASK_ID, SEEDS, SITES, V_RANGE, _ragged_host

MODEL_SEED, MODEL_P = SEEDS[1], 0.2            # tests/test_gpu_pretrain_fixed.py: one draw per head
STEP_SEED, STEP_P, STEP_DRAWS = 7, 0.2, 48      # tests/test_gpu_step_pretrain_replay.py: advance() before every draw, < 48 draws


def ragged_host():
    return _ragged_host()


def dims(host):
    T, max_vl, D = host["f_v_feats"].shape
    B, NF = host["c_attn_masks"].shape
    return dict(T=T, max_sl=host["f_sub_input_ids"].shape[1], max_vl=max_vl, Lf=host["f_attn_masks"].shape[1], B=B, NF=NF, D=D)


def mlm_statement(host, seed, p):
    ln = host["lengths"]
    return R.mlm_mask(host["f_sub_input_ids"].numpy(), ln["sub_nfrm"], ln["sub_ntok"], host["f_attn_masks"].shape[1], seed, SITES["mlm"],
                      R.threshold(p), MASK_ID, V_RANGE, CLS)


def mfm_statement(host, seed, p):
    d = dims(host)
    return R.mfm_mask(host["lengths"], d["T"], d["max_vl"], d["NF"], seed, SITES["mfm"], R.threshold(p))


def fom_statement(host, seed, p):
    return R.fom_shuffle(host["lengths"]["vid_nfrm"], dims(host)["NF"], seed, SITES["fom"], R.threshold(p))


def draws_without_overflow():
    """(seed, p) of every draw the GPU tests make on the ragged batch with the default capacities."""
    out, seed = [(MODEL_SEED, MODEL_P), (STEP_SEED, STEP_P)], STEP_SEED
    for _ in range(STEP_DRAWS):
        seed = R.advance(seed)
        out.append((seed, STEP_P))
    return out


def partition_statement(mask):
    """(order, rank, m) of hero_mask_partition in numpy: the set indices ascending, then the unset ones ascending."""
    m = np.asarray(mask).reshape(-1) != 0
    order = np.concatenate([np.flatnonzero(m), np.flatnonzero(~m)]).astype(np.int32)
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size, dtype=np.int32)
    return order, rank, int(m.sum())


def host_task_batches(host, seed, p):
    """The task batches on the HOST from the statement's masks, with the keys the oracle reads (python lists included)."""
    s = mlm_statement(host, seed, p)
    mlm = {"input_ids": torch.from_numpy(s["input_ids"]), "position_ids": host["f_sub_pos_ids"], "v_feat": host["f_v_feats"],
           "f_pos_ids": host["f_v_pos_ids"], "attn_masks": host["f_attn_masks"], "gather_index": host["f_gather_index"],
           "txt_mask_tgt": torch.from_numpy(s["txt_mask_tgt"]), "txt_labels": torch.from_numpy(s["txt_labels"])}
    f = mfm_statement(host, seed, p)
    c, fm = torch.from_numpy(f["c_v_masks"]), torch.from_numpy(f["f_v_masks"])
    base = {k: v for k, v in host.items() if k != "lengths"}
    mfm = dict(base)
    mfm.update(f_v_feats=host["f_v_feats"].masked_fill(fm.unsqueeze(-1), 0), c_v_feats=host["c_v_feats"].masked_fill(c.unsqueeze(-1), 0),
               f_v_masks=fm, c_v_masks=c, feat_targets=host["c_v_feats"][c])
    orders, targets = fom_statement(host, seed, p)
    fom = dict(base)
    fom.update(shuffled_orders=torch.from_numpy(orders), targets=torch.from_numpy(targets))
    return {"mlm": mlm, "mfm": mfm, "fom": fom}
