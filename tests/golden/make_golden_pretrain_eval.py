#!/usr/bin/env python3
"""Golden vectors for pre-training validation (hero_amd/pretrain_eval.py) by running the *reference's own* validate_mlm /
validate_mffr / validate_mfm_nce / validate_fom / validate_vsm (pretrain.py:409-608) on tiny loaders with the weights of
tests/golden/tiny_model.npz.

Container-only (needs the reference tree), like make_golden_pretrain.py, whose stubs and synthetic collate it reuses.  What
pretrain.py imports at module level beyond the model (TensorBoard logger, the LMDB datasets, the data loaders) is stubbed
here; `all_gather_list` (Horovod on a GPU) is the one-rank identity.

Writes tests/golden/case_pretrain_eval.npz:
  in.<i>.<key>        the two video batches and the per-task keys (MLM targets / labels, MFM masks / targets, FOM orders /
                      targets, VSM queries / targets / q_vidx), built as in make_golden_pretrain.py
                      (every other MLM label and FOM target is then set to the reference's own prediction, so that the
                      counts of an untrained model are neither zero nor everything)
  mlm.<i>.scores      per batch, what each validator scored:  model(batch, 'mlm', compute_loss=False)
  mffr.<i>.pred       model(batch, 'mffr', compute_loss=False)
  nce.<i>.feats / .neg / .logits     model(batch, 'mfm-nce', compute_loss=False) and v_encoder.mfm_nce(..., compute_loss=False)
  fom.<i>.scores      model(batch, 'fom', compute_loss=False)
  vsm.<i>.st_ed / .neg_ctx / .neg_q  model(batch, 'vsm', compute_loss=True) in eval mode ('sum' reduction)
  log.<task>.<key>    the returned dictionaries without the *_per_s keys

Asserted here: in every scored row the largest logit exceeds the second largest by more than 1e-3, so fp32 noise cannot move
a count (rows with exact ties are the kernel tests' business).

Run:  python tests/golden/make_golden_pretrain_eval.py
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G            # noqa: E402  (stubs + synthetic collate)

OPTS = types.SimpleNamespace(lw_st_ed=0.01, lw_neg_ctx=8.0, lw_neg_q=8.0)
MIN_GAP = 1e-3


def install_pretrain_stubs():
    """Module-level imports of pretrain.py that need packages outside the model: stand-ins with the imported names."""
    tbx = types.ModuleType("tensorboardX")
    tbx.SummaryWriter = object
    data = types.ModuleType("data")
    for name in ("SubTokLmdb", "VideoMlmDataset", "mlm_collate", "MfmDataset", "mfm_collate", "VsmDataset", "vsm_collate",
                 "FomDataset", "fom_collate", "FomEvalDataset", "fom_eval_collate", "PrefetchLoader", "MetaLoader"):
        setattr(data, name, None)
    load_data = types.ModuleType("load_data")
    load_data.load_video_sub_dataset = None
    sys.modules.update({"tensorboardX": tbx, "data": data, "load_data": load_data})
    if "tqdm" not in sys.modules:
        try:
            import tqdm            # noqa: F401
        except ImportError:
            t = types.ModuleType("tqdm")
            t.tqdm = lambda it=None, **kw: it
            sys.modules["tqdm"] = t


class Tap:
    """The model as the validators see it, recording every output they score."""

    def __init__(self, model):
        self.model, self.outs = model, []
        self.v_encoder = types.SimpleNamespace(mfm_nce=self.mfm_nce)

    def __call__(self, batch, task, compute_loss=True):
        out = self.model(batch, task, compute_loss=compute_loss)
        self.outs.append(out)
        return out

    def mfm_nce(self, *a, **kw):
        out = self.model.v_encoder.mfm_nce(*a, **kw)
        self.outs.append(out)
        return out

    def eval(self):
        self.model.eval()

    def train(self):
        self.model.train()


def gap_ok(scores):
    top = scores.detach().double().topk(2, dim=-1).values
    assert float((top[:, 0] - top[:, 1]).min()) > MIN_GAP, "a scored row has its two largest logits within %g" % MIN_GAP


def video_batches(gen):
    subs = [[[([0, 1, 2], 6), ([3, 4], 5), ([], 4), ([6, 7], 7)], [([0, 1], 4), ([2, 3, 4], 7)], [([1, 2, 3, 4], 5), ([5], 3), ([7, 8], 6)]],
            [[([0, 1], 5), ([2], 4), ([3, 4, 5], 6)], [([0], 3), ([1, 2], 6), ([], 5), ([4, 5, 6], 4)]]]
    frames = [[9, 6, 10], [7, 8]]
    return [(G.synth_video_batch(gen, s, f), s, f) for s, f in zip(subs, frames)]


def task_keys(gen, vb, subs, n_frames):
    """The per-task batch keys of one video batch (data/mlm.py:134-176, data/mfm.py:77-97, data/fom.py:50-93, data/vsm.py:105-145)."""
    d = {}
    T, Lf = vb["f_attn_masks"].shape
    tgt = torch.zeros(T, Lf, dtype=torch.bool)
    for r in range(T):
        valid = torch.nonzero(vb["f_attn_masks"][r]).reshape(-1)
        tgt[r, valid[-2]] = True                                  # a subtitle token
        if r % 3 == 0:
            tgt[r, valid[-3]] = True
    d["txt_mask_tgt"] = tgt
    d["txt_labels"] = torch.randint(3, 160, (int(tgt.sum()),), generator=gen)
    B, NF = vb["c_attn_masks"].shape
    cm = torch.zeros(B, NF, dtype=torch.bool)
    fm = torch.zeros(T, vb["f_v_feats"].shape[1], dtype=torch.bool)
    row = 0
    for b, vs in enumerate(subs):
        picked = set(torch.randperm(n_frames[b], generator=gen)[:2].tolist())
        for f in picked:
            cm[b, f] = True
        for _, (fr, _nt) in enumerate(vs):
            for j, f in enumerate(fr):
                if f in picked:
                    fm[row, j] = True
            row += 1
    d["c_v_masks"], d["f_v_masks"] = cm, fm
    d["feat_targets"] = vb["c_v_feats"][cm].clone()
    orders = torch.arange(NF).unsqueeze(0).repeat(B, 1)
    targets = torch.full((B, NF), -1, dtype=torch.long)
    for b, nf in enumerate(n_frames):
        pos = torch.randperm(nf, generator=gen)[:3]
        perm = pos[torch.randperm(3, generator=gen)]
        orders[b, pos] = perm
        targets[b, perm] = pos
    d["shuffled_orders"], d["fom_targets"] = orders, targets
    per = 2
    qi, qp, qm = G.synth_queries(gen, B * per, [3 + int(x) for x in torch.randint(0, 5, (B * per,), generator=gen)])
    tg = torch.zeros(B * per, 2, dtype=torch.long)
    for m in range(B * per):
        a, b_ = sorted(torch.randint(0, n_frames[m // per], (2,), generator=gen).tolist())
        tg[m, 0], tg[m, 1] = a, b_
    tg[1, 0] = -1                                                 # one ignored start (padding_value -1)
    d.update({"vsm.query_input_ids": qi, "vsm.query_pos_ids": qp, "vsm.query_attn_masks": qm, "vsm.targets": tg,
              "vsm.q_vidx": torch.arange(B * per) // per})
    return d


def loaders(vbs, keys):
    """The five loaders (lists of batch dicts) from the stored keys - the same assembly as tests/pretrain_eval_reference.py."""
    out = {"mlm": [], "mffr": [], "mfm-nce": [], "fom": [], "vsm": []}
    for vb, k in zip(vbs, keys):
        out["mlm"].append({"input_ids": vb["f_sub_input_ids"], "position_ids": vb["f_sub_pos_ids"], "v_feat": vb["f_v_feats"],
                           "f_pos_ids": vb["f_v_pos_ids"], "attn_masks": vb["f_attn_masks"], "gather_index": vb["f_gather_index"],
                           "txt_mask_tgt": k["txt_mask_tgt"], "txt_labels": k["txt_labels"]})
        for task in ("mffr", "mfm-nce"):
            b = dict(vb)
            b["c_v_feats"] = vb["c_v_feats"].clone()               # forward_mfm mutates it
            b["f_v_feats"] = vb["f_v_feats"].masked_fill(k["f_v_masks"].unsqueeze(-1), 0)
            b.update({"c_v_masks": k["c_v_masks"], "f_v_masks": k["f_v_masks"], "feat_targets": k["feat_targets"]})
            out[task].append(b)
        fb = dict(vb)
        fb.update({"shuffled_orders": k["shuffled_orders"], "targets": k["fom_targets"],
                   "vids": ["v%d" % i for i in range(vb["c_attn_masks"].shape[0])]})
        out["fom"].append(fb)
        sb = dict(vb)
        sb.update({n[4:]: v for n, v in k.items() if n.startswith("vsm.")})
        out["vsm"].append(sb)
    return out


def main():
    G.install_stubs()
    install_pretrain_stubs()
    sys.path.insert(0, G.REF)
    import pretrain as P                           # noqa: reference import
    from model.pretrain import HeroForPretraining  # noqa: reference import
    P.all_gather_list = lambda x: [x]              # one rank

    z = np.load(os.path.join(HERE, "tiny_model.npz"), allow_pickle=False)
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    model = HeroForPretraining.from_pretrained(
        os.path.join(HERE, "tiny_config.json"), state_dict=sd, vfeat_dim=G.VFEAT, max_frm_seq_len=G.MAX_FRM,
        lw_neg_ctx=OPTS.lw_neg_ctx, lw_neg_q=OPTS.lw_neg_q, lw_st_ed=OPTS.lw_st_ed, ranking_loss_type="hinge",
        use_hard_negative=False, hard_pool_size=20, margin=0.1, use_all_neg=True, drop_svmr_prob=0.0)
    model.eval()
    gen = torch.Generator().manual_seed(23)
    made = video_batches(gen)
    vbs = [m[0] for m in made]
    keys = [task_keys(gen, *m) for m in made]
    # an untrained model predicts no random label: every other MLM label and FOM target becomes the reference's own
    # prediction (labels and targets do not enter the forward pass), so the counts are neither 0 nor everything
    with torch.no_grad():
        for b_mlm, b_fom, k in zip(loaders(vbs, keys)["mlm"], loaders(vbs, keys)["fom"], keys):
            k["txt_labels"][::2] = model(b_mlm, "mlm", compute_loss=False).argmax(-1)[::2]
            flat = k["fom_targets"].reshape(-1)
            at = torch.nonzero(flat != -1).reshape(-1)[::2]
            flat[at] = model({n: v for n, v in b_fom.items() if n not in ("targets", "vids")}, "fom", compute_loss=False).argmax(-1)[at]
    d = {}
    for i, (vb, k) in enumerate(zip(vbs, keys)):
        for name, v in G.pack_batch(vb).items():
            d["in.%d.%s" % (i, name[3:])] = v
        for name, v in k.items():
            d["in.%d.%s" % (i, name)] = v.numpy()
    ld = loaders(vbs, keys)
    n = len(vbs)

    def run(fn, task, *extra):
        tap = Tap(model)
        log = fn(tap, [dict(b) for b in ld[task]], *extra)
        for k, v in log.items():
            if not k.endswith("_per_s"):
                d["log.%s.%s" % (task, k)] = np.float64(v)
        return tap.outs

    outs = run(P.validate_mlm, "mlm")
    for i in range(n):
        gap_ok(outs[i])
        d["mlm.%d.scores" % i] = outs[i].detach().numpy()
    outs = run(P.validate_mffr, "mffr")
    for i in range(n):
        d["mffr.%d.pred" % i] = outs[i].detach().numpy()
    outs = run(P.validate_mfm_nce, "mfm-nce")
    for i in range(n):
        (feats, neg), logits = outs[2 * i], outs[2 * i + 1]
        gap_ok(logits)
        d["nce.%d.feats" % i], d["nce.%d.neg" % i], d["nce.%d.logits" % i] = feats.detach().numpy(), neg.detach().numpy(), logits.detach().numpy()
    outs = run(P.validate_fom, "fom")
    for i in range(n):
        gap_ok(outs[i][keys[i]["fom_targets"].reshape(-1) != -1])
        d["fom.%d.scores" % i] = outs[i].detach().numpy()
    outs = run(P.validate_vsm, "vsm", OPTS)
    for i in range(n):
        for name, v in zip(("st_ed", "neg_ctx", "neg_q"), outs[i]):
            d["vsm.%d.%s" % (i, name)] = v.detach().numpy()
    assert not model.training
    np.savez_compressed(os.path.join(HERE, "case_pretrain_eval.npz"), **d)
    for k in sorted(d):
        if k.startswith("log."):
            print(k, float(d[k]))


if __name__ == "__main__":
    main()
