"""Video retrieval (HeroForVr), video-only corpora and the retrieval validators on the GPU, on the tiny golden model and the batches
of tests/golden/case_vr.npz (video-only and video + subtitles).  fp32 compute; the bounds are the ones tests/test_gpu_pretrain.py
carries for the same VSM-head quantities on this model (1e-3 relative, north_star), and for a gradient never less than ten
times the error of the reference's own fp32 run against its float64 one (`grad32_err`)."""
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hero_amd import collate as C
from hero_amd import retrieval as HR
from oracle import hero_oracle as O
from tests import didemo_reference as DR
from tests.util import GOLDEN, rel_err, to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-3
Z = DR.load_vr()
DESC = Z["desc"]
FEATS = {v["vid"]: torch.from_numpy(Z["feat." + v["vid"]]) for v in DESC["videos"]}
OPTS = dict(learning_rate=3e-4, warmup_steps=2, num_train_steps=100, gradient_accumulation_steps=1)


def tiny(cls, **kw):
    import hero_amd
    from hero_amd import functional as HF
    from hero_amd.utils.misc import set_dropout
    hero_amd.set_compute_dtype(torch.float32)
    HF.set_grad_sink(None)
    HF.clear_weight_cache()
    P, cfgj, vfeat, max_frm = O.load_npz_model(os.path.join(GOLDEN, "tiny_model.npz"))
    model = cls.from_pretrained(os.path.join(GOLDEN, "tiny_config.json"), {k: v.clone() for k, v in P.items()}, vfeat_dim=vfeat,
                                max_frm_seq_len=max_frm, **kw).cuda()
    model.train()
    set_dropout(model, 0.0)
    return model


def tiny_vr():
    from hero_amd.model import HeroForVr
    return tiny(HeroForVr, margin=0.1, lw_neg_ctx=10.0, lw_neg_q=10.0, use_all_neg=True)


def tiny_vcmr():
    from hero_amd.model import HeroForVcmr
    return tiny(HeroForVcmr, margin=0.1, lw_neg_ctx=8.0, lw_neg_q=8.0, lw_st_ed=0.01, ranking_loss_type="hinge", use_hard_negative=False,
                hard_pool_size=20, use_all_neg=True, drop_svmr_prob=0.0)


def close(got, want):
    got, want = got.detach().float().cpu().reshape(-1), torch.as_tensor(want).float().reshape(-1)
    assert rel_err(got, want) < TOL, (got, want)
    for a, c in zip(got.tolist(), want.tolist()):
        assert abs(a - c) < TOL * max(abs(c), 1e-2), (got, want)


@pytest.mark.parametrize("name,task", [("vr_vonly", "msrvtt_video_only"), ("vr_sub", "msrvtt_video_sub")])
def test_losses_scores_and_gradients_match_the_reference(name, task):
    model = tiny_vr()
    b = to_dev(DR.batch_of(Z, name), "cuda")
    pre = "vr.%s." % name
    fused = []
    inner = model._head_is_fusable
    model._head_is_fusable = lambda *a, **k: fused.append(inner(*a, **k)) or fused[-1]
    out = model(b, task=task, compute_loss=True)
    assert fused == [True] and len(out) == 2                        # training mode takes the fused head
    (out[0] + out[1]).backward()
    close(out[0], Z[pre + "train_neg_ctx"])
    close(out[1], Z[pre + "train_neg_q"])
    named = dict(model.named_parameters())
    grads = [k[len(pre + "grad."):] for k in Z if k.startswith(pre + "grad.")]
    assert len(grads) == 5
    for n in grads:
        bound = max(TOL, 10 * float(Z[pre + "grad32_err." + n]))
        assert rel_err(named[n].grad, torch.from_numpy(Z[pre + "grad." + n])) < bound, (n, rel_err(named[n].grad, torch.from_numpy(Z[pre + "grad." + n])))
    model.eval()
    with torch.no_grad():
        ec, eq = model(b, task=task, compute_loss=True)
        scores = model(b, task=task, compute_loss=False)
    close(ec, Z[pre + "eval_neg_ctx"])
    close(eq, Z[pre + "eval_neg_q"])
    close(scores, Z[pre + "scores"])
    assert tuple(scores.shape) == (5, 5) and ec.shape == eq.shape == (5,)


def test_a_hundred_frame_video_only_row_reaches_the_long_attention_class():
    """A [CLS; frames] row of 101 positions (the tiny golden model stops at 16 frames): a seeded model with 100 frame positions,
    videos of 100 / 10 / 37 frames, HIP fp32 against the CPU oracle at tests/test_gpu_parity.py's bounds for such a comparison."""
    import hero_amd
    from hero_amd.model import HeroForVr
    from tests.util import config_file, elem_rel_err
    hero_amd.set_compute_dtype(torch.float32)
    layer = dict(attention_probs_dropout_prob=0.1, hidden_act="gelu", hidden_dropout_prob=0.1, hidden_size=128, initializer_range=0.02,
                 intermediate_size=256, max_position_embeddings=130, num_attention_heads=2, type_vocab_size=2)
    cfg = {"f_config": dict(layer, num_hidden_layers=2, vocab_size=160), "c_config": dict(layer, num_hidden_layers=1),
           "q_config": dict(layer, num_hidden_layers=0, type_vocab_size=1, vocab_size=160)}
    torch.manual_seed(0)
    model = HeroForVr.from_pretrained(config_file(cfg, "vr_long_rows.json"), {}, vfeat_dim=96, max_frm_seq_len=100, lw_neg_ctx=10.0, lw_neg_q=10.0)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    P = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.cuda().eval()
    feats = [torch.randn(n, 96, generator=g) for n in (100, 10, 37)]
    queries = [torch.randint(3, 160, (n,), generator=g).tolist() for n in (4, 9, 6)]
    batch = C.vr_collate([C.vr_item(C.video_only_item(f), "v%d" % i, [q]) for i, (f, q) in enumerate(zip(feats, queries))])
    assert batch["f_attn_masks"].shape == (3, 101) and batch["f_attn_masks"].sum(1).tolist() == [101, 11, 38]
    ocfg = O.cfg_from_json(cfg)
    with torch.no_grad():
        ref = O.forward_repr(batch, P, ocfg)
        q_seq = O.f_encoder_txt(batch["query_input_ids"], batch["query_pos_ids"], batch["query_attn_masks"], P, ocfg)
        ref_scores = O.video_level_scores(O.query_feat_encoder(q_seq, batch["query_attn_masks"], P, ocfg), ref, batch["c_attn_masks"])
        b = to_dev(batch, "cuda")
        out = model.v_encoder(b, "repr")
        scores = model(b, task="msrvtt_video_only", compute_loss=False)
    assert rel_err(out, ref, batch["c_attn_masks"]) < 2e-4                # FP32_TOL of tests/test_gpu_parity.py
    assert elem_rel_err(out, ref, batch["c_attn_masks"]) < 1e-3
    assert rel_err(scores, ref_scores) < TOL


def test_device_collate_serves_a_video_only_batch():
    from hero_amd.model.model import build_frame_map
    b = DR.batch_of(Z, "vr_vonly")
    mine = C.vr_collate([C.vr_item(C.video_only_item(FEATS[q["vid"]]), q["vid"], [q["tokens"]]) for q in DESC["queries"]])
    dc = C.DeviceCollate.for_batch(mine, "cuda", vfeat_dim=b["c_v_feats"].shape[2])
    assert dc.Lf == b["f_attn_masks"].shape[1] == 11 and dc.max_sl == 1
    dc.update(mine["lengths"], c_v_feats=b["c_v_feats"].cuda())
    torch.cuda.synchronize()
    for k in ("f_gather_index", "f_attn_masks", "c_attn_masks", "f_v_feats"):
        assert torch.equal(getattr(dc, k).cpu(), b[k]), k
    B, NF = b["c_attn_masks"].shape
    offs, ent, inv = build_frame_map(b["num_subs"], b["sub_idx2frame_idx"], B, NF, dc.Lf, "cpu")
    nnz = int(offs[-1])
    assert torch.equal(dc.offsets.cpu(), offs) and torch.equal(dc.entries.cpu()[:nnz], ent[:nnz]) and torch.equal(dc.inverse.cpu(), inv)
    # and the model gives the same bits from the device-collated batch
    model = tiny_vr().eval()
    dev = to_dev(b, "cuda")
    with torch.no_grad():
        want = model(dev, task="msrvtt_video_only", compute_loss=False)
        dev.update(dc.batch_entries())
        got = model(dev, task="msrvtt_video_only", compute_loss=False)
    assert torch.equal(got, want)


def two_shapes():
    """The fixture's five-query batch and a three-query one (other widths of every tensor), tagged as two buckets."""
    qs = DESC["queries"]
    items = [C.vr_item(C.video_only_item(FEATS[q["vid"]]), q["vid"], [q["tokens"]]) for q in qs]
    a, b = to_dev(C.vr_collate(items), "cuda"), to_dev(C.vr_collate([items[0], items[1], items[3]]), "cuda")
    assert a["query_input_ids"].shape != b["query_input_ids"].shape and a["c_v_feats"].shape[0] != b["c_v_feats"].shape[0]
    a["_bucket"], b["_bucket"] = "five", "three"
    return a, b


def train_run(mode):
    """Six micro-steps (accumulation 1) on two alternating batch shapes, hard negatives switched on after the third.  In 'graph'
    mode the first call runs its two eager warm-up steps inside, so the calls are A B A B and the steps A A A | B A B in all
    modes.  'eager': the same launches issued one by one on the device-side optimiser state (micro_step(eager=True));
    'host': TrainStep(use_graph=False), whose optimiser step takes its step count and learning rate from the host."""
    from hero_amd import functional as HF
    from hero_amd.step import TrainStep
    model = tiny_vr()
    a, b = two_shapes()
    random.seed(5)
    ts = TrainStep(model, opts=OPTS, task="msrvtt_video_only", use_graph=mode != "host")
    losses = []
    try:
        for batch in ([a, b, a, b] if mode == "graph" else [a, a, a, b, a, b]):
            if ts.micro == 3:
                model.set_hard_negative(True, 2, 10.0)
            before = ts.micro
            loss = (ts.micro_step(batch, eager=True) if mode == "eager" else ts.micro_step(batch)).clone()
            if ts.micro - before > 1:
                losses += [x.clone() for x in ts.warmup_losses]
            losses.append(loss)
        assert ts.micro == 6
        torch.cuda.synchronize()
        ts.state_dict()                                            # brings the per-parameter steps to the host
        steps = {n: ts.optimizer.state[p].get("step", 0) if p in ts.optimizer.state else 0 for n, p in model.named_parameters()}
    finally:
        HF.set_grad_sink(None)
        HF.clear_weight_cache()
    return dict(losses=torch.stack(losses).cpu(), params={k: v.detach().clone() for k, v in model.named_parameters()}, steps=steps,
                counts=dict(ts.counts), hard=model.use_hard_negative)


def test_graph_replay_and_eager_steps_end_with_the_same_bits():
    e, g = train_run("eager"), train_run("graph")
    assert g["counts"]["replayed"] == 3 and g["counts"]["captures"] == 3 and e["counts"]["captures"] == e["counts"]["replayed"] == 0, g["counts"]
    assert e["hard"] and g["hard"] and len(e["losses"]) == len(g["losses"]) == 6
    assert torch.isfinite(e["losses"]).all() and int((e["losses"] > 0).sum()) >= 5      # a hinge loss may reach 0 at the end, not before
    assert torch.equal(g["losses"], e["losses"]), (g["losses"], e["losses"])
    diff = [k for k in e["params"] if not torch.equal(g["params"][k], e["params"][k])]
    assert not diff, diff
    assert g["steps"] == e["steps"] and max(e["steps"].values()) == 6
    assert e["steps"]["video_query_linear.weight"] == 0            # lw_st_ed == 0: the start / end term's parameters never move
    # the plain eager trainer (host-side step count and learning rate) under tests/test_gpu_step_recipe.py's bounds
    h = train_run("host")
    torch.testing.assert_close(g["losses"], h["losses"], rtol=2e-4, atol=1e-5)
    worst = max(rel_err(g["params"][k], h["params"][k]) for k in h["params"])
    assert worst < 5e-4 and g["steps"] == h["steps"], worst


def test_didemo_video_only_batches_train_through_the_vcmr_path():
    """vcmr_collate over video_only_item videos (DiDeMo video-only): the three training losses against the CPU oracle, and one
    TrainStep micro-step of task 'didemo_video_only' gives their sum."""
    from hero_amd import functional as HF
    from hero_amd.step import TrainStep
    qs = DESC["queries"]
    batch = C.vcmr_collate([C.vcmr_item(C.video_only_item(FEATS[q["vid"]]), q["vid"], [(q["tokens"], q["ts"])],
                                        frame_interval=DESC["frame_interval"]) for q in qs])
    P, cfgj, _, _ = O.load_npz_model(os.path.join(GOLDEN, "tiny_model.npz"))
    want = [float(x) for x in O.vsm_losses(batch, P, O.cfg_from_json(cfgj), lw_st_ed=0.01, lw_neg_ctx=8.0, lw_neg_q=8.0, margin=0.1)]
    model = tiny_vcmr()
    b = to_dev(batch, "cuda")
    got = model(b, task="didemo_video_only", compute_loss=True)
    close(torch.stack([x.reshape(()) for x in got]), want)
    assert want[0] > 0 and want[1] > 0
    try:
        loss = TrainStep(model, opts=OPTS, task="didemo_video_only").micro_step(b)
        close(loss, sum(want))
    finally:
        HF.set_grad_sink(None)
        HF.clear_weight_cache()


def two_batch_loaders():
    qs = DESC["queries"]
    vr = [([q["qid"]], C.vr_item(C.video_only_item(FEATS[q["vid"]]), q["vid"], [q["tokens"]])) for q in qs]
    vcmr = [C.vcmr_item(C.video_only_item(FEATS[q["vid"]]), q["vid"], [(q["tokens"], q["ts"])], frame_interval=DESC["frame_interval"]) for q in qs]
    return ([to_dev(C.vr_eval_collate(vr[:3]), "cuda"), to_dev(C.vr_eval_collate(vr[3:]), "cuda")],
            [to_dev(C.vcmr_collate(vcmr[:3]), "cuda"), to_dev(C.vcmr_collate(vcmr[3:]), "cuda")])


@pytest.mark.parametrize("which", ["vr", "vcmr"])
def test_in_training_validators_match_the_reference(which):
    from hero_amd.retrieval_eval import validate_vcmr, validate_vr
    vr, vcmr = two_batch_loaders()
    opts = SimpleNamespace(**Z["val.%s.opts" % which])
    model = tiny_vr() if which == "vr" else tiny_vcmr()
    log = (validate_vr(model, vr, opts) if which == "vr" else validate_vcmr(model, vcmr, opts))
    assert model.training
    want = Z["val.%s.log" % which]
    assert set(log) == set(want) | {"valid/ex_per_s"}
    for k, v in want.items():
        print(k, log[k], v)
        assert abs(log[k] - v) < 1e-3 * max(abs(v), 1.0), (k, log[k], v)


def full_inputs(corpus):
    qs = DESC["queries"]
    if corpus == "vonly":
        videos = {v: C.video_only_item(f) for v, f in FEATS.items()}
    else:
        videos = {v["vid"]: C.video_item(FEATS[v["vid"]], [(si, list(fr)) for si, fr in v["subs"]], v["sub_tokens"], sep=DESC["sep"]) for v in DESC["videos"]}
    return videos, qs


@pytest.mark.parametrize("corpus", ["vonly", "sub"])
def test_validate_full_vr_gives_the_reference_log_and_submission(corpus):
    from hero_amd.retrieval_eval import validate_full_vr
    videos, qs = full_inputs(corpus)
    items = [C.vr_full_eval_item(q["qid"], q["tokens"], q["vid"]) for q in qs]
    loader = [C.vr_full_eval_collate(items[:3]), C.vr_full_eval_collate(items[3:])]
    model = tiny_vr()
    opts = SimpleNamespace(max_clip_len=16, max_vr_video=2, vr_eval_video_batch_size=2, task="msrvtt_video_only")
    val_log, sub = validate_full_vr(model, videos, loader, "val", opts)
    assert model.training
    want_log, want_sub, tol = Z["full.%s.val_log" % corpus], Z["full.%s.submission" % corpus], float(Z["full.score_tol"])
    assert {k: v for k, v in val_log.items() if not k.endswith("_ex_per_s")} == want_log and val_log["valid/vr_val_ex_per_s"] > 0
    assert sub["video2idx"] == want_sub["video2idx"] and len(sub["VR"]) == len(want_sub["VR"]) == 5
    for mine, ref in zip(sub["VR"], want_sub["VR"]):
        assert mine["desc_id"] == ref["desc_id"] and mine["desc"] == ref["desc"] and len(mine["predictions"]) == len(ref["predictions"]) == 2
        for (v, s0, e0, s), (rv, rs0, re0, rs) in zip(mine["predictions"], ref["predictions"]):
            assert (v, s0, e0) == (rv, rs0, re0) and abs(s - rs) < tol, (mine, ref)     # every gap is > 10 tol (asserted by the generator)


def test_validate_full_vcmr_with_four_annotators_equals_the_host_statement():
    from hero_amd.retrieval_eval import validate_full_vcmr
    videos, qs = full_inputs("vonly")
    model = tiny_vcmr()
    nfr = {v: f.shape[0] for v, f in FEATS.items()}
    rng = np.random.default_rng(3)
    query_data = {}
    for q in qs:                                                   # three annotators at the query's own moment on the 5 s grid, one elsewhere
        a = 5.0 * int(q["ts"][0] // 5)
        query_data[q["qid"]] = {"ts": [[a, a + 5.0]] * 3 + [[a + 5.0 * int(rng.integers(1, 3)), a + 15.0]]}
    items = [C.vcmr_full_eval_item(q["qid"], q["tokens"], q["vid"], ts=q["ts"], n_frames=nfr[q["vid"]]) for q in qs]
    loader = [C.vcmr_full_eval_collate(items[:3]), C.vcmr_full_eval_collate(items[3:])]
    kw = dict(q2c_alpha=20, max_vcmr_video=3, min_pred_l=1, max_pred_l=6, max_before_nms=30)
    opts = SimpleNamespace(max_clip_len=16, full_eval_tasks=["VCMR", "SVMR", "VR"], max_after_nms=10, nms_thd=0.5, vfeat_interval=1.5,
                           query_data=query_data, **kw)
    val_log, sub = validate_full_vcmr(model, videos, loader, "val", opts)
    assert model.training and set(sub) == {"VCMR", "SVMR", "VR", "video2idx"} and all(len(sub[t]) == 5 for t in ("VCMR", "SVMR", "VR"))
    assert all(len(e["predictions"]) <= 10 for t in ("VCMR", "SVMR") for e in sub[t])
    # the host statement on the same search output
    names = sorted(videos)
    model.eval()
    index = HR.encode_corpus(model, [to_dev(C.video_collate([videos[v] for v in names]), "cuda")], 16)
    gt_ts, gt_n = HR.pack_gt_ts([query_data[q["qid"]]["ts"] for q in qs])
    want = {}
    for nms_thd in (-1, 0.5):
        meter = HR.RecallMeter(vfeat_interval=1.5)
        for lo, hi in ((0, 3), (3, 5)):
            b = to_dev(loader[0 if lo == 0 else 1], "cuda")
            gt = torch.tensor([names.index(q["vid"]) for q in qs[lo:hi]], dtype=torch.int32, device="cuda")
            out = index.search(model, b["query_input_ids"], b["query_pos_ids"], b["query_attn_masks"], tasks=("VCMR", "SVMR", "VR"), gt_vidx=gt, **kw)
            post = {k: v.cpu() for k, v in HR.postprocess_host(out, vfeat_interval=1.5, nms_thd=nms_thd, max_after_nms=10).items()}
            g = gt.cpu().numpy()
            for task in ("vcmr", "svmr"):
                st, ed = post[task + "_nms_st"].numpy(), post[task + "_nms_ed"].numpy()
                video = post["vcmr_nms_video"].numpy() if task == "vcmr" else np.where(st >= 0, g.reshape(-1, 1), -1)
                first = DR.first_hit_multi(video, st, ed, g, gt_ts[lo:hi].numpy(), gt_n[lo:hi].numpy(), 1.5, meter.iou_thds, 100)
                meter.add_first(task.upper(), torch.from_numpy(first), min(100, st.shape[1]))
        want[nms_thd] = meter.compute()
    for t in ("VCMR", "SVMR"):
        for k, v in want[-1][t].items():
            assert val_log["valid_val_%s/%s_%s" % (t, t, k)] == v, (t, k)
        for k, v in want[0.5][t].items():
            assert val_log["valid_val_%s_nms_0.5/%s_%s" % (t, t, k)] == v, (t, k)
    assert any(k.startswith("valid_val_VR/VR_r") for k in val_log) and val_log["valid/vcmr_val_ex_per_s"] > 0
