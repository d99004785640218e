"""The float64 restatements of tests/tvc_reference.py, checked on the CPU against the reference's own formulation
(model/tvc.py:19-64 op for op, in float64) and against tests/golden/case_tvc.npz; the TVC collates, the state-dict names, the
PyTorch route of HeroForTvc, and the library boundary of the captioning kernels."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import tvc_reference as R
from tests.util import GOLDEN


@pytest.fixture(scope="module")
def built_lib():
    from hero_amd import build
    return build.build()


@pytest.mark.parametrize("eps", [0.1, 1.0])
@pytest.mark.parametrize("C", [8, 160, 50272])
def test_closed_form_equals_kl_div(C, eps):
    """loss = H0 - (conf - s)(x_t - lse) - s (sum x - C lse) against F.kl_div(log_softmax(x), smoothed, 'none').sum(1), both in
    float64, values and gradients.  Bound: the kl_div side sums C products of size <= |ln s| + |log p| ~ 25 weighted by targets
    that add up to 1, so its rounding is below C * 2^-53 * 25 = 1.4e-10 at C = 50272; measured 5e-15."""
    g = torch.Generator().manual_seed(C)
    rows = 6
    x = (torch.randn(rows, C, generator=g, dtype=torch.float64) * 3.0)
    labels = torch.randint(0, C, (rows,), generator=g)
    labels[0], labels[1] = 0, C - 1                                               # the first and the last column
    labels[3] = -1                                                                # one ignored row
    valid = labels != -1
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    closed = R.smooth_loss_closed(xa, labels, eps)
    kl = R.smooth_loss_kl(xb, labels, eps)
    assert float(closed.detach()[~valid].abs().max()) == 0.0
    assert float((closed.detach()[valid] - kl.detach()).abs().max()) <= 1.4e-10
    w = torch.randn(rows, generator=g, dtype=torch.float64)
    (closed * w).sum().backward()
    (kl * w[valid]).sum().backward()
    assert float(xa.grad[~valid].abs().max()) == 0.0
    assert float((xa.grad - xb.grad).abs().max()) <= 1.4e-10
    # the gradient formula of the header: (softmax - s - (conf - s) [c == t]) * upstream
    s, conf = eps / (C - 1), 1.0 - eps
    want = torch.softmax(x, 1) - s
    want[torch.arange(rows)[valid], labels[valid]] -= conf - s
    want = want * w.unsqueeze(1) * valid.unsqueeze(1)
    assert float((xa.grad - want).abs().max()) <= 1e-14


def test_smooth_loss_of_uniform_logits_by_hand():
    """x = 0: log p = -ln C for every class, so loss = H0 + ln C * (conf + (C - 1) s) = H0 + ln C."""
    C, eps = 160, 0.1
    s, conf = eps / (C - 1), 1.0 - eps
    h0 = conf * math.log(conf) + (C - 1) * s * math.log(s)
    out = R.smooth_loss(torch.zeros(2, C), torch.tensor([5, -1]), eps, mean=True)
    assert abs(float(out["loss"][0]) - (h0 + math.log(C))) <= 1e-13 and float(out["loss"][1]) == 0.0
    assert out["count"] == 1
    none = R.smooth_loss(torch.zeros(2, C), torch.tensor([-1, -1]), eps, mean=True)    # no valid row: loss 0, zero gradient
    assert float(none["sum"]) == 0.0 and float(none["dx"].abs().max()) == 0.0


def test_reference_attention_masks_are_additive():
    """The restatement follows model/tvc.py:130-133, 184-185: -10000 is ADDED.  A query cannot see later keys, a masked key
    gets probability exp(-10000) = 0, and a caption whose keys are ALL masked keeps softmax(scores) - shift invariance - which
    is the uniform distribution when its key rows are equal (zero-padded encoder rows all project to the key bias)."""
    g = torch.Generator().manual_seed(3)
    N, Lq, Lk, H = 2, 5, 7, 2
    q, k, v = (torch.randn(N * L, H * 64, generator=g) for L in (Lq, Lk, Lk))
    m = torch.ones(N, Lk)
    m[0, 4:] = 0
    m[1] = 0
    k.view(N, Lk, -1)[1] = k.view(N, Lk, -1)[1, :1]                                # equal key rows in the fully masked caption
    out = R.attention(q, k, v, N, Lq, Lk, H, key_mask_add=(1 - m) * -10000.0)
    assert float(out["P"][0, :, :, 4:].max()) == 0.0
    assert float((out["P"][1] - 1.0 / Lk).abs().max()) <= 1e-15
    mean_v = v.view(N, Lk, -1)[1].double().mean(0)
    assert float((out["ctx"].view(N, Lq, -1)[1] - mean_v).abs().max()) <= 1e-14
    c = R.attention(q[:N * Lq], q, q, N, Lq, Lq, H, causal=True)
    assert float(torch.triu(c["P"], diagonal=1).max()) == 0.0


def test_dropout_draw_keeps_one_minus_p():
    mult = R.dropout_multipliers(seed=1234, site=7, threshold16=int(round(0.25 * 65536)), scale=1 / 0.75, N=3, H=2, Lq=33, Lk=50)
    kept = float((mult > 0).double().mean())
    assert abs(kept - 0.75) < 0.02 and set(mult.unique().tolist()) == {0.0, 1 / 0.75}
    other = R.dropout_multipliers(seed=1234, site=8, threshold16=int(round(0.25 * 65536)), scale=1 / 0.75, N=3, H=2, Lq=33, Lk=50)
    assert not torch.equal(mult, other)


def test_envelope_query_needs_no_gpu(built_lib):
    """hero_dec_attention_in_envelope answers on the host; hero_amd.tvc.in_envelope wraps it."""
    from hero_amd import tvc
    assert tvc.in_envelope(torch.bfloat16, 60, 100) and tvc.in_envelope(torch.float32, 64, 128) and tvc.in_envelope(torch.float32, 1, 1)
    for dtype, Lq, Lk in ((torch.float32, 65, 10), (torch.float32, 10, 129), (torch.float32, 0, 10), (torch.bfloat16, 10, 0),
                          (torch.float16, 10, 10)):
        assert not tvc.in_envelope(dtype, Lq, Lk), (dtype, Lq, Lk)


# ---- against tests/golden/case_tvc.npz (the reference's own batches, model outputs and decode) -----------------------------------

Z = np.load(os.path.join(GOLDEN, "case_tvc.npz"))
DESC = json.loads(str(Z["desc"]))


def ref_batch(prefix):
    out = {}
    for k in Z.files:
        if k.startswith(prefix + "."):
            a = Z[k]
            out[k[len(prefix) + 1:]] = json.loads(str(a)) if a.dtype.kind == "U" else torch.from_numpy(a)
    return out


def rebuild(which):
    from hero_amd import collate as C
    want = ref_batch({"train": "out", "val": "val", "eval": "eval"}[which])
    items = []
    for i, v in enumerate(DESC["videos"]):
        video = C.video_item(torch.from_numpy(Z["feat." + v["vid"]]), [(sid, list(fr)) for sid, fr in want["sub_idx2frame_idx"][i]],
                             v["sub_tokens"], sep=2, sub_ctx_len=0)
        if which == "train":
            items.append(C.tvc_item(video, [(c["tokens"], c["ts"]) for c in v["captions"]], bos=DESC["bos"], eos=DESC["eos"],
                                    frame_interval=DESC["frame_interval"]))
        else:
            clips = [(str(c["id"]), c["ts"], "caption %d" % c["id"]) for c in v["captions"]]
            items.append(C.tvc_val_item(video, clips, v["vid"], frame_interval=DESC["frame_interval"], with_gts=which == "val"))
    return {"train": C.tvc_collate, "val": C.tvc_val_collate, "eval": C.tvc_eval_collate}[which](items), want


@pytest.mark.parametrize("which", ["train", "val", "eval"])
def test_tvc_collates_equal_the_reference_collates(which):
    got, want = rebuild(which)
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape, (k, g.shape, w.shape, g.dtype, w.dtype)
            assert torch.equal(g, w), k
        else:
            assert json.loads(json.dumps(g)) == w, k
    assert isinstance(got["clip_ranges"], tuple) and all(isinstance(r, tuple) and isinstance(s, tuple) for r in got["clip_ranges"] for s in r)
    assert set(got) - set(want) == {"lengths", "cap_frame_index"}
    # the one extra key agrees with clip_ranges: row v * NF + frame for the frames of [st, ed), -1 behind them
    idx, NF = got["cap_frame_index"], got["c_v_feats"].shape[1]
    segs = [(v, st, ed) for v, rs in enumerate(got["clip_ranges"]) for st, ed in rs]
    assert idx.dtype == torch.int32 and idx.shape == got["cap_attn_mask"].shape
    for r, (v, st, ed) in enumerate(segs):
        assert idx[r].tolist() == [v * NF + f for f in range(st, ed)] + [-1] * (idx.shape[1] - (ed - st))
    assert torch.equal(idx >= 0, got["cap_attn_mask"].bool())


def test_tvc_st_ed_label_rounds_half_to_even_and_clamps():
    from hero_amd.collate import tvc_frame_index, tvc_st_ed_label
    assert tvc_st_ed_label([0.0, 3.75], 9) == (0, 2)            # 2.5 -> 2 (half up would give 3)
    assert tvc_st_ed_label([0.0, 5.25], 9) == (0, 4)            # 3.5 -> 4
    assert tvc_st_ed_label([3.2, 7.6], 20) == (2, 5)
    assert tvc_st_ed_label([3.2, 3.9], 9) == (2, 3)             # at least one frame
    assert tvc_st_ed_label([6.0, 20.0], 6) == (4, 6)            # clamped at the video's end
    assert tvc_st_ed_label([9.0, 12.0], 6) == (6, 6)            # starts at the end: the empty segment
    assert tvc_st_ed_label([40.0, 50.0], 6) == (6, 6)
    assert tvc_st_ed_label([0.2, 0.4], 6, frame_interval=2.0) == (0, 1)
    ranges = tuple(tuple(tuple(r) for r in rs) for rs in ref_batch("out")["clip_ranges"])
    assert ranges == (((0, 3), (2, 3), (0, 2)), ((4, 6),), ((0, 5), (8, 9)))
    assert tvc_frame_index((((6, 6),),), 6).tolist() == [[-1]]    # an empty segment still has one (padded) position
    with pytest.raises(IndexError):
        tvc_frame_index((((5, 7),),), 6)


def _tvc_config():
    from tests.util import config_file
    cfg = json.load(open(os.path.join(GOLDEN, "tiny_config.json")))
    cfg["d_config"] = DESC["d_config"]
    return config_file(cfg, "tiny_tvc.json")


def _params():
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    sd.update({k[len("param."):]: torch.from_numpy(Z[k].astype(np.float32)) for k in Z.files if k.startswith("param.")})
    return sd, int(z["__vfeat__"]), int(z["__max_frm__"])


def test_state_dict_keys_equal_the_reference():
    from hero_amd.model import HeroForTvc
    sd, vfeat, max_frm = _params()
    model = HeroForTvc.from_pretrained(_tvc_config(), sd, vfeat_dim=vfeat, max_frm_seq_len=max_frm)
    assert sorted(model.state_dict().keys()) == json.loads(str(Z["state_keys"]))
    assert "decoder.layer.1.intermidiate.dense.weight" in model.state_dict() and "decoder.tri_mask" in model.state_dict()
    emb = model.v_encoder.f_encoder
    assert emb.lm_head.decoder.weight is emb.embeddings.word_embeddings.weight            # the shared table
    with pytest.raises(ValueError, match="Unrecognized task"):
        model({}, task="tvr")


def test_float64_restatement_reproduces_the_reference_scores_and_losses():
    """The decoder from the stored parameters and encoder outputs, in float64, against what the reference computed in fp32:
    scores over D = 128 and two layers are a few hundred fp32 roundings - 1e-5 relative to the largest score (the bound of
    tests/test_cpu_violin.py) - and the losses follow the scores at the same relative size."""
    sd, _, _ = _params()
    b = ref_batch("out")
    scores = R.decoder_scores(sd, torch.from_numpy(Z["enc_out"]), b["cap_attn_mask"], b["cap_input_ids"],
                              b["cap_pos_ids"].expand_as(b["cap_input_ids"]), n_layers=DESC["d_config"]["num_hidden_layers"],
                              H=DESC["d_config"]["num_attention_heads"])
    want = torch.from_numpy(Z["scores"]).double()
    assert float((scores - want).abs().max() / want.abs().max()) < 1e-5
    labels = b["cap_tgt_ids"].reshape(-1)
    V = scores.shape[-1]
    lsr = R.smooth_loss_closed(scores.reshape(-1, V), labels, 0.1)[labels != -1]
    want_lsr = torch.from_numpy(Z["loss_lsr"]).double()
    assert lsr.shape == want_lsr.shape and float((lsr - want_lsr).abs().max() / want_lsr.abs().max()) < 1e-5
    ce = R.smooth_loss(scores.reshape(-1, V), labels, 1.0)                               # for the log-softmax only
    nll = -(torch.log_softmax(scores.reshape(-1, V), 1).gather(1, labels.clamp_min(0).unsqueeze(1)).squeeze(1)) * (labels != -1)
    want_ce = torch.from_numpy(Z["loss_ce"]).double()
    assert ce["count"] == int((labels != -1).sum()) and nll.shape == want_ce.shape
    assert float((nll - want_ce).abs().max() / want_ce.abs().max()) < 1e-5
    # the two `.mean()`s divide by different counts: valid positions against all positions
    assert abs(float(lsr.mean()) - float(Z["mean_lsr"])) < 1e-4 and abs(float(nll.mean()) - float(Z["mean_ce"])) < 1e-4
    assert abs(float(nll.sum() / ce["count"]) - float(Z["mean_ce"])) > 0.1


def test_cpu_route_is_the_pytorch_formulation_and_matches_the_fixture():
    """CPU tensors take the PyTorch formulation of the decoder kept in the module (the encoder has no CPU route, so the
    fixture's encoder outputs go in): scores, both loss vectors and the greedy decode against the reference's, at the project's
    fp32 gate (rel_err < 2e-4)."""
    from hero_amd.model import HeroForTvc, TvcGenerator
    from hero_amd.utils.misc import set_dropout
    from tests.util import rel_err
    sd, vfeat, max_frm = _params()
    b = ref_batch("out")
    enc = torch.from_numpy(Z["enc_out"])
    args = (enc, b["cap_attn_mask"], b["cap_input_ids"], b["cap_pos_ids"], b["cap_tgt_ids"])
    for lsr, key in ((0.1, "loss_lsr"), (0.0, "loss_ce")):
        model = HeroForTvc.from_pretrained(_tvc_config(), dict(sd), vfeat_dim=vfeat, max_frm_seq_len=max_frm, lsr=lsr)
        model.train()
        set_dropout(model, 0.0)
        with torch.no_grad():
            loss = model.decode(*args, compute_loss=True)
            assert loss.shape == Z[key].shape and rel_err(loss, torch.from_numpy(Z[key])) < 2e-4
    with torch.no_grad():
        assert rel_err(model.decode(*args, compute_loss=False), torch.from_numpy(Z["scores"])) < 2e-4
    ids = TvcGenerator(model, 8, DESC["bos"], int(Z["greedy_eos"])).greedy_decode(b, encoder_outputs=enc)
    assert ids == json.loads(str(Z["greedy"]))
    assert float(Z["greedy_margin"]) >= 1e-3
