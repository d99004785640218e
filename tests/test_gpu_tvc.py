"""HeroForTvc on the GPU with the tiny configuration, against tests/golden/case_tvc.npz - the reference's own batches, scores,
loss vectors, gradients and greedy decode (tests/golden/make_golden_tvc.py) - and against its own PyTorch formulation of the
decoder.

Tolerances (none is taken from the code under test)
  * fused path against the fixture, fp32: what tests/test_gpu_parity.py::test_training_losses_grads_adamw_match_reference holds
    reference vectors to - scores and losses rel_err < FP32_TOL = 2e-4, gradients rel_err < 1e-3.
  * fused path against the PyTorch formulation of the same module, fp32: both sides share the encoder, so the difference is the
    decoder's arithmetic only; scores and losses at FP32_TOL, every gradient at min(1e-3, max(16 * 2^-24, 4 x grad32_err)) where
    grad32_err is the error of the reference's own fp32 run against its float64 run that the fixture records (4.2e-7 .. 1.4e-6),
    as tests/test_gpu_violin.py does.
  * graph replay against eager: tests/test_gpu_step.py::test_graph_replay_matches_eager's rtol 2e-4, atol 1e-5."""
import json
import os

import numpy as np
import pytest
import torch

from tests.util import GOLDEN, config_file, rel_err, to_dev

pytestmark = pytest.mark.gpu
FP32_TOL = 2e-4
GRAD_TOL = 1e-3
FLOOR = 16 * 2.0 ** -24
Z = np.load(os.path.join(GOLDEN, "case_tvc.npz"))
DESC = json.loads(str(Z["desc"]))
GRADS = sorted(k[len("grad."):] for k in Z.files if k.startswith("grad."))


@pytest.fixture(autouse=True)
def _fp32_default():
    import hero_amd
    hero_amd.set_compute_dtype(torch.float32)
    yield
    hero_amd.set_compute_dtype(torch.bfloat16)


def load_model(fused=True, lsr=0.1):
    from hero_amd.model import HeroForTvc
    from hero_amd.utils.misc import set_dropout
    cfg = json.load(open(os.path.join(GOLDEN, "tiny_config.json")))
    cfg["d_config"] = DESC["d_config"]
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    sd.update({k[len("param."):]: torch.from_numpy(Z[k].astype(np.float32)) for k in Z.files if k.startswith("param.")})
    model = HeroForTvc.from_pretrained(config_file(cfg, "tiny_tvc.json"), sd, vfeat_dim=int(z["__vfeat__"]),
                                       max_frm_seq_len=int(z["__max_frm__"]), lsr=lsr).cuda()
    model.fused_decoder = fused
    model.train()
    set_dropout(model, 0.0)
    return model


def load_batch(prefix="out", with_index=True):
    from hero_amd.collate import tvc_frame_index
    out = {}
    for k in Z.files:
        if k.startswith(prefix + "."):
            a = Z[k]
            out[k[len(prefix) + 1:]] = json.loads(str(a)) if a.dtype.kind == "U" else torch.from_numpy(a)
    out["clip_ranges"] = tuple(tuple(tuple(r) for r in rs) for rs in out["clip_ranges"])
    if with_index:
        out["cap_frame_index"] = tvc_frame_index(out["clip_ranges"], out["c_v_feats"].shape[1])
    return to_dev(out, "cuda")


_RUNS = {}


def run(fused, lsr):
    """loss vector, its mean through caption_loss (which is what is differentiated), scores and the gradients: once per mode."""
    key = (fused, lsr)
    if key not in _RUNS:
        from hero_amd import functional as HF
        HF.clear_weight_cache()
        model = load_model(fused, lsr)
        b = load_batch()
        mean = model.caption_loss(b)
        mean.backward()
        with torch.no_grad():
            vec = model(b, "train", compute_loss=True)
            scores = model(b, "train", compute_loss=False)
        torch.cuda.synchronize()
        params = dict(model.named_parameters())
        _RUNS[key] = dict(mean=float(mean.detach()), vec=vec.detach().clone(), scores=scores.detach().clone(),
                          grads={n: params[n].grad.detach().clone() for n in GRADS})
    return _RUNS[key]


@pytest.mark.parametrize("lsr,vec_key,grad_key", [(0.1, "loss_lsr", "grad."), (0.0, "loss_ce", "gradce.")], ids=["lsr0.1", "lsr0"])
def test_fused_path_matches_the_reference_fixture(lsr, vec_key, grad_key):
    r = run(True, lsr)
    want = torch.from_numpy(Z[vec_key])
    assert r["vec"].shape == want.shape                                          # valid positions only / ALL positions
    e_vec, e_sc = rel_err(r["vec"], want), rel_err(r["scores"], torch.from_numpy(Z["scores"]))
    print("\n[tvc] fixture lsr %g: loss vector %.3e  scores %.3e  mean %.6f (reference %.6f)" % (lsr, e_vec, e_sc, r["mean"], float(want.mean())), end="")
    assert e_vec < FP32_TOL and e_sc < FP32_TOL
    assert abs(r["mean"] - float(want.mean())) < FP32_TOL * abs(float(want.mean()))       # caption_loss == forward(batch).mean()
    if lsr == 0.0:
        tgt = Z["out.cap_tgt_ids"].reshape(-1)
        assert want.numel() == tgt.size and float(r["vec"][torch.from_numpy(tgt == -1)].abs().max()) == 0.0
    for n in GRADS:
        e = rel_err(r["grads"][n], torch.from_numpy(Z[grad_key + n]))
        print("\n[tvc] fixture lsr %g: grad %-70s %.3e" % (lsr, n, e), end="")
        assert e < GRAD_TOL, (n, e)


@pytest.mark.parametrize("lsr", [0.1, 0.0], ids=["lsr0.1", "lsr0"])
def test_fused_path_matches_the_pytorch_formulation(lsr):
    f, t = run(True, lsr), run(False, lsr)
    assert f["vec"].shape == t["vec"].shape
    e_vec, e_sc = rel_err(f["vec"], t["vec"]), rel_err(f["scores"], t["scores"])
    print("\n[tvc] fused vs torch lsr %g: loss vector %.3e  scores %.3e  means %.6f %.6f" % (lsr, e_vec, e_sc, f["mean"], t["mean"]), end="")
    assert e_vec < FP32_TOL and e_sc < FP32_TOL and abs(f["mean"] - t["mean"]) < FP32_TOL * abs(t["mean"])
    for n in GRADS:
        tol = min(GRAD_TOL, max(FLOOR, 4 * float(Z["grad32_err." + n])))
        e = rel_err(f["grads"][n], t["grads"][n])
        print("\n[tvc] fused vs torch lsr %g: grad %-60s %.3e  tol %.3e" % (lsr, n, e, tol), end="")
        assert e < tol, (n, e, tol)


def test_fused_route_runs_the_kernels_and_a_lowered_limit_takes_the_pytorch_route(monkeypatch):
    """The routing itself: inside the envelope the decoder attentions are hero_dec_attention_fwd launches (2 layers x 2); with
    the Python-side limit below the caption length - a shape 'outside the envelope' without launching one - none is, and the
    result is the PyTorch formulation's."""
    from hero_amd import tvc as T
    calls = []
    real = T.k_dec_attn_fwd
    monkeypatch.setattr(T, "k_dec_attn_fwd", lambda *a, **k: (calls.append(a[3:8]), real(*a, **k))[1])
    model, b = load_model(True), load_batch()
    with torch.no_grad():
        fused = model(b, "train", compute_loss=False)
    Lt, Lv = b["cap_input_ids"].shape[1], b["cap_attn_mask"].shape[1]
    assert len(calls) == 4 and calls[0][1:3] == (Lt, Lt) and calls[1][1:3] == (Lt, Lv) and calls[0][4] and not calls[1][4]
    del calls[:]
    model.max_lq = Lt - 1
    with torch.no_grad():
        routed = model(b, "train", compute_loss=False)
    assert calls == []
    assert rel_err(routed, run(False, 0.1)["scores"]) < 1e-6 and rel_err(routed, fused) < FP32_TOL
    with pytest.raises(ValueError, match="Unrecognized task"):
        model(b, task="violin")


def test_encode_reads_cap_frame_index_or_builds_it_from_clip_ranges():
    model = load_model(True)
    with torch.no_grad():
        a = model.encode(load_batch(with_index=True))
        b = model.encode(load_batch(with_index=False))
    assert torch.equal(a, b)
    assert rel_err(a, torch.from_numpy(Z["enc_out"])) < FP32_TOL
    assert float(a[torch.from_numpy(Z["out.cap_attn_mask"] == 0).cuda()].abs().max()) == 0.0      # zero padding


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
def test_greedy_decode_returns_the_reference_ids(fused):
    from hero_amd.model import TvcGenerator
    model = load_model(fused)
    model.eval()
    gen = TvcGenerator(model, 8, DESC["bos"], int(Z["greedy_eos"]))
    assert gen.greedy_decode(load_batch()) == json.loads(str(Z["greedy"]))
    assert float(Z["greedy_margin"]) >= 1e-3                                     # no arg-max of the fixture is a near tie


def _second_batch(b):
    """The same captions over other frames: every segment that can moves one frame to the right (lengths, masks and shapes stay),
    and the caption tokens are permuted among the captions of equal length - new `cap_frame_index`, new ids."""
    NF = b["c_v_feats"].shape[1]
    idx = b["cap_frame_index"].clone()
    n_valid = b["c_attn_masks"].sum(1)
    for r in range(idx.shape[0]):
        row = idx[r][idx[r] >= 0]
        v = int(row[0]) // NF
        if int(row[-1]) + 1 < v * NF + int(n_valid[v]):
            idx[r, :row.numel()] = row + 1
    assert not torch.equal(idx, b["cap_frame_index"])
    out = dict(b)
    out["cap_frame_index"] = idx
    ids = b["cap_input_ids"].clone()
    ids[:, 1:] = torch.where(ids[:, 1:] == 1, ids[:, 1:], (ids[:, 1:] * 7 + 3) % 157 + 3)
    out["cap_input_ids"] = ids
    return out


def _train(use_graph, n_micro):
    from hero_amd import functional as HF
    from hero_amd.step import TVC_OPTS, TrainStep
    HF.clear_weight_cache()
    model = load_model(True)
    static = load_batch()
    first = {k: v.clone() for k, v in static.items() if torch.is_tensor(v)}
    second = _second_batch(first)
    ts = TrainStep(model, opts=dict(TVC_OPTS, learning_rate=1e-3, lr_mul=2.0, warmup_steps=2, num_train_steps=100), task="tvc",
                   use_graph=use_graph)
    if use_graph:
        ts.prepare(static)                                                        # 4 eager warm-up micro-steps on the first batch, then the capture
    else:
        for _ in range(4):
            ts.micro_step(static)
    losses = []
    for i in range(n_micro):
        src = second if i % 2 else first
        for k in ("cap_frame_index", "cap_input_ids"):
            static[k].copy_(src[k])
        HF.refresh_memo()
        losses.append(ts.micro_step(static).clone())
    torch.cuda.synchronize()
    HF.set_grad_sink(None)
    return model, torch.stack(losses).cpu(), ts


def test_graph_replay_matches_eager_on_changing_batches():
    """TrainStep(task='tvc', use_graph=True): captured once, replayed on two alternating batches copied into the captured
    buffers - the second one with another `cap_frame_index` and other caption ids, so an index or a count frozen at capture
    would show - against the same micro-steps run eagerly."""
    m_e, l_e, _ = _train(False, 6)
    m_g, l_g, ts = _train(True, 6)
    assert ts.counts["replayed"] == 6 and ts.counts["eager_in_graph_mode"] == 0
    print("\n[tvc] losses eager %s\n[tvc] losses graph %s" % (l_e.tolist(), l_g.tolist()), end="")
    torch.testing.assert_close(l_g, l_e, rtol=2e-4, atol=1e-5)
    assert abs(float(l_e[1]) - float(l_e[0])) > 1e-3                             # the second batch IS another batch
    pe, pg = dict(m_e.named_parameters()), dict(m_g.named_parameters())
    for k in pe:
        torch.testing.assert_close(pg[k], pe[k], rtol=2e-4, atol=1e-5, msg=k)
    p0 = torch.from_numpy(Z["param.decoder.layer.0.self_attention.key.weight"].astype(np.float32)).cuda()
    assert float((pe["decoder.layer.0.self_attention.key.weight"].detach() - p0).abs().max()) > 1e-4    # it trains


def test_tvc_task_puts_the_decoder_in_the_lr_mul_groups_and_unknown_models_raise():
    from hero_amd import functional as HF
    from hero_amd.step import TVC_OPTS, TrainStep
    from tests.util import load_tiny
    assert TVC_OPTS["learning_rate"] == 1e-4 and TVC_OPTS["lr_mul"] == 10.0 and TVC_OPTS["betas"] == [0.9, 0.98]
    assert TVC_OPTS["grad_norm"] == 1.0 and TVC_OPTS["warmup_steps"] == 700 and TVC_OPTS["num_train_steps"] == 7000
    model = load_model(True)
    ts = TrainStep(model, opts=TVC_OPTS, task="tvc")
    head = {id(p) for n, p in model.named_parameters() if "v_encoder" not in n}
    assert {id(p) for g in ts.optimizer.param_groups[:2] for p in g["params"]} == head and len(head) > 30
    ts.micro_step(load_batch())
    ts.micro_step(load_batch())
    lr = ts.optimizer.param_groups[2]["lr"]
    assert ts.optimizer.param_groups[0]["lr"] == pytest.approx(10.0 * lr) and lr > 0
    HF.set_grad_sink(None)
    other, _, _ = load_tiny("cuda")
    with pytest.raises(ValueError, match="captioning model"):
        TrainStep(other, task="tvc").micro_step(load_batch())
    HF.set_grad_sink(None)
