"""HeroForViolin on the GPU with the tiny configuration, against tests/golden/case_violin.npz - the reference's own batches,
forward, gradients and validation figures (tests/golden/make_golden_violin.py) - and against its own PyTorch formulation of
the head.

Tolerances (none is taken from the code under test)
  * fused head against the PyTorch formulation, fp32: both sides share everything but the head, so the rule of
    tests/test_gpu_violin_kernels.py applies - 4 x PyTorch-fp32's own error, floored at 16 * 2^-24.  PyTorch-fp32's own error
    of each gradient is the one the fixture records: the reference's fp32 run against its float64 run (`grad32_err.<param>`,
    3.0e-8 .. 1.4e-6), and never looser than the 1e-3 the fixture check below holds.  Loss and logits: the floor, relative to
    max(1, |value|) - the fixture's logits stay below 8, where the fused loss and the reference's are the same function.
  * fused path against the fixture, fp32: what tests/test_gpu_parity.py::test_training_losses_grads_adamw_match_reference
    holds reference vectors to - loss and logits rel_err < FP32_TOL = 2e-4, gradients rel_err < 1e-3.
  * graph replay against eager: tests/test_gpu_step.py::test_graph_replay_matches_eager's rtol 2e-4, atol 1e-5."""
import json
import os

import numpy as np
import pytest
import torch

from tests.util import GOLDEN, rel_err, to_dev

pytestmark = pytest.mark.gpu
FP32_TOL = 2e-4
GRAD_TOL = 1e-3
FLOOR = 16 * 2.0 ** -24
Z = np.load(os.path.join(GOLDEN, "case_violin.npz"))
GRADS = sorted(k[len("grad."):] for k in Z.files if k.startswith("grad."))
KERNELS = ("hero_frame_pool_fwd", "hero_frame_pool_bwd", "hero_bce_head_fwd", "hero_bce_head_bwd")


@pytest.fixture(autouse=True)
def _fp32_default():
    import hero_amd
    hero_amd.set_compute_dtype(torch.float32)
    yield
    hero_amd.set_compute_dtype(torch.bfloat16)


def load_model(fused=True):
    from hero_amd.model import HeroForViolin
    from hero_amd.utils.misc import set_dropout
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    sd.update({k[len("param."):]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith("param.")})
    model = HeroForViolin.from_pretrained(os.path.join(GOLDEN, "tiny_config.json"), sd, vfeat_dim=int(z["__vfeat__"]),
                                          max_frm_seq_len=int(z["__max_frm__"])).cuda()
    model.fused_head = fused
    model.train()
    set_dropout(model, 0.0)
    return model


def load_batch(prefix="out"):
    out = {}
    for k in Z.files:
        if k.startswith(prefix + "."):
            a = Z[k]
            out[k[len(prefix) + 1:]] = json.loads(str(a)) if a.dtype.kind == "U" else torch.from_numpy(a)
    return to_dev(out, "cuda")


def run(fused):
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    model = load_model(fused)
    b = load_batch()
    loss = model(b, task="violin", compute_loss=True)
    loss.backward()
    with torch.no_grad():
        logits = model(b, task="violin", compute_loss=False)
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    return float(loss.detach()), logits.detach().clone(), {n: params[n].grad.detach().clone() for n in GRADS}


_RUNS = {}


def _spy_on_kernels(monkeypatch):
    """Counts the calls of the four VIOLIN entry points that go through the binding."""
    from hero_amd import _lib as Lb
    calls = {}
    for name in KERNELS:
        real = getattr(Lb.lib(), name)
        calls[name] = []
        monkeypatch.setattr(Lb.lib(), name, lambda *a, real=real, name=name: (calls[name].append(1), real(*a))[1])
    return calls


def cached_run(fused):
    if fused not in _RUNS:
        _RUNS[fused] = run(fused)
    return _RUNS[fused]


def test_fused_head_equals_pytorch_formulation(monkeypatch):
    calls = _spy_on_kernels(monkeypatch)
    _RUNS.pop(True, None)
    fl, fz, fg = cached_run(True)
    assert all(calls[k] for k in KERNELS), "fused_head = True did not reach the kernels: %s" % {k: len(v) for k, v in calls.items()}
    assert len(calls["hero_frame_pool_fwd"]) == 2 and len(calls["hero_bce_head_fwd"]) == 2      # the loss pass and the logits pass
    for v in calls.values():
        del v[:]
    _RUNS.pop(False, None)
    tl, tz, tg = cached_run(False)
    assert not any(calls.values())
    assert fz.shape == tz.shape == (6, 1) and fz.dtype == torch.float32
    bad = []
    e_loss = abs(fl - tl) / max(1.0, abs(tl))
    e_z = float(((fz - tz).abs() / tz.abs().clamp_min(1.0)).max())
    print("\n[violin] loss fused %.8f  pytorch %.8f  err %.3e  logits err %.3e  tol %.3e" % (fl, tl, e_loss, e_z, FLOOR), end="")
    bad += [("loss", e_loss)] if e_loss > FLOOR else []
    bad += [("logits", e_z)] if e_z > FLOOR else []
    for n in GRADS:
        tol = min(GRAD_TOL, max(FLOOR, 4 * float(Z["grad32_err." + n])))
        err = rel_err(fg[n], tg[n])
        print("\n[violin] grad %-70s err %.3e  tol %.3e" % (n, err, tol), end="")
        bad += [(n, err, tol)] if err > tol else []
    assert len(GRADS) == 5 and not bad, bad


def test_fused_path_matches_reference_vectors():
    loss, logits, g = cached_run(True)
    want = float(Z["violin_loss"])
    assert abs(loss - want) / abs(want) < FP32_TOL
    assert logits.shape == Z["logits"].shape and rel_err(logits, torch.from_numpy(Z["logits"])) < FP32_TOL
    worst = {n: rel_err(g[n], torch.from_numpy(Z["grad." + n])) for n in GRADS}
    print("\n[violin] against the fixture: %s" % {k: "%.3e" % v for k, v in worst.items()})
    assert len(worst) == 5 and not {k: v for k, v in worst.items() if v > GRAD_TOL}, worst


def test_validate_violin_gives_the_reference_figures():
    from hero_amd.violin import validate_violin
    b = load_batch("eval")
    model = load_model(True)
    val_log, results = validate_violin(model, [b], split="val")
    assert results == json.loads(str(Z["val.results"]))
    assert val_log["valid/val_acc"] == float(Z["val.acc"])
    assert abs(val_log["valid/val_loss"] - float(Z["val.loss"])) < FP32_TOL * float(Z["val.loss"])
    assert not model.training and "qids" in b              # eval(), and the caller's batch keeps its qids
    val_log2, results2 = validate_violin(model, [b, b], split="test")      # two batches accumulate; twice the same one: the same means
    assert results2 == results and val_log2["valid/test_acc"] == val_log["valid/val_acc"]
    assert abs(val_log2["valid/test_loss"] - val_log["valid/val_loss"]) < 1e-6


def _train(use_graph, n_micro):
    from hero_amd import functional as HF
    from hero_amd.step import TrainStep
    HF.clear_weight_cache()
    torch.manual_seed(0)
    model = load_model(True)
    b = load_batch()
    ts = TrainStep(model, opts=dict(learning_rate=1e-4, lr_mul=8.0, warmup_steps=2, num_train_steps=100), task="violin",
                   use_graph=use_graph)
    losses = [ts.micro_step(b).clone() for _ in range(n_micro)]
    torch.cuda.synchronize()
    HF.set_grad_sink(None)
    return model, torch.stack(losses).cpu(), ts


def test_train_step_graph_replay_matches_eager():
    m_e, l_e, ts_e = _train(False, 8)
    m_g, l_g, ts = _train(True, 4)            # graph mode runs 2 x accumulation = 4 eager warm-up micro-steps inside its first call
    assert ts.counts["replayed"] == 4 and ts.opts.gradient_accumulation_steps == 2
    torch.testing.assert_close(l_g, l_e[4:], rtol=2e-4, atol=1e-5)
    want = float(Z["violin_loss"])
    assert abs(float(l_e[0]) - want) < FP32_TOL * want
    assert float(l_e[-1]) < float(l_e[0])                                                # it trains
    pe, pg = dict(m_e.named_parameters()), dict(m_g.named_parameters())
    for k in ("violin_pool.weight", "violin_pred_head.linear_2.weight", "violin_pred_head.linear_2.bias",
              "v_encoder.f_encoder.encoder.layer.1.attention.self.key.weight"):
        torch.testing.assert_close(pg[k], pe[k], rtol=2e-4, atol=1e-5)
    for k in ("violin_pool.weight", "violin_pred_head.linear_2.weight", "violin_pred_head.linear_2.bias"):
        assert not torch.equal(pe[k].cpu(), torch.from_numpy(Z["param." + k]))           # the head's parameters moved
    # the head's two optimiser groups carry lr * lr_mul, the rest lr
    from hero_amd.optim import get_lr_sched
    lr = get_lr_sched(ts_e.global_step, ts_e.opts)
    groups = ts_e.optimizer.param_groups
    head = {id(p) for n, p in m_e.named_parameters() if n.startswith("violin_")}
    assert {id(p) for g in groups[:2] for p in g["params"]} == head and len(groups) > 2
    assert [g["lr"] for g in groups[:2]] == [lr * 8.0] * 2 and all(g["lr"] == lr for g in groups[2:]) and lr > 0


def test_over_long_sequence_raises():
    from hero_amd import _lib as Lb
    model = load_model(True)
    b = load_batch()
    limit = Lb.lib().hero_attention_max_len(Lb.F32, 1)
    n = limit - b["c_attn_masks"].shape[1] + 1
    S = b["q_input_ids"].shape[0]
    b["q_input_ids"] = torch.ones(S, n, dtype=torch.long, device="cuda")
    b["q_attn_masks"] = torch.ones(S, n, dtype=torch.long, device="cuda")
    b["q_pos_ids"] = torch.arange(n, device="cuda").unsqueeze(0)
    with pytest.raises(ValueError, match="at most %d" % limit):
        model(b, task="violin", compute_loss=True)


def test_unknown_task_raises():
    with pytest.raises(ValueError, match="Unrecognized task"):
        load_model(True)(load_batch(), task="tvqa")


def test_frame_count_outside_the_envelope_takes_the_pytorch_route(monkeypatch):
    """L > 256: the kernels' frame limit lowered to 8 stands in for it - the fixture's 10 frames are then outside the envelope
    exactly as 257 are outside the real one (the tiny model's position table ends at 16 frames).  No kernel call; the answer is
    the PyTorch route's, and it is the fixture's."""
    from hero_amd import violin as V
    assert V.MAX_L == 256 and not V.pool_in_envelope(257, 300, 128) and V.pool_in_envelope(256, 300, 128)
    calls = _spy_on_kernels(monkeypatch)
    monkeypatch.setattr(V, "MAX_L", 8)
    assert not V.pool_in_envelope(10, 22, 128)
    model = load_model(True)
    loss = model(load_batch(), task="violin", compute_loss=True)
    loss.backward()
    assert not any(calls.values())
    tl, _, tg = cached_run(False)
    assert float(loss.detach()) == tl and torch.equal(model.violin_pool.weight.grad, tg["violin_pool.weight"])
    assert abs(float(loss.detach()) - float(Z["violin_loss"])) < FP32_TOL * float(Z["violin_loss"])
