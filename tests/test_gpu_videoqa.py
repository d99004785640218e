"""HeroForVideoQA (TVQA / How2QA) on the GPU with the tiny configuration, against tests/golden/case_videoqa.npz - the reference's
own batch, forward and gradients (tests/golden/make_golden_videoqa.py) - and against its own PyTorch formulation of the head.

Tolerances (none is taken from the code under test)
  * fused pool against the PyTorch formulation, fp32: both sides share everything but the head, so the rule of
    tests/test_gpu_qa_pool_kernels.py applies - 4 x PyTorch-fp32's own error, floored at 16 * 2^-24.  PyTorch-fp32's own
    error of each gradient is the one the fixture records: the reference's fp32 run against its float64 run
    (`<case>.grad32_err.<param>`, 1.4e-6 .. 3.5e-4), and never looser than the 1e-3 the fixture check below holds.
    Losses: the floor, relative to max(1, |loss|).
  * fused path against the fixture, fp32: what tests/test_gpu_parity.py::test_training_losses_grads_adamw_match_reference
    holds reference vectors to - losses and logits rel_err < FP32_TOL = 2e-4, gradients rel_err < 1e-3.
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
LW_ST_ED = 0.4
Z = np.load(os.path.join(GOLDEN, "case_videoqa.npz"))
GRADS = sorted(k[len("a5.grad."):] for k in Z.files if k.startswith("a5.grad."))


@pytest.fixture(autouse=True)
def _fp32_default():
    import hero_amd
    hero_amd.set_compute_dtype(torch.float32)
    yield
    hero_amd.set_compute_dtype(torch.bfloat16)


def load_model(fused=True):
    from hero_amd.model import HeroForVideoQA
    from hero_amd.utils.misc import set_dropout
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    sd.update({k[len("param."):]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith("param.")})
    model = HeroForVideoQA.from_pretrained(os.path.join(GOLDEN, "tiny_config.json"), sd, vfeat_dim=int(z["__vfeat__"]),
                                           max_frm_seq_len=int(z["__max_frm__"])).cuda()
    model.fused_pool = fused
    model.train()
    set_dropout(model, 0.0)
    return model


def load_batch(case):
    out = {}
    for k in Z.files:
        if k.startswith(case + ".out."):
            a = Z[k]
            out[k[len(case) + 5:]] = json.loads(str(a)) if a.dtype.kind == "U" else torch.from_numpy(a)
    return to_dev(out, "cuda")


def run(case, fused):
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    model = load_model(fused)
    qa_loss, temporal_loss = model(load_batch(case), task="tvqa" if case == "a5" else "how2qa", compute_loss=True)
    (qa_loss + LW_ST_ED * temporal_loss).backward()
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    return float(qa_loss), float(temporal_loss), {n: params[n].grad.detach().clone() for n in GRADS}


_RUNS = {}


def _spy_on_kernel(monkeypatch):
    """Counts the calls of hero_qa_pool_fwd that go through the binding."""
    from hero_amd import _lib as Lb
    calls, real = [], Lb.lib().hero_qa_pool_fwd
    monkeypatch.setattr(Lb.lib(), "hero_qa_pool_fwd", lambda *a: (calls.append(1), real(*a))[1])
    return calls


def cached_run(case, fused):
    if (case, fused) not in _RUNS:
        _RUNS[(case, fused)] = run(case, fused)
    return _RUNS[(case, fused)]


@pytest.mark.parametrize("case", ["a5", "a4"])
def test_fused_pool_equals_pytorch_formulation(case, monkeypatch):
    calls = _spy_on_kernel(monkeypatch)
    _RUNS.pop((case, True), None)
    fq, ft, fg = cached_run(case, True)
    assert calls, "fused_pool = True did not reach the kernels"
    del calls[:]
    tq, tt, tg = cached_run(case, False)
    assert not calls
    bad = []
    for name, a, b in (("qa_loss", fq, tq), ("temporal_loss", ft, tt)):
        err = abs(a - b) / max(1.0, abs(b))
        print("\n[videoqa] %s %-14s fused %.8f  pytorch %.8f  err %.3e  tol %.3e" % (case, name, a, b, err, FLOOR), end="")
        bad += [(name, err)] if err > FLOOR else []
    for n in GRADS:
        tol = min(GRAD_TOL, max(FLOOR, 4 * float(Z["%s.grad32_err.%s" % (case, n)])))
        err = rel_err(fg[n], tg[n])
        print("\n[videoqa] %s grad %-70s err %.3e  tol %.3e" % (case, n, err, tol), end="")
        bad += [(n, err, tol)] if err > tol else []
    assert not bad, bad


@pytest.mark.parametrize("case", ["a5", "a4"])
def test_fused_path_matches_reference_vectors(case):
    q, t, g = cached_run(case, True)
    assert abs(q - float(Z[case + ".qa_loss"])) / abs(float(Z[case + ".qa_loss"])) < FP32_TOL
    assert abs(t - float(Z[case + ".temporal_loss"])) / abs(float(Z[case + ".temporal_loss"])) < FP32_TOL
    worst = {n: rel_err(g[n], torch.from_numpy(Z["%s.grad.%s" % (case, n)])) for n in GRADS}
    print("\n[videoqa] %s against the fixture: %s" % (case, {k: "%.3e" % v for k, v in worst.items()}))
    assert len(worst) == 5 and not {k: v for k, v in worst.items() if v > GRAD_TOL}, worst


@pytest.mark.parametrize("case", ["a5", "a4"])
def test_logits_match_reference_vectors(case):
    model = load_model(True)
    with torch.no_grad():
        logits = model(load_batch(case), task="tvqa", compute_loss=False)
    want = torch.from_numpy(Z[case + ".logits"])
    assert logits.shape == want.shape and logits.dtype == torch.float32
    assert rel_err(logits, want) < FP32_TOL


def _train(use_graph, n_micro):
    from hero_amd import functional as HF
    from hero_amd.step import TrainStep
    HF.clear_weight_cache()
    torch.manual_seed(0)
    model = load_model(True)
    b = load_batch("a5")
    ts = TrainStep(model, opts=dict(learning_rate=1e-3, lr_mul=10.0, warmup_steps=2, num_train_steps=100, lw_st_ed=LW_ST_ED),
                   task="tvqa", use_graph=use_graph)
    losses = [ts.micro_step(b).clone() for _ in range(n_micro)]
    torch.cuda.synchronize()
    HF.set_grad_sink(None)
    return model, torch.stack(losses).cpu(), ts


def test_train_step_graph_replay_matches_eager():
    m_e, l_e, _ = _train(False, 10)
    m_g, l_g, ts = _train(True, 6)            # graph mode runs 4 eager warm-up micro-steps inside its first call
    assert ts.counts["replayed"] == 6
    torch.testing.assert_close(l_g, l_e[4:], rtol=2e-4, atol=1e-5)
    q, t = float(Z["a5.qa_loss"]), float(Z["a5.temporal_loss"])
    assert abs(float(l_e[0]) - (q + LW_ST_ED * t)) < FP32_TOL * (q + LW_ST_ED * t)      # qa_loss + lw_st_ed * temporal_loss
    assert float(l_e[-1]) < float(l_e[0])                                                # it trains
    pe, pg = dict(m_e.named_parameters()), dict(m_g.named_parameters())
    for k in ("qa_pool.weight", "st_ed_pool.weight", "qa_pred_head.linear_2.weight"):
        assert rel_err(pg[k], pe[k]) < 5e-4, k
        assert not torch.equal(pe[k].cpu(), torch.from_numpy(Z["param." + k]))           # the head's parameters moved


def test_over_long_sequence_raises():
    from hero_amd import _lib as Lb
    model = load_model(True)
    b = load_batch("a5")
    limit = Lb.lib().hero_attention_max_len(Lb.F32, 1)
    n = limit - b["c_attn_masks"].shape[1] + 1
    S = b["qa_input_ids"].shape[0]
    b["qa_input_ids"] = torch.ones(S, n, dtype=torch.long, device="cuda")
    b["qa_attn_masks"] = torch.ones(S, n, dtype=torch.long, device="cuda")
    b["qa_pos_ids"] = torch.arange(n, device="cuda").unsqueeze(0)
    with pytest.raises(ValueError, match="at most %d" % limit):
        model(b, task="tvqa", compute_loss=True)


def test_unknown_task_raises():
    with pytest.raises(ValueError, match="Unrecognized task"):
        load_model(True)(load_batch("a5"), task="tvr")


def test_answer_count_outside_the_envelope_takes_the_pytorch_route(monkeypatch):
    """A > 8: the 15 rows of the a5 batch fed as ONE video with 15 answer copies.  No kernel call; fused_pool = True gives what
    fused_pool = False gives; and what the head computed is right: its two pooled outputs against the float64 restatement on
    the very inputs it was given, within the `pooled` bound of tests/test_gpu_qa_pool_kernels.py (4 x PyTorch-fp32's worst
    error there, at shapes up to (2, 8, 256, 256, 1024) - this one is (1, 15, 10, 128))."""
    from hero_amd.model import HeroForVideoQA
    from tests import qa_reference as R
    from tests.test_gpu_qa_pool_kernels import TOL
    from tests.util import elem_rel_err
    calls = _spy_on_kernel(monkeypatch)
    seen, real = [], HeroForVideoQA.get_modularized_video

    def spied(self, frame_embeddings, frame_mask):
        out = real(self, frame_embeddings, frame_mask)
        seen.append((frame_embeddings.detach(), frame_mask.detach(), out[0].detach(), out[1].detach()))
        return out
    monkeypatch.setattr(HeroForVideoQA, "get_modularized_video", spied)
    outs = []
    for fused in (True, False):
        model = load_model(fused)
        b = load_batch("a5")
        b["targets"] = torch.tensor([[7]], device="cuda")
        b["ts_targets"] = torch.tensor([[1, 4]], device="cuda")
        q, t = model(b, task="tvqa", compute_loss=True)
        (q + LW_ST_ED * t).backward()
        outs.append((float(q), float(t), model.qa_pool.weight.grad.clone()))
    assert not calls and len(seen) == 2
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
    X, m, se, qa = seen[0]
    assert X.shape[:2] == (1, 15) and m.min() == 0                               # one video, 15 copies, masked frames in it
    ref = R.forward(X, m, model.qa_pool.weight.detach(), model.st_ed_pool.weight.detach())
    for name, got in (("qa_pooled", qa), ("se_pooled", se)):
        err = elem_rel_err(got, ref[name])
        print("\n[videoqa] A = 15 %s against float64: %.3e  tol %.3e" % (name, err, TOL["pooled"]), end="")
        assert err <= TOL["pooled"], (name, err)
