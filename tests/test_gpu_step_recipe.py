"""hipGraph replay of the reference's own recipe (config/train-tvr-8gpu.json: drop_svmr_prob 0.8, hard negatives and loss weights
switched during the run): the start / end term behind a device gate that follows the host's per-micro-step draw, the optimiser
step that skips the term's own parameters in windows that never used it, and graphs re-recorded when the schedule moves.

Tiny golden model, case_train.npz (4 videos, 10 frames, hidden 128; the start / end term is 3 % of the loss), fp32, dropout 0,
accumulation 2 - as tests/test_gpu_step.py.  Graph against eager under that file's bounds: losses rtol 2e-4 / atol 1e-5, every
parameter rel_err < 5e-4."""
import os
import random

import pytest
import torch

from oracle import hero_oracle as O
from tests.util import GOLDEN, load_tiny, rel_err, to_dev

pytestmark = pytest.mark.gpu

OPTS = dict(learning_rate=1e-3, warmup_steps=2, num_train_steps=100)
ONLY_ST_ED = ("video_query_linear.weight", "video_query_linear.bias", "video_st_predictor.weight", "video_ed_predictor.weight")
ENCODER = "v_encoder.f_encoder.encoder.layer.0.attention.self.query.weight"
DROP = 0.8


def draws(seed, n, p=DROP):
    """The gates of n micro-steps after random.seed(seed), as the model's eager branch draws them (model/pretrain.py:74-75)."""
    random.seed(seed)
    return [random.random() > p for _ in range(n)]


def run(mode, n_micro, seed=None, events=None, record=False, **model_kw):
    """mode 'eager' (the model draws), 'graph' (use_graph=True), 'gated_eager' (eager launches, a StEdGate attached by hand).
    events: {micro-step count: fn(model)} applied when the trainer has run that many micro-steps (warm-up included).
    Returns a dict: losses of all n_micro micro-steps, parameters, per-parameter Adam steps, counts, ..."""
    import hero_amd
    from hero_amd import functional as HF
    from hero_amd.head import StEdGate
    from hero_amd.step import TrainStep
    from hero_amd.utils.misc import set_dropout
    hero_amd.set_compute_dtype(torch.float32)
    HF.set_grad_sink(None)
    HF.clear_weight_cache()
    model, _, _ = load_tiny("cuda", **model_kw)
    model.train()
    set_dropout(model, 0.0)
    batch, _ = O.load_npz_case(os.path.join(GOLDEN, "case_train.npz"))
    b = to_dev(batch, "cuda")
    parts = []
    if record:                                             # the three loss terms of every forward of this run
        inner = model.forward

        def forward(*a, **k):
            out = inner(*a, **k)
            parts.append([o.detach().clone() for o in out])
            return out
        model.forward = forward
    ts = TrainStep(model, opts=OPTS, use_graph=mode == "graph")
    if mode == "gated_eager":
        StEdGate(torch.device("cuda")).attach(model)
    if seed is not None:
        random.seed(seed)
    losses, captures_at = [], []
    try:
        while ts.micro < n_micro:
            if events and ts.micro in events:
                events[ts.micro](model)
            before = ts.micro, ts.counts["captures"]
            loss = ts.micro_step(b).clone()
            if ts.micro - before[0] > 1:                   # the first graph-mode call: its eager warm-up micro-steps ran inside
                losses += [x.clone() for x in ts.warmup_losses]
            losses.append(loss)
            if ts.counts["captures"] != before[1]:
                captures_at.append(before[0])
        torch.cuda.synchronize()
        next_draw = random.random()
        ts.state_dict()                                    # brings the per-parameter steps to the host
        steps = {n: ts.optimizer.state[p].get("step", 0) if p in ts.optimizer.state else 0 for n, p in model.named_parameters()}
    finally:
        HF.set_grad_sink(None)
        HF.clear_weight_cache()
    return dict(losses=torch.stack(losses).cpu(), params={k: v.detach().clone() for k, v in model.named_parameters()}, steps=steps,
                counts=dict(ts.counts), captures_at=captures_at, next_draw=next_draw,
                parts=[torch.stack([x.reshape(()) for x in p]).cpu() for p in parts], gate=getattr(model, "st_ed_gate", None))


def same_run(got, want):
    torch.testing.assert_close(got["losses"], want["losses"], rtol=2e-4, atol=1e-5)
    worst = max(rel_err(got["params"][k], want["params"][k]) for k in want["params"])
    assert worst < 5e-4, worst
    assert got["steps"] == want["steps"], {k: (got["steps"][k], want["steps"][k]) for k in want["steps"] if got["steps"][k] != want["steps"][k]}


_GRAPH = {}


def graph_run(seed):
    """The replayed 16 micro-steps of a seed, run once for the tests that read them."""
    if seed not in _GRAPH:
        _GRAPH[seed] = run("graph", 16, seed=seed, drop_svmr_prob=DROP)
    return _GRAPH[seed]


@pytest.mark.parametrize("seed", [10, 20])
def test_graph_replay_follows_the_host_draw(seed):
    gates = draws(seed, 17)
    nxt, gates = gates[16], gates[:16]
    windows = [(gates[i], gates[i + 1]) for i in range(0, 16, 2)]
    # a Python whose generator differs must fail here, not test nothing
    assert (False, False) in windows and (True, True) in windows and ((False, True) in windows or (True, False) in windows), gates
    if seed == 10:
        assert not any(gates[:4]) and sum(any(w) for w in windows) == 4            # the term is first used after the graphs exist
    e = run("eager", 16, seed=seed, record=True, drop_svmr_prob=DROP)
    g = graph_run(seed)                                                             # no RuntimeError
    assert g["gate"] is not None and e["gate"] is None
    assert g["counts"]["captures"] == 1 and g["counts"]["replayed"] == 12 and g["counts"]["eager_in_graph_mode"] == 0
    same_run(g, e)
    # the draws: one per micro-step in both runs, none by the capture - the next number is the 17th of the sequence
    draws(seed, 16)
    want_next = random.random()
    assert e["next_draw"] == want_next == g["next_draw"]
    assert (want_next > DROP) == nxt
    # Adam steps: the term's own parameters advance in the windows that used the term, everything else in all eight
    on_windows = sum(any(w) for w in windows)
    for k in ONLY_ST_ED:
        assert g["steps"][k] == on_windows, (k, g["steps"][k], on_windows)
    assert g["steps"][ENCODER] == 8
    # a gated-off micro-step's loss is the two ranking terms alone; a gated-on one carries the third
    assert len(e["parts"]) == 16
    for i, (on, parts) in enumerate(zip(gates, e["parts"])):
        rank = parts[1] + parts[2]
        if on:
            assert float(parts[0]) > 50 * (2e-4 * float(rank) + 1e-5), (i, parts)     # far above the tolerance: a stuck gate fails
            torch.testing.assert_close(g["losses"][i], parts.sum(), rtol=2e-4, atol=1e-5)
        else:
            assert float(parts[0]) == 0.0
            torch.testing.assert_close(g["losses"][i], rank, rtol=2e-4, atol=1e-5)


def test_gated_eager_and_gated_replay_give_the_same_bits():
    g = graph_run(10)
    e = run("gated_eager", 16, seed=10, drop_svmr_prob=DROP)
    assert e["counts"]["captures"] == 0 and e["counts"]["replayed"] == 0
    assert torch.equal(g["losses"], e["losses"]), (g["losses"] - e["losses"]).abs().max()
    assert g["steps"] == e["steps"]


def _hard(model):
    model.set_hard_negative(True, 1, 10.0)


@pytest.mark.parametrize("variant", ["weights_move", "term_joins"])
def test_schedule_changes_reach_the_replayed_step(variant):
    if variant == "weights_move":
        kw = dict(drop_svmr_prob=0.0)
        events = {6: _hard, 10: lambda m: m.set_train_st_ed(0.05)}
        captures_at, eager_steps = [0, 6, 10], 0
    else:
        kw = dict(drop_svmr_prob=0.0, lw_st_ed=0)
        events = {6: lambda m: m.set_train_st_ed(0.01)}
        captures_at, eager_steps = [0, 8], 2                  # the window in which the term joins runs eagerly, then one re-record
    e = run("eager", 14, events=events, **kw)
    g = run("graph", 14, events=events, **kw)
    same_run(g, e)
    if variant == "weights_move":
        assert float(e["losses"][6]) > 2 * float(e["losses"][5])                   # the hard negatives are felt (pool 1, weight 10)
    else:
        assert e["steps"][ONLY_ST_ED[0]] == 4 and e["steps"][ENCODER] == 7
    # each change re-records once, at a window start (the first entry is the capture itself: micro-step 0)
    assert g["counts"]["captures"] == len(captures_at) and g["captures_at"] == captures_at
    assert all(m % 2 == 0 for m in g["captures_at"])
    assert g["counts"]["eager_in_graph_mode"] == eager_steps
    assert g["gate"] is None                                                       # drop_svmr_prob = 0: nothing is gated


def test_setters_that_change_nothing_keep_the_graphs():
    same = {6: lambda m: (m.set_hard_negative(False, 20, 10), m.set_train_st_ed(0.01))}
    g = run("graph", 10, events=same, drop_svmr_prob=0.0)
    assert g["counts"]["captures"] == 1 and g["captures_at"] == [0]


def test_vsm_windows_in_a_task_mix():
    """HeroForPretraining, windows vsm, mlm, mlm, vsm, mlm behind two warm-up windows of each task, as
    tests/test_gpu_step.py::test_multi_task_graph_replay_keeps_per_parameter_adam_steps - now with drop_svmr_prob = 0.8."""
    import hero_amd
    from hero_amd import functional as HF
    from hero_amd.model import HeroForPretraining
    from hero_amd.model.layers import BertEncoder
    from hero_amd.step import TrainStep
    from hero_amd.utils.misc import set_dropout
    from tests.test_oracle_golden import _task_batches
    seed = 20
    gates = draws(seed, 9)
    vsm_windows = [(gates[i], gates[i + 1]) for i in range(0, 8, 2)]
    assert sorted({sum(w) for w in vsm_windows}) == [0, 1, 2], gates
    hero_amd.set_compute_dtype(torch.float32)
    pre, _ = O.load_npz_case(os.path.join(GOLDEN, "case_pretrain.npz"))
    mlm, _, _ = _task_batches(pre)
    vsm, _ = O.load_npz_case(os.path.join(GOLDEN, "case_train.npz"))
    batches = {"mlm": to_dev(mlm, "cuda"), "vsm": to_dev(vsm, "cuda")}
    windows = ["vsm", "mlm", "mlm", "vsm", "mlm"]

    def one(use_graph):
        HF.set_grad_sink(None)
        HF.clear_weight_cache()
        model, _, _ = load_tiny("cuda", cls=HeroForPretraining, drop_svmr_prob=DROP)
        model.train()
        set_dropout(model, 0.0)
        ts = TrainStep(model, opts=OPTS, task="vsm", use_graph=use_graph)
        random.seed(seed)
        for t in ("vsm", "mlm"):
            if use_graph:
                ts.prepare(batches[t], t)
            else:
                for _ in range(4):
                    ts.micro_step(batches[t], t)
        for t in windows:
            for _ in range(2):
                ts.micro_step(batches[t], t)
        torch.cuda.synchronize()
        nxt = random.random()
        ts.state_dict()
        steps = {n: ts.optimizer.state[p].get("step", 0) if p in ts.optimizer.state else 0 for n, p in model.named_parameters()}
        HF.set_grad_sink(None)
        return {k: v.detach().clone() for k, v in model.named_parameters()}, steps, nxt

    BertEncoder.allow_packing = False
    try:
        pe, se, ne = one(False)
        pg, sg, ng = one(True)
    finally:
        BertEncoder.allow_packing = True
        HF.clear_weight_cache()
        hero_amd.set_compute_dtype(torch.bfloat16)
    # eight vsm micro-steps drew eight numbers; the ten mlm micro-steps (and the captures) drew none
    draws(seed, 8)
    want_next = random.random()
    assert ne == want_next == ng
    on = sum(any(w) for w in vsm_windows)
    assert se["video_query_linear.weight"] == on and se["v_encoder.f_encoder.lm_head.dense.weight"] == 5 and se[ENCODER] == 9
    assert sg == se, {k: (sg[k], se[k]) for k in se if sg[k] != se[k]}
    worst = max(rel_err(pg[k], pe[k]) for k in pe)
    assert worst < 5e-4, worst


def test_pytorch_formulation_of_the_head_behind_a_gate():
    """fused_head = False: the term is always computed and multiplied by the gate word read as a float tensor."""
    import hero_amd
    from hero_amd import functional as HF
    from hero_amd.head import StEdGate
    from hero_amd.utils.misc import set_dropout
    hero_amd.set_compute_dtype(torch.float32)
    HF.set_grad_sink(None)
    HF.clear_weight_cache()
    try:
        model, _, _ = load_tiny("cuda", drop_svmr_prob=DROP)
        model.train()
        set_dropout(model, 0.0)
        model.fused_head = False
        batch, _ = O.load_npz_case(os.path.join(GOLDEN, "case_train.npz"))
        b = to_dev(batch, "cuda")
        model.drop_svmr_prob = 0.0                             # ungated: the term is always kept
        plain = [x.detach().clone().reshape(()) for x in model(b, task="tvr", compute_loss=True)]
        model.drop_svmr_prob = DROP
        gate = StEdGate(torch.device("cuda")).attach(model)
        own = dict(model.named_parameters())
        state = random.getstate()
        for on in (True, False):
            model.zero_grad(set_to_none=True)
            gate.set(on)
            out = model(b, task="tvr", compute_loss=True)
            sum(o.sum() for o in out).backward()
            torch.cuda.synchronize()
            got = [x.detach().reshape(()) for x in out]
            torch.testing.assert_close(got[1], plain[1], rtol=1e-6, atol=0)
            torch.testing.assert_close(got[2], plain[2], rtol=1e-6, atol=0)
            if on:
                torch.testing.assert_close(got[0], plain[0], rtol=1e-6, atol=0)
                assert float(plain[0]) > 0 and all(float(own[k].grad.abs().max()) > 0 for k in ONLY_ST_ED)
            else:
                assert float(got[0]) == 0.0
                assert all(float(own[k].grad.abs().max()) == 0.0 for k in ONLY_ST_ED)
                assert float(own[ENCODER].grad.abs().max()) > 0
        assert random.getstate() == state                      # with a gate the model draws nothing
    finally:
        HF.set_grad_sink(None)
        HF.clear_weight_cache()
        hero_amd.set_compute_dtype(torch.bfloat16)
