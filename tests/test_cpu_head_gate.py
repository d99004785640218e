"""Host side of the gated start / end term (no GPU): the draw sequence of hero_amd.head.StEdGate, the window flag, the model's
head_generation counter, and the three gated entry points in the built library."""
import ctypes
import os
import random
import re
from types import SimpleNamespace

import pytest
import torch

from tests.util import GOLDEN, load_tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_draw_is_the_eager_branchs_sequence(monkeypatch):
    from hero_amd.head import StEdGate
    p, n = 0.8, 40
    random.seed(7)
    want = [random.random() > p for _ in range(n)]            # model/pretrain.py:74-75
    after = random.random()
    assert any(want) and not all(want)
    gate = StEdGate("cpu")
    calls = []
    real = random.random
    monkeypatch.setattr(random, "random", lambda: calls.append(1) or real())
    random.seed(7)
    got = []
    for i in range(n):
        got.append(gate.draw(p))
        assert len(calls) == i + 1                            # exactly one number per micro-step
        assert gate.on == got[-1] and gate.gate.tolist() == [int(got[-1])]
    assert got == want
    monkeypatch.undo()
    assert random.random() == after


def test_trainer_draws_only_where_the_model_would():
    """One call per micro-step of a head task in training with lw_st_ed != 0 - none for other tasks, none with lw_st_ed == 0,
    none without a gate: the places where the model's own branch draws nothing either."""
    from hero_amd.head import StEdGate
    from hero_amd.step import draw_st_ed_gate
    gate = StEdGate("cpu")
    model = SimpleNamespace(st_ed_gate=gate, training=True, lw_st_ed=0.01, drop_svmr_prob=0.8)
    random.seed(3)
    state = random.getstate()
    for task in ("mlm", "mfm-nce", "fom", "tvqa", "tvc"):
        assert draw_st_ed_gate(model, task) is None
    model.lw_st_ed = 0
    assert draw_st_ed_gate(model, "tvr") is None and draw_st_ed_gate(model, "vsm") is None
    model.lw_st_ed, model.st_ed_gate = 0.01, None
    assert draw_st_ed_gate(model, "tvr") is None
    assert random.getstate() == state
    model.st_ed_gate = gate
    want = [random.random() > 0.8 for _ in range(6)]
    random.setstate(state)
    got = []
    for task in ("tvr", "vsm", "how2r", "didemo_video_sub", "didemo_video_only", "tvr"):
        assert draw_st_ed_gate(model, task) is gate
        got.append(gate.on)
    assert got == want


def test_close_window_reports_the_or_and_clears_it():
    from hero_amd.head import StEdGate
    gate = StEdGate("cpu")
    assert gate.close_window() is False and gate.used.tolist() == [0]
    for window, want in (((False, False), False), ((True, False), True), ((False, True), True), ((True, True), True),
                         ((False, False), False)):
        for on in window:
            gate.set(on)
            assert gate.gate.tolist() == [int(on)]
        assert gate.close_window() is want
        assert gate.used.tolist() == [int(want)]
        assert gate.window is False
    assert gate.gate.dtype == torch.int32 and gate.used.dtype == torch.int32


def test_head_generation_moves_only_when_a_setter_changes_a_value():
    from hero_amd.head import StEdGate
    model, _, _ = load_tiny("cpu", hard_neg_weight=10)
    assert model.st_ed_gate is None and model.head_generation == 0
    model.set_hard_negative(False, 20, 10)
    model.set_train_st_ed(0.01)
    assert model.head_generation == 0
    model.set_hard_negative(True, 20, 10)
    assert model.head_generation == 1 and model.use_hard_negative is True
    model.set_hard_negative(True, 20, 10)
    assert model.head_generation == 1
    model.set_hard_negative(True, 1, 10.0)
    assert model.head_generation == 2 and model.hard_pool_size == 1
    model.set_train_st_ed(0.05)
    assert model.head_generation == 3 and model.lw_st_ed == 0.05
    model.set_train_st_ed(0.05)
    assert model.head_generation == 3
    names = {id(p): n for n, p in model.named_parameters()}
    assert [names[id(p)] for p in model.st_ed_only_parameters()] == [
        "video_query_linear.weight", "video_query_linear.bias", "video_st_predictor.weight", "video_ed_predictor.weight"]
    gate = StEdGate("cpu").attach(model)
    assert model.st_ed_gate is gate and set(gate.tensor_gates) == set(model.st_ed_only_parameters())
    assert all(w is gate.used for w in gate.tensor_gates.values())


def test_adamw_refuses_gates_without_device_step_counts():
    from hero_amd.head import StEdGate
    from hero_amd.optim import AdamW
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    gate = StEdGate("cpu")
    gate.tensor_gates = {p: gate.used}
    with pytest.raises(RuntimeError, match="step_tensor"):
        AdamW([p]).step(tensor_gates=gate)


def test_gated_entry_points_exist_with_their_argument_lists():
    import json
    from hero_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "hero_hip.h")).read()
    want = {"hero_st_ed_fwd_gated": "const HeroStEd* a, const int32_t* gate, hero_stream_t stream",
            "hero_st_ed_bwd_gated": "const HeroStEd* a, const int32_t* gate, hero_stream_t stream",
            "hero_adamw_multi_gated": "const HeroAdamWMulti* a, const int32_t* tensor_gate, hero_stream_t stream"}
    handle = ctypes.CDLL(build.build())
    for name, args in want.items():
        assert re.search(r"^int %s\(%s\);" % (name, re.escape(args)), header, flags=re.M), name
        assert hasattr(handle, name) and name in _lib.EXPORTS
    handle.hero_abi_version.restype = ctypes.c_int
    assert handle.hero_abi_version() == 3 == _lib.ABI_VERSION
    table = json.load(open(os.path.join(GOLDEN, "abi_sizes.json")))
    assert _lib.abi_struct_sizes() == table["3"]
