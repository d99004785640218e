"""hero_amd.pretrain_eval end to end on the GPU: the tiny model (tests/golden/tiny_model.npz, fp32 compute mode) on the golden
loaders through the real validators, against the dictionaries the REFERENCE's validate_* returned for the same loaders
(tests/golden/case_pretrain_eval.npz).  Counts exactly (the maker asserts a gap of 1e-3 between the two largest logits of every
scored row); losses, l2 and cosine within the 1e-3 relative that tests/test_gpu_pretrain.py carries for the same heads."""
import os
import types

import pytest
import torch

from tests import pretrain_eval_reference as R
from tests.util import GOLDEN, load_tiny, to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-3
CASE = os.path.join(GOLDEN, "case_pretrain_eval.npz")
COUNTS = {"mlm": ("acc",), "mfm-nce": ("acc",), "fom": ("valid/acc",), "mffr": (), "vsm": ()}


def _model(dtype=torch.float32):
    import hero_amd
    from hero_amd import functional as HF
    from hero_amd.model.pretrain import HeroForPretraining
    hero_amd.set_compute_dtype(dtype)
    HF.set_grad_sink(None)
    model, _, _ = load_tiny("cuda", cls=HeroForPretraining)
    model.train()
    return model


def _loaders():
    loaders, outs = R.load_golden(CASE)
    return {t: [to_dev(b, "cuda") for b in bs] for t, bs in loaders.items()}, R.golden_logs(outs)


def _run(model, loaders):
    from hero_amd import pretrain_eval as E
    opts = types.SimpleNamespace(**R.VSM_OPTS)
    return {"mlm": E.validate_mlm(model, loaders["mlm"]), "mffr": E.validate_mffr(model, loaders["mffr"]),
            "mfm-nce": E.validate_mfm_nce(model, loaders["mfm-nce"]), "fom": E.validate_fom(model, loaders["fom"]),
            "vsm": E.validate_vsm(model, loaders["vsm"], opts)}


@pytest.fixture(scope="module")
def kernel_logs():
    model = _model()
    loaders, want = _loaders()
    logs = _run(model, loaders)
    assert model.training
    return logs, want


def test_validators_match_the_reference(kernel_logs):
    logs, want = kernel_logs
    for task, ref in want.items():
        got = {k: v for k, v in logs[task].items() if not k.endswith("_per_s")}
        assert set(got) == set(ref) and len(logs[task]) == len(ref) + 1, task
        for k, v in ref.items():
            print(task, k, got[k], v)
            if k in COUNTS[task]:
                assert got[k] == v, (task, k, got[k], v)
            else:
                assert abs(got[k] - v) <= TOL * abs(v), (task, k, got[k], v)


def test_fallbacks_agree_with_the_kernels(kernel_logs, monkeypatch):
    """The same loaders with the kernels bypassed (float64 PyTorch ops on the same head outputs): equal counts; the means of the
    row losses within the kernels' own per-row tolerances (1e-4 + 1e-4 |loss| for the cross-entropy rows, the recorded fp32 bounds
    for l2 and cosine)."""
    from hero_amd import pretrain_eval as E
    logs, _ = kernel_logs
    monkeypatch.setattr(E, "KERNELS", [False])
    model = _model()
    loaders, _ = _loaders()
    ref = _run(model, loaders)
    for task, keys in COUNTS.items():
        for k in keys:
            assert logs[task][k] == ref[task][k], (task, k)
    for task, k in (("mlm", "loss"), ("mfm-nce", "loss"), ("fom", "valid/loss")):
        assert abs(logs[task][k] - ref[task][k]) <= 1e-4 + 1e-4 * abs(ref[task][k]), (task, k, logs[task][k], ref[task][k])
    for task in ("mffr", "mfm-nce"):
        l2 = "loss" if task == "mffr" else "l2"
        assert abs(logs[task][l2] - ref[task][l2]) <= R.FEAT_L2_REL * ref[task][l2], (task, logs[task][l2], ref[task][l2])
        assert abs(logs[task]["cosine"] - ref[task]["cosine"]) <= R.FEAT_COS_ABS, (task, logs[task]["cosine"], ref[task]["cosine"])
    for k, v in ref["vsm"].items():
        if not k.endswith("_per_s"):
            assert abs(logs["vsm"][k] - v) <= 1e-6 * abs(v), k                      # no kernel of this module on that path


def test_bf16_heads_are_scored_as_they_are_stored(monkeypatch):
    """bf16 compute mode: the kernels read the heads' GEMM outputs (bf16 for MLM and MFM-NCE) as stored; the float64 fallback on
    the same stored values gives the same counts, and losses within the per-row tolerance of the cross-entropy arithmetic."""
    import hero_amd
    from hero_amd import pretrain_eval as E
    tasks = ("mlm", "mfm-nce", "fom")
    run = lambda m, ld: {"mlm": E.validate_mlm(m, ld["mlm"]), "mfm-nce": E.validate_mfm_nce(m, ld["mfm-nce"]),    # noqa: E731
                         "fom": E.validate_fom(m, ld["fom"])}
    try:
        seen = []
        real = E.ce_eval
        monkeypatch.setattr(E, "ce_eval", lambda logits, *a, **k: seen.append(logits.dtype) or real(logits, *a, **k))
        got = run(_model(torch.bfloat16), _loaders()[0])
        # two MLM and two MFM-NCE batches: the bf16 GEMM outputs; the two FOM batches in whatever dtype that head's GEMM writes
        assert len(seen) == 6 and seen[:4] == [torch.bfloat16] * 4 and all(d in (torch.bfloat16, torch.float32) for d in seen[4:])
        monkeypatch.setattr(E, "KERNELS", [False])
        ref = run(_model(torch.bfloat16), _loaders()[0])
    finally:
        hero_amd.set_compute_dtype(torch.float32)
    for task in tasks:
        for k, v in ref[task].items():
            if k.endswith("_per_s"):
                continue
            print(task, k, got[task][k], v)
            if k in COUNTS[task]:
                assert got[task][k] == v, (task, k)
            elif k.endswith("loss"):
                assert abs(got[task][k] - v) <= 1e-4 + 1e-4 * abs(v), (task, k, got[task][k], v)


def test_validate_returns_the_prefixed_keys(kernel_logs):
    from hero_amd import pretrain_eval as E
    logs, _ = kernel_logs
    model = _model()
    loaders, _ = _loaders()
    out = E.validate(model, {"mlm_tv": loaders["mlm"], "vsm_how2": loaders["vsm"]}, types.SimpleNamespace(**R.VSM_OPTS))
    assert set(out) == {"mlm_tv_" + k for k in logs["mlm"]} | {"vsm_how2_" + k for k in logs["vsm"]}
    assert model.training
    assert out["mlm_tv_acc"] == logs["mlm"]["acc"] and abs(out["mlm_tv_loss"] - logs["mlm"]["loss"]) <= 1e-6 * logs["mlm"]["loss"]
    assert abs(out["vsm_how2_valid/loss_overall"] - logs["vsm"]["valid/loss_overall"]) <= 1e-6 * logs["vsm"]["valid/loss_overall"]
