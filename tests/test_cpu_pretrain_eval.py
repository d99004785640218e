"""hero_amd.pretrain_eval without a GPU: the float64 PyTorch fallbacks of ce_eval / feat_eval against the numpy statement
(tests/pretrain_eval_reference.py), the validators' bookkeeping against the dictionaries the REFERENCE's own validate_* returned
(tests/golden/case_pretrain_eval.npz, written by tests/golden/make_golden_pretrain_eval.py), two gloo ranks against one, and the
fp32 error bound the GPU test of hero_feat_eval uses."""
import os
import types

import numpy as np
import pytest
import torch

from tests import pretrain_eval_reference as R
from tests.util import GOLDEN

CASE = os.path.join(GOLDEN, "case_pretrain_eval.npz")


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---- fallbacks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in R.CE_SHAPES if s[1] < 5000], ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=str)
@pytest.mark.parametrize("inv_temp", [1.0, 0.7])
def test_ce_eval_fallback_matches_the_statement(shape, dtype, inv_temp):
    from hero_amd import pretrain_eval as E
    rows, cols, ld = shape
    x, y = R.ce_case(rows, cols, ld)
    want, want_pred = R.ce_eval(x, y, cols, inv_temp, R.CE_IGNORE)
    logits, labels = torch.from_numpy(x).to(dtype), torch.from_numpy(y)
    assert torch.equal(logits.double(), torch.from_numpy(x).double())                # the grid is exact in every dtype
    acc, pred = E.ce_eval(logits, labels, ncols=cols, ignore_index=R.CE_IGNORE, inv_temp=inv_temp, want_pred=True)
    assert acc.dtype == torch.float64 and acc.shape == (3,) and pred.dtype == torch.int32
    assert torch.equal(pred.long(), torch.from_numpy(want_pred))
    assert acc[1].item() == want[1] and acc[2].item() == want[2]
    assert _rel(acc[0].item(), want[0]) <= 1e-12
    # a pre-filled triple is added to
    acc2 = E.ce_eval(logits, labels, ncols=cols, ignore_index=R.CE_IGNORE, inv_temp=inv_temp, acc=torch.tensor([1.5, 2.0, 3.0], dtype=torch.float64))
    assert acc2[1].item() == want[1] + 2 and acc2[2].item() == want[2] + 3 and _rel(acc2[0].item(), want[0] + 1.5) <= 1e-12


def test_ce_eval_fallback_edge_cases():
    from hero_amd import pretrain_eval as E
    pre = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    acc, pred = E.ce_eval(torch.zeros(0, 16), torch.zeros(0, dtype=torch.long), acc=pre.clone(), want_pred=True)
    assert torch.equal(acc, pre) and pred.numel() == 0                              # rows == 0: untouched
    x = torch.tensor([[0.0, -0.0, -1.0], [2.0, 2.0, 2.0], [-1.0, 3.0, 3.0]])
    acc, pred = E.ce_eval(x, torch.tensor([1, 0, 2]), want_pred=True)
    assert pred.tolist() == [0, 0, 1] and acc[1].item() == 1 and acc[2].item() == 3   # -0 ties with +0; the lowest column wins
    acc = E.ce_eval(x, torch.tensor([-100, 3, 1]))                                  # default ignore_index, label == cols
    assert acc[2].item() == 1 and acc[1].item() == 1
    with pytest.raises(ValueError):
        E.ce_eval(x, torch.tensor([0, 0, 0]), acc=torch.zeros(3))                   # the counters are float64


@pytest.mark.parametrize("rows", R.FEAT_ROWS)
@pytest.mark.parametrize("cols", R.FEAT_COLS)
def test_feat_eval_fallback_matches_the_statement(rows, cols):
    from hero_amd import pretrain_eval as E
    p, t = R.feat_case(rows, cols)
    want = R.feat_eval(p, t)
    for dtype in (torch.float32, torch.bfloat16):
        acc = E.feat_eval(torch.from_numpy(p).to(dtype), torch.from_numpy(t).to(dtype))
        assert acc[2].item() == rows
        assert _rel(acc[0].item(), want[0]) <= 1e-12 and abs(acc[1].item() - want[1]) <= 1e-12 * rows
    l2, cos = R.feat_eval_rows(p, t)
    assert cos[rows - 1] == 0.0 and (rows == 1 or l2[0] == 0.0)                     # the zero target row; pred == target
    pre = torch.tensor([0.5, 0.25, 7.0], dtype=torch.float64)
    acc = E.feat_eval(torch.from_numpy(p), torch.from_numpy(t), acc=pre.clone())
    assert acc[2].item() == rows + 7 and _rel(acc[0].item(), want[0] + 0.5) <= 1e-12
    assert torch.equal(E.feat_eval(torch.zeros(0, 8), torch.zeros(0, 8), acc=pre.clone()), pre)


def test_cosine_statement_is_the_installed_torchs():
    """F.cosine_similarity in float64, its eps rule included: tiny rows are where the rules of different releases part."""
    import torch.nn.functional as F
    g = np.random.default_rng(3)
    p, t = g.standard_normal((6, 9)), g.standard_normal((6, 9))
    p[0] *= 1e-9
    t[0] *= 1e-9
    p[1] = 0.0
    t[2] = 0.0
    p[3] *= 1e-9
    want = F.cosine_similarity(torch.from_numpy(p), torch.from_numpy(t), dim=-1).numpy()
    np.testing.assert_allclose(R.feat_eval_rows(p, t)[1], want, rtol=1e-13, atol=0)


def test_feat_eval_bound_is_4x_the_fp32_error():
    """The bound the GPU test holds hero_feat_eval to: the kernel's accumulation order restated in float32 against float64, over
    the shapes of that test; recorded with a factor of 4 (rounded up, never more than 5)."""
    worst_l2 = worst_cos = 0.0
    for rows in R.FEAT_ROWS:
        for cols in R.FEAT_COLS:
            p, t = R.feat_case(rows, cols)
            l2, cos = R.feat_eval_rows(p, t)
            for vector in (True, False):
                a, b = R.feat_eval_rows_f32(p, t, vector)
                assert a.dtype == np.float32 and b.dtype == np.float32
                worst_l2 = max(worst_l2, float(np.max(np.abs(a - l2) / np.where(l2 > 0, l2, 1.0))))
                worst_cos = max(worst_cos, float(np.max(np.abs(b - cos))))
                assert rows == 1 or a[0] == 0.0
    assert 4 * worst_l2 <= R.FEAT_L2_REL <= 5 * worst_l2, worst_l2
    assert 4 * worst_cos <= R.FEAT_COS_ABS <= 5 * worst_cos, worst_cos


# ---- validators --------------------------------------------------------------------------------------------------------------
class _StubEncoder:
    """What the validators ask of model.v_encoder, answered with the outputs the reference scored (in loader order).  The
    logits come back as the heads hand them over: wider than `ncols`, the padding above every real column."""

    def __init__(self, outs, order):
        self.outs, self.order, self.at = outs, list(order), {}

    def _next(self, task):
        i = self.at.get(task, 0)
        self.at[task] = i + 1
        return self.order[i]

    @staticmethod
    def _padded(a, pad):
        x = torch.from_numpy(a)
        return torch.cat([x, torch.full((x.shape[0], pad), 1e4)], 1).contiguous(), x.shape[1]

    def mlm_logits(self, batch):
        return self._padded(self.outs["mlm.%d.scores" % self._next("mlm")], 5)

    def fom_logits(self, batch):
        return torch.from_numpy(self.outs["fom.%d.scores" % self._next("fom")])

    def __call__(self, batch, task, compute_loss=True):
        assert compute_loss is False
        if task == "mffr":
            return torch.from_numpy(self.outs["mffr.%d.pred" % self._next("mffr")])
        assert task == "mfm-nce"
        self.cur = self._next("mfm-nce")
        return torch.from_numpy(self.outs["nce.%d.feats" % self.cur]), torch.from_numpy(self.outs["nce.%d.neg" % self.cur])

    def mfm_nce_logits(self, feats, pos, neg):
        assert pos.shape == feats.shape
        return self._padded(self.outs["nce.%d.logits" % self.cur], 3)


class _StubModel(torch.nn.Module):
    def __init__(self, outs, order):
        super().__init__()
        self.v_encoder = _StubEncoder(outs, order)
        self.outs = outs
        self.modes = []

    def forward(self, batch, task, compute_loss=True):
        assert task == "vsm" and compute_loss
        self.modes.append((self.training, torch.is_grad_enabled()))
        i = self.v_encoder._next("vsm")
        return tuple(torch.from_numpy(self.outs["vsm.%d.%s" % (i, k)]) for k in ("st_ed", "neg_ctx", "neg_q"))


def _validate_all(loaders, outs, order):
    from hero_amd import pretrain_eval as E
    model = _StubModel(outs, order)
    model.train()
    opts = types.SimpleNamespace(**R.VSM_OPTS)
    pick = lambda task: [loaders[task][i] for i in order]                           # noqa: E731
    logs = {"mlm": E.validate_mlm(model, pick("mlm")), "mffr": E.validate_mffr(model, pick("mffr")),
            "mfm-nce": E.validate_mfm_nce(model, pick("mfm-nce")), "fom": E.validate_fom(model, pick("fom")),
            "vsm": E.validate_vsm(model, pick("vsm"), opts)}
    assert model.training and model.modes and all(m == (False, False) for m in model.modes)   # eval + no_grad inside, train() after
    return logs


def _check_logs(logs, want):
    for task, ref in want.items():
        got = {k: v for k, v in logs[task].items() if not k.endswith("_per_s")}
        assert set(got) == set(ref), task
        assert len(logs[task]) == len(ref) + 1                                      # plus the one *_per_s key
        for k, v in ref.items():
            assert _rel(got[k], v) <= 1e-6, (task, k, got[k], v)                   # the reference sums fp32 .item()s
    assert logs["mlm"]["acc"] == want["mlm"]["acc"] and logs["fom"]["valid/acc"] == want["fom"]["valid/acc"]
    assert logs["mfm-nce"]["acc"] == want["mfm-nce"]["acc"]


def test_validators_reproduce_the_reference_dictionaries():
    loaders, outs = R.load_golden(CASE)
    want = R.golden_logs(outs)
    assert set(want) == set(R.TASKS) and 0 < want["mlm"]["acc"] < 1 and 0 < want["fom"]["valid/acc"] < 1
    _check_logs(_validate_all(loaders, outs, range(len(loaders["mlm"]))), want)


def test_numpy_bookkeeping_reproduces_the_reference_dictionaries():
    loaders, outs = R.load_golden(CASE)
    n = len(loaders["mlm"])
    logs = {
        "mlm": R.mlm_log([(outs["mlm.%d.scores" % i], outs["mlm.%d.scores" % i].shape[1], loaders["mlm"][i]["txt_labels"].numpy()) for i in range(n)]),
        "mffr": R.mffr_log([(outs["mffr.%d.pred" % i], loaders["mffr"][i]["feat_targets"].numpy(), int(loaders["mffr"][i]["c_v_masks"].sum()))
                            for i in range(n)]),
        "mfm-nce": R.mfm_nce_log([(outs["nce.%d.feats" % i], loaders["mfm-nce"][i]["feat_targets"].numpy(), outs["nce.%d.logits" % i],
                                   outs["nce.%d.logits" % i].shape[1]) for i in range(n)]),
        "fom": R.fom_log([(outs["fom.%d.scores" % i], loaders["fom"][i]["targets"].numpy()) for i in range(n)]),
        "vsm": R.vsm_log([(len(loaders["vsm"][i]["q_vidx"]), outs["vsm.%d.st_ed" % i], outs["vsm.%d.neg_ctx" % i], outs["vsm.%d.neg_q" % i])
                          for i in range(n)], **R.VSM_OPTS)}
    for task, ref in R.golden_logs(outs).items():
        for k, v in ref.items():
            assert _rel(logs[task][k], v) <= 1e-6, (task, k)


def test_validate_dispatches_by_prefix_and_prefixes_the_keys():
    from hero_amd import pretrain_eval as E
    loaders, outs = R.load_golden(CASE)
    model = _StubModel(outs, range(len(loaders["mlm"])))
    model.train()
    log = E.validate(model, {"mlm_tv": loaders["mlm"], "fom_how2": loaders["fom"]}, types.SimpleNamespace(**R.VSM_OPTS))
    assert set(log) == {"mlm_tv_loss", "mlm_tv_acc", "mlm_tv_tok_per_s", "fom_how2_valid/loss", "fom_how2_valid/acc", "fom_how2_valid/ex_per_s"}
    assert model.training
    want = R.golden_logs(outs)
    assert _rel(log["mlm_tv_loss"], want["mlm"]["loss"]) <= 1e-6 and log["fom_how2_valid/acc"] == want["fom"]["valid/acc"]
    with pytest.raises(ValueError, match="Undefined task"):
        E.validate(model, {"vr": []}, None)


def test_a_validator_reads_the_host_once(monkeypatch):
    """No .item() per batch: the counters are read by one tolist() per counter tensor after the loop."""
    from hero_amd import pretrain_eval as E
    loaders, outs = R.load_golden(CASE)
    model = _StubModel(outs, range(len(loaders["mlm"])))
    reads = []
    monkeypatch.setattr(torch.Tensor, "item", lambda self: reads.append("item") or 0.0)
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: reads.append("tolist") or real(self))
    E.validate_mlm(model, loaders["mlm"])
    assert reads == ["tolist"]
    del reads[:]
    E.validate_mfm_nce(model, loaders["mfm-nce"])
    assert reads == ["tolist", "tolist"]


def _two_ranks(rank, world):
    loaders, outs = R.load_golden(CASE)
    logs = _validate_all(loaders, outs, [rank])                                     # each rank holds one of the two batches
    return {t: {k: v for k, v in d.items() if not k.endswith("_per_s")} for t, d in logs.items()}


def test_two_gloo_ranks_give_the_one_rank_numbers():
    from tests.test_cpu_distributed import spawn
    loaders, outs = R.load_golden(CASE)
    assert len(loaders["mlm"]) == 2
    one = _validate_all(loaders, outs, [0, 1])
    for logs in spawn(_two_ranks):
        for task, d in logs.items():
            for k, v in d.items():
                assert _rel(v, one[task][k]) <= 1e-12, (task, k, v, one[task][k])
        assert logs["mlm"]["acc"] == one["mlm"]["acc"]
