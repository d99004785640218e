"""Video retrieval on the CPU: HeroForVr's interface, the PyTorch formulation of its losses and scores (oracle/hero_oracle.py)
against the reference's numbers (tests/golden/case_vr.npz), the in-training validators on a stub model that replays the
reference's per-batch outputs, and the several-annotator recall rule (tests/didemo_reference.py) against the reference's
eval_retrieval dictionaries."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hero_amd.model import HeroForVcmr, HeroForVr
from hero_amd.retrieval import RecallMeter
from hero_amd.retrieval_eval import validate_vcmr, validate_vr
from oracle import hero_oracle as O
from tests import didemo_reference as DR
from tests.util import GOLDEN

Z = DR.load_vr()


def tiny_vr(**kw):
    P, cfgj, vfeat, max_frm = O.load_npz_model(os.path.join(GOLDEN, "tiny_model.npz"))
    args = dict(margin=0.1, lw_neg_ctx=10.0, lw_neg_q=10.0, use_all_neg=True)
    args.update(kw)
    return HeroForVr.from_pretrained(os.path.join(GOLDEN, "tiny_config.json"), {k: v.clone() for k, v in P.items()}, vfeat_dim=vfeat,
                                     max_frm_seq_len=max_frm, **args)


def test_state_dict_keys_and_defaults_are_the_references():
    model = tiny_vr()
    assert sorted(model.state_dict().keys()) == Z["state_keys"]
    assert isinstance(model, HeroForVcmr) and model.lw_st_ed == 0 and model.drop_svmr_prob == 1.0
    assert (model.lw_neg_ctx, model.lw_neg_q, model.margin, model.use_all_neg, model.use_hard_negative) == (10.0, 10.0, 0.1, True, False)
    import inspect
    d = {k: p.default for k, p in inspect.signature(HeroForVr.__init__).parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(ranking_loss_type="hinge", margin=0.1, lw_neg_ctx=1, lw_neg_q=1, use_hard_negative=False, hard_pool_size=20,
                     hard_neg_weight=10, use_all_neg=True)                        # model/vr.py:13-17


def test_constructor_and_forward_refuse_what_the_reference_refuses():
    with pytest.raises(AssertionError, match="lw_neg_ctx or lw_neg_q"):
        tiny_vr(lw_neg_ctx=0, lw_neg_q=0)
    tiny_vr(lw_neg_ctx=0, lw_neg_q=1.0)
    model = tiny_vr()
    for task in ("tvr", "didemo_video_only", "vsm"):
        with pytest.raises(ValueError, match="Unrecognized task"):
            model({}, task=task)


@pytest.mark.parametrize("name", ["vr_vonly", "vr_sub"])
def test_pytorch_formulation_gives_the_reference_losses_and_scores(name):
    P, cfgj, _, _ = O.load_npz_model(os.path.join(GOLDEN, "tiny_model.npz"))
    cfg = O.cfg_from_json(cfgj)
    b = DR.batch_of(Z, name)
    _, l_ctx, l_q = O.vsm_losses(b, P, cfg, lw_st_ed=0.0, lw_neg_ctx=10.0, lw_neg_q=10.0, margin=0.1)
    pre = "vr.%s." % name
    np.testing.assert_allclose(l_ctx.numpy(), Z[pre + "train_neg_ctx"], rtol=1e-4, atol=1e-6)      # tests/test_cpu_collate.py's bound
    np.testing.assert_allclose(l_q.numpy(), Z[pre + "train_neg_q"], rtol=1e-4, atol=1e-6)
    frames = O.forward_repr(b, P, cfg)
    q_seq = O.f_encoder_txt(b["query_input_ids"], b["query_pos_ids"], b["query_attn_masks"], P, cfg)
    scores = O.video_level_scores(O.query_feat_encoder(q_seq, b["query_attn_masks"], P, cfg), frames, b["c_attn_masks"])
    np.testing.assert_allclose(scores.numpy(), Z[pre + "scores"], rtol=1e-4, atol=1e-6)


class Replay:
    """A model that hands a validator the reference's per-batch outputs."""

    def __init__(self, outs):
        self.outs, self.training, self.seen = list(outs), True, []

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode

    def __call__(self, batch, task, compute_loss=True):
        assert compute_loss and not self.training and "qids" not in batch and not torch.is_grad_enabled()
        self.seen.append(task)
        return self.outs.pop(0)


def loaders():
    ev = DR.batch_of(Z, "vr_vonly_eval")
    two = [dict(q_vidx=ev["q_vidx"][:3], qids=ev["qids"][:3]), dict(q_vidx=ev["q_vidx"][3:], qids=ev["qids"][3:])]
    vr = [tuple(torch.from_numpy(Z["val.vr.%d.%s" % (i, k)]) for k in ("neg_ctx", "neg_q")) for i in range(2)]
    vcmr = [tuple(torch.from_numpy(Z["val.vcmr.%d.%s" % (i, k)]) for k in ("st_ed", "neg_ctx", "neg_q")) for i in range(2)]
    return two, vr, vcmr


@pytest.mark.parametrize("which", ["vr", "vcmr"])
def test_validators_reproduce_the_reference_dictionaries(which, monkeypatch):
    two, vr, vcmr = loaders()
    opts = SimpleNamespace(**Z["val.%s.opts" % which])
    model = Replay(vr if which == "vr" else vcmr)
    reads = []
    monkeypatch.setattr(torch.Tensor, "item", lambda self: reads.append("item") or 0.0)
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: reads.append("tolist") or real(self))
    log = (validate_vr if which == "vr" else validate_vcmr)(model, two, opts)
    monkeypatch.undo()
    assert reads == ["tolist"]                                                    # one host read, after the loader is exhausted
    assert model.training and model.seen == [opts.task] * 2 and all("qids" in b for b in two)
    want = Z["val.%s.log" % which]
    assert set(log) == set(want) | {"valid/ex_per_s"} and log["valid/ex_per_s"] > 0
    for k, v in want.items():
        assert abs(log[k] - v) <= 1e-6 * max(1.0, abs(v)), (k, log[k], v)
    assert ("valid/loss_st_ed" in log) == (which == "vcmr")


@pytest.mark.parametrize("name", DR.DIDEMO_CASES)
def test_restatement_gives_the_reference_metrics(name):
    case = DR.didemo_cases(Z)[name]
    got = DR.meter_from_rows(RecallMeter(vfeat_interval=case["interval"]), case).compute()
    assert got["VCMR"] == case["metrics"]["VCMR"] and got["SVMR"] == case["metrics"]["SVMR"]
    assert any(0 < v < 100 for v in got["VCMR"].values())


def test_the_cases_tell_the_rules_apart():
    need1 = first_only = False
    for case in DR.didemo_cases(Z).values():
        right = DR.meter_from_rows(RecallMeter(vfeat_interval=case["interval"]), case).compute()
        need1 |= DR.meter_from_rows(RecallMeter(vfeat_interval=case["interval"]), case, need=1).compute() != right
        first_only |= DR.meter_from_rows(RecallMeter(vfeat_interval=case["interval"]), case, only_first=True).compute() != right
    assert need1 and first_only
