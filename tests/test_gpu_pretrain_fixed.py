"""The pre-training heads on the fixed-capacity batches of PretrainMasker.static_batch: the tiny golden
model, fp32, dropout off, the ragged two-video batch of tests/test_gpu_pretrain_mask.py.  Per head the 0-dim loss and the
gradients of the parameters tests/test_gpu_configs.py lists for it (the cross-modal layer index is the tiny model's last,
1, where that file names HERO-base's 5) against oracle/hero_oracle.py on a batch assembled on the host from the statement's
masks, within the gates that file carries for the head against the oracle (MFFR shares MFM-NCE's: the same rows and
regression stack); and against the compact form (mlm_batch / mfm_batch / fom_batch, host-read counts) on the same masks,
within twice the gate - both lie within one gate of the oracle.  tests/test_cpu_pretrain_fixed.py holds that none of these
draws overflows the default capacities; the overflow policy has its own case."""
import json

import pytest
import torch

from oracle import hero_oracle as O
from tests import pretrain_fixed_cases as C
from tests.test_gpu_pretrain_mask import _device, _masker
from tests.util import load_tiny

pytestmark = pytest.mark.gpu

LOSS_GATE = 5e-3                  # relative, every head (tests/test_gpu_configs.py)
GRAD_GATE = {"mlm": 0.06, "mfm-nce": 0.055, "mffr": 0.055, "fom": 0.03}       # relative L2; frame_transform: 0.05
MFM_GRADS = ["v_encoder.feat_regress.net.0.weight", "v_encoder.feat_regress.net.3.weight", "v_encoder.mask_embedding.weight",
             "v_encoder.f_encoder.img_embeddings.mask_embedding.weight", "v_encoder.c_encoder.encoder.layer.0.intermediate.dense.weight",
             "v_encoder.f_encoder.encoder.layer.1.intermediate.dense.weight"]
GRADS = {
    "mlm": ["v_encoder.f_encoder.embeddings.word_embeddings.weight", "v_encoder.f_encoder.lm_head.dense.weight"],
    "mfm-nce": MFM_GRADS, "mffr": MFM_GRADS,
    "fom": ["v_encoder.fom_output.linear_1.weight", "v_encoder.fom_output.linear_2.weight", "v_encoder.fom_output.LayerNorm.weight",
            "v_encoder.frame_transform.net.1.weight", "v_encoder.c_encoder.embeddings.position_embeddings.weight",
            "v_encoder.f_encoder.encoder.layer.0.attention.self.query.weight"],
}
MASK_TASK = {"mlm": "mlm", "mfm-nce": "mfm", "mffr": "mfm", "fom": "fom"}


def l2_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def _setup():
    import hero_amd
    from hero_amd import functional as HF
    from hero_amd.model import HeroForPretraining
    from hero_amd.utils.misc import set_dropout
    hero_amd.set_compute_dtype(torch.float32)
    HF.set_grad_sink(None)
    HF.clear_weight_cache()
    model, P, cfg = load_tiny("cuda", cls=HeroForPretraining)
    model.train()
    set_dropout(model, 0.0)
    return model, P, cfg


def _oracle_mean(task, batch, Pq, cfg):
    if task == "mlm":
        return O.mlm_loss(batch, Pq, cfg).mean()
    if task == "fom":
        return O.fom_loss(batch, Pq, cfg)
    return O.mfm_loss(batch, Pq, cfg, loss="nce" if task == "mfm-nce" else "regression").mean()


def _grads(model, names):
    params = dict(model.named_parameters())
    out = {n: params[n].grad.detach().clone() for n in names}
    model.zero_grad(set_to_none=True)
    return out


@pytest.mark.parametrize("task", ["mlm", "mfm-nce", "mffr", "fom"])
def test_fixed_capacity_head_against_the_oracle_and_the_compact_form(task):
    from hero_amd import functional as HF
    model, P, cfg = _setup()
    host = C.ragged_host()
    dev, ln = _device(host)
    seed, p, names = C.MODEL_SEED, C.MODEL_P, GRADS[task]
    which = MASK_TASK[task]
    m = _masker(host, p, seed).draw_fixed(dev, ln, which)
    fixed = m.static_batch(which)
    assert fixed is m.static_batch(which) and fixed["_static_buffers"] is True and fixed["_masker"] is m
    got = model(fixed, task=task, compute_loss=True)
    assert got.dim() == 0 and bool(torch.isfinite(got))
    got.backward()
    g_fixed = _grads(model, names)
    compact = {"mlm": m.mlm_batch, "mfm": m.mfm_batch, "fom": lambda: m.fom_batch(pairs=False)}[which]()
    loss_c = model(compact, task=task, compute_loss=True).mean()
    loss_c.backward()
    g_compact = _grads(model, names)
    Pq = {k: v.clone().requires_grad_(k in names) for k, v in P.items()}
    if task == "mlm":
        Pq["v_encoder.f_encoder.lm_head.decoder.weight"] = Pq["v_encoder.f_encoder.embeddings.word_embeddings.weight"]      # tied
    ref = _oracle_mean(task, C.host_task_batches(host, seed, p)[which], Pq, cfg)
    ref.backward()
    assert m.overflow.tolist() == [0, 0]
    rel = lambda a, b: abs(float(a) - float(b)) / abs(float(b))     # noqa: E731
    got, loss_c, ref = got.detach(), loss_c.detach(), ref.detach()
    report = {"loss.fixed": float(got), "loss.compact": float(loss_c), "loss.oracle": float(ref),
              "loss.fixed_vs_oracle": rel(got, ref), "loss.compact_vs_oracle": rel(loss_c, ref), "loss.fixed_vs_compact": rel(got, loss_c)}
    for n in names:
        report["grad.fixed_vs_oracle." + n] = l2_err(g_fixed[n], Pq[n].grad)
        report["grad.compact_vs_oracle." + n] = l2_err(g_compact[n], Pq[n].grad)
        report["grad.fixed_vs_compact." + n] = l2_err(g_fixed[n], g_compact[n])
    print(task, json.dumps(report, indent=1))
    HF.reset_caches()
    assert report["loss.fixed_vs_oracle"] < LOSS_GATE and report["loss.compact_vs_oracle"] < LOSS_GATE, report
    assert report["loss.fixed_vs_compact"] < 2 * LOSS_GATE, report
    for n in names:
        gate = 0.05 if "frame_transform" in n else GRAD_GATE[task]
        assert report["grad.fixed_vs_oracle." + n] < gate and report["grad.compact_vs_oracle." + n] < gate, (n, report)
        assert report["grad.fixed_vs_compact." + n] < 2 * gate, (n, report)


def test_mlm_overflow_keeps_the_first_rows_and_counts_the_draw():
    """mlm_rows = 8 with p = 1: every token is masked in the input, the first 8 (nonzero order) carry the loss, the mean divides
    by 8, and the draw is counted.  Bound: 1e-3 relative, what this fp32 model holds against the fp32 oracle in smoke()."""
    from hero_amd import functional as HF
    from hero_amd.pretrain_data import PretrainMasker
    from tests.test_gpu_pretrain_mask import CLS, MASK_ID, SITES, V_RANGE
    model, P, cfg = _setup()
    host = C.ragged_host()
    dev, ln = _device(host)
    seed = C.MODEL_SEED
    m = PretrainMasker.for_batch(host, "cuda", MASK_ID, V_RANGE, CLS, mlm_prob=1.0, sites=SITES, mlm_rows=8).set_seed(seed)
    m.draw_fixed(dev, ln, "mlm")
    batch = m.static_batch("mlm")
    assert batch["txt_mask_rows"].shape == batch["txt_labels"].shape == (8,)
    got = model(batch, task="mlm", compute_loss=True)
    assert int(m.counts[0]) > 8 and m.overflow.tolist() == [1, 0]
    assert torch.equal(batch["input_ids"].cpu(), torch.from_numpy(C.mlm_statement(host, seed, 1.0)["input_ids"]))       # all still masked in the input
    with torch.no_grad():
        ref = O.mlm_loss(C.host_task_batches(host, seed, 1.0)["mlm"], P, cfg)
    assert ref.numel() == int(m.counts[0])
    want = float(ref[:8].mean())
    print("overflow: loss", float(got), "oracle mean of the first 8", want, "count", int(m.counts[0]))
    assert abs(float(got) - want) < 1e-3 * abs(want)
    m.redraw("mlm")
    assert m.overflow.tolist() == [2, 0]
    HF.reset_caches()
