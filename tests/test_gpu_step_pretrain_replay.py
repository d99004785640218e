"""Pre-training under hipGraph replay with a FRESH mask draw every micro-step: TrainStep(use_graph=True)
on PretrainMasker.static_batch(task) against an eager TrainStep on the same batches - same initial weights, same seed word,
accumulation 2.  Twelve micro-steps of MLM, then eight of MFM-NCE, then eight of FOM (in graph mode the first four of each task
are its eager warm-up, the rest are replays of ONE capture per task).  Both runs draw once per micro-step in front of it, so
they see the same masks; nothing the step derives from a mask has a mask-dependent shape, so the replayed launches are the
eager ones: losses, parameters and per-parameter Adam steps must be torch.equal.  New frame features are copied into the
clean buffers twice on the way.  The replayed steps run under torch.cuda.set_sync_debug_mode("error"): no host read.

Tiny golden model, fp32, dropout 0, the ragged two-video batch of tests/test_gpu_pretrain_mask.py;
tests/test_cpu_pretrain_fixed.py holds that none of these draws overflows the default capacities."""
import pytest
import torch

from tests import pretrain_fixed_cases as C
from tests.test_gpu_pretrain_mask import _device, _masker
from tests.util import load_tiny

pytestmark = pytest.mark.gpu

OPTS = dict(learning_rate=1e-3, warmup_steps=2, num_train_steps=100, gradient_accumulation_steps=2)
SCHEDULE = ["mlm"] * 12 + ["mfm-nce"] * 8 + ["fom"] * 8
MASK_TASK = {"mlm": "mlm", "mfm-nce": "mfm", "fom": "fom"}
NEW_FEATS_AT = (8, 18)            # micro-step counts (window starts, behind a task's capture) at which new features arrive


def _new_feats(dev, at):
    """New clean frame features, written into the buffers the batches and the captured graphs hold."""
    g = torch.Generator().manual_seed(100 + at)
    for k in ("c_v_feats", "f_v_feats"):
        dev[k].copy_(torch.randn(dev[k].shape, generator=g).to(dev[k].device))


def run(use_graph):
    import hero_amd
    from hero_amd import functional as HF
    from hero_amd.model import HeroForPretraining
    from hero_amd.step import TrainStep
    from hero_amd.utils.misc import set_dropout
    hero_amd.set_compute_dtype(torch.float32)
    HF.set_grad_sink(None)
    HF.reset_caches()
    model, _, _ = load_tiny("cuda", cls=HeroForPretraining)
    model.train()
    set_dropout(model, 0.0)
    host = C.ragged_host()
    dev, ln = _device(host)
    m = _masker(host, C.STEP_P, C.STEP_SEED)
    for which in ("mlm", "mfm", "fom"):                   # binds the clean batch; every micro-step draws again
        m.draw_fixed(dev, ln, which)
    batches = {t: m.static_batch(MASK_TASK[t]) for t in MASK_TASK}
    watch = {"mlm": m.input_ids, "mfm-nce": m.c_v_masks, "fom": m.shuffled_orders}
    ts = TrainStep(model, opts=OPTS, task="mlm", use_graph=use_graph)
    losses, masks, replayed_calls = [], [], 0
    prev = torch.cuda.get_sync_debug_mode()
    try:
        while ts.micro < len(SCHEDULE):
            task = SCHEDULE[ts.micro]
            if ts.micro in NEW_FEATS_AT:
                _new_feats(dev, ts.micro)
            before = ts.micro
            replay = use_graph and task in ts._graphs
            if replay:
                torch.cuda.set_sync_debug_mode("error")
                replayed_calls += 1
            try:
                loss = ts.micro_step(batches[task], task=task).clone()
                mask = watch[task].clone()
            finally:
                torch.cuda.set_sync_debug_mode(prev)
            if ts.micro - before > 1:                      # the first graph-mode call of a task: its warm-up micro-steps ran inside
                losses += [x.clone() for x in ts.warmup_losses]
                masks += [None] * len(ts.warmup_losses)
            losses.append(loss)
            masks.append((task, mask, replay))
        torch.cuda.synchronize()
        ts.state_dict()                                    # brings the per-parameter steps to the host
        steps = {n: ts.optimizer.state[p].get("step", 0) if p in ts.optimizer.state else 0 for n, p in model.named_parameters()}
        out = dict(losses=torch.stack(losses).cpu(), params={k: v.detach().clone().cpu() for k, v in model.named_parameters()}, steps=steps,
                   counts=dict(ts.counts), masks=masks, replayed_calls=replayed_calls, overflow=m.overflow.tolist(),
                   seed=int(m.seed.item()) & ((1 << 64) - 1))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
        HF.set_grad_sink(None)
        HF.reset_caches()
    return out


def test_replay_with_a_fresh_draw_per_micro_step_equals_the_eager_run():
    from tests import pretrain_mask_reference as R
    g = run(True)
    e = run(False)
    assert len(g["losses"]) == len(e["losses"]) == len(SCHEDULE) and bool(torch.isfinite(e["losses"]).all())
    # one capture per task; of each task's micro-steps all but the four warm-up ones were replays, none fell back to eager launches
    # (a task's first call runs the warm-up AND its first replay; the 13 later calls are the ones run under the sync check)
    assert g["counts"]["captures"] == 3 and g["counts"]["replayed"] == len(SCHEDULE) - 3 * 4 == 16 and g["replayed_calls"] == 13
    assert g["counts"]["eager_in_graph_mode"] == 0 and e["counts"]["captures"] == 0 and e["counts"]["replayed"] == 0
    # the replayed masks move: consecutive replayed steps of a task read different draws
    pairs = 0
    for a, b in zip(g["masks"], g["masks"][1:]):
        if a is not None and b is not None and a[0] == b[0] and a[2] and b[2]:
            assert not torch.equal(a[1], b[1]), a[0]
            pairs += 1
    assert pairs == 6 + 2 + 2
    # one draw per micro-step in both runs, none by the captures: the seed word is the statement's after 28 steps
    seed = C.STEP_SEED
    for _ in SCHEDULE:
        seed = R.advance(seed)
    assert g["seed"] == e["seed"] == seed
    assert g["overflow"] == e["overflow"] == [0, 0]
    # the same run, bit for bit
    assert torch.equal(g["losses"], e["losses"]), (g["losses"] - e["losses"]).abs().max()
    diff = [k for k in e["params"] if not torch.equal(g["params"][k], e["params"][k])]
    assert not diff, diff
    assert g["steps"] == e["steps"], {k: (g["steps"][k], e["steps"][k]) for k in e["steps"] if g["steps"][k] != e["steps"][k]}
    # the losses moved with the masks and the new features (a replay stuck on its capture's masks repeats itself)
    assert len({float(x) for x in g["losses"][4:12]}) == 8
