"""Beam-search captioning on the GPU with the tiny configuration: TvcGenerator.beam_decode on the kernels' route
(hero_beam_select, the grouped and beam entry points of the one-row attention kernel), eager and under graph replay, against
the float64 search of tests/tvc_beam_reference.py driven through the SAME module's PyTorch step (fused_decoder = False), against
the fixture's greedy ids, and the routing: no copy of the cache, no replication of the encoder keys.

Ids are compared on the captions whose gap (tests/tvc_beam_reference.py) is >= 1e-4 at every step and whose two best final
scores are >= 1e-4 apart; the tests assert how many that leaves out.  fp32 throughout except the bf16 smoke test, which claims
no id equality (random bf16 near-ties already separate the greedy paths).  Scores: rel_err < 2e-4.

Measured on the CPU with the fixture's encoder outputs (tests/test_cpu_tvc_beam.py asserts the first line):
    eos = 30   all six captions counted, smallest gap 7.7e-4; 17 of 18 beams finish; most captions end on a beam other than 0
    eos = 81   the fixture's own: caption 2 has a gap of 3.9e-5 and is left out; the two best final scores of caption 1 are
               5.7e-5 apart, so its pick is not counted either"""
import json
import os

import numpy as np
import pytest
import torch

from tests import tvc_beam_reference as R
from tests.util import GOLDEN, config_file, rel_err, to_dev

pytestmark = pytest.mark.gpu
GAP, FP32_TOL = 1e-4, 2e-4
Z = np.load(os.path.join(GOLDEN, "case_tvc.npz"))
DESC = json.loads(str(Z["desc"]))
GREEDY = json.loads(str(Z["greedy"]))
STEPS = 8


@pytest.fixture(autouse=True)
def _fp32_default():
    import hero_amd
    hero_amd.set_compute_dtype(torch.float32)
    yield
    hero_amd.set_compute_dtype(torch.bfloat16)


def load_model(fused=True):
    from hero_amd.model import HeroForTvc
    from hero_amd.utils.misc import set_dropout
    cfg = json.load(open(os.path.join(GOLDEN, "tiny_config.json")))
    cfg["d_config"] = DESC["d_config"]
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    sd.update({k[len("param."):]: torch.from_numpy(Z[k].astype(np.float32)) for k in Z.files if k.startswith("param.")})
    model = HeroForTvc.from_pretrained(config_file(cfg, "tiny_tvc.json"), sd, vfeat_dim=int(z["__vfeat__"]),
                                       max_frm_seq_len=int(z["__max_frm__"])).cuda()
    model.fused_decoder = fused
    model.eval()
    set_dropout(model, 0.0)
    return model


def load_batch():
    from hero_amd.collate import tvc_frame_index
    out = {}
    for k in Z.files:
        if k.startswith("out."):
            a = Z[k]
            out[k[len("out."):]] = json.loads(str(a)) if a.dtype.kind == "U" else torch.from_numpy(a)
    out["clip_ranges"] = tuple(tuple(tuple(r) for r in rs) for rs in out["clip_ranges"])
    out["cap_frame_index"] = tvc_frame_index(out["clip_ranges"], out["c_v_feats"].shape[1])
    return to_dev(out, "cuda")


def shifted_batch(b):
    """The same captions over other frames (tests/test_gpu_tvc_decode.py): every segment that can moves one frame to the right."""
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
    return out


def generator(model, eos=None, **kw):
    from hero_amd.model import TvcGenerator
    return TvcGenerator(model, STEPS, DESC["bos"], int(Z["greedy_eos"]) if eos is None else eos, **kw)


def reference_search(model, enc, mask, B, eos):
    """The float64 search over the module's PyTorch step on the GPU (the step's scores are the search's input values)."""
    was, model.fused_decoder = model.fused_decoder, False
    try:
        state = model.init_decode_state(enc, mask, STEPS, B)
        assert not state.fused

        def step_fn(t, last, parents):
            if parents is not None:
                model.reorder_decode_state(state, parents.cuda())
            return model.decode_step(state, last.cuda())
        return R.search(step_fn, enc.shape[0], B, STEPS, DESC["bos"], eos)
    finally:
        model.fused_decoder = was


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_beam_of_one_is_the_greedy_decode(use_graph):
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    gen = generator(load_model(True), kv_cache=True, use_graph=use_graph)
    assert gen.beam_decode(load_batch(), 1) == GREEDY
    assert gen.counts["captures"] == int(use_graph) and gen.counts["replayed"] == STEPS * int(use_graph)


@pytest.mark.parametrize("eos,max_gap_out,max_pick_out", [(30, 0, 0), (81, 1, 1)], ids=["eos30", "eos81"])
def test_beam_of_three_equals_the_float64_search(eos, max_gap_out, max_pick_out):
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    model, b = load_model(True), load_batch()
    with torch.no_grad():
        enc = model.encode(b)
    N = enc.shape[0]
    want = reference_search(model, enc, b["cap_attn_mask"], 3, eos)
    by_gap, by_pick = want["gaps"].min(dim=1).values < GAP, want["pick_margin"] < GAP
    out = by_gap | by_pick
    print("\n[tvc-beam] eos=%d: min gap per caption %s, pick margins %s, finished %d / %d, best beams %s; left out %s"
          % (eos, ["%.2e" % g for g in want["gaps"].min(dim=1).values.tolist()], ["%.2e" % g for g in want["pick_margin"].tolist()],
             want["finished"], 3 * N, want["best"].tolist(), out.nonzero().view(-1).tolist()), end="")
    assert N == 6 and int(by_gap.sum()) <= max_gap_out and int(by_pick.sum()) <= max_pick_out
    if eos == 30:
        assert want["finished"] >= 15 and int((want["best"] != 0).sum()) > N // 2       # the finished-beam rules are exercised
    state = model.init_decode_state(enc, b["cap_attn_mask"], STEPS, 3)
    assert state.fused and state.rows == 3 * N
    ids, scores = generator(model, eos, kv_cache=True).beam_decode(b, 3, encoder_outputs=enc, return_scores=True)
    keep = (~out).nonzero().view(-1).tolist()
    assert [ids[n] for n in keep] == [want["ids"][n] for n in keep]
    e = rel_err(torch.tensor(scores, dtype=torch.float64)[keep], want["scores"][keep])
    print("  score rel_err %.3e" % e, end="")
    assert e < FP32_TOL
    # the module's own PyTorch route agrees, too
    model.fused_decoder = False
    torch_ids = generator(model, eos, kv_cache=True).beam_decode(b, 3, encoder_outputs=enc)
    assert [torch_ids[n] for n in keep] == [want["ids"][n] for n in keep]


def test_beam_decode_copies_no_cache_and_projects_the_encoder_rows_once(monkeypatch):
    """S steps at B = 3: 2 layers x S step launches and row launches over N * B rows, S selections, no launch of the full kernel,
    exactly 2 K|V projections of the N * Lv encoder rows (none of N * B * Lv), no index_select, and the caches stay where they are."""
    from hero_amd import functional as HF
    from hero_amd import tvc as T
    HF.clear_weight_cache()
    calls = {"step": 0, "row": 0, "fwd": 0, "select": 0, "enc_kv": 0, "wide_kv": 0, "gather": 0}
    model, b = load_model(True), load_batch()
    N, Lv = b["cap_attn_mask"].shape
    D, B = model.config.d_config.hidden_size, 3

    def counted(name, real):
        def fn(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return fn
    real_linear = HF.k_linear

    def linear(x2, Wc, *a, **k):
        kv_weights = {HF.packed((la.dec_enc_attention.key.weight, la.dec_enc_attention.value.weight), x2.dtype).data_ptr()
                      for la in model.decoder.layer}
        if tuple(Wc.shape) == (2 * D, D) and Wc.data_ptr() in kv_weights:
            calls["enc_kv" if x2.shape[0] == N * Lv else "wide_kv"] += 1
        return real_linear(x2, Wc, *a, **k)
    states = []
    real_init = model.init_decode_state

    def init(*a, **k):
        states.append(real_init(*a, **k))
        states[-1].where = [c.data_ptr() for c in states[-1].cache] + [c.data_ptr() for c in states[-1].cross_kv]
        return states[-1]
    with torch.no_grad():
        enc = model.encode(b)
    monkeypatch.setattr(T, "k_dec_attn_step", counted("step", T.k_dec_attn_step))
    monkeypatch.setattr(T, "k_dec_attn_row", counted("row", T.k_dec_attn_row))
    monkeypatch.setattr(T, "k_dec_attn_fwd", counted("fwd", T.k_dec_attn_fwd))
    monkeypatch.setattr(T, "k_beam_select", counted("select", T.k_beam_select))
    monkeypatch.setattr(HF, "k_linear", linear)
    monkeypatch.setattr(torch.Tensor, "index_select", counted("gather", torch.Tensor.index_select))
    monkeypatch.setattr(model, "init_decode_state", init)
    ids = generator(model, 30, kv_cache=True).beam_decode(b, B, encoder_outputs=enc)
    assert len(ids) == N
    assert calls == {"step": 2 * STEPS, "row": 2 * STEPS, "fwd": 0, "select": STEPS, "enc_kv": 2, "wide_kv": 0, "gather": 0}
    state, = states
    assert state.fused and [tuple(c.shape) for c in state.cache] == [(N * B, STEPS, 2 * D)] * 2
    assert [tuple(c.shape) for c in state.cross_kv] == [(N * Lv, 2 * D)] * 2 and tuple(state.mask_add.shape) == (N, Lv)
    assert [c.data_ptr() for c in state.cache] + [c.data_ptr() for c in state.cross_kv] == state.where
    # outside the selection kernel's envelope the PyTorch route is taken, and it gives the same ids
    model.max_beam = B - 1
    for k in calls:
        calls[k] = 0
    assert generator(model, 30, kv_cache=True).beam_decode(b, B, encoder_outputs=enc) == ids
    assert not states[-1].fused and calls["select"] == 0 and calls["step"] == 0 and calls["gather"] > 0
    with pytest.raises(ValueError, match="kernels' route"):
        generator(model, 30, kv_cache=True, use_graph=True).beam_decode(b, B, encoder_outputs=enc)


def test_graph_replay_serves_changing_batches_of_one_shape():
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    model = load_model(True)
    first = load_batch()
    second = shifted_batch(first)
    eager = generator(model, 30, kv_cache=True)
    want = [eager.beam_decode(first, 3, return_scores=True), eager.beam_decode(second, 3, return_scores=True)]
    print("\n[tvc-beam] graph: batches decode to %s and %s" % (want[0][0], want[1][0]), end="")
    gen = generator(model, 30, kv_cache=True, use_graph=True)
    for n, i in enumerate((0, 1, 0, 1, 1)):
        assert gen.beam_decode(second if i else first, 3, return_scores=True) == want[i], i
        assert gen.counts["replayed"] == (n + 1) * STEPS
    assert gen.counts["captures"] == 1 and len(gen._graphs) == 1
    assert gen.greedy_decode(first) == eager.greedy_decode(first)                        # greedy and beam graphs share the table
    assert gen.counts["captures"] == 2 and len(gen._graphs) == 2 and gen.counts["replayed"] == 6 * STEPS


def test_bf16_beam_decode_runs_and_returns_well_formed_lists():
    import hero_amd
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    hero_amd.set_compute_dtype(torch.bfloat16)
    model, b = load_model(True), load_batch()
    V = model.config.f_config.vocab_size
    for use_graph in (False, True):
        ids, scores = generator(model, 30, kv_cache=True, use_graph=use_graph).beam_decode(b, 3, return_scores=True)
        assert len(ids) == len(scores) == b["cap_attn_mask"].shape[0]
        assert all(len(r) <= STEPS and all(0 <= i < V and i != 30 for i in r) for r in ids)
        assert all(np.isfinite(s) and s <= 0.0 for s in scores)
