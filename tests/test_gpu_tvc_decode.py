"""Incremental captioning decode on the GPU with the tiny configuration: HeroForTvc.init_decode_state / decode_step and
TvcGenerator(kv_cache=True[, use_graph=True]) against tests/golden/case_tvc.npz (the reference's scores and greedy decode), against
the uncached decoder of the same model, and the routing onto the one-row kernels.

Tolerances (none is taken from the code under test)
  * fp32 step scores against the uncached scores and against the fixture: FP32_TOL = 2e-4 of tests/test_gpu_tvc.py (rel_err).
  * bf16 step scores: the rel_err of the UNCACHED bf16 scores against the fp32 scores is measured in the same run - that path
    exists without the cache and is not changed by it - and the cached bf16 scores must stay within 2 x that figure of the same
    fp32 scores: the factor covers another GEMM tile route at M = N rows and another summation order in the attention.
    Measured on an AMD Instinct MI355X: uncached 6.222e-03, cached 6.222e-03, bound 1.244e-02 (fp32, for comparison: the step
    scores are within 5.7e-07 of the uncached ones and 7.6e-07 of the fixture's).
  * ids: exact."""
import json
import os

import numpy as np
import pytest
import torch

from tests.util import GOLDEN, config_file, rel_err, to_dev

pytestmark = pytest.mark.gpu
FP32_TOL = 2e-4
Z = np.load(os.path.join(GOLDEN, "case_tvc.npz"))
DESC = json.loads(str(Z["desc"]))
GREEDY = json.loads(str(Z["greedy"]))
STEPS = 8                                        # the max_step of the fixture's greedy decode


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
    model.train()                                # with every dropout at 0, as tests/test_gpu_tvc.py compares scores; the generators get .eval()
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
    """The same captions over other frames: every segment that can moves one frame to the right (lengths, masks and shapes
    stay), so the encoder rows a caption attends to - and with them the decode - change."""
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


def generator(model, **kw):
    from hero_amd.model import TvcGenerator
    return TvcGenerator(model, STEPS, DESC["bos"], int(Z["greedy_eos"]), **kw)


def step_scores(model, b, enc):
    """Teacher forcing: the fixture's input ids position by position -> [N, Lt, vocab]."""
    ids = b["cap_input_ids"]
    state = model.init_decode_state(enc, b["cap_attn_mask"], ids.shape[1])
    return state, torch.stack([model.decode_step(state, ids[:, t]) for t in range(ids.shape[1])], dim=1)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_cached_greedy_decode_returns_the_reference_ids(use_graph):
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    gen = generator(load_model(True).eval(), kv_cache=True, use_graph=use_graph)
    assert gen.greedy_decode(load_batch()) == GREEDY
    assert float(Z["greedy_margin"]) >= 1e-3                                     # no arg-max of the fixture is a near tie
    assert gen.counts["captures"] == int(use_graph) and gen.counts["replayed"] == STEPS * int(use_graph)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
def test_teacher_forced_step_scores_match_the_uncached_scores_and_the_fixture(fused):
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    model, b = load_model(fused), load_batch()
    with torch.no_grad():
        enc = model.encode(b)
        full = model(b, "train", compute_loss=False)
    state, got = step_scores(model, b, enc)
    assert state.fused == fused and got.shape == full.shape
    want = torch.from_numpy(Z["scores"])
    for t in range(got.shape[1]):
        e_full, e_ref = rel_err(got[:, t], full[:, t]), rel_err(got[:, t], want[:, t])
        print("\n[tvc-decode] %s step %d: vs uncached %.3e  vs fixture %.3e" % ("fused" if fused else "torch", t, e_full, e_ref), end="")
        assert e_full < FP32_TOL and e_ref < FP32_TOL, (t, e_full, e_ref)
    if fused:
        assert int(state.pos) == got.shape[1] and state.pid.tolist() == [got.shape[1]] * state.N


def test_cached_decode_runs_the_one_row_kernels_and_projects_the_encoder_rows_once(monkeypatch):
    """S steps: 2 layers x S step launches, 2 x S row launches, no launch of the full kernel, and exactly 2 K|V projections of the
    encoder rows.  With the Python-side limit below max_step no new kernel runs, the PyTorch step is taken and the ids stay."""
    from hero_amd import functional as HF
    from hero_amd import tvc as T
    HF.clear_weight_cache()
    calls = {"step": 0, "row": 0, "fwd": 0, "enc_kv": 0}
    model, b = load_model(True), load_batch()
    N, Lv = b["cap_attn_mask"].shape
    D = model.config.d_config.hidden_size
    assert N * Lv != N

    def counted(name, real):
        def fn(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return fn
    real_linear = HF.k_linear

    def linear(x2, Wc, *a, **k):
        # a GEMM of the encoder rows with the packed key | value weights of a decoder-encoder attention
        kv_weights = {HF.packed((la.dec_enc_attention.key.weight, la.dec_enc_attention.value.weight), x2.dtype).data_ptr()
                      for la in model.decoder.layer}
        if x2.shape[0] == N * Lv and tuple(Wc.shape) == (2 * D, D) and Wc.data_ptr() in kv_weights:
            calls["enc_kv"] += 1
        return real_linear(x2, Wc, *a, **k)
    monkeypatch.setattr(T, "k_dec_attn_step", counted("step", T.k_dec_attn_step))
    monkeypatch.setattr(T, "k_dec_attn_row", counted("row", T.k_dec_attn_row))
    monkeypatch.setattr(T, "k_dec_attn_fwd", counted("fwd", T.k_dec_attn_fwd))
    monkeypatch.setattr(HF, "k_linear", linear)
    with torch.no_grad():
        enc = model.encode(b)
    assert generator(model, kv_cache=True).greedy_decode(b, encoder_outputs=enc) == GREEDY
    assert calls == {"step": 2 * STEPS, "row": 2 * STEPS, "fwd": 0, "enc_kv": 2}
    # the uncached loop, for contrast: the full kernel, and the encoder rows projected in every step
    for k in calls:
        calls[k] = 0
    assert generator(model).greedy_decode(b, encoder_outputs=enc) == GREEDY
    assert calls == {"step": 0, "row": 0, "fwd": 4 * STEPS, "enc_kv": 2 * STEPS}
    for k in calls:
        calls[k] = 0
    model.max_cache = STEPS - 1
    state = model.init_decode_state(enc, b["cap_attn_mask"], STEPS)
    assert not state.fused
    assert generator(model, kv_cache=True).greedy_decode(b, encoder_outputs=enc) == GREEDY
    assert calls == {"step": 0, "row": 0, "fwd": 0, "enc_kv": 0}
    model.max_cache, model.max_lk = T.MAX_LK, Lv - 1                               # the limit on the encoder length, likewise
    assert not model.init_decode_state(enc, b["cap_attn_mask"], STEPS).fused
    with pytest.raises(ValueError, match="kernels' route"):
        generator(model, kv_cache=True, use_graph=True).greedy_decode(b, encoder_outputs=enc)


def test_graph_replay_serves_changing_batches_of_one_shape():
    """One generator, two batches of equal shape and different content, in both orders: ONE capture, and the ids of the eager
    cached decode every time - a buffer or a position frozen at capture would show."""
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    model = load_model(True).eval()
    first = load_batch()
    second = shifted_batch(first)
    with torch.no_grad():
        assert not torch.equal(model.encode(first), model.encode(second))
    eager = generator(model, kv_cache=True)
    want = [eager.greedy_decode(first), eager.greedy_decode(second)]
    assert want[0] == GREEDY
    print("\n[tvc-decode] second batch decodes to %s" % (want[1],), end="")
    gen = generator(model, kv_cache=True, use_graph=True)
    for i in (0, 1, 0, 0, 1):
        assert gen.greedy_decode(second if i else first) == want[i], i
    assert gen.counts["captures"] == 1 and gen.counts["replayed"] == 5 * STEPS and len(gen._graphs) == 1


def test_bf16_step_scores_stay_within_twice_the_uncached_bf16_error():
    import hero_amd
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    model, b = load_model(True), load_batch()
    with torch.no_grad():
        ref32 = model(b, "train", compute_loss=False).float()
    hero_amd.set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        uncached = model(b, "train", compute_loss=False)
        enc = model.encode(b)
    state, cached = step_scores(model, b, enc)
    assert state.fused and cached.dtype == torch.bfloat16
    e_unc, e_cached = rel_err(uncached, ref32), rel_err(cached, ref32)
    print("\n[tvc-decode] bf16 scores vs fp32: uncached %.3e  cached %.3e  bound %.3e" % (e_unc, e_cached, 2 * e_unc), end="")
    assert e_unc > 0 and e_cached <= 2 * e_unc
