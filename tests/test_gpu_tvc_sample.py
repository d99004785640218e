"""Sampled captioning on the GPU: TvcGenerator.sample_decode on the kernels' route (hero_sample_select on the beam state: N * S
rows over N blocks of encoder keys, the ancestry table at the identity), eager and under graph replay, and early exit at `eos`
for sample_decode and beam_decode - with the tiny configuration of tests/golden/case_tvc.npz in fp32 and one HERO-base case in
bf16 (random weights, 4 captions, Lv 20, 8 steps, vocabulary 50272).

The reference is the float64 decode of tests/tvc_sample_reference.py driven through the FUSED step of the same module: the step's
own scores are the reference's input values, so what is compared is the selection and the bookkeeping, not the drift of the
decoder.  Rows count where every step's kept size is determined and no draw is a near-tie (DELTA, GAMMA of the reference); the
tests assert how many that leaves out.  Between the fused and the PyTorch route the step scores differ in their last bits, so
that comparison uses margins of 1e-4, the gap of tests/test_gpu_tvc_beam.py.  Scores: rel_err < 2e-4."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import tvc_sample_reference as R
from tests.util import GOLDEN, config_file, rel_err, to_dev

pytestmark = pytest.mark.gpu
FP32_TOL, ROUTE_MARGIN = 2e-4, 1e-4
Z = np.load(os.path.join(GOLDEN, "case_tvc.npz"))
DESC = json.loads(str(Z["desc"]))
GREEDY = json.loads(str(Z["greedy"]))
STEPS, EOS = 8, 30
BASE = dict(attention_probs_dropout_prob=0.1, hidden_act="gelu", hidden_dropout_prob=0.1, hidden_size=768, initializer_range=0.02,
            intermediate_size=3072, max_position_embeddings=514, num_attention_heads=12, type_vocab_size=2)


@pytest.fixture(autouse=True)
def _fp32_default():
    import hero_amd
    from hero_amd import functional as HF
    hero_amd.set_compute_dtype(torch.float32)
    HF.clear_weight_cache()
    yield
    hero_amd.set_compute_dtype(torch.bfloat16)


def load_model(eos_bias=None):
    from hero_amd.model import HeroForTvc
    from hero_amd.utils.misc import set_dropout
    cfg = json.load(open(os.path.join(GOLDEN, "tiny_config.json")))
    cfg["d_config"] = DESC["d_config"]
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    sd.update({k[len("param."):]: torch.from_numpy(Z[k].astype(np.float32)) for k in Z.files if k.startswith("param.")})
    model = HeroForTvc.from_pretrained(config_file(cfg, "tiny_tvc.json"), sd, vfeat_dim=int(z["__vfeat__"]),
                                       max_frm_seq_len=int(z["__max_frm__"])).cuda()
    model.eval()
    set_dropout(model, 0.0)
    if eos_bias is not None:
        with torch.no_grad():
            model.v_encoder.f_encoder.lm_head.bias[eos_bias[0]] += eos_bias[1]
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


def generator(model, eos=EOS, **kw):
    from hero_amd.model import TvcGenerator
    return TvcGenerator(model, STEPS, DESC["bos"], eos, kv_cache=True, **kw)


def reference_decode(model, enc, mask, S, bos, eos, seed, params, **kw):
    """The float64 decode over the module's step on the route `model.fused_decoder` selects (the step's scores are its inputs)."""
    state = model.init_decode_state(enc, mask, STEPS, S, beam_tables=True)
    assert state.fused == model.fused_decoder
    return R.decode(lambda t, last: model.decode_step(state, last.cuda()), enc.shape[0], S, STEPS, bos, eos, seed, *params, **kw)


def base_case():
    """HERO-base decoder (2 layers, hidden 768, vocabulary 50272), random weights, bf16: 4 captions over Lv = 20 frames."""
    import hero_amd
    from hero_amd.model import HeroForTvc
    cfg = {"f_config": dict(BASE, num_hidden_layers=1, vocab_size=50272), "c_config": dict(BASE, num_hidden_layers=1),
           "d_config": dict(BASE, num_hidden_layers=2, max_position_embeddings=1024, type_vocab_size=1, vocab_size=50272)}
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(cfg, f)
    torch.manual_seed(0)
    hero_amd.set_compute_dtype(torch.bfloat16)
    model = HeroForTvc.from_pretrained(f.name, {}, vfeat_dim=64, max_frm_seq_len=32, lsr=0.1).cuda()
    os.unlink(f.name)
    model.eval()
    g = torch.Generator().manual_seed(1)
    N, Lv = 4, 20
    enc = torch.randn(N, Lv, 768, generator=g).cuda()
    lens_v = torch.randint(1, Lv + 1, (N,), generator=g)
    lens_v[0] = Lv
    return model, {"cap_attn_mask": (torch.arange(Lv).unsqueeze(0) < lens_v.unsqueeze(1)).long().cuda()}, enc


def compare(got_ids, got_scores, want, what, min_counted):
    counted = np.nonzero(want["determined"])[0].tolist()
    print("\n[tvc-sample] %s: %d of %d rows counted, finished %d" % (what, len(counted), len(want["determined"]), want["finished"]), end="")
    assert len(counted) >= min_counted
    assert [got_ids[r] for r in counted] == [want["all_ids"][r] for r in counted]
    e = rel_err(torch.tensor(got_scores, dtype=torch.float64)[counted], torch.from_numpy(want["all_scores"])[counted])
    print("  score rel_err %.3e" % e, end="")
    assert e < FP32_TOL


def test_fused_decode_equals_the_float64_decode_and_the_torch_route():
    model, b = load_model(), load_batch()
    with torch.no_grad():
        enc = model.encode(b)
    N, S, seed, params = enc.shape[0], 3, 11, (0.9, 40, 0.95)
    want = reference_decode(model, enc, b["cap_attn_mask"], S, DESC["bos"], EOS, seed, params)
    gen = generator(model)
    ids, scores = gen.sample_decode(b, S, *params, seed=seed, return_all=True, return_scores=True, encoder_outputs=enc)
    assert len(ids) == S * N
    compare(ids, scores, want, "tiny fp32 fused", S * N - 1)
    assert want["finished"] >= 3 and len({tuple(r) for r in ids}) > N                  # finished rows and differing samples are exercised
    if want["determined"].all() and float(want["pick_margin"].min()) > ROUTE_MARGIN:
        assert gen.sample_decode(b, S, *params, seed=seed, encoder_outputs=enc) == want["ids"]
    # the PyTorch route on the same device, wherever the margins hold on both routes
    wide_f = reference_decode(model, enc, b["cap_attn_mask"], S, DESC["bos"], EOS, seed, params, delta=ROUTE_MARGIN, gamma=ROUTE_MARGIN)
    model.fused_decoder = False
    wide_t = reference_decode(model, enc, b["cap_attn_mask"], S, DESC["bos"], EOS, seed, params, delta=ROUTE_MARGIN, gamma=ROUTE_MARGIN)
    torch_ids = generator(model).sample_decode(b, S, *params, seed=seed, return_all=True, encoder_outputs=enc)
    both = np.nonzero(wide_f["determined"] & wide_t["determined"])[0].tolist()
    print("; fused vs PyTorch route: %d of %d rows counted" % (len(both), S * N), end="")
    assert len(both) >= (S * N) // 2
    assert [torch_ids[r] for r in both] == [ids[r] for r in both]


def test_hero_base_bf16_decode_equals_the_float64_decode():
    model, b, enc = base_case()
    N, S, seed, params, eos = enc.shape[0], 3, 2024, (0.8, 50, 0.9), 2
    want = reference_decode(model, enc, b["cap_attn_mask"], S, 0, eos, seed, params)
    from hero_amd.model import TvcGenerator
    for use_graph in (False, True):
        gen = TvcGenerator(model, STEPS, 0, eos, kv_cache=True, use_graph=use_graph)
        ids, scores = gen.sample_decode(b, S, *params, seed=seed, return_all=True, return_scores=True, encoder_outputs=enc)
        compare(ids, scores, want, "HERO-base bf16 %s" % ("replay" if use_graph else "eager"), S * N - 2)
        V = model.config.f_config.vocab_size
        assert all(len(r) <= STEPS and all(0 <= i < V and i != eos for i in r) for r in ids)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_top_k_of_one_is_the_greedy_decode(use_graph):
    model, b = load_model(), load_batch()
    gen = generator(model, int(Z["greedy_eos"]), use_graph=use_graph)
    assert gen.sample_decode(b, top_k=1, seed=5, temperature=0.6) == GREEDY == gen.greedy_decode(b)
    assert gen.sample_decode(b, 2, top_k=1, seed=6, return_all=True) == [r for r in GREEDY for _ in range(2)]


def test_graph_replay_serves_batches_and_seeds_without_a_new_capture():
    model = load_model()
    first = load_batch()
    second = shifted_batch(first)
    params = (0.9, 40, 0.95)
    eager, gen = generator(model), generator(model, use_graph=True)

    def run(g, batch, seed, top_p=params[2]):
        return g.sample_decode(batch, 3, params[0], params[1], top_p, seed=seed, return_all=True, return_scores=True)
    want = {(i, seed): run(eager, batch, seed) for i, batch in enumerate((first, second)) for seed in (1, 2)}
    assert want[(0, 1)] != want[(0, 2)]
    for n, (i, seed) in enumerate(((0, 1), (1, 1), (0, 2), (1, 2), (0, 1))):
        assert run(gen, second if i else first, seed) == want[(i, seed)], (i, seed)
        assert gen.counts["replayed"] == (n + 1) * STEPS == gen.counts["steps"]
    assert gen.counts["captures"] == 1 and len(gen._graphs) == 1
    assert run(gen, first, 1, top_p=0.5) == run(eager, first, 1, top_p=0.5)              # a launch scalar changed: one more capture
    assert gen.counts["captures"] == 2 and len(gen._graphs) == 2
    assert gen.beam_decode(first, 3) == eager.beam_decode(first, 3)                      # the graph table is shared with the other kinds
    assert gen.counts["captures"] == 3 and gen.counts["replayed"] == 7 * STEPS


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_early_exit_gives_the_results_of_the_full_run_in_fewer_steps(use_graph):
    b = load_batch()
    model = load_model(eos_bias=(EOS, 1.0e4))                                           # every row finishes within two steps
    decodes = (lambda g, stop: g.sample_decode(b, 3, 0.9, 0, 0.95, seed=5, return_all=True, return_scores=True, stop_at_eos=stop),
               lambda g, stop: g.beam_decode(b, 3, return_scores=True, stop_at_eos=stop))
    for decode in decodes:
        full, early = generator(model, use_graph=use_graph), generator(model, use_graph=use_graph)
        assert decode(early, True) == decode(full, False)
        assert full.counts["steps"] == STEPS and early.counts["steps"] == 4             # the first look, after check_every = 4 steps
        assert full.counts["replayed"] == STEPS * int(use_graph) and early.counts["replayed"] == 4 * int(use_graph)   # one replay per step, as before
        assert full.counts["captures"] == early.counts["captures"] == int(use_graph)
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    model = load_model()                                                                # the fixture's own weights: same results, never more steps
    for decode in decodes:
        full, early = generator(model, use_graph=use_graph), generator(model, use_graph=use_graph, check_every=1)
        assert decode(early, True) == decode(full, False)
        assert early.counts["steps"] <= full.counts["steps"] == STEPS


def test_samples_share_the_encoder_keys_and_leave_the_ancestry_at_the_identity(monkeypatch):
    from hero_amd import tvc as T
    model, b = load_model(), load_batch()
    N, Lv = b["cap_attn_mask"].shape
    D, S = model.config.d_config.hidden_size, 3
    states, calls = [], {"sample": 0, "beam": 0}
    real_init = model.init_decode_state

    def init(*a, **k):
        states.append(real_init(*a, **k))
        return states[-1]

    def counted(name, real):
        def fn(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return fn
    monkeypatch.setattr(model, "init_decode_state", init)
    monkeypatch.setattr(T, "k_sample_select", counted("sample", T.k_sample_select))
    monkeypatch.setattr(T, "k_beam_select", counted("beam", T.k_beam_select))
    ids = generator(model).sample_decode(b, S, 0.9, 40, 0.95, seed=3, return_all=True)
    assert len(ids) == S * N and calls == {"sample": STEPS, "beam": 0}
    state, = states
    assert state.fused and state.rows == S * N and state.beam == S
    assert [tuple(c.shape) for c in state.cross_kv] == [(N * Lv, 2 * D)] * 2 and tuple(state.mask_add.shape) == (N, Lv)
    assert [tuple(c.shape) for c in state.cache] == [(S * N, STEPS, 2 * D)] * 2
    assert torch.equal(state.tables.anc, torch.arange(S * N, dtype=torch.int32, device="cuda").unsqueeze(1).expand(S * N, STEPS))
    assert int(state.tables.kept.min()) >= 0 and int(state.tables.len.max()) <= STEPS
