"""Sampled captioning on the CPU: the float64 statement of tests/tvc_sample_reference.py judges its own cases (the two measured
bounds DELTA and GAMMA, and how many rows of every case they leave undetermined), then the PyTorch formulation
hero_amd.model.tvc.sample_select_torch - same hash, fp32 ordering and noise - against it: token for token over the case grid of
the GPU kernel tests, the tie rule, the distribution of the draws (Pearson's chi-square, deterministic: fixed seeds), the limits,
and TvcGenerator.sample_decode / early exit on CPU tensors with the tiny configuration of tests/golden/case_tvc.npz (the encoder
has no CPU route, so the fixture's encoder outputs go in, as in tests/test_cpu_tvc_beam.py).

A row whose kept size is not determined (j_lo != j_hi) or whose draw is a near-tie is NOT skipped: its kept size must lie in the
bracket and its token must be admissible for that kept size.  Measured here: no row of any case is undetermined."""
import json
import os

import numpy as np
import pytest
import torch

from tests import tvc_sample_reference as R
from tests.util import GOLDEN, config_file, rel_err

Z = np.load(os.path.join(GOLDEN, "case_tvc.npz"))
DESC = json.loads(str(Z["desc"]))
GREEDY = json.loads(str(Z["greedy"]))
STEPS, EOS = 8, 30


@pytest.fixture(scope="module")
def built_lib():
    from hero_amd import build
    return build.build()


def torch_tables(tables, N, S):
    from hero_amd.model.tvc import BeamTables
    tb = BeamTables(N, S, np.asarray(tables["ids"]).shape[1], "cpu", False)
    tb.cum = torch.from_numpy(np.asarray(tables["cum"], dtype=np.float64)).float()
    tb.fin, tb.len = (torch.from_numpy(np.asarray(tables[k])).long().clone() for k in ("fin", "len"))
    tb.ids = torch.from_numpy(np.asarray(tables["ids"])).long().clone()
    return tb


def check_step(got_tokens, got_kept, tb, case, what):
    """One step of another implementation against the float64 step: kept in the bracket, the token admissible for that kept
    size, the tables following from the token; -> the number of rows that were not simply equal to the reference."""
    want, t, before = case["want"], case["t"], case["tables"]
    soft = 0
    for r in range(len(got_tokens)):
        v, j = int(got_tokens[r]), int(got_kept[r])
        if not want["live"][r]:
            assert (v, j) == (R.SELECT_EOS, 0) and float(tb["cum"][r]) == float(np.float32(before["cum"][r])), (what, r)
            assert int(tb["len"][r]) == int(before["len"][r]) and int(tb["fin"][r]) == 1, (what, r)
            continue
        assert want["j_lo"][r] <= j <= want["j_hi"][r], (what, r, j, want["j_lo"][r], want["j_hi"][r])
        assert v in R.admissible(want, r, j), (what, r, v, R.draw(want, r, j))
        soft += int(v != want["last"][r] or j != want["kept"][r])
        assert int(tb["len"][r]) == int(before["len"][r]) + 1 and int(tb["fin"][r]) == int(v == R.SELECT_EOS), (what, r)
        cum = R.cum_after(want, before, r, v)
        assert abs(float(tb["cum"][r]) - cum) <= 2e-4 * max(abs(cum), 1.0), (what, r)
    ids = np.asarray(tb["ids"])
    keep = np.arange(ids.shape[1]) != t
    assert np.array_equal(ids[:, keep], np.asarray(before["ids"])[:, keep]) and np.array_equal(ids[:, t], np.asarray(got_tokens)), what
    return soft


def test_recorded_bounds_cover_the_measured_float32_errors_and_the_cases_are_determined():
    mass, score = R.measure_bounds()
    print("\n[tvc-sample] float32 restatements against float64: prefix mass %.3e, z + g %.3e; DELTA %.1e GAMMA %.1e"
          % (mass, score, R.DELTA, R.GAMMA), end="")
    assert 4 * mass <= R.DELTA <= 8 * mass and 4 * score <= R.GAMMA <= 8 * score
    rows = undetermined = near = resampled = 0
    for c in R.all_cases():
        case = R.select_case(*c)
        determined, gapped = R.case_conditions(case["want"])
        assert determined >= R.MIN_DETERMINED and gapped >= R.MIN_GAPPED, (c, determined, gapped)
        assert case["want"]["live"].any(), c
        w = case["want"]
        rows += int(w["live"].sum())
        undetermined += int(((w["j_lo"] != w["j_hi"]) & w["live"]).sum())
        near += int(((w["gap"] <= R.GAMMA) & w["live"]).sum())
        resampled += int(case["attempt"] > 0)
    print("; %d live rows, %d undetermined kept sizes, %d near-ties, %d cases drawn again" % (rows, undetermined, near, resampled), end="")
    assert rows > 1500


def test_torch_route_equals_the_float64_step_over_the_case_grid():
    from hero_amd.model.tvc import sample_select_torch
    soft = 0
    for c in R.all_cases():
        N, S, V, dtype, mid, params = c
        case = R.select_case(*c)
        tb = torch_tables(case["tables"], N, S)
        tokens, kept = sample_select_torch(case["logits"][:, :V], tb, case["t"], R.SELECT_EOS, R.SELECT_SEED, *params)
        got = {"cum": tb.cum.double().numpy(), "len": tb.len.numpy(), "fin": tb.fin.numpy(), "ids": tb.ids.numpy()}
        soft += check_step(tokens.numpy(), kept.numpy(), got, case, c)
        if not params[2] < 1.0:
            assert kept[torch.from_numpy(case["want"]["live"])].eq(min(params[1], V) if params[1] else V).all(), c
    assert soft == 0                      # float64 masses, and no near-tie in any case: the reference's own answer everywhere


@pytest.mark.parametrize("top_p", [1.0, 0.5], ids=["top_k", "boundary_inside_the_run"])
def test_tie_rule_keeps_the_lowest_tokens_of_an_equal_run(top_p):
    from hero_amd.model.tvc import sample_select_torch
    case = R.tie_case(top_p)
    V, rows, allowed = case["V"], case["R"], case["top"][:case["kept"]]
    seen = []
    for t in case["positions"]:
        tables = R.initial_tables(rows, 12)
        want = R.select_step(case["logits"], tables, t, R.SELECT_EOS, R.SELECT_SEED, *case["params"])
        assert want["kept"].tolist() == [case["kept"]] * rows and (want["j_lo"] == want["j_hi"]).all()
        tokens, kept = sample_select_torch(case["logits"], torch_tables(tables, 1, rows), t, R.SELECT_EOS, R.SELECT_SEED, *case["params"])
        assert tokens.tolist() == want["last"].tolist() and kept.tolist() == want["kept"].tolist()
        seen += tokens.tolist()
    assert len(seen) == 200 and set(seen) == set(allowed), (sorted(set(seen)), allowed)


@pytest.mark.parametrize("top_k,bound", [(0, 44.3), (4, 21.1)], ids=["softmax", "top4"])
def test_draws_follow_the_softmax(top_k, bound):
    """20 000 draws; 44.3 and 21.1 are the 0.9999 quantiles of chi-square with 15 and 3 degrees of freedom."""
    from hero_amd.model.tvc import sample_select_torch
    case = R.distribution_case(top_k)
    tokens = []
    for t in case["positions"]:
        tables = R.initial_tables(case["R"], 128)
        got, _ = sample_select_torch(case["logits"], torch_tables(tables, 1, case["R"]), t, R.SELECT_EOS, case["seed"], *case["params"])
        if t % 25 == 0:
            want = R.select_step(case["logits"], tables, t, R.SELECT_EOS, case["seed"], *case["params"])
            assert got.tolist() == want["last"].tolist()
        tokens += got.tolist()
    chi = R.chi_square(tokens, case["logits"][0].numpy(), top_k)
    print("\n[tvc-sample] chi-square over %d draws, top_k=%d: %.2f (bound %.1f)" % (len(tokens), top_k, chi, bound), end="")
    assert len(tokens) == 20000 and chi < bound


def test_limits():
    from hero_amd.model.tvc import sample_select_torch
    g = torch.Generator().manual_seed(5)
    R_, V = 6, 1000
    logits = (4.0 * torch.randn(R_, V, generator=g)).bfloat16().float()
    logits[0, 17] = logits[0, 400] = logits[0].max() + 1.0                          # a tie at the maximum: the lower token
    first_max = [int(torch.nonzero(row == row.max())[0]) for row in logits]
    assert first_max[0] == 17
    for seed, temperature in ((0, 1.0), (12345, 0.3), (2 ** 64 - 1, 2.5)):
        tb = torch_tables(R.initial_tables(R_, 4), 1, R_)
        tokens, kept = sample_select_torch(logits, tb, 1, R.SELECT_EOS, seed, temperature, 1, 0.3)
        assert tokens.tolist() == first_max and kept.tolist() == [1] * R_
    tb = torch_tables(R.initial_tables(R_, 4), 1, R_)
    tokens, kept = sample_select_torch(logits, tb, 0, R.SELECT_EOS, 9, 1.0, 0, 1.0)
    assert kept.tolist() == [V] * R_
    # finished rows re-emit eos at an unchanged score; cum is the RAW log-probability of the token, not the filtered one
    tables = R.initial_tables(R_, 4)
    tables["cum"] = np.linspace(-5.0, -1.0, R_)
    tables["fin"] = np.array([0, 1, 0, 1, 0, 0])
    tables["len"] = np.array([2, 1, 2, 2, 2, 2])
    tb = torch_tables(tables, 1, R_)
    tokens, kept = sample_select_torch(logits, tb, 2, R.SELECT_EOS, 77, 0.7, 20, 0.8)
    logp = torch.log_softmax(logits.double(), dim=1)
    for r in range(R_):
        if tables["fin"][r]:
            assert int(tokens[r]) == R.SELECT_EOS and int(kept[r]) == 0 and float(tb.cum[r]) == float(np.float32(tables["cum"][r]))
            assert int(tb.len[r]) == tables["len"][r] and int(tb.fin[r]) == 1 and int(tb.ids[r, 2]) == R.SELECT_EOS
        else:
            assert 1 <= int(kept[r]) <= 20
            assert abs(float(tb.cum[r]) - (tables["cum"][r] + float(logp[r, tokens[r]]))) < 1e-5


# ---- the generator on CPU tensors ----------------------------------------------------------------------------------------------
def _model(eos_bias=None):
    from hero_amd.model import HeroForTvc
    from hero_amd.utils.misc import set_dropout
    cfg = json.load(open(os.path.join(GOLDEN, "tiny_config.json")))
    cfg["d_config"] = DESC["d_config"]
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    sd.update({k[len("param."):]: torch.from_numpy(Z[k].astype(np.float32)) for k in Z.files if k.startswith("param.")})
    model = HeroForTvc.from_pretrained(config_file(cfg, "tiny_tvc.json"), sd, vfeat_dim=int(z["__vfeat__"]),
                                       max_frm_seq_len=int(z["__max_frm__"]))
    model.eval()
    set_dropout(model, 0.0)
    if eos_bias is not None:
        with torch.no_grad():
            model.v_encoder.f_encoder.lm_head.bias[eos_bias[0]] += eos_bias[1]
    return model


def _batch():
    return {k[len("out."):]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith("out.") and Z[k].dtype.kind != "U"}


def _gen(model, eos=EOS, **kw):
    from hero_amd.model import TvcGenerator
    return TvcGenerator(model, STEPS, DESC["bos"], eos, kv_cache=True, **kw)


def reference_decode(model, enc, mask, S, eos, seed, params, length_penalty=1.0):
    """The float64 decode over the module's own PyTorch step (the step's scores are the reference's input values)."""
    state = model.init_decode_state(enc, mask, STEPS, S, beam_tables=True)
    assert not state.fused
    return R.decode(lambda t, last: model.decode_step(state, last), enc.shape[0], S, STEPS, DESC["bos"], eos, seed, *params,
                    length_penalty=length_penalty)


def test_top_k_of_one_is_the_greedy_decode():
    model, b, enc = _model(), _batch(), torch.from_numpy(Z["enc_out"])
    eos = int(Z["greedy_eos"])
    gen = _gen(model, eos)
    assert gen.sample_decode(b, top_k=1, seed=3, temperature=0.5, encoder_outputs=enc) == GREEDY
    assert gen.sample_decode(b, top_k=1, encoder_outputs=enc) == gen.greedy_decode(b, encoder_outputs=enc)


def test_three_samples_equal_the_float64_decode_and_its_pick():
    model, b, enc = _model(), _batch(), torch.from_numpy(Z["enc_out"])
    N, params, seed = enc.shape[0], (0.9, 40, 0.95), 11
    want = reference_decode(model, enc, b["cap_attn_mask"], 3, EOS, seed, params)
    print("\n[tvc-sample] cpu: %d of %d rows determined, finished %d, picks %s, pick margin %.2e"
          % (int(want["determined"].sum()), 3 * N, want["finished"], want["best"].tolist(), float(want["pick_margin"].min())), end="")
    assert want["determined"].all() and float(want["pick_margin"].min()) > 1e-4
    gen = _gen(model)
    ids, scores = gen.sample_decode(b, 3, *params, seed=seed, return_all=True, return_scores=True, encoder_outputs=enc)
    assert len(ids) == len(scores) == 3 * N and ids == want["all_ids"]
    assert rel_err(torch.tensor(scores, dtype=torch.float64), torch.from_numpy(want["all_scores"])) < 2e-4
    picked, best_scores = gen.sample_decode(b, 3, *params, seed=seed, return_scores=True, encoder_outputs=enc)
    assert picked == want["ids"] == [ids[3 * n + int(want["best"][n])] for n in range(N)]
    assert rel_err(torch.tensor(best_scores, dtype=torch.float64), torch.from_numpy(want["scores"])) < 2e-4
    assert len({tuple(r) for r in ids}) > N                                            # the samples of a caption differ
    # one seed, one result; another seed, another
    assert gen.sample_decode(b, 3, *params, seed=seed, return_all=True, encoder_outputs=enc) == ids
    assert gen.sample_decode(b, 3, *params, seed=seed + 1, return_all=True, encoder_outputs=enc) != ids
    # the state: N blocks of encoder keys under 3 N rows, the ancestry at the identity
    state = model.init_decode_state(enc, b["cap_attn_mask"], STEPS, 3, beam_tables=True)
    assert state.rows == 3 * N and state.cross_k[0].shape[0] == N
    state.tables.reset_sampling()
    assert state.tables.cum.eq(0).all() and torch.equal(state.tables.anc[:, 0], torch.arange(3 * N))


def test_early_exit_gives_the_results_of_the_full_run():
    b, enc = _batch(), torch.from_numpy(Z["enc_out"])
    N = enc.shape[0]
    # every row finishes at step 0: the output bias at eos is raised above everything else
    model = _model(eos_bias=(EOS, 1.0e4))
    for decode in (lambda g, stop: g.sample_decode(b, 3, 0.9, 0, 0.95, seed=5, return_all=True, return_scores=True, stop_at_eos=stop,
                                                   encoder_outputs=enc),
                   lambda g, stop: g.beam_decode(b, 3, return_scores=True, stop_at_eos=stop, encoder_outputs=enc)):
        full, early = _gen(model, check_every=2), _gen(model, check_every=2)
        want, got = decode(full, False), decode(early, True)
        assert got == want and all(r == [] for r in got[0])
        assert full.counts["steps"] == STEPS and early.counts["steps"] == 2
    # an ordinary model: same captions and scores, never more steps
    model = _model()
    for decode in (lambda g, stop: g.sample_decode(b, 2, 1.0, 20, 1.0, seed=8, return_all=True, return_scores=True, stop_at_eos=stop,
                                                   encoder_outputs=enc),
                   lambda g, stop: g.beam_decode(b, 3, return_scores=True, stop_at_eos=stop, encoder_outputs=enc)):
        full, early = _gen(model), _gen(model)
        assert decode(early, True) == decode(full, False)
        assert early.counts["steps"] <= full.counts["steps"] == STEPS
    # an eos that the greedy path never emits: no row ever finishes, every step runs
    never = next(v for v in range(5, 200) if all(v not in r for r in GREEDY) and v != int(Z["greedy_eos"]))
    gen = _gen(model, never, check_every=1)
    ids = gen.sample_decode(b, top_k=1, stop_at_eos=True, encoder_outputs=enc)
    assert all(len(r) == STEPS for r in ids) and gen.counts["steps"] == STEPS and len(ids) == N


def test_argument_errors():
    from hero_amd.model import TvcGenerator
    model, b, enc = _model(), _batch(), torch.from_numpy(Z["enc_out"])
    with pytest.raises(ValueError, match="kv_cache"):
        TvcGenerator(model, STEPS, DESC["bos"], EOS).sample_decode(b, encoder_outputs=enc)
    gen = _gen(model)
    for kw, what in ((dict(n_samples=0), "n_samples"), (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
                     (dict(temperature=float("inf")), "temperature"), (dict(top_p=0.0), "top_p"), (dict(top_p=-0.5), "top_p"),
                     (dict(top_k=-1), "top_k")):
        with pytest.raises(ValueError, match=what):
            gen.sample_decode(b, encoder_outputs=enc, **kw)
    with pytest.raises(ValueError, match="check_every"):
        _gen(model, check_every=0)
    with pytest.raises(ValueError, match="kernels' route"):
        _gen(model, use_graph=True).sample_decode(b, 2, encoder_outputs=enc)


def test_sample_envelope_query_needs_no_gpu(built_lib):
    """hero_sample_in_envelope answers on the host; hero_amd.tvc.in_envelope_sample wraps it."""
    from hero_amd import _lib as Lb
    from hero_amd import tvc
    q = Lb.lib().hero_sample_in_envelope
    for dtype in (Lb.F32, Lb.BF16):
        assert q(dtype, 50272, 1) == 1 and q(dtype, 65536, 128) == 1 and q(dtype, 1, 60) == 1
        assert q(dtype, 0, 8) == 0 and q(dtype, 65537, 8) == 0 and q(dtype, 1000, 129) == 0 and q(dtype, 1000, 0) == 0
    assert q(7, 1000, 8) == 0
    for dtype in (torch.float32, torch.bfloat16):
        assert tvc.in_envelope_sample(dtype, 50272, 60) and not tvc.in_envelope_sample(dtype, 65537, 60)
    assert not tvc.in_envelope_sample(torch.float16, 1000, 8)
