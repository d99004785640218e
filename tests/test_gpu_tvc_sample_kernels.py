"""hero_sample_select (hero_amd/csrc/sample.hip) through the wrapper of hero_amd.tvc and the raw ctypes entry point, against the
float64 step of tests/tvc_sample_reference.py on the SAME input values (the cases and their seeds live there;
tests/test_cpu_tvc_sample.py measures the two bounds and asserts on the CPU how many rows they leave undetermined).

Per live row: `kept` lies in the bracket [j_lo, j_hi] of the reference (the kept sizes at top_p -/+ DELTA) and is exactly
min(top_k, V) when top-p is off; the token is the reference's draw for the kernel's OWN kept size (in a near-tie, gap <= GAMMA,
either of the two best); fin, len, ids and last follow from the token exactly; cum is within the project's fp32 gate
rel_err < 2e-4 of the float64 value, as in tests/test_gpu_tvc_beam_kernels.py.  The columns of ids other than t, and cum / len /
fin of finished rows, stay bit for bit.  Ties, the distribution of the draws, reproducibility and the envelope are exact by
construction."""
import numpy as np
import pytest
import torch

from tests import tvc_sample_reference as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu
FP32_TOL = 2e-4
EOS, TCAP = R.SELECT_EOS, R.SELECT_TCAP
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def device_tables(tables):
    return {"cum": torch.from_numpy(np.asarray(tables["cum"], dtype=np.float64)).float().cuda(),
            "fin": torch.from_numpy(np.asarray(tables["fin"])).int().cuda(), "len": torch.from_numpy(np.asarray(tables["len"])).int().cuda(),
            "ids": torch.from_numpy(np.asarray(tables["ids"])).int().cuda().contiguous()}


def seed_word(seed):
    s = int(seed) & ((1 << 64) - 1)
    return torch.tensor([s - (1 << 64) if s >= (1 << 63) else s], dtype=torch.int64, device="cuda")


def run_sample(logits, tb, t, N, S, V, params, seed=R.SELECT_SEED, eos=EOS, device_pos=False, offset=0):
    """-> (last [R], kept [R]) int32 on the CPU; the tables are updated in place."""
    from hero_amd import tvc as T
    last = torch.full((N * S,), -1, dtype=torch.int32, device="cuda")
    kept = torch.full((N * S,), -1, dtype=torch.int32, device="cuda")
    pos = torch.tensor([t - offset], dtype=torch.int32, device="cuda") if device_pos else t
    T.k_sample_select(logits[:, :V], tb["cum"], tb["fin"], tb["len"], tb["ids"], last, kept, seed if torch.is_tensor(seed) else seed_word(seed),
                      pos, N, S, V, eos, *params, pos_offset=offset if device_pos else 0)
    torch.cuda.synchronize()
    return last.cpu(), kept.cpu()


def check_step(last, kept, tb, before, want, t, params, V, what, eos=EOS):
    """The kernel's step against the float64 step `want` of the same inputs -> (rows that differ from the reference's own answer,
    the cum rel_err over the live rows)."""
    live = want["live"]
    got = {k: v.cpu() for k, v in tb.items()}
    soft, cum_want = 0, []
    for r in range(len(live)):
        v, j = int(last[r]), int(kept[r])
        if not live[r]:
            assert (v, j) == (eos, 0), (what, r, v, j)
            assert got["cum"][r].view(torch.int32) == before["cum"][r].cpu().view(torch.int32), (what, r)
            assert int(got["len"][r]) == int(before["len"][r]) and int(got["fin"][r]) == int(before["fin"][r]), (what, r)
            continue
        assert want["j_lo"][r] <= j <= want["j_hi"][r], (what, r, j, int(want["j_lo"][r]), int(want["j_hi"][r]))
        if not params[2] < 1.0:
            assert j == (min(params[1], V) if params[1] else V), (what, r, j)
        assert v in R.admissible(want, r, j), (what, r, v, R.draw(want, r, j))
        soft += int(v != want["last"][r] or j != want["kept"][r])
        assert int(got["len"][r]) == int(before["len"][r]) + 1 and int(got["fin"][r]) == int(v == eos), (what, r)
        cum_want.append(float(before["cum"][r]) + want["x"][r, v] - want["lse"][r])
    keep = torch.arange(got["ids"].shape[1]) != t
    assert torch.equal(got["ids"][:, keep], before["ids"].cpu()[:, keep]), what
    assert torch.equal(got["ids"][:, t], last), what
    e = rel_err(got["cum"].double()[torch.from_numpy(live)], torch.tensor(cum_want, dtype=torch.float64)) if cum_want else 0.0
    assert e < FP32_TOL, (what, e)
    return soft, e


@pytest.mark.parametrize("mid", [False, True], ids=["t0", "mid"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", R.SELECT_VOCABS)
@pytest.mark.parametrize("N,S", R.SELECT_SHAPES)
def test_sample_step_matches_the_float64_step(N, S, V, dtype, mid):
    soft = worst = 0
    for i, params in enumerate(R.params_of(V)):
        case = R.select_case(N, S, V, dtype, mid, params)
        want, t = case["want"], case["t"]
        logits = case["logits"].cuda()
        for device_pos in ((False, True) if V == 160 else ((mid + i) % 2 == 1,)):   # both sources at the small vocabulary, alternating elsewhere
            tb = device_tables(case["tables"])
            before = {k: v.clone() for k, v in tb.items()}
            last, kept = run_sample(logits, tb, t, N, S, V, params, device_pos=device_pos, offset=-1 if device_pos else 0)
            s, e = check_step(last, kept, tb, before, want, t, params, V, (N, S, V, dtype, mid, params, device_pos))
            soft, worst = soft + s, max(worst, e)
    print("\n[sample-select] N=%d S=%d V=%d %s t=%d: %d rows off the reference's own answer, cum rel_err %.3e"
          % (N, S, V, dtype, case["t"], soft, worst), end="")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ld", [R.ODD_VOCAB, R.ODD_VOCAB + 1], ids=["scalar_rows", "vector_rows_with_a_tail"])
def test_a_vocabulary_that_is_no_multiple_of_four(ld, dtype):
    V, N, S, t = R.ODD_VOCAB, 2, 3, 3
    g = torch.Generator().manual_seed(31 + ld)
    logits = torch.full((N * S, ld), 60.0)
    logits[:, :V] = (4.0 * torch.randn(N * S, V, generator=g)).bfloat16().float()
    logits = logits.to(dtype)
    tables = R.initial_tables(N * S, TCAP)
    tables["fin"][4] = 1
    for params in R.SELECT_PARAMS:
        want = R.select_step(logits[:, :V], tables, t, EOS, R.SELECT_SEED, *params)
        assert (want["j_lo"] == want["j_hi"]).all() and (want["gap"][want["live"]] > R.GAMMA).all()      # from the reference alone
        tb = device_tables(tables)
        before = {k: v.clone() for k, v in tb.items()}
        last, kept = run_sample(logits.cuda(), tb, t, N, S, V, params)
        check_step(last, kept, tb, before, want, t, params, V, (ld, dtype, params))
        assert last.tolist() == want["last"].tolist() and kept.tolist() == want["kept"].tolist()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top_p", [1.0, 0.5], ids=["top_k", "boundary_inside_the_run"])
def test_tie_rule_keeps_the_lowest_tokens_of_an_equal_run(top_p, dtype):
    case = R.tie_case(top_p)
    V, rows, allowed = case["V"], case["R"], case["top"][:case["kept"]]
    logits = case["logits"].to(dtype).cuda()
    seen = []
    for t in case["positions"]:
        tables = R.initial_tables(rows, TCAP)
        want = R.select_step(case["logits"], tables, t, EOS, R.SELECT_SEED, *case["params"])
        last, kept = run_sample(logits, device_tables(tables), t, 4, rows // 4, V, case["params"], device_pos=t % 2 == 1)
        assert last.tolist() == want["last"].tolist() and kept.tolist() == [case["kept"]] * rows
        seen += last.tolist()
    assert len(seen) == 200 and set(seen) == set(allowed), (sorted(set(seen)), allowed)


@pytest.mark.parametrize("top_k,bound", [(0, 44.3), (4, 21.1)], ids=["softmax", "top4"])
def test_draws_follow_the_softmax_and_equal_the_reference_draw_for_draw(top_k, bound):
    case = R.distribution_case(top_k)
    logits = case["logits"].cuda()
    tokens = []
    for t in case["positions"]:
        tables = R.initial_tables(case["R"], 128)
        want = R.select_step(case["logits"], tables, t, EOS, case["seed"], *case["params"])
        last, _ = run_sample(logits, device_tables(tables), t, 1, case["R"], case["V"], case["params"], seed=case["seed"])
        assert last.tolist() == want["last"].tolist(), t
        tokens += last.tolist()
    chi = R.chi_square(tokens, case["logits"][0].numpy(), top_k)
    print("\n[sample-select] chi-square over %d draws, top_k=%d: %.2f (bound %.1f)" % (len(tokens), top_k, chi, bound), end="")
    assert len(tokens) == 20000 and chi < bound


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_runs_give_the_same_bits_and_the_seed_word_is_read_on_the_device(dtype):
    params = R.SELECT_PARAMS[3]
    case = R.select_case(5, 3, 50272, dtype, True, params)
    word = seed_word(R.SELECT_SEED)
    runs = []
    for seed in (R.SELECT_SEED, R.SELECT_SEED, R.SELECT_SEED + 1):
        word.fill_(int(seed_word(seed)))                                                # the same buffer, the same launch arguments
        tb = device_tables(case["tables"])
        last, kept = run_sample(case["logits"].cuda(), tb, case["t"], 5, 3, 50272, params, seed=word, device_pos=True, offset=-1)
        runs.append([tb["cum"].view(torch.int32).cpu(), last, kept] + [tb[k].cpu() for k in ("fin", "len", "ids")])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert not torch.equal(runs[0][1], runs[2][1]) and torch.equal(runs[0][2], runs[2][2])     # other draws from the same kept sets
    want = R.select_step(case["logits"][:, :50272], case["tables"], case["t"], EOS, R.SELECT_SEED + 1, *params)
    live = torch.from_numpy(want["live"])
    assert torch.equal(runs[2][1].long()[live], torch.from_numpy(want["last"])[live])


def test_calls_outside_the_envelope_are_refused_without_a_launch():
    import ctypes as C
    from hero_amd import _lib as L
    from hero_amd import tvc as T
    lib = L.lib()
    N, S, V = 2, 3, 160
    logits = torch.randn(N * S, V, device="cuda")
    tb = device_tables(R.initial_tables(N * S, TCAP))
    last = torch.full((N * S,), -1, dtype=torch.int32, device="cuda")
    kept = torch.full((N * S,), -1, dtype=torch.int32, device="cuda")
    word = seed_word(1)
    before = {k: v.clone() for k, v in tb.items()}

    def call(N=N, S=S, V=V, ld=V, Tcap=TCAP, dtype=L.F32, logits_ptr=logits.data_ptr(), pos=0, eos=EOS, inv_t=1.0, top_k=0, top_p=1.0,
             seed_ptr=L.ptr(word), kept_ptr=L.ptr(kept)):
        return lib.hero_sample_select(logits_ptr, L.ptr(tb["cum"]), L.ptr(tb["fin"]), L.ptr(tb["len"]), L.ptr(tb["ids"]), L.ptr(last), kept_ptr,
                                      seed_ptr, None, pos, N, S, V, ld, Tcap, eos, C.c_float(inv_t), top_k, C.c_float(top_p), dtype, L.stream())
    bad = [dict(N=0), dict(S=0), dict(V=0, ld=0), dict(V=65537, ld=65537), dict(Tcap=0), dict(Tcap=129), dict(ld=V - 1), dict(logits_ptr=None),
           dict(dtype=7), dict(pos=TCAP), dict(pos=-1), dict(eos=V), dict(eos=-1), dict(inv_t=0.0), dict(inv_t=-1.0), dict(inv_t=float("inf")),
           dict(inv_t=float("nan")), dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=float("nan")), dict(seed_ptr=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"hero_sample_select" in lib.hero_last_error(), kw
    torch.cuda.synchronize()
    assert all(torch.equal(tb[k], before[k]) for k in tb) and last.eq(-1).all() and kept.eq(-1).all()
    q = lib.hero_sample_in_envelope
    assert [q(L.F32, 0, TCAP), q(L.F32, 65537, TCAP), q(L.F32, V, 0), q(L.F32, V, 129), q(7, V, TCAP)] == [0] * 5
    assert q(L.F32, V, TCAP) == 1 and q(L.BF16, 65536, 128) == 1 and q(L.F32, 1, 1) == 1
    assert call(kept_ptr=None) == 0                                                    # inside the envelope, `kept` left out: it runs
    torch.cuda.synchronize()
    assert last.ge(0).all() and kept.eq(-1).all()
    with pytest.raises(ValueError, match="envelope"):
        T.k_sample_select(logits, tb["cum"], tb["fin"], tb["len"], tb["ids"], last, kept, word, 0, N, S, V + 1, EOS, 1.0, 0, 1.0)
    for params in ((0.0, 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0)):
        with pytest.raises(ValueError, match="temperature"):
            T.k_sample_select(logits, tb["cum"], tb["fin"], tb["len"], tb["ids"], last, kept, word, 0, N, S, V, EOS, *params)
    # a device position outside [0, Tcap) leaves everything alone
    state = {k: v.clone() for k, v in tb.items()}
    last.fill_(-1)
    T.k_sample_select(logits, tb["cum"], tb["fin"], tb["len"], tb["ids"], last, None, word, torch.tensor([TCAP], dtype=torch.int32, device="cuda"),
                      N, S, V, EOS, 1.0, 0, 1.0)
    torch.cuda.synchronize()
    assert all(torch.equal(tb[k], state[k]) for k in tb) and last.eq(-1).all()
