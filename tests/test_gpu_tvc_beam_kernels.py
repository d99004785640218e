"""hero_beam_select (hero_amd/csrc/beam.hip) and the two beam entry points of the one-row attention kernel,
hero_dec_attention_row_grouped and hero_dec_attention_step_beam (hero_amd/csrc/dec_attention.hip), through the wrappers of
hero_amd.tvc and the raw ctypes entry points.

Selection: against the float64 step of tests/tvc_beam_reference.py on the SAME input values (the cases and their seeds live
there; tests/test_cpu_tvc_beam.py checks on the CPU that they leave out at most one caption in ten).  A caption takes part in
the comparison if its gap is >= 1e-4: |score| < 64, fp32 spacing 7.6e-6 there.  On those captions parents, tokens, fin, len, ids,
anc and last are exact and cum is within the project's fp32 gate rel_err < 2e-4; on ALL captions the columns behind t stay.
Ties, finished beams, the in-place permutation and the envelope are exact by construction and do not use the gap.

Attention: bit-identical to the existing entry points on physically replicated keys / a physically gathered cache."""
import ctypes as C

import pytest
import torch

from tests import tvc_beam_reference as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu
GAP, FP32_TOL = 1e-4, 2e-4
EOS, TCAP = R.SELECT_EOS, R.SELECT_TCAP
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def device_tables(tables):
    return {"cum": tables["cum"].float().cuda(), "fin": tables["fin"].int().cuda(), "len": tables["len"].int().cuda(),
            "ids": tables["ids"].int().cuda().contiguous(), "anc": tables["anc"].int().cuda().contiguous()}


def run_select(logits, tb, t, N, B, V, eos=EOS, device_pos=False, offset=0):
    """-> last [R] int32; the tables are updated in place."""
    from hero_amd import tvc as T
    R_ = N * B
    last = torch.full((R_,), -1, dtype=torch.int32, device="cuda")
    ws = torch.zeros((R_ * B,), dtype=torch.int64, device="cuda")
    pos = torch.tensor([t - offset], dtype=torch.int32, device="cuda") if device_pos else t
    T.k_beam_select(logits[:, :V], tb["cum"], tb["fin"], tb["len"], tb["ids"], tb["anc"], last, ws, pos, N, B, V, eos,
                    pos_offset=offset if device_pos else 0)
    torch.cuda.synchronize()
    return last


@pytest.mark.parametrize("mid", [False, True], ids=["t0", "mid"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", R.SELECT_VOCABS)
@pytest.mark.parametrize("N,B", R.SELECT_SHAPES)
def test_select_matches_the_float64_step(N, B, V, dtype, mid):
    case = R.select_case(N, B, V, dtype, mid)
    want, t = case["want"], case["t"]
    for device_pos in ((False, True) if V == 160 else (mid,)):          # both sources at the small vocabulary, alternating elsewhere
        tb = device_tables(case["tables"])
        before = {k: v.clone() for k, v in tb.items()}
        last = run_select(case["logits"].cuda(), tb, t, N, B, V, device_pos=device_pos, offset=-1 if device_pos else 0)
        counted = case["gap"] >= GAP
        rows = counted.repeat_interleave(B)
        print("\n[beam-select] N=%d B=%d V=%d %s t=%d: %d of %d captions counted, min gap %.3e"
              % (N, B, V, dtype, t, int(counted.sum()), N, float(case["gap"].min())), end="")
        assert torch.equal(tb["ids"][:, t + 1:], before["ids"][:, t + 1:]) and torch.equal(tb["anc"][:, t + 1:], before["anc"][:, t + 1:])
        if not bool(counted.any()):
            continue
        parent = tb["anc"][:, t].cpu().long() - (torch.arange(N * B) // B) * B
        assert torch.equal(parent[rows], want["parent"][rows])
        assert torch.equal(last.cpu().long()[rows], want["last"][rows])
        for k in ("fin", "len", "ids", "anc"):
            assert torch.equal(tb[k].cpu().long()[rows], want[k][rows]), k
        e = rel_err(tb["cum"].cpu().double()[rows], want["cum"][rows])
        print("  cum rel_err %.3e" % e, end="")
        assert e < FP32_TOL


def select_small(logits, cum, fin, length=None, ids=None, anc=None, t=0, B=None, tcap=TCAP, eos=EOS):
    """One caption, given tables -> (tables after the step, last), all on the CPU."""
    B = B or logits.shape[0]
    tb = {"cum": torch.tensor(cum, dtype=torch.float32).cuda(), "fin": torch.tensor(fin, dtype=torch.int32).cuda(),
          "len": torch.tensor(length if length is not None else [t] * B, dtype=torch.int32).cuda(),
          "ids": (ids if ids is not None else torch.zeros(B, tcap)).int().cuda().contiguous(),
          "anc": (anc if anc is not None else torch.arange(B).unsqueeze(1).repeat(1, tcap)).int().cuda().contiguous()}
    last = run_select(logits.cuda(), tb, t, 1, B, logits.shape[1], eos=eos)
    return {k: v.cpu() for k, v in tb.items()}, last.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_ties_go_to_the_lower_token_and_the_lower_beam(dtype):
    V = 160
    logits = (torch.arange(V) % 4).float().repeat(3, 1).to(dtype)                      # the maximum 3 at v = 3, 7, 11, ...
    tb, last = select_small(logits, [0.0, R.DEAD, R.DEAD], [0, 0, 0])
    assert last.tolist() == [3, 7, 11] and tb["anc"][:, 0].tolist() == [0, 0, 0]
    assert tb["cum"][0] == tb["cum"][1] == tb["cum"][2]
    row = torch.zeros(V)
    row[17], row[90] = 9.0, 8.0
    tb, last = select_small(row.repeat(2, 1).to(dtype), [-1.0, -1.0], [0, 0], t=3)     # two identical rows under one cum
    assert last.tolist() == [17, 17] and tb["anc"][:, 3].tolist() == [0, 1] and tb["cum"][0] == tb["cum"][1]


def test_finished_beams_offer_only_eos_at_their_score_and_still_compete():
    g = torch.Generator().manual_seed(77)
    V, t = 1000, 4
    logits = 3.0 * torch.randn(3, V, generator=g)
    ids = torch.randint(0, V, (3, TCAP), generator=g)
    tb, last = select_small(logits, [-2.0, -1.5, -3.0], [0, 1, 0], length=[4, 2, 4], ids=ids, t=t)
    want, _ = R.select_step(logits, {"cum": torch.tensor([-2.0, -1.5, -3.0]), "fin": torch.tensor([0, 1, 0]),
                                     "len": torch.tensor([4, 2, 4]), "ids": ids, "anc": torch.arange(3).unsqueeze(1).repeat(1, TCAP)}, t, 3, EOS)
    parents = tb["anc"][:, t].tolist()
    assert parents == want["parent"].tolist() and last.tolist() == want["last"].tolist()
    assert parents.count(1) == 1 and parents[0] == 1                                   # once, and best: a live candidate is below -2
    assert last[0] == EOS and float(tb["cum"][0]) == -1.5 and int(tb["len"][0]) == 2 and int(tb["fin"][0]) == 1
    assert tb["len"][1:].tolist() == [5, 5] and tb["ids"][0, :t].tolist() == ids[1, :t].tolist()
    # every beam finished, scores descending: the tables stay, column t becomes eos
    anc = torch.randint(0, 3, (3, TCAP), generator=g)
    tb, last = select_small(logits, [-1.0, -2.0, -3.0], [1, 1, 1], length=[2, 3, 4], ids=ids, anc=anc, t=t)
    assert tb["cum"].tolist() == [-1.0, -2.0, -3.0] and tb["len"].tolist() == [2, 3, 4] and tb["fin"].tolist() == [1, 1, 1]
    assert last.tolist() == [EOS] * 3 and tb["ids"][:, t].tolist() == [EOS] * 3 and tb["anc"][:, t].tolist() == [0, 1, 2]
    keep = torch.arange(TCAP) != t
    assert torch.equal(tb["ids"][:, keep], ids[:, keep].int()) and torch.equal(tb["anc"][:, keep], anc[:, keep].int())


def test_in_place_update_follows_a_cyclic_parent_assignment():
    """Parents [1, 2, 0]: every row is read by another row's update, so a write before the last read would show."""
    g = torch.Generator().manual_seed(78)
    V, t = 160, 11
    ids, anc = torch.randint(0, V, (3, TCAP), generator=g), torch.randint(0, 3, (3, TCAP), generator=g)
    tb, last = select_small(torch.randn(3, V, generator=g), [-3.0, -1.0, -2.0], [1, 1, 1], length=[5, 6, 7], ids=ids, anc=anc, t=t)
    assert tb["anc"][:, t].tolist() == [1, 2, 0] and tb["cum"].tolist() == [-1.0, -2.0, -3.0] and tb["len"].tolist() == [6, 7, 5]
    for i, p in enumerate([1, 2, 0]):
        assert tb["ids"][i, :t].tolist() == ids[p, :t].tolist() and tb["anc"][i, :t].tolist() == anc[p, :t].tolist()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_runs_give_the_same_bits(dtype):
    case = R.select_case(5, 3, 50272, dtype, True)
    runs = []
    for _ in range(2):
        tb = device_tables(case["tables"])
        last = run_select(case["logits"].cuda(), tb, case["t"], 5, 3, 50272, device_pos=True, offset=-1)
        runs.append([tb["cum"].view(torch.int32).cpu(), last.cpu()] + [tb[k].cpu() for k in ("fin", "len", "ids", "anc")])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_calls_outside_the_envelope_are_refused_without_a_launch():
    from hero_amd import _lib as L
    from hero_amd import tvc as T
    lib = L.lib()
    N, B, V = 2, 3, 160
    logits = torch.randn(N * B, V, device="cuda")
    tb = device_tables(R.initial_tables(N, B, TCAP))
    last = torch.full((N * B,), -1, dtype=torch.int32, device="cuda")
    ws = torch.zeros((N * 8 * 8,), dtype=torch.int64, device="cuda")
    before = {k: v.clone() for k, v in tb.items()}

    def call(B=B, V=V, ld=V, Tcap=TCAP, dtype=L.F32, logits_ptr=logits.data_ptr(), pos=0):
        return lib.hero_beam_select(logits_ptr, L.ptr(tb["cum"]), L.ptr(tb["fin"]), L.ptr(tb["len"]), L.ptr(tb["ids"]), L.ptr(tb["anc"]),
                                    L.ptr(last), L.ptr(ws), None, pos, N, B, V, ld, Tcap, EOS, dtype, L.stream())
    bad = [dict(B=0), dict(B=9), dict(V=2), dict(V=65537, ld=65537), dict(Tcap=129), dict(ld=V - 1), dict(logits_ptr=None), dict(dtype=7),
           dict(pos=TCAP)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"hero_beam_select" in lib.hero_last_error(), kw
    torch.cuda.synchronize()
    assert all(torch.equal(tb[k], before[k]) for k in tb) and last.eq(-1).all()
    q = lib.hero_beam_in_envelope
    assert [q(L.F32, V, 0, TCAP), q(L.F32, V, 9, TCAP), q(L.F32, 2, 3, TCAP), q(L.F32, 65537, 3, TCAP), q(L.F32, V, 3, 129), q(7, V, 3, TCAP)] == [0] * 6
    assert q(L.F32, V, B, TCAP) == 1 and q(L.BF16, 65536, 8, 128) == 1
    assert call() == 0                                                                 # the same call inside the envelope runs
    torch.cuda.synchronize()
    assert last.ge(0).all()
    with pytest.raises(ValueError, match="envelope"):
        T.k_beam_select(logits, tb["cum"], tb["fin"], tb["len"], tb["ids"], tb["anc"], last, ws, 0, N, B, V + 1, EOS)


# ---- attention ------------------------------------------------------------------------------------------------------------
def row_grouped(q, kv, mask, N, group, Lk, H):
    """The raw entry point (the wrapper routes group = 1 to hero_dec_attention_row)."""
    from hero_amd import _lib as L
    D, es = H * 64, q.element_size()
    out = torch.empty((N, D), dtype=q.dtype, device=q.device)
    p = L.ptr(kv)
    L.check(L.lib().hero_dec_attention_row_grouped(L.ptr(q), p, p + D * es, L.ptr(mask), L.ptr(out), N, group, Lk, H, D, 2 * D, 0.125,
                                                   L.dt(q), L.stream()))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Lk", [1, 20, 128])
@pytest.mark.parametrize("group", [1, 3, 8])
def test_grouped_row_attention_equals_the_row_kernel_on_replicated_keys(group, Lk, dtype):
    from hero_amd import tvc as T
    nb, H = 3, 2
    N, D = nb * group, H * 64
    g = torch.Generator().manual_seed(500 + 10 * group + Lk)
    q = torch.randn(N, D, generator=g).to(dtype).cuda()
    kv = torch.randn(nb * Lk, 2 * D, generator=g).to(dtype).cuda()
    valid = torch.tensor([Lk, max(1, Lk // 3), max(1, Lk - 1)])
    mask = ((torch.arange(Lk).unsqueeze(0) >= valid.unsqueeze(1)).float() * -10000.0).cuda()
    kv_rep = kv.view(nb, Lk, 2 * D).repeat_interleave(group, dim=0).reshape(N * Lk, 2 * D).contiguous()
    want = T.k_dec_attn_row(q, kv_rep, mask.repeat_interleave(group, dim=0).contiguous(), N, Lk, H)
    assert torch.equal(row_grouped(q, kv, mask, N, group, Lk, H), want)
    assert torch.equal(T.k_dec_attn_row(q, kv, mask, N, Lk, H, group=group), want)
    assert torch.equal(row_grouped(q, kv, None, N, group, Lk, H), T.k_dec_attn_row(q, kv_rep, None, N, Lk, H))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("t", [0, 1, 63, 64, 127])
def test_beam_step_attention_equals_the_step_kernel_on_a_gathered_cache(t, dtype):
    from hero_amd import tvc as T
    nb, B, H, Tcap = 2, 3, 2, 128
    N, D = nb * B, H * 64
    g = torch.Generator().manual_seed(700 + t)
    qkv = torch.randn(N, 3 * D, generator=g).to(dtype).cuda()
    cache = torch.randn(N, Tcap, 2 * D, generator=g).to(dtype).cuda()
    pos = torch.tensor([t], dtype=torch.int32, device="cuda")
    own = torch.arange(N, dtype=torch.int32).unsqueeze(1).repeat(1, Tcap).cuda()
    # the identity table: the step kernel itself, cache contents included
    c0, c1 = cache.clone(), cache.clone()
    want = T.k_dec_attn_step(qkv, c0, pos, N, H)
    assert torch.equal(T.k_dec_attn_step(qkv, c1, pos, N, H, anc=own), want) and torch.equal(c0, c1)
    # a random in-caption ancestry against the same kernel on a cache gathered to match
    anc = ((torch.arange(N).unsqueeze(1) // B) * B + torch.randint(0, B, (N, Tcap), generator=g)).int().cuda()
    flat = (anc.long() * Tcap + torch.arange(Tcap, device="cuda").unsqueeze(0)).view(-1)
    gathered = cache.view(N * Tcap, 2 * D).index_select(0, flat).view(N, Tcap, 2 * D).contiguous()
    want = T.k_dec_attn_step(qkv, gathered, pos, N, H)
    c2 = cache.clone()
    assert torch.equal(T.k_dec_attn_step(qkv, c2, t, N, H, anc=anc), want)             # the host position, too
    expect = cache.clone()
    expect[:, t] = qkv[:, D:]                                                          # only position t of the row's OWN cache row changes
    assert torch.equal(c2, expect) and torch.equal(gathered[:, t], qkv[:, D:])
    # entries outside [0, N) are clamped into it
    wild, clamped = anc.clone(), anc.clone()
    wild[0, :], clamped[0, :] = -5, 0
    wild[N - 1, :], clamped[N - 1, :] = N + 7, N - 1
    assert torch.equal(T.k_dec_attn_step(qkv, cache.clone(), pos, N, H, anc=wild), T.k_dec_attn_step(qkv, cache.clone(), pos, N, H, anc=clamped))


def test_beam_attention_argument_errors():
    from hero_amd import _lib as L
    from hero_amd import tvc as T
    q = torch.zeros(6, 64, device="cuda")
    kv = torch.zeros(2 * 4, 128, device="cuda")
    with pytest.raises(ValueError, match="whole number of groups"):
        T.k_dec_attn_row(q, kv, None, 6, 4, 1, group=4)
    assert L.lib().hero_dec_attention_row_grouped(L.ptr(q), L.ptr(kv), L.ptr(kv) + 256, None, L.ptr(q), 6, 0, 4, 1, 64, 128, C.c_float(0.125),
                                                  L.F32, L.stream()) == -1
    assert b"hero_dec_attention_row_grouped" in L.lib().hero_last_error()
    qkv, cache = torch.zeros(6, 192, device="cuda"), torch.zeros(6, 8, 128, device="cuda")
    assert L.lib().hero_dec_attention_step_beam(L.ptr(qkv), L.ptr(cache), None, L.ptr(q), None, 0, 6, 8, 1, C.c_float(0.125), L.F32,
                                                L.stream()) == -1
    assert b"hero_dec_attention_step_beam" in L.lib().hero_last_error()
    with pytest.raises(ValueError, match="anc"):
        T.k_dec_attn_step(qkv, cache, 0, 6, 1, anc=torch.zeros(6, 7, dtype=torch.int32, device="cuda"))
