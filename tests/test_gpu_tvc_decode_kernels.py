"""hero_dec_attention_row / hero_dec_attention_step (hero_amd/csrc/dec_attention.hip): one query row per (caption, head) against
the encoder keys or against a growing key/value cache, through hero_amd.tvc.k_dec_attn_row / k_dec_attn_step and the raw ctypes
entry points, against the float64 restatement tests/tvc_reference.attention (cross cases with Lq = 1; step cases as the causal
attention over L = t + 1 rows, of which row t is taken).

Step cases (N, H, cached keys t, Tcap) - the smallest shapes that reach each failure mode:

    (1, 1, 0, 1)        empty cache, degenerate
    (3, 2, 6, 8)        below a wave
    (5, 2, 10, 16)      N * H = 10, a partial workgroup
    (2, 3, 63, 64)      exactly one wave of keys
    (2, 1, 64, 128)     one key past a wave
    (2, 2, 127, 128)    last row of the envelope
    (2, 12, 29, 30)     the recipe

Cross cases (N, H, Lk, key mask):

    (1, 1, 1, none)     degenerate
    (3, 2, 9, ragged)   ragged lengths down to ONE valid key
    (2, 1, 65, ragged)  one key past a wave
    (2, 12, 100, ragged)  the recipe
    (2, 2, 128, ragged)   corner of the envelope
    (4, 2, 33, last caption fully masked, equal key rows, distinct value rows)

Both dtypes.  Inputs are drawn once in the kernel's dtype and the same rounded values go to the reference, so only the arithmetic
is judged.  The masks are ADDITIVE: the fully masked caption keeps softmax of its shifted scores, the uniform distribution for its
equal key rows, and ctx is the mean of V.

Tolerance (the rule of tests/test_gpu_tvc_kernels.py; nothing is taken from the kernel's output): the element-wise error
(tests.util.elem_rel_err) of the fp32 PyTorch formulation (model/tvc.py's ops, fp32, same inputs, on the GPU) against the float64
restatement, worst over this file's cases x dtypes, times 4, floored at 16 * 2^-24 = 9.54e-7.  bf16-stored ctx: per element
|a - b| <= 2^-8 |b| + TOL * rms(b).  Every test prints the kernel's and PyTorch-fp32's figures (-s).

Measured on an AMD Instinct MI355X (gfx950), ROCm PyTorch, this file's inputs:

    output     worst PyTorch-fp32 error (case)                      x 4        TOL
    ctx        1.510e-06  (cross recipe, fp32 (2, 12, 100, ragged))   6.04e-06   6.04e-06

(the worst step case is the recipe, fp32 (2, 12, 29, 30), at 1.172e-06; the steps of the sequence test stay below both).  The
kernel's own worst figure in the same run, for the record (it is not where the constant comes from): 1.635e-06 in fp32, the same
cross recipe case; bf16-stored ctx 2.5e-03 = 0.65 x 2^-8.
"""
import pytest
import torch

from tests import tvc_reference as R
from tests.util import elem_rel_err

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
MEASURED_CTX = 1.510e-6     # worst PyTorch-fp32 figure over the cases x dtypes (the table above)
TOL = max(FLOOR, 4 * MEASURED_CTX)
SENTINEL = 77.0             # exact in both dtypes

STEP_CASES = {  # (N, H, cached keys t, Tcap)
    "empty": (1, 1, 0, 1),
    "below_wave": (3, 2, 6, 8),
    "partial_group": (5, 2, 10, 16),
    "one_wave": (2, 3, 63, 64),
    "past_wave": (2, 1, 64, 128),
    "last_row": (2, 2, 127, 128),
    "recipe": (2, 12, 29, 30),
}
CROSS_CASES = {  # (N, H, Lk, key mask: None | "ragged" | "full" = last caption fully masked)
    "degenerate": (1, 1, 1, None),
    "ragged_small": (3, 2, 9, "ragged"),
    "past_wave": (2, 1, 65, "ragged"),
    "recipe": (2, 12, 100, "ragged"),
    "corner": (2, 2, 128, "ragged"),
    "fully_masked": (4, 2, 33, "full"),
}
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
_CACHE = {}


def key_lengths(N, Lk, how):
    """Valid keys per caption.  "ragged": all Lk for the first caption, then fewer - a third with two captions, down to a SINGLE
    key for the last of three or more.  "full": the last caption has none."""
    if how is None:
        return None
    if how == "full":
        return [Lk - 3 * n for n in range(N - 1)] + [0]
    if N == 2:
        return [Lk, max(1, Lk // 3)]
    return [Lk - (n * (Lk - 1)) // (N - 1) for n in range(N)]


def torch_attention_fp32(q, k, v, N, Lq, Lk, H, mask_add, causal):
    """model/tvc.py:67-104 / BertSelfAttention under tri_mask in fp32 on the GPU -> ctx [N*Lq, H*64]."""
    def split(x, L):
        return x.float().reshape(N, L, H, 64).permute(0, 2, 1, 3)
    s = torch.matmul(split(q, Lq), split(k, Lk).transpose(-1, -2)) / 8.0
    if mask_add is not None:
        s = s + mask_add.reshape(N, 1, 1, Lk)
    if causal:
        tri = torch.tril(torch.ones(Lq, Lk, device=q.device), diagonal=0)
        s = s + ((1.0 - tri) * -10000.0).unsqueeze(0).unsqueeze(1)
    return torch.matmul(torch.softmax(s, dim=-1), split(v, Lk)).permute(0, 2, 1, 3).reshape(N * Lq, H * 64)


def step_data(name, dtype):
    """Inputs, the float64 restatement and the PyTorch-fp32 result of a step case: computed once, shared, never modified.
    qkv [N, 3D] is the step's packed row, hist [N, t, 2D] the K|V of the cached positions; the reference sees the L = t + 1 rows
    (queries of the earlier rows are drawn too, only row t is compared)."""
    key = ("step", name, dtype)
    if key not in _CACHE:
        N, H, t, Tcap = STEP_CASES[name]
        D, L = H * 64, t + 1
        g = torch.Generator().manual_seed(6000 + 13 * len(name) + t)
        qkv = torch.randn(N, 3 * D, generator=g).to(dtype).cuda()
        hist = torch.randn(N, t, 2 * D, generator=g).to(dtype).cuda()
        q_early = torch.randn(N, t, D, generator=g).to(dtype).cuda()
        q = torch.cat([q_early, qkv[:, None, :D]], dim=1).reshape(N * L, D)
        k = torch.cat([hist[:, :, :D], qkv[:, None, D:2 * D]], dim=1).reshape(N * L, D)
        v = torch.cat([hist[:, :, D:], qkv[:, None, 2 * D:]], dim=1).reshape(N * L, D)
        ref = R.attention(q, k, v, N, L, L, H, causal=True)["ctx"].view(N, L, D)[:, t]
        t32 = torch_attention_fp32(q, k, v, N, L, L, H, None, True).view(N, L, D)[:, t]
        _CACHE[key] = dict(qkv=qkv, hist=hist, ref=ref, t32=t32, dims=(N, H, t, Tcap))
    return _CACHE[key]


def fresh_cache(c, dtype, tail=None):
    """[N, Tcap, 2D]: the cached positions, the sentinel (or `tail`) in the rows from t on."""
    N, H, t, Tcap = c["dims"]
    cache = torch.full((N, Tcap, 2 * H * 64), SENTINEL, dtype=dtype, device="cuda")
    if tail is not None:
        cache[:, t:] = tail
    cache[:, :t] = c["hist"]
    return cache


def cross_data(name, dtype):
    key = ("cross", name, dtype)
    if key not in _CACHE:
        N, H, Lk, how = CROSS_CASES[name]
        D = H * 64
        g = torch.Generator().manual_seed(7000 + 7 * len(name) + Lk)
        q = torch.randn(N, D, generator=g).to(dtype)
        k, v = (torch.randn(N * Lk, D, generator=g).to(dtype) for _ in range(2))
        lens = key_lengths(N, Lk, how)
        mask_add = None
        if lens is not None:
            m = torch.zeros(N, Lk)
            for n, ln in enumerate(lens):
                m[n, :ln] = 1
            mask_add = ((1 - m) * -10000.0).cuda()
            if how == "full":
                k.view(N, Lk, -1)[-1] = k.view(N, Lk, -1)[-1, :1]                 # the key bias, Lk times
        q, k, v = q.cuda(), k.cuda(), v.cuda()
        ref = R.attention(q, k, v, N, 1, Lk, H, key_mask_add=mask_add)["ctx"]
        t32 = torch_attention_fp32(q, k, v, N, 1, Lk, H, mask_add, False)
        _CACHE[key] = dict(q=q, k=k, v=v, mask_add=mask_add, lens=lens, ref=ref, t32=t32, dims=(N, H, Lk))
    return _CACHE[key]


def run_cross(c, k=None, v=None):
    from hero_amd.tvc import k_dec_attn_row
    N, H, Lk = c["dims"]
    kv = torch.cat([c["k"] if k is None else k, c["v"] if v is None else v], dim=1).contiguous()
    return k_dec_attn_row(c["q"], kv, c["mask_add"], N, Lk, H)


def judge(case, got, ref, t32):
    ek, et = elem_rel_err(got, ref), elem_rel_err(t32, ref)
    if got.dtype == torch.bfloat16:
        a, b = got.detach().double().cpu(), ref.double().cpu()
        ok = bool(((a - b).abs() <= 2.0 ** -8 * b.abs() + TOL * b.pow(2).mean().sqrt()).all())
    else:
        ok = ek <= TOL
    print("\n[tvc-decode] %-28s kernel %.3e  torch-fp32 %.3e  tol %.3e %s" % (case, ek, et, TOL, "" if ok else "MISS"), end="")
    return ok, ek


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_step_against_float64_and_the_cache_row_it_writes(name, dtype):
    from hero_amd.tvc import k_dec_attn_step
    c = step_data(name, dtype)
    N, H, t, Tcap = c["dims"]
    D = H * 64
    cache = fresh_cache(c, dtype)
    before = cache.clone()
    ctx = k_dec_attn_step(c["qkv"], cache, t, N, H)
    assert ctx.dtype == dtype and tuple(ctx.shape) == (N, D)
    ok, _ = judge("step/%s/%s" % (name, IDS[DTYPES.index(dtype)]), ctx, c["ref"], c["t32"])
    assert ok
    # exact: row t holds the K|V columns of qkv, every other row is what it was (the sentinel behind t)
    assert torch.equal(cache[:, t], c["qkv"][:, D:])
    assert torch.equal(cache[:, :t], before[:, :t]) and torch.equal(cache[:, t + 1:], before[:, t + 1:])
    assert bool((cache[:, t + 1:].float() == SENTINEL).all())
    # exact: a device position gives the bits of the host position, and a second run the bits of the first
    pos = torch.tensor([t], dtype=torch.int32, device="cuda")
    cache2 = fresh_cache(c, dtype)
    ctx2 = k_dec_attn_step(c["qkv"], cache2, pos, N, H)
    assert torch.equal(ctx, ctx2) and torch.equal(cache, cache2)
    assert torch.equal(ctx, k_dec_attn_step(c["qkv"], fresh_cache(c, dtype), t, N, H))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_step_does_not_see_cache_rows_behind_its_position(dtype):
    """Exact: other random values in the cache rows > t leave ctx bit-identical."""
    from hero_amd.tvc import k_dec_attn_step
    for name in ("below_wave", "partial_group", "past_wave"):
        c = step_data(name, dtype)
        N, H, t, Tcap = c["dims"]
        g = torch.Generator().manual_seed(21)
        tail = torch.randn(N, Tcap - t, 2 * H * 64, generator=g).to(dtype).cuda()
        a = k_dec_attn_step(c["qkv"], fresh_cache(c, dtype), t, N, H)
        b = k_dec_attn_step(c["qkv"], fresh_cache(c, dtype, tail), t, N, H)
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_sequence_of_steps_from_an_empty_cache(dtype):
    """T = 12 steps with the device position incremented between the launches: every step's ctx against row t of the float64
    causal attention over the T rows, and the final cache equal to K|V bit for bit."""
    from hero_amd.tvc import k_dec_attn_step
    N, H, T = 3, 2, 12
    D = H * 64
    g = torch.Generator().manual_seed(31)
    qkv = torch.randn(N, T, 3 * D, generator=g).to(dtype).cuda()
    q, k, v = (qkv[:, :, i * D:(i + 1) * D].reshape(N * T, D) for i in range(3))
    ref = R.attention(q, k, v, N, T, T, H, causal=True)["ctx"].view(N, T, D)
    t32 = torch_attention_fp32(q, k, v, N, T, T, H, None, True).view(N, T, D)
    cache = torch.full((N, T, 2 * D), SENTINEL, dtype=dtype, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    bad = []
    for t in range(T):
        ctx = k_dec_attn_step(qkv[:, t].contiguous(), cache, pos, N, H)
        pos.add_(1)
        ok, _ = judge("sequence/%s/t%d" % (IDS[DTYPES.index(dtype)], t), ctx, ref[:, t], t32[:, t])
        if not ok:
            bad.append(t)
        assert bool((cache[:, t + 1:].float() == SENTINEL).all())
    assert not bad, bad
    assert torch.equal(cache, qkv[:, :, D:])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(CROSS_CASES))
def test_cross_row_against_float64(name, dtype):
    c = cross_data(name, dtype)
    N, H, Lk = c["dims"]
    ctx = run_cross(c)
    assert ctx.dtype == dtype and tuple(ctx.shape) == (N, H * 64)
    ok, _ = judge("cross/%s/%s" % (name, IDS[DTYPES.index(dtype)]), ctx, c["ref"], c["t32"])
    assert ok
    assert torch.equal(ctx, run_cross(c))                                         # two runs: the same bits


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_masked_keys_do_not_reach_the_output(dtype):
    """Exact: changing the K / V rows of masked keys leaves ctx bit-identical (captions with at least one valid key)."""
    for name in ("ragged_small", "past_wave", "recipe", "corner"):
        c = cross_data(name, dtype)
        N, H, Lk = c["dims"]
        g = torch.Generator().manual_seed(12)
        k2, v2 = c["k"].clone().view(N, Lk, -1), c["v"].clone().view(N, Lk, -1)
        for n, ln in enumerate(c["lens"]):
            k2[n, ln:] = torch.randn(Lk - ln, H * 64, generator=g).to(dtype).cuda()
            v2[n, ln:] = torch.randn(Lk - ln, H * 64, generator=g).to(dtype).cuda()
        assert not torch.equal(k2, c["k"].view(N, Lk, -1))
        assert torch.equal(run_cross(c), run_cross(c, k=k2.view(N * Lk, -1), v=v2.view(N * Lk, -1)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fully_masked_caption_gives_the_mean_of_v(dtype):
    c = cross_data("fully_masked", dtype)
    N, H, Lk = c["dims"]
    got = run_cross(c)[-1:]
    mean_v = c["v"].view(N, Lk, -1)[-1].double().mean(0, keepdim=True).cpu()
    err = elem_rel_err(got, mean_v)
    print("\n[tvc-decode] fully_masked/%s mean-of-V error %.3e  tol %.3e" % (IDS[DTYPES.index(dtype)], err, TOL), end="")
    if dtype == torch.bfloat16:
        assert bool(((got.double().cpu() - mean_v).abs() <= 2.0 ** -8 * mean_v.abs() + TOL * mean_v.pow(2).mean().sqrt()).all())
    else:
        assert err <= TOL


def test_guards_are_error_codes_without_a_launch():
    from hero_amd import _lib as Lb
    from hero_amd import tvc
    lib = Lb.lib()
    z = torch.zeros(129 * 128, device="cuda")
    cache = torch.full((130 * 128,), 9.0, device="cuda")
    out = torch.full((64,), 9.0, device="cuda")
    p, cp, o, st = Lb.ptr(z), Lb.ptr(cache), Lb.ptr(out), Lb.stream()
    for N, Tcap, pos, dtype in ((1, 129, 0, Lb.F32), (1, 8, 8, Lb.F32), (1, 8, -1, Lb.BF16), (0, 8, 0, Lb.F32), (1, 0, 0, Lb.F32),
                                (1, 8, 0, 7)):
        assert lib.hero_dec_attention_step(p, cp, o, None, pos, N, Tcap, 1, 0.125, dtype, st) == -1, (N, Tcap, pos, dtype)
        assert lib.hero_last_error()
    for N, Lk, ldq, ldkv, dtype in ((1, 129, 64, 128, Lb.F32), (1, 0, 64, 128, Lb.BF16), (0, 8, 64, 128, Lb.F32), (1, 8, 64, 128, 7),
                                    (1, 8, 60, 128, Lb.F32), (1, 8, 64, 32, Lb.F32)):
        assert lib.hero_dec_attention_row(p, p, p, None, o, N, Lk, 1, ldq, ldkv, 0.125, dtype, st) == -1, (N, Lk, ldq, ldkv, dtype)
    assert lib.hero_dec_attention_step(None, cp, o, None, 0, 1, 8, 1, 0.125, Lb.F32, st) == -1                 # null operand
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()) and bool((cache == 9.0).all())                # nothing was launched
    q, c8 = torch.zeros(2, 192, device="cuda"), torch.zeros(2, 8, 128, device="cuda")
    with pytest.raises(ValueError, match="envelope"):
        tvc.k_dec_attn_step(q, torch.zeros(2, 129, 128, device="cuda"), 0, 2, 1)
    with pytest.raises(ValueError, match="position"):
        tvc.k_dec_attn_step(q, c8, 8, 2, 1)
    with pytest.raises(ValueError, match="position"):
        tvc.k_dec_attn_step(q, c8, torch.zeros(1, dtype=torch.int64, device="cuda"), 2, 1)
    with pytest.raises(ValueError, match="cache"):
        tvc.k_dec_attn_step(q, c8.bfloat16(), 0, 2, 1)
    with pytest.raises(ValueError, match="envelope"):
        tvc.k_dec_attn_row(torch.zeros(1, 64, device="cuda"), torch.zeros(129, 128, device="cuda"), None, 1, 129, 1)
    with pytest.raises(ValueError, match="key mask"):
        tvc.k_dec_attn_row(torch.zeros(1, 64, device="cuda"), torch.zeros(8, 128, device="cuda"), torch.zeros(1, 9, device="cuda"), 1, 8, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bad", ["Tcap", "minus_one"])
def test_a_device_position_outside_the_cache_writes_zeros_and_no_row(dtype, bad):
    """The cache is allocated with two spare sentinel rows per caption and Tcap passed as the logical size: a wrong guard shows as
    a changed sentinel instead of a write outside the allocation."""
    from hero_amd import _lib as Lb
    N, H, Tcap = 3, 2, 6
    D = H * 64
    g = torch.Generator().manual_seed(41)
    qkv = torch.randn(N, 3 * D, generator=g).to(dtype).cuda()
    # one leading spare block as well, so that row -1 of caption 0 is inside the allocation too
    store = torch.full((1 + N, Tcap + 2, 2 * D), SENTINEL, dtype=dtype, device="cuda")
    cache = store[1:]
    ctx = torch.full((N, D), 9.0, dtype=dtype, device="cuda")
    pos = torch.tensor([Tcap if bad == "Tcap" else -1], dtype=torch.int32, device="cuda")
    Lb.check(Lb.lib().hero_dec_attention_step(Lb.ptr(qkv), cache.data_ptr(), Lb.ptr(ctx), Lb.ptr(pos), 0, N, Tcap, H, 0.125, Lb.dt(qkv),
                                              Lb.stream()))
    torch.cuda.synchronize()
    assert bool((store.float() == SENTINEL).all())
    assert bool((ctx.float() == 0.0).all())
