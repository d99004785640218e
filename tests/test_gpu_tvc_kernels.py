"""hero_dec_attention_fwd / _bwd (hero_amd/csrc/dec_attention.hip) and hero_smooth_ce_fwd / _bwd (hero_amd/csrc/loss.hip) through
hero_amd.tvc and through the raw ctypes entry points, against the float64 restatements of tests/tvc_reference.py.

Attention cases (N, Lq, Lk, H, causal, key mask) - the smallest shapes that reach each failure mode:

    (3, 7, 7, 2, causal, none)        below a tile
    (2, 33, 33, 2, causal, none)      one past 32
    (2, 64, 64, 3, causal, none)      the causal corner
    (1, 1, 1, 1, causal, none)        degenerate
    (3, 5, 9, 2, no, ragged)          ragged key lengths, one caption with a single valid key
    (2, 30, 100, 12, no, ragged)      the recipe
    (2, 64, 128, 2, no, ragged)       the corner of the envelope
    (2, 1, 65, 1, no, ragged)         a single query row, one key past a wave
    (4, 17, 33, 2, no, one caption fully masked)

Causal cases run in both operand forms (one fused [N*L, 3*H*64] buffer; a [N*L, H*64] query and a [N*L, 2*H*64] key/value
buffer, which must give the same bits); the others have Lq != Lk and exist in the separate form only.  Both dtypes.  Inputs are
drawn once in the kernel's input dtype and the same rounded values go to the reference, so only the arithmetic is judged.

The masks are ADDITIVE (model/tvc.py:130-133, 184-185).  softmax is shift invariant, so a caption whose keys are all masked
keeps softmax(scores) over its Lk keys; that is the uniform distribution - and ctx the mean of V - when its key rows are equal,
which is what the model produces (the encoder rows of an empty segment are zero padding and all project to the key bias).  The
fully masked caption of this file has equal key rows and distinct value rows.

Loss cases (rows, cols, ld): (1, 8, 8), (5, 160, 160), (3, 1000, 1024) with the padding columns filled with 3e4, (7, 50272, 50272);
mixed ignored rows, eps in {0.1, 1.0}.

Tolerance (the rule of tests/test_gpu_violin_kernels.py; nothing is taken from a kernel's output): the element-wise error
(tests.util.elem_rel_err) of the fp32 PyTorch formulation (model/tvc.py's ops and autograd, fp32, same inputs, on the GPU) against
the float64 restatement, worst over this file's cases x dtypes, times 4, floored at 16 * 2^-24 = 9.54e-7.  bf16-stored outputs
(ctx, dq, dk, dv, dlogits in bf16): per element |a - b| <= 2^-8 |b| + TOL * rms(b).  dlogits is a sum of terms that cancel
(softmax - s - ...); it is judged element-wise like the rest, the rms floor of elem_rel_err carries the cancelling elements.
Every test prints the kernel's and PyTorch-fp32's figures (-s).

Measured on an AMD Instinct MI355X (gfx950), ROCm PyTorch, this file's inputs:

    output     worst PyTorch-fp32 error (case)                      x 4        TOL
    ctx        1.535e-06  (recipe,  fp32 (2, 30, 100, 12))           6.14e-06   6.14e-06
    dq         1.643e-06  (recipe,  fp32 (2, 30, 100, 12))           6.57e-06   6.57e-06
    dk         3.458e-06  (corner,  fp32 (2, 64, 128, 2))            1.38e-05   1.38e-05
    dv         1.848e-06  (corner,  fp32 (2, 64, 128, 2))            7.39e-06   7.39e-06
    loss       1.201e-07  (C160,    fp32 (5, 160, 160), eps 1)       4.80e-07   9.54e-07 (the floor)
    dlogits    2.082e-06  (vocab,   fp32 (7, 50272, 50272), eps 1)   8.33e-06   8.33e-06

The kernels' own worst figures in the same run, for the record (they are not where the constants come from): ctx 1.5e-06,
dq 1.5e-06, dk 4.0e-06, dv 2.2e-06 in fp32, loss 8.0e-08, dlogits 6.5e-07 in fp32.
"""
import pytest
import torch

from tests import tvc_reference as R
from tests.util import elem_rel_err

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
# worst PyTorch-fp32 figure per output over the cases x dtypes (the table above), times 4, floored
MEASURED = {"ctx": 1.535e-6, "dq": 1.643e-6, "dk": 3.458e-6, "dv": 1.848e-6, "loss": 1.201e-7, "dlogits": 2.082e-6}
TOL = {k: max(FLOOR, 4 * v) for k, v in MEASURED.items()}

ATTN_CASES = {  # (N, Lq, Lk, H, causal, key mask: None | "ragged" | "full" = last caption fully masked)
    "below_tile": (3, 7, 7, 2, True, None),
    "L33": (2, 33, 33, 2, True, None),
    "causal_corner": (2, 64, 64, 3, True, None),
    "degenerate": (1, 1, 1, 1, True, None),
    "ragged_small": (3, 5, 9, 2, False, "ragged"),
    "recipe": (2, 30, 100, 12, False, "ragged"),
    "corner": (2, 64, 128, 2, False, "ragged"),
    "one_query": (2, 1, 65, 1, False, "ragged"),
    "fully_masked": (4, 17, 33, 2, False, "full"),
}
LOSS_CASES = {  # (rows, cols, ld)
    "C8": (1, 8, 8),
    "C160": (5, 160, 160),
    "C1000_ld1024": (3, 1000, 1024),
    "vocab": (7, 50272, 50272),
}
EPS = [0.1, 1.0]
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


def torch_attention_fp32(q, k, v, N, Lq, Lk, H, mask_add, causal, dctx):
    """model/tvc.py:67-104 / BertSelfAttention under tri_mask in fp32 on the GPU, with autograd."""
    def split(x, L):
        return x.float().reshape(N, L, H, 64).permute(0, 2, 1, 3).clone().requires_grad_(True)
    qh, kh, vh = split(q, Lq), split(k, Lk), split(v, Lk)
    s = torch.matmul(qh, kh.transpose(-1, -2)) / 8.0
    if mask_add is not None:
        s = s + mask_add.reshape(N, 1, 1, Lk)
    if causal:
        tri = torch.tril(torch.ones(Lq, Lk, device=q.device), diagonal=0)
        s = s + ((1.0 - tri) * -10000.0).unsqueeze(0).unsqueeze(1)
    ctx = torch.matmul(torch.softmax(s, dim=-1), vh).permute(0, 2, 1, 3).reshape(N * Lq, H * 64)
    (ctx * dctx.float()).sum().backward()
    back = lambda g, L: g.permute(0, 2, 1, 3).reshape(N * L, H * 64)      # noqa: E731
    return {"ctx": ctx.detach(), "dq": back(qh.grad, Lq), "dk": back(kh.grad, Lk), "dv": back(vh.grad, Lk)}


def attn_data(name, dtype):
    """Inputs, the float64 restatement and the PyTorch-fp32 results of a case: computed once, shared, never modified."""
    key = ("attn", name, dtype)
    if key not in _CACHE:
        N, Lq, Lk, H, causal, how = ATTN_CASES[name]
        g = torch.Generator().manual_seed(4000 + 7 * len(name) + Lk)
        q, k, v, dctx = (torch.randn(N * L, H * 64, generator=g).to(dtype) for L in (Lq, Lk, Lk, Lq))
        lens = key_lengths(N, Lk, how)
        mask_add = None
        if lens is not None:
            m = torch.zeros(N, Lk)
            for n, ln in enumerate(lens):
                m[n, :ln] = 1
            mask_add = ((1 - m) * -10000.0).cuda()
            if how == "full":
                k.view(N, Lk, -1)[-1] = k.view(N, Lk, -1)[-1, :1]                 # the key bias, Lk times
        q, k, v, dctx = q.cuda(), k.cuda(), v.cuda(), dctx.cuda()
        ref = R.attention(q, k, v, N, Lq, Lk, H, key_mask_add=mask_add, causal=causal, dctx=dctx)
        t32 = torch_attention_fp32(q, k, v, N, Lq, Lk, H, mask_add, causal, dctx)
        _CACHE[key] = dict(q=q, k=k, v=v, dctx=dctx, mask_add=mask_add, lens=lens, ref=ref, t32=t32, dims=(N, Lq, Lk, H, causal))
    return _CACHE[key]


def run_attention(c, form, drop=None, q=None, k=None, v=None):
    """Forward and backward through DecAttnCoreFn in one operand form -> ctx, dq, dk, dv in the row layout of the operands."""
    from hero_amd.tvc import DecAttnCoreFn
    N, Lq, Lk, H, causal = c["dims"]
    D = H * 64
    q, k, v = (c["q"] if q is None else q), (c["k"] if k is None else k), (c["v"] if v is None else v)
    if form == "fused":
        buf = torch.cat([q, k, v], dim=1).requires_grad_(True)
        out = DecAttnCoreFn.apply(buf, None, c["mask_add"], N, Lq, Lk, H, causal, drop)
        out.backward(c["dctx"])
        return out.detach(), buf.grad[:, :D], buf.grad[:, D:2 * D], buf.grad[:, 2 * D:]
    qb, kvb = q.clone().requires_grad_(True), torch.cat([k, v], dim=1).requires_grad_(True)
    out = DecAttnCoreFn.apply(qb, kvb, c["mask_add"], N, Lq, Lk, H, causal, drop)
    out.backward(c["dctx"])
    return out.detach(), qb.grad, kvb.grad[:, :D], kvb.grad[:, D:]


def forms(c):
    return ("fused", "separate") if c["dims"][1] == c["dims"][2] else ("separate",)


class Report:
    def __init__(self, case):
        self.case, self.bad = case, []

    def tensor(self, group, name, got, ref, t32):
        ek, et, tol = elem_rel_err(got, ref), elem_rel_err(t32, ref), TOL[group]
        if got.dtype == torch.bfloat16:
            a, b = got.detach().double().cpu(), ref.double().cpu()
            ok = bool(((a - b).abs() <= 2.0 ** -8 * b.abs() + tol * b.pow(2).mean().sqrt()).all())
        else:
            ok = ek <= tol
        print("\n[tvc] %-28s %-8s kernel %.3e  torch-fp32 %.3e  tol %.3e %s" % (self.case, name, ek, et, tol, "" if ok else "MISS"), end="")
        if not ok:
            self.bad.append((name, ek, tol))

    def done(self):
        assert not self.bad, (self.case, self.bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(ATTN_CASES))
def test_attention_against_float64(name, dtype):
    c = attn_data(name, dtype)
    ref, t32 = c["ref"], c["t32"]
    r = Report("%s/%s" % (name, IDS[DTYPES.index(dtype)]))
    first = None
    for form in forms(c):
        got = run_attention(c, form)
        if first is None:
            first = got
            for key, x in zip(("ctx", "dq", "dk", "dv"), got):
                assert x.dtype == dtype
                r.tensor(key, key, x, ref[key], t32[key])
        else:
            for x, y in zip(first, got):                                          # the operand form changes addresses only
                assert torch.equal(x, y)
    r.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_causal_rows_do_not_see_later_keys(dtype):
    """Exact: changing K / V rows > i leaves the output rows <= i bit-identical (what greedy decoding over a fixed id buffer
    relies on)."""
    for name in ("below_tile", "L33", "causal_corner"):
        c = attn_data(name, dtype)
        N, L, _, H, _ = c["dims"]
        i = L // 2
        g = torch.Generator().manual_seed(11)
        k2, v2 = c["k"].clone().view(N, L, -1), c["v"].clone().view(N, L, -1)
        k2[:, i + 1:] = torch.randn(N, L - i - 1, H * 64, generator=g).to(dtype).cuda()
        v2[:, i + 1:] = torch.randn(N, L - i - 1, H * 64, generator=g).to(dtype).cuda()
        a = run_attention(c, "fused")[0].view(N, L, -1)
        b = run_attention(c, "fused", k=k2.view(N * L, -1), v=v2.view(N * L, -1))[0].view(N, L, -1)
        assert torch.equal(a[:, :i + 1], b[:, :i + 1])
        assert not torch.equal(a[:, i + 1:], b[:, i + 1:])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_masked_keys_do_not_reach_the_output(dtype):
    """Exact: changing the K / V rows of masked keys leaves ctx bit-identical (captions with at least one valid key)."""
    for name in ("ragged_small", "recipe", "one_query"):
        c = attn_data(name, dtype)
        N, Lq, Lk, H, _ = c["dims"]
        g = torch.Generator().manual_seed(12)
        k2, v2 = c["k"].clone().view(N, Lk, -1), c["v"].clone().view(N, Lk, -1)
        for n, ln in enumerate(c["lens"]):
            k2[n, ln:] = torch.randn(Lk - ln, H * 64, generator=g).to(dtype).cuda()
            v2[n, ln:] = torch.randn(Lk - ln, H * 64, generator=g).to(dtype).cuda()
        assert not torch.equal(k2, c["k"].view(N, Lk, -1))
        a = run_attention(c, "separate")[0]
        b = run_attention(c, "separate", k=k2.view(N * Lk, -1), v=v2.view(N * Lk, -1))[0]
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fully_masked_caption_attends_uniformly(dtype):
    c = attn_data("fully_masked", dtype)
    N, Lq, Lk, H, _ = c["dims"]
    ctx, dq, dk, dv = run_attention(c, "separate")
    mean_v = c["v"].view(N, Lk, -1)[-1].double().mean(0).cpu()
    got = ctx.view(N, Lq, -1)[-1]
    err = elem_rel_err(got, mean_v.expand(Lq, -1))
    print("\n[tvc] fully_masked/%s mean-of-V error %.3e  tol %.3e" % (IDS[DTYPES.index(dtype)], err, TOL["ctx"]), end="")
    if dtype == torch.bfloat16:
        b = mean_v.expand(Lq, -1)
        assert bool(((got.double().cpu() - b).abs() <= 2.0 ** -8 * b.abs() + TOL["ctx"] * b.pow(2).mean().sqrt()).all())
    else:
        assert err <= TOL["ctx"]
    for x in (dq, dk, dv):
        assert bool(torch.isfinite(x.float()).all())
    # uniform attention: every key of that caption receives the same share of dctx, dV[j] = sum_i dctx[i] / Lk
    want = c["dctx"].view(N, Lq, -1)[-1].double().sum(0).cpu() / Lk
    assert elem_rel_err(dv.view(N, Lk, -1)[-1].float(), want.expand(Lk, -1)) <= (2.0 ** -8 if dtype == torch.bfloat16 else TOL["dv"])


def _drop(p, site, seed_tensor):
    from hero_amd import _lib as Lb
    return Lb.Dropout(seed_tensor.data_ptr(), site, max(1, int(round(p * 65536.0))), 1.0 / (1.0 - p))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dropout_is_replayed_by_the_backward(dtype):
    """Same site: same bits.  Another site: another mask.  With the multipliers restated from the counter-based draw
    (tests/tvc_reference.dropout_multipliers) forward and backward match the float64 restatement; and the adjoint identity
    <dctx, ctx(V)> == <dV, V> holds (ctx is linear in V for a fixed mask), as in test_attention_dropout_adjoint."""
    seed = torch.tensor([20240607], dtype=torch.int64, device="cuda")
    for name in ("L33", "recipe"):
        c = attn_data(name, dtype)
        N, Lq, Lk, H, causal = c["dims"]
        form = forms(c)[0]
        d7, d8 = _drop(0.25, 7, seed), _drop(0.25, 8, seed)
        a, b, other, plain = run_attention(c, form, d7), run_attention(c, form, d7), run_attention(c, form, d8), run_attention(c, form)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert not torch.equal(a[0], other[0]) and not torch.equal(a[0], plain[0])
        mult = R.dropout_multipliers(20240607, 7, d7.threshold16, 1.0 / 0.75, N, H, Lq, Lk)
        assert abs(float((mult > 0).double().mean()) - 0.75) < 0.03
        ref = R.attention(c["q"], c["k"], c["v"], N, Lq, Lk, H, key_mask_add=c["mask_add"], causal=causal, mult=mult, dctx=c["dctx"])
        r = Report("dropout/%s/%s" % (name, IDS[DTYPES.index(dtype)]))
        for key, x in zip(("ctx", "dq", "dk", "dv"), a):
            r.tensor(key, key, x, ref[key], c["t32"][key])                         # the fp32 column is the run WITHOUT dropout
        r.done()
        lhs = float((c["dctx"].double() * a[0].double()).sum())
        rhs = float((a[3].double() * c["v"].double()).sum())
        size = float((c["dctx"].double() * a[0].double()).abs().sum())             # what is summed
        bound = (2.0 ** -8 if dtype == torch.bfloat16 else TOL["dv"]) * size
        print("\n[tvc] adjoint/%s/%s |lhs - rhs| %.3e  bound %.3e" % (name, IDS[DTYPES.index(dtype)], abs(lhs - rhs), bound), end="")
        assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attention_two_runs_are_bitwise_equal(dtype):
    for name in ("L33", "recipe", "corner"):
        c = attn_data(name, dtype)
        for x, y in zip(run_attention(c, forms(c)[0]), run_attention(c, forms(c)[0])):
            assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attention_backward_writes_every_element(dtype):
    """The raw entry points on sentinel-filled outputs: nothing of dq / dk / dv (or ctx, stats) keeps the sentinel, and the
    upstream gradient is read from the device buffer given (a scaled dctx scales the three gradients)."""
    from hero_amd import _lib as Lb
    c = attn_data("ragged_small", dtype)
    N, Lq, Lk, H, causal = c["dims"]
    D = H * 64
    q, kv = c["q"], torch.cat([c["k"], c["v"]], dim=1).contiguous()
    es = q.element_size()
    ctx, stats = torch.full((N * Lq, D), 77.0, dtype=dtype, device="cuda"), torch.full((N, H, Lq, 2), 77.0, device="cuda")
    args = (N, Lq, Lk, H, D, 2 * D, 0, 0.125, Lb.dt(q), None, Lb.stream())
    Lb.check(Lb.lib().hero_dec_attention_fwd(Lb.ptr(q), Lb.ptr(kv), Lb.ptr(kv) + D * es, Lb.ptr(c["mask_add"]), Lb.ptr(ctx), Lb.ptr(stats), *args))
    assert int((ctx.float() == 77.0).sum()) == 0 and int((stats == 77.0).sum()) == 0
    outs = []
    for scale in (1.0, 0.25):
        dctx = (c["dctx"].float() * scale).to(dtype)
        dq, dkv = torch.full_like(q, 77.0), torch.full_like(kv, 77.0)
        Lb.check(Lb.lib().hero_dec_attention_bwd(Lb.ptr(q), Lb.ptr(kv), Lb.ptr(kv) + D * es, Lb.ptr(c["mask_add"]), Lb.ptr(stats), Lb.ptr(dctx),
                                                 Lb.ptr(dq), Lb.ptr(dkv), Lb.ptr(dkv) + D * es, *args))
        assert int((dq.float() == 77.0).sum()) == 0 and int((dkv.float() == 77.0).sum()) == 0
        outs.append((dq, dkv))
    r = Report("raw/%s" % IDS[DTYPES.index(dtype)])
    r.tensor("dq", "dq", outs[0][0], c["ref"]["dq"], c["t32"]["dq"])
    r.tensor("dq", "dq/4", outs[1][0], c["ref"]["dq"] * 0.25, c["t32"]["dq"] * 0.25)      # 0.25 is exact in both dtypes
    r.tensor("dk", "dk/4", outs[1][1][:, :D], c["ref"]["dk"] * 0.25, c["t32"]["dk"] * 0.25)
    r.tensor("dv", "dv/4", outs[1][1][:, D:], c["ref"]["dv"] * 0.25, c["t32"]["dv"] * 0.25)
    r.done()


def test_attention_outside_the_envelope_is_an_error_code():
    from hero_amd import _lib as Lb
    from hero_amd import tvc
    z = torch.zeros(64, device="cuda")
    out = torch.full((64,), 9.0, device="cuda")
    p, o = Lb.ptr(z), Lb.ptr(out)
    for N, Lq, Lk, H, ldq, ldkv, dtype in ((1, 65, 8, 1, 64, 64, Lb.F32), (1, 8, 129, 1, 64, 64, Lb.F32), (1, 0, 8, 1, 64, 64, Lb.F32),
                                          (1, 8, 0, 1, 64, 64, Lb.BF16), (1, 8, 8, 0, 64, 64, Lb.F32), (-1, 8, 8, 1, 64, 64, Lb.F32),
                                          (1, 8, 8, 1, 64, 64, 7)):
        assert Lb.lib().hero_dec_attention_in_envelope(dtype, Lq, Lk) == int(dtype in (Lb.F32, Lb.BF16) and 1 <= Lq <= 64 and 1 <= Lk <= 128)
        assert Lb.lib().hero_dec_attention_fwd(p, p, p, None, o, o, N, Lq, Lk, H, ldq, ldkv, 0, 0.125, dtype, None, Lb.stream()) == -1
        assert "envelope" in Lb.lib().hero_last_error().decode()
        assert Lb.lib().hero_dec_attention_bwd(p, p, p, None, p, p, o, o, o, N, Lq, Lk, H, ldq, ldkv, 0, 0.125, dtype, None, Lb.stream()) == -1
    # leading dimensions below H * 64 or not a multiple of 8
    assert Lb.lib().hero_dec_attention_fwd(p, p, p, None, o, o, 1, 8, 8, 2, 64, 128, 0, 0.125, Lb.F32, None, Lb.stream()) == -1
    assert Lb.lib().hero_dec_attention_fwd(p, p, p, None, o, o, 1, 8, 8, 1, 68, 64, 0, 0.125, Lb.F32, None, Lb.stream()) == -1
    assert Lb.lib().hero_dec_attention_fwd(p, p, p, None, o, o, 0, 8, 8, 1, 64, 64, 0, 0.125, Lb.F32, None, Lb.stream()) == 0   # N == 0: no launch
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())                                               # nothing was launched
    assert not tvc.in_envelope(torch.float32, 65, 8) and tvc.in_envelope(torch.bfloat16, 64, 128)
    with pytest.raises(ValueError, match="envelope"):
        tvc.DecAttnCoreFn.apply(torch.zeros(65, 192, device="cuda"), None, None, 1, 65, 65, 1, True, None)


# ---- the smoothed loss ---------------------------------------------------------------------------------------------------------
def torch_loss_fp32(x, labels, eps, w):
    """LabelSmoothingLoss (model/tvc.py:42-64) in fp32 on the GPU with autograd -> losses of all rows (0 at ignored ones), dx."""
    x = x.float().clone().requires_grad_(True)
    valid = labels != -1
    loss = torch.zeros(x.shape[0], device=x.device)
    if bool(valid.any()):
        vl = R.smooth_loss_kl(x, labels, eps)
        (vl * w[valid]).sum().backward()
        loss[valid] = vl.detach()
    return {"loss": loss, "dx": x.grad if x.grad is not None else torch.zeros_like(x)}


def loss_data(name, dtype, eps):
    key = ("loss", name, dtype, eps)
    if key not in _CACHE:
        rows, cols, ld = LOSS_CASES[name]
        g = torch.Generator().manual_seed(5000 + cols)
        x = (torch.randn(rows, ld, generator=g) * 3.0).to(dtype)
        x[:, cols:] = 3.0e4                                                       # padding columns: large, and must not matter
        labels = torch.randint(0, cols, (rows,), generator=g)
        labels[0] = cols - 1
        if rows > 2:
            labels[1] = -1                                                        # mixed ignored rows
            labels[rows - 1] = 0
        w = torch.rand(rows, generator=g) + 0.5
        x, labels, w = x.cuda(), labels.cuda(), w.cuda()
        ref = R.smooth_loss(x[:, :cols], labels, eps, dloss_rows=w)
        _CACHE[key] = dict(x=x, labels=labels, w=w, ref=ref, t32=torch_loss_fp32(x[:, :cols], labels, eps, w), dims=(rows, cols, ld))
    return _CACHE[key]


def run_loss(c, eps, alias=False):
    """The raw entry points; `alias` lets dlogits overwrite a copy of the logits."""
    from hero_amd import _lib as Lb
    rows, cols, ld = c["dims"]
    x = c["x"].clone()
    loss, lse, sc = (torch.full((n,), 55.0, device="cuda") for n in (rows, rows, 2))
    Lb.check(Lb.lib().hero_smooth_ce_fwd(Lb.ptr(x), Lb.ptr(c["labels"]), Lb.ptr(loss), Lb.ptr(lse), Lb.ptr(sc), rows, cols, ld, Lb.dt(x),
                                         eps, -1, Lb.stream()))
    dx = x if alias else torch.full_like(x, 55.0)
    one = torch.ones(1, device="cuda")
    Lb.check(Lb.lib().hero_smooth_ce_bwd(Lb.ptr(x), Lb.ptr(c["labels"]), Lb.ptr(lse), Lb.ptr(one), Lb.ptr(c["w"]), None, Lb.ptr(dx), rows, cols,
                                         ld, Lb.dt(x), eps, -1, Lb.stream()))
    return loss, sc, dx


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_smooth_loss_against_float64(name, dtype, eps):
    c = loss_data(name, dtype, eps)
    rows, cols, ld = c["dims"]
    ref, t32 = c["ref"], c["t32"]
    loss, sc, dx = run_loss(c, eps)
    r = Report("%s/%s/eps%g" % (name, IDS[DTYPES.index(dtype)], eps))
    r.tensor("loss", "loss", loss, ref["loss"], t32["loss"])
    r.tensor("loss", "sum", sc[:1], ref["sum"].reshape(1), t32["loss"].sum().reshape(1))
    assert sc[1].item() == ref["count"]
    assert dx.dtype == dtype and int((dx.float() == 55.0).sum()) == 0
    assert int((dx[:, cols:] != 0).sum()) == 0                                    # padding columns: zero gradient
    assert int((dx[c["labels"] == -1] != 0).sum()) == 0 and int((loss[c["labels"] == -1] != 0).sum()) == 0
    r.tensor("dlogits", "dlogits", dx[:, :cols], ref["dx"], t32["dx"])
    r.done()
    again = run_loss(c, eps)                                                       # bitwise repeatability
    aliased = run_loss(c, eps, alias=True)                                         # dlogits aliasing logits
    for x, y, z in zip((loss, sc, dx), again, aliased):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_smooth_loss_nodes_and_mean_mode(dtype):
    """SmoothCeFn returns the raw kernels' rows and pair; SmoothCeMeanFn is the mean over the VALID rows with the count read on
    the device (an upstream of 0.5 is read from the device too)."""
    from hero_amd import tvc
    eps = 0.1
    c = loss_data("C160", dtype, eps)
    rows, cols, ld = c["dims"]
    raw_loss, raw_sc, raw_dx = run_loss(c, eps)
    x = c["x"].clone().requires_grad_(True)
    loss, sc = tvc.smooth_ce(x, c["labels"], eps, ncols=cols)
    (loss * c["w"]).sum().backward()
    assert torch.equal(loss.detach(), raw_loss) and torch.equal(sc.detach(), raw_sc) and torch.equal(x.grad, raw_dx)
    x2 = c["x"].clone().requires_grad_(True)
    mean = tvc.smooth_ce_mean(x2, c["labels"], eps, ncols=cols)
    (mean * 0.5).backward()
    ref = R.smooth_loss(c["x"][:, :cols], c["labels"], eps, mean=True, upstream=0.5)
    r = Report("mean/%s" % IDS[DTYPES.index(dtype)])
    want = (ref["sum"] / ref["count"]).reshape(1)
    r.tensor("loss", "mean", mean.detach().reshape(1), want, (c["t32"]["loss"].sum() / ref["count"]).reshape(1))
    t32 = torch_loss_fp32(c["x"][:, :cols], c["labels"], eps, torch.full((rows,), 0.5 / ref["count"], device="cuda"))
    r.tensor("dlogits", "dlogits", x2.grad[:, :cols], ref["dx"], t32["dx"])
    r.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_smooth_loss_with_every_row_ignored(dtype):
    from hero_amd import tvc
    x = torch.randn(4, 160, device="cuda").to(dtype).requires_grad_(True)
    labels = torch.full((4,), -1, dtype=torch.long, device="cuda")
    mean = tvc.smooth_ce_mean(x, labels, 0.1)
    mean.backward()
    assert mean.item() == 0.0 and int((x.grad != 0).sum()) == 0
    loss, sc = tvc.smooth_ce(x.detach(), labels, 0.1)
    assert sc.tolist() == [0.0, 0.0] and int((loss != 0).sum()) == 0


@pytest.mark.parametrize("eps", EPS)
def test_smooth_loss_of_large_logits_stays_finite(eps):
    """|x| = 3e4 (a bf16 number): the row maximum is subtracted before the exponentials."""
    for dtype in DTYPES:
        x = torch.full((3, 1000), -3.0e4, device="cuda")
        x[0, 5], x[1, 7], x[2, ::2] = 3.0e4, 3.0e4, 3.0e4
        x = x.to(dtype)
        labels = torch.tensor([5, 8, 0], device="cuda")                           # right, wrong, one of many
        c = dict(x=x, labels=labels, w=torch.ones(3, device="cuda"), dims=(3, 1000, 1000))
        loss, sc, dx = run_loss(c, eps)
        ref = R.smooth_loss(x, labels, eps)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(sc).all()) and bool(torch.isfinite(dx.float()).all())
        err = elem_rel_err(loss, ref["loss"])
        print("\n[tvc] large/%s/eps%g loss error %.3e  tol %.3e" % (IDS[DTYPES.index(dtype)], eps, err, TOL["loss"]), end="")
        assert err <= TOL["loss"]


def test_smooth_loss_bad_arguments_are_error_codes():
    from hero_amd import _lib as Lb
    z = torch.zeros(64, device="cuda")
    lab = torch.zeros(4, dtype=torch.long, device="cuda")
    out = torch.full((64,), 9.0, device="cuda")
    p, o, lb = Lb.ptr(z), Lb.ptr(out), Lb.ptr(lab)
    for rows, cols, ld, dtype, eps in ((2, 8, 4, Lb.F32, 0.1), (2, 1, 8, Lb.F32, 0.1), (2, 8, 8, 7, 0.1), (2, 8, 8, Lb.F32, 0.0),
                                       (2, 8, 8, Lb.F32, 1.5), (-1, 8, 8, Lb.F32, 0.1)):
        assert Lb.lib().hero_smooth_ce_fwd(p, lb, o, o, o, rows, cols, ld, dtype, eps, -1, Lb.stream()) == -1, (rows, cols, ld, dtype, eps)
        assert Lb.lib().hero_smooth_ce_bwd(p, lb, p, p, None, None, o, rows, cols, ld, dtype, eps, -1, Lb.stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())
