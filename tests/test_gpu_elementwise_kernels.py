"""hero_add, hero_relu_bwd, hero_gelu_bwd and hero_cast (hero_amd/csrc/rows.hip) through the raw ctypes entry points, in f32 and
bf16: the kernels that share the `n >> 2` float4 body, the 2048-workgroup grid cap and (hero_cast) the `n & 3` tail.

Sizes: 4 (one float4), 1000 (a partial workgroup), 2 * 2097152 + 8 (every thread of the capped grid takes a second grid-stride
trip, and two more quads follow); hero_cast also 1, 2, 3, 5, 1001 and 2 * 2097152 + 3 for its tail.  n = 6 is refused by the
three n % 4 == 0 entries.  Inputs are drawn once in the kernel's dtype and widened for the reference; every output lives between
64 sentinel elements on each side, and the inputs are bit-unchanged after the launch.

    hero_add       exact in f32 (one fp32 addition = torch's); in bf16 the fp32 sum rounded once (= torch's bf16 addition)
    hero_relu_bwd  exact: dy where y > 0, else 0; y holds +0.0, -0.0, the smallest positive subnormal and normal of the dtype
    hero_gelu_bwd  dy * gelu'(u) against the float64 erf form (optim_reference.gelu_grad_ref); u uniform over [-8, 8] plus 0, +-30
    hero_cast      bit-equal to tensor.to(dtype) for all four dtype pairs: round-to-nearest-even ties, fp32 subnormals, +-inf, +-0;
                   NaN stays NaN

Tolerance of hero_gelu_bwd (the rule of tests/test_gpu_violin_kernels.py; nothing is taken from a kernel's output): the
element-wise error (tests.util.elem_rel_err) of PyTorch's own fp32 `dy * gelu'(u)` (autograd of F.gelu, fp32, same inputs, on
the GPU) against the float64 form, worst over the cases, times 4, floored at 16 * 2^-24 = 9.54e-7; the bf16-stored output adds
its rounding: per element |a - b| <= 2^-8 |b| + TOL * rms(b).  Every gelu test prints the kernel's and PyTorch-fp32's figures (-s).

Measured on an AMD Instinct MI355X (gfx950), ROCm PyTorch, this file's inputs:

    output   worst PyTorch-fp32 error (case)                          x 4        TOL
    gelu     2.003e-07  (n = 2 * 2097152 + 8, fp32)                     8.01e-07   9.54e-07 (the floor)

The kernel's own worst figure in the same run, for the record (it is not where the constant comes from): 2.2e-07 in fp32
(bf16-stored: 3.3e-03 = its rounding, inside the bf16 bound).
"""
import pytest
import torch
import torch.nn.functional as F

from tests import optim_reference as R
from tests.util import elem_rel_err

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
MEASURED = {"gelu": 2.003e-7}             # worst PyTorch-fp32 figure over the cases (the table above), times 4, floored
TOL = {k: max(FLOOR, 4 * v) for k, v in MEASURED.items()}

G = 64
SENT = -776.0                          # exact in fp32 and bf16
BIG = 2 * 2097152
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
SIZES = [4, 1000, BIG + 8]
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


@pytest.fixture(scope="module")
def HF():
    from hero_amd import functional
    return functional


@pytest.fixture(scope="module")
def Lb():
    from hero_amd import _lib
    _lib.lib()
    return _lib


def bits(t):
    return t.contiguous().view(INT[t.dtype])


def guarded(n, dtype):
    """(buffer, the n-element output view inside it): G sentinels on each side, the view pre-filled with sentinels too."""
    buf = torch.full((n + 2 * G,), SENT, dtype=dtype, device="cuda")
    return buf, buf[G:G + n]


def intact(buf, n):
    return bool((buf[:G] == SENT).all()) and bool((buf[G + n:] == SENT).all())


def run3(Lb, fn, a, b):
    """out <- fn(a, b) for one of the three two-input entries; checks the guards and that the inputs are unchanged."""
    n = a.numel()
    a0, b0 = a.clone(), b.clone()
    buf, out = guarded(n, a.dtype)
    Lb.check(fn(a.data_ptr(), b.data_ptr(), out.data_ptr(), n, Lb.dt(a), Lb.stream()))
    torch.cuda.synchronize()
    assert intact(buf, n) and torch.equal(bits(a), bits(a0)) and torch.equal(bits(b), bits(b0))
    return out


def draw(n, dtype, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=gen) * scale).to(dtype).cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", SIZES)
def test_add(Lb, n, dtype):
    a, b = draw(n, dtype, 100 + n % 97), draw(n, dtype, 200 + n % 97, scale=3.0)
    out = run3(Lb, Lb.lib().hero_add, a, b)
    want = (a.cpu().float() + b.cpu().float()).to(dtype)  # one IEEE fp32 addition on the CPU; bf16: that sum rounded once
    assert torch.equal(bits(out.cpu()), bits(want))
    assert torch.equal(bits(out), bits(a + b))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", SIZES)
def test_relu_bwd(Lb, n, dtype):
    dy, y = draw(n, dtype, 300 + n % 97), draw(n, dtype, 400 + n % 97)
    edge = torch.tensor([0.0, -0.0, 0.0, torch.finfo(dtype).tiny], dtype=dtype)
    edge[2:3] = torch.tensor([1], dtype=INT[dtype]).view(dtype)                   # the smallest subnormal: bit pattern 1
    edge = edge.cuda()
    y[:4] = edge
    if n > 8:
        y[-4:] = edge.flip(0)
    assert bits(y)[1].item() != 0 and y[2].item() > 0                              # -0.0 and the subnormal arrived as such
    out = run3(Lb, Lb.lib().hero_relu_bwd, dy, y)
    want = torch.where(y.cpu().double() > 0, dy.cpu().double(), torch.zeros((), dtype=torch.float64)).to(dtype)
    assert torch.equal(bits(out.cpu()), bits(want))
    assert out[0].item() == 0 and out[1].item() == 0 and torch.equal(bits(out[2:4]), bits(dy[2:4]))


def gelu_inputs(n, dtype):
    gen = torch.Generator().manual_seed(500 + n % 97)
    u = torch.rand(n, generator=gen) * 16.0 - 8.0
    u[:3] = torch.tensor([0.0, 30.0, -30.0])
    if n > 8:
        u[-3:] = torch.tensor([-30.0, 30.0, 0.0])
    return torch.randn(n, generator=gen).to(dtype).cuda(), u.to(dtype).cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", SIZES)
def test_gelu_bwd(Lb, n, dtype):
    dy, u = gelu_inputs(n, dtype)
    out = run3(Lb, Lb.lib().hero_gelu_bwd, dy, u)
    ref = dy.double().cpu() * R.gelu_grad_ref(u)
    uf = u.float().clone().requires_grad_(True)
    F.gelu(uf).backward(dy.float())
    ek, et = elem_rel_err(out, ref), elem_rel_err(uf.grad, ref)
    if dtype == torch.bfloat16:
        a = out.double().cpu()
        ok = bool(((a - ref).abs() <= 2.0 ** -8 * ref.abs() + TOL["gelu"] * ref.pow(2).mean().sqrt()).all())
    else:
        ok = ek <= TOL["gelu"]
    print("\n[elementwise] gelu_bwd/n%d/%s kernel %.3e  torch-fp32 %.3e  tol %.3e %s" % (n, IDS[DTYPES.index(dtype)], ek, et, TOL["gelu"], "" if ok else "MISS"), end="")
    assert bool(torch.isfinite(out.float()).all())
    assert out[0].item() == 0.5 * dy[0].item()                                    # gelu'(0) = 1/2 exactly
    assert out[1].item() == dy[1].item() and out[2].item() == 0                   # gelu'(+-30) = 1, 0 in fp32
    assert ok, (ek, TOL["gelu"])


@pytest.mark.parametrize("entry", ["hero_add", "hero_relu_bwd", "hero_gelu_bwd"])
def test_n_not_a_multiple_of_4_is_an_error(Lb, entry):
    a = torch.ones(8, device="cuda")
    out = torch.full((8,), 9.0, device="cuda")
    for dtype in (Lb.F32, Lb.BF16):
        assert getattr(Lb.lib(), entry)(a.data_ptr(), a.data_ptr(), out.data_ptr(), 6, dtype, Lb.stream()) != 0
        assert entry in Lb.lib().hero_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())                                               # nothing was launched


CODE = {torch.float32: 0, torch.bfloat16: 1}


def cast_inputs(n, dtype):
    """Random values over many binades with the edge values cycled through the first and the last elements (so that the
    float4 body and the scalar tail both see them)."""
    gen = torch.Generator().manual_seed(600 + n % 97)
    x = torch.randn(n, generator=gen) * torch.exp(torch.rand(n, generator=gen) * 40.0 - 20.0)
    edge = torch.tensor([1.00390625, 1.01171875, -1.00390625, -1.01171875,         # ties between two bf16: to the even one
                         1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23, # one fp32 ulp off a tie
                         1.0e-40, -1.0e-40, 2.0 ** -149, 2.0 ** -134 + 2.0 ** -149,  # fp32 subnormals (bf16's smallest is 2^-133)
                         float("inf"), -float("inf"), 0.0, -0.0, 3.4028234663852886e38, float("nan")])   # fp32's largest: rounds up to bf16 inf
    k = min(n, edge.numel())
    x[:k] = edge[:k]
    if n > 2 * edge.numel():
        x[-edge.numel():] = edge.flip(0)
    return x.to(dtype).cuda()


@pytest.mark.parametrize("dst", DTYPES, ids=["to_fp32", "to_bf16"])
@pytest.mark.parametrize("src", DTYPES, ids=["from_fp32", "from_bf16"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 1001, BIG + 3])
def test_cast(Lb, n, src, dst):
    x = cast_inputs(n, src)
    x0 = x.clone()
    buf, out = guarded(n, dst)
    Lb.check(Lb.lib().hero_cast(x.data_ptr(), out.data_ptr(), n, CODE[src], CODE[dst], Lb.stream()))
    torch.cuda.synchronize()
    assert intact(buf, n) and torch.equal(bits(x), bits(x0))
    want = x.cpu().to(dst).cuda()                                                 # the CPU conversion: round to nearest even
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(out), nan)                                     # NaN stays NaN (its payload is not compared)
    assert torch.equal(bits(out)[~nan], bits(want)[~nan])
    if n >= 16 and src == torch.float32:
        assert int(nan.sum()) >= 1 and bool(torch.isinf(want).any()) and int((want == 0).sum()) >= 2
