"""hero_sumsq, hero_adamw and hero_adamw_multi (hero_amd/csrc/rows.hip) through the raw ctypes ABI, and hero_amd.optim.AdamW
called directly, against the float64 restatement of tests/optim_reference.py (held against oracle.hero_oracle.adamw_step and
clip_grad_norm_ by tests/test_cpu_optim_reference.py).

Inputs are drawn once in fp32 and the same values, widened, go to the restatement - the hyper-parameters too: they cross the ABI
as C floats, and the restatement gets the float the kernel was handed (optim_reference.f32).  Every tensor a kernel touches lives
inside a larger buffer with 64 sentinel elements on each side; after each launch the sentinels of p, m, v (and shadow) and the
whole of g are bit-unchanged.  Gradient magnitudes are log-uniform over [1e-8, 10] with random sign, every 13th element exactly 0.

hero_adamw_multi: ONE launch over ten tensors of 1, 3, 4, 5, 16383, 16384, 16385, 2 * 16384 + 7, 33000 and 16384 + 6 elements
(one 16384-element chunk per workgroup; remainders 0 - 3 for the scalar tail; the last tensor's p, g, m, v start one float past
a 16-byte boundary: the kernel's scalar branch), three hyper-parameter groups that differ in every field, step 7 with lags
0 / 3 / 6 (lag 6: tensor step 1 from m = v = 0, where eps decides the update for |g| <~ eps), every other tensor p = 0 exactly
(the update is judged without cancellation against a weight of size 1), chunks listed in a fixed shuffled order.
hero_adamw: n in {1, 3, 4, 5, 1000, 2 * 2097152 + 5} (the last: a second grid-stride trip for every thread, and a tail), steps
1 and 7, with / without clipping + grad_scale, with / without the bf16 shadow.  hero_sumsq: n in {0, 1, 3, 4, 5, 1023, 33000,
2 * 2097152 + 3} of N(0,1) plus one 1e3 outlier among 1e-3 values.  hero_sumsq and hero_adamw read float4 with no fallback: a
misaligned pointer is an argument error before any launch, and no test launches them on one.

Tolerance (the rule of tests/test_gpu_violin_kernels.py; nothing is taken from a kernel's output): the element-wise error
(tests.util.elem_rel_err) of the fp32 PyTorch restatement of the same formulas (`adamw_t32`: fp32 tensors and fp32 scalars, same
inputs, on the GPU) against the float64 restatement, worst over this file's cases, times 4, floored at 16 * 2^-24 = 9.54e-7.
`dp` is p on the tensors / elements that start from p = 0.  Every test prints the kernel's and PyTorch-fp32's figures (-s).

Measured on an AMD Instinct MI355X (gfx950), ROCm PyTorch, this file's inputs:

    output   worst PyTorch-fp32 error (case)                          x 4        TOL
    dp       9.570e-07  (multi/tensor_steps call 2, n = 16383)          3.83e-06   3.83e-06
    m        2.896e-07  (multi/clip, n = 16390)                         1.16e-06   1.16e-06
    v        2.268e-07  (multi/clip, n = 16385)                         9.07e-07   9.54e-07 (the floor)
    p        2.096e-07  (class/eager4, the 16385-element parameter)     8.38e-07   9.54e-07 (the floor)
    sumsq    3.534e-08  (n = 3, two calls)                              1.41e-07   9.54e-07 (the floor)

The kernels' own worst figures in the same run, for the record (they are not where the constants come from):
dp 9.6e-07, m 2.9e-07, v 2.3e-07, p 2.1e-07, sumsq 3.4e-08.  The library is built with -ffp-contract=off and fp32 division and
square root are correctly rounded on both sides, so the kernels and the PyTorch-fp32 restatement agree to all printed digits.
"""
import ctypes as C
import math

import pytest
import torch

from tests import optim_reference as R
from tests.util import elem_rel_err

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
# worst PyTorch-fp32 figure per output over this file's cases (the table above), times 4, floored
MEASURED = {"p": 2.096e-7, "dp": 9.570e-7, "m": 2.896e-7, "v": 2.268e-7, "sumsq": 3.534e-8}
TOL = {k: max(FLOOR, 4 * v) for k, v in MEASURED.items()}

G = 64                                  # sentinel elements on each side of every tensor
SENT = -776.0                           # exact in fp32 and bf16; no kernel result of this file equals it
BIG = 2 * 2097152                       # grid_for caps at 2048 workgroups x 256 threads x 4 elements = 2097152


@pytest.fixture(scope="module")
def HF():
    from hero_amd import functional
    return functional


@pytest.fixture(scope="module")
def Lb():
    from hero_amd import _lib
    _lib.lib()
    return _lib


class Guarded:
    """A device tensor of src's values inside a larger buffer: G sentinels before and after; `off` shifts the start by that
    many elements (off = 1: one float past a 16-byte boundary)."""

    def __init__(self, src, off=0, dtype=torch.float32):
        n = src.numel()
        self.buf = torch.full((n + 2 * G + off,), SENT, dtype=dtype, device="cuda")
        self.lo, self.n = G + off, n
        self.t = self.buf[self.lo:self.lo + n]
        self.t.copy_(src.to(dtype))
        assert self.buf.data_ptr() % 256 == 0 and self.t.data_ptr() % 16 == (off * self.buf.element_size()) % 16

    def intact(self):
        return bool((self.buf[:self.lo] == SENT).all()) and bool((self.buf[self.lo + self.n:] == SENT).all())

    def ptr(self):
        return self.t.data_ptr()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def t32(x):
    return torch.tensor(x, dtype=torch.float32, device="cuda")


def adamw_t32(p, g, m, v, step, lr, beta1, beta2, eps, wd, gscale):
    """The PyTorch-fp32 restatement: optim_reference.adamw_ref's formulas on fp32 GPU tensors with fp32 scalars (gscale: an fp32
    device scalar)."""
    p, g, m, v = (x.detach().float().cuda() for x in (p, g, m, v))
    lr, b1, b2, eps, wd, st = t32(lr), t32(beta1), t32(beta2), t32(eps), t32(wd), t32(float(step))
    g = g * gscale
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr * torch.sqrt(1.0 - torch.pow(b2, st)) / (1.0 - torch.pow(b1, st)) * m / (v.sqrt() + eps)
    p = p - lr * wd * p
    return p, m, v


def clip_t32(sumsq, max_norm, grad_scale):
    """optim_reference.clip_scale in fp32 on the GPU (sumsq: an fp32 device scalar)."""
    norm = sumsq.sqrt() * abs(grad_scale)
    return t32(grad_scale) * torch.clamp(t32(max_norm) / (norm + 1e-6), max=1.0)


class Report:
    def __init__(self, case):
        self.case, self.bad = case, []

    def tensor(self, group, name, got, ref, tf32, mask=None):
        ek, et = elem_rel_err(got, ref, mask), elem_rel_err(tf32, ref, mask)
        ok = ek <= TOL[group]
        print("\n[optim] %-34s %-6s %-5s kernel %.3e  torch-fp32 %.3e  tol %.3e %s" % (self.case, name, group, ek, et, TOL[group], "" if ok else "MISS"), end="")
        if not ok:
            self.bad.append((name, ek, TOL[group]))

    def done(self):
        assert not self.bad, (self.case, self.bad)


def sumsq_of(Lb, tensors, ws=None):
    """hero_sumsq over device tensors (16-byte aligned), accumulated into one fresh scalar."""
    out = torch.zeros(1, device="cuda")
    ws = torch.empty(2048, device="cuda") if ws is None else ws
    for t in tensors:
        Lb.check(Lb.lib().hero_sumsq(t.data_ptr(), t.numel(), out.data_ptr(), ws.data_ptr(), Lb.stream()))
    torch.cuda.synchronize()
    return out


# ---- hero_adamw_multi --------------------------------------------------------------------------------------------------
_CASE = []


def case():
    if not _CASE:
        _CASE.append(R.multi_case())
    return _CASE[0]


SLOTS = [(3 * i + 1) % 16 for i in range(len(R.MULTI_SIZES))]     # distinct slots in a 16-entry counter table


class MultiRun:
    """The tensors of a case on the device (guarded), the descriptor table and the shuffled chunk lists."""

    def __init__(self, Lb, tensors, slots=False):
        self.Lb, self.tensors = Lb, tensors
        self.dev = []
        for i, t in enumerate(tensors):
            off = 1 if i == R.MISALIGNED else 0
            self.dev.append({k: Guarded(t[k], off) for k in "pgmv"})
        descs = (Lb.TensorDesc * len(tensors))()
        chunks = []
        for i, (t, d) in enumerate(zip(tensors, self.dev)):
            descs[i] = Lb.TensorDesc(d["p"].ptr(), d["g"].ptr(), d["m"].ptr(), d["v"].ptr(), t["n"], t["group"], SLOTS[i] if slots else t["lag"])
            chunks += [(i, c) for c in range(-(-t["n"] // R.CHUNK))]
        assert Lb.lib().hero_adamw_multi_chunk() == R.CHUNK
        order = torch.randperm(len(chunks), generator=torch.Generator().manual_seed(99)).tolist()
        chunks = [chunks[j] for j in order]
        assert chunks != sorted(chunks)
        self.descs = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
        self.ct = torch.tensor([c[0] for c in chunks], dtype=torch.int32).cuda()
        self.ci = torch.tensor([c[1] for c in chunks], dtype=torch.int32).cuda()
        self.n_chunks = len(chunks)

    def launch(self, step=R.MULTI_STEP, sumsq=None, max_grad_norm=0.0, grad_scale=1.0, step_ptr=None, lr_ptr=None, lr_mul=1.0,
               tsteps=None, n_chunks=None):
        Lb = self.Lb
        a = Lb.AdamWMulti()
        a.descs, a.chunk_tensor, a.chunk_index = self.descs.data_ptr(), self.ct.data_ptr(), self.ci.data_ptr()
        a.n_chunks = self.n_chunks if n_chunks is None else n_chunks
        for gi, (lr, b1, b2, eps, wd) in enumerate(R.GROUPS):
            a.groups[gi] = Lb.AdamWGroup(lr * lr_mul, b1, b2, eps, wd)
        for gi in range(len(R.GROUPS), 8):
            a.groups[gi] = Lb.AdamWGroup(float("nan"), float("nan"), float("nan"), float("nan"), float("nan"))   # never indexed
        a.step = step
        a.grad_sumsq, a.max_grad_norm, a.grad_scale = Lb.ptr(sumsq), max_grad_norm, grad_scale
        a.step_ptr, a.lr_ptr, a.tensor_steps, a.n_tensors = Lb.ptr(step_ptr), Lb.ptr(lr_ptr), Lb.ptr(tsteps), len(self.tensors)
        rc = Lb.lib().hero_adamw_multi(C.byref(a), Lb.stream())
        torch.cuda.synchronize()
        return rc

    def guards_ok(self):
        for t, d in zip(self.tensors, self.dev):
            assert d["p"].intact() and d["m"].intact() and d["v"].intact() and d["g"].intact(), t["n"]
            assert same_bits(d["g"].t.cpu(), t["g"]), t["n"]                    # g is read-only

    def out(self, i):
        return tuple(self.dev[i][k].t.clone() for k in "pmv")

    def grads(self):
        """The gradients as 16-byte aligned device tensors (hero_sumsq's contract): the misaligned one is copied."""
        return [d["g"].t if d["g"].ptr() % 16 == 0 else d["g"].t.clone() for d in self.dev]


def judge_multi(name, run, gscale=1.0, gscale32=None, steps=None, tensors=None):
    """Every tensor of the run against the restatement with the tensor's own step, its group's hyper-parameters and `gscale`."""
    tensors = run.tensors if tensors is None else tensors
    gscale32 = t32(gscale) if gscale32 is None else gscale32
    r = Report(name)
    for i, t in enumerate(tensors):
        hp = R.group_f32(t["group"])
        step = t["step"] if steps is None else steps[i]
        ref = R.adamw_ref(t["p"], t["g"], t["m"], t["v"], step, *hp, gscale=gscale)
        tf = adamw_t32(t["p"], t["g"], t["m"], t["v"], step, *hp, gscale=gscale32)
        got = run.out(i)
        tag = "n%d" % t["n"]
        r.tensor("dp" if t["p0"] else "p", tag, got[0], ref[0], tf[0])
        r.tensor("m", tag, got[1], ref[1], tf[1])
        r.tensor("v", tag, got[2], ref[2], tf[2])
    run.guards_ok()
    r.done()


def true_sumsq():
    return sum(R.sumsq_ref(t["g"]) for t in case())


def test_multi_no_clipping_ignores_the_threshold(Lb):
    run = MultiRun(Lb, case())
    assert run.launch(sumsq=None, max_grad_norm=0.5) == 0
    judge_multi("multi/no_sumsq", run)


@pytest.mark.parametrize("grad_scale", [1.0, 0.125], ids=["clip", "clip_scaled"])
def test_multi_clipping_that_clips(Lb, grad_scale):
    """norm = sqrt(sumsq) * |grad_scale| is about 600 * grad_scale; the threshold is a sixth of it."""
    run = MultiRun(Lb, case())
    sumsq = sumsq_of(Lb, run.grads())
    s64 = true_sumsq()
    r = Report("multi/sumsq")
    s32 = torch.stack([g.pow(2).sum() for g in run.grads()]).sum().reshape(1)
    r.tensor("sumsq", "all", sumsq, torch.tensor([s64], dtype=torch.float64), s32)
    r.done()
    max_norm = R.f32(100.0 * grad_scale)
    scale = R.clip_scale(s64, max_norm, grad_scale)
    assert abs(scale) < 0.25 * grad_scale                                         # it clips
    assert run.launch(sumsq=sumsq, max_grad_norm=max_norm, grad_scale=grad_scale) == 0
    judge_multi("multi/clip gs=%g" % grad_scale, run, gscale=scale, gscale32=clip_t32(s32[0], max_norm, grad_scale))


def test_multi_clipping_that_does_not_clip_is_bitwise_the_unclipped_run(Lb):
    plain, clipped = MultiRun(Lb, case()), MultiRun(Lb, case())
    sumsq = sumsq_of(Lb, clipped.grads())
    assert math.sqrt(true_sumsq()) < 1e3
    assert plain.launch(sumsq=None) == 0
    assert clipped.launch(sumsq=sumsq, max_grad_norm=1e4) == 0
    for i in range(len(case())):
        for a, b in zip(plain.out(i), clipped.out(i)):
            assert same_bits(a, b), case()[i]["n"]
    judge_multi("multi/no_clip", clipped)


def test_multi_step_ptr_overrides_step(Lb):
    run = MultiRun(Lb, case())
    assert run.launch(step=1, step_ptr=torch.tensor([R.MULTI_STEP], dtype=torch.int32, device="cuda")) == 0
    judge_multi("multi/step_ptr", run)


def test_multi_lr_ptr_overrides_the_group_rates(Lb):
    run = MultiRun(Lb, case())
    lrs = torch.tensor([g[0] for g in R.GROUPS] + [float("nan")] * 5, dtype=torch.float32, device="cuda")
    assert run.launch(lr_ptr=lrs, lr_mul=3.0) == 0
    judge_multi("multi/lr_ptr", run)


def test_multi_tensor_steps_advance_by_one_per_call(Lb):
    """Device-side per-tensor counters in the slots step_lag names: each call advances the listed tensors' counters by exactly
    one, leaves every other slot alone, and corrects the bias with the advanced count (a.step is then unused: it is 1 here)."""
    tensors = case()
    run = MultiRun(Lb, tensors, slots=True)
    start = [1000 + j for j in range(16)]
    for i, t in enumerate(tensors):
        start[SLOTS[i]] = t["step"] - 1
    counters = Guarded(torch.tensor(start, dtype=torch.int32), dtype=torch.int32)
    for call in (1, 2):
        assert run.launch(step=1, tsteps=counters.t) == 0
        want = list(start)
        for i, t in enumerate(tensors):
            want[SLOTS[i]] = t["step"] - 1 + call
        assert counters.t.tolist() == want and counters.intact()
        judge_multi("multi/tensor_steps call %d" % call, run, steps=[t["step"] - 1 + call for t in tensors], tensors=tensors)
        # the second call starts from what the first one left (the kernel's own fp32 state)
        tensors = [dict(t, p=run.out(i)[0].cpu(), m=run.out(i)[1].cpu(), v=run.out(i)[2].cpu()) for i, t in enumerate(tensors)]
        run.tensors = tensors


def test_multi_no_chunks_is_ok_and_writes_nothing(Lb):
    run = MultiRun(Lb, case(), slots=True)
    counters = torch.arange(16, dtype=torch.int32, device="cuda")
    assert run.launch(n_chunks=0, tsteps=counters) == 0
    assert counters.tolist() == list(range(16))
    for i, t in enumerate(case()):
        for got, k in zip(run.out(i), "pmv"):
            assert same_bits(got.cpu(), t[k])
    run.guards_ok()


# ---- hero_adamw -----------------------------------------------------------------------------------------------------------
HP = R.GROUPS[0]
_SINGLE = {}


def single_data(n, step):
    """fp32 CPU inputs of a hero_adamw case: every other element of p is exactly 0; step 1 starts from m = v = 0."""
    if (n, step) not in _SINGLE:
        gen = torch.Generator().manual_seed(8000 + n % 1000 + step)
        g = R.log_uniform_grad(n, gen)
        p = torch.randn(n, generator=gen)
        p[::2] = 0.0
        if step == 1:
            m, v = torch.zeros(n), torch.zeros(n)
        else:
            m = 0.1 * torch.randn(n, generator=gen)
            v = m * m * (0.5 + 1.5 * torch.rand(n, generator=gen))
        _SINGLE.clear()                                                           # one case alive at a time: the largest is 67 MB
        _SINGLE[(n, step)] = dict(n=n, p=p, g=g, m=m, v=v, zero=p == 0)
    return _SINGLE[(n, step)]


def run_single(Lb, t, step, sumsq=None, max_grad_norm=0.0, grad_scale=1.0, shadow=False):
    d = {k: Guarded(t[k]) for k in "pgmv"}
    sh = Guarded(torch.full((t["n"],), 5.0), dtype=torch.bfloat16) if shadow else None
    lr, b1, b2, eps, wd = HP
    a = Lb.AdamW(d["p"].ptr(), d["g"].ptr(), d["m"].ptr(), d["v"].ptr(), t["n"], lr, b1, b2, eps, wd, step, Lb.ptr(sumsq), max_grad_norm,
                 grad_scale, sh.ptr() if shadow else None)
    Lb.check(Lb.lib().hero_adamw(C.byref(a), Lb.stream()))
    torch.cuda.synchronize()
    for k in "pgmv":
        assert d[k].intact(), k
    assert same_bits(d["g"].t.cpu(), t["g"])
    if shadow:
        assert sh.intact()
        # the fused compute copy: the kernel's own fp32 result rounded to nearest-even, tail elements included
        assert torch.equal(sh.t.view(torch.int16), d["p"].t.to(torch.bfloat16).view(torch.int16))
    return d["p"].t, d["m"].t, d["v"].t


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000, BIG + 5])
def test_adamw_single_against_float64(Lb, n, step):
    t = single_data(n, step)
    hp = tuple(R.f32(x) for x in HP)
    for clipped in (False, True):
        name = "single/n%d/step%d/%s" % (n, step, "clip_scaled" if clipped else "plain")
        if clipped:
            gdev = t["g"].cuda()
            sumsq, s64 = sumsq_of(Lb, [gdev]), R.sumsq_ref(t["g"])
            grad_scale = 0.125
            max_norm = R.f32(0.5 * math.sqrt(s64) * grad_scale) if s64 > 0 else 1.0    # half the norm of the scaled gradients
            kw = dict(sumsq=sumsq, max_grad_norm=max_norm, grad_scale=grad_scale)
            gscale, gscale32 = R.clip_scale(s64, max_norm, grad_scale), clip_t32(gdev.pow(2).sum(), max_norm, grad_scale)
            assert s64 == 0 or abs(gscale) < 0.51 * grad_scale
        else:
            kw, gscale, gscale32 = {}, 1.0, t32(1.0)
        got = run_single(Lb, t, step, **kw)
        with_shadow = run_single(Lb, t, step, shadow=True, **kw)
        for a, b in zip(got, with_shadow):
            assert same_bits(a, b)                                                 # the shadow store changes nothing else
        ref = R.adamw_ref(t["p"], t["g"], t["m"], t["v"], step, *hp, gscale=gscale)
        tf = adamw_t32(t["p"], t["g"], t["m"], t["v"], step, *hp, gscale=gscale32)
        r = Report(name)
        if n > 1:
            r.tensor("p", "p", got[0], ref[0], tf[0], mask=~t["zero"])
        r.tensor("dp", "dp", got[0], ref[0], tf[0], mask=t["zero"])
        r.tensor("m", "m", got[1], ref[1], tf[1])
        r.tensor("v", "v", got[2], ref[2], tf[2])
        r.done()


def test_adamw_single_rejects_misaligned_pointers(Lb):
    """p, g, m, v are read as float4 and shadow is written 8 bytes at a time, with no scalar fallback: anything else is an
    argument error before any launch."""
    n = 1000
    bufs = {k: torch.full((n + 8,), 0.5, device="cuda") for k in "pgmv"}
    sh = torch.full((n + 8,), 0.5, dtype=torch.bfloat16, device="cuda")
    lr, b1, b2, eps, wd = HP
    for bad in ("p", "g", "m", "v", "shadow"):
        ptrs = [bufs[k][1:].data_ptr() if k == bad else bufs[k].data_ptr() for k in "pgmv"]
        shp = sh[2:].data_ptr() if bad == "shadow" else sh.data_ptr()
        assert ptrs[0] % 16 == (4 if bad == "p" else 0) and shp % 8 == (4 if bad == "shadow" else 0)
        a = Lb.AdamW(*ptrs, n, lr, b1, b2, eps, wd, 1, None, 0.0, 1.0, shp)
        assert Lb.lib().hero_adamw(C.byref(a), Lb.stream()) != 0, bad
        assert "hero_adamw" in Lb.lib().hero_last_error().decode() and "aligned" in Lb.lib().hero_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((b == 0.5).all()) for b in bufs.values()) and bool((sh == 0.5).all())       # nothing was launched


# ---- hero_sumsq -----------------------------------------------------------------------------------------------------------
SUMSQ_CASES = {"n0": 0, "n1": 1, "n3": 3, "n4": 4, "n5": 5, "n1023": 1023, "n33000": 33000, "big": BIG + 3, "outlier": 33000}


@pytest.mark.parametrize("name", list(SUMSQ_CASES))
def test_sumsq_against_float64(Lb, name):
    n = SUMSQ_CASES[name]
    gen = torch.Generator().manual_seed(9000 + n % 1000)
    if name == "outlier":
        g = torch.full((n,), 1e-3)
        g[12345] = 1e3
    else:
        g = torch.randn(max(n, 1), generator=gen)                                 # n = 0: a valid pointer, no element read
    dev, ws = Guarded(g), Guarded(torch.zeros(2048))
    ref = R.sumsq_ref(g[:n])
    s32 = dev.t[:n].pow(2).sum()
    results = []
    for rep in range(3):
        out = Guarded(torch.tensor([0.25]))
        for calls in (1, 2):
            Lb.check(Lb.lib().hero_sumsq(dev.ptr(), n, out.ptr(), ws.ptr(), Lb.stream()))
            torch.cuda.synchronize()
            results.append(out.t.clone())
            if rep == 0:
                want = torch.tensor([0.25 + calls * ref], dtype=torch.float64)
                if n == 0:
                    assert same_bits(out.t.cpu(), torch.tensor([0.25]))
                else:
                    r = Report("sumsq/%s/calls%d" % (name, calls))
                    r.tensor("sumsq", "sum", out.t, want, 0.25 + calls * s32.reshape(1))      # the += into the caller's scalar
                    r.done()
        assert out.intact() and dev.intact() and ws.intact() and same_bits(dev.t.cpu(), g)
    for rep in (1, 2):                                                            # fixed summation order: identical bits
        assert same_bits(results[2 * rep], results[0]) and same_bits(results[2 * rep + 1], results[1])


def test_sumsq_rejects_a_misaligned_gradient(Lb):
    buf = torch.ones(1032, device="cuda")
    out, ws = torch.full((1,), 0.25, device="cuda"), torch.empty(2048, device="cuda")
    view = buf[1:1001]
    assert view.data_ptr() % 16 == 4
    assert Lb.lib().hero_sumsq(view.data_ptr(), 1000, out.data_ptr(), ws.data_ptr(), Lb.stream()) != 0
    msg = Lb.lib().hero_last_error().decode()
    assert "hero_sumsq" in msg and "aligned" in msg
    torch.cuda.synchronize()
    assert out.item() == 0.25


# ---- hero_amd.optim.AdamW ---------------------------------------------------------------------------------------------
def _step_and_judge(name, opt, params, grads, hps, expect_steps, frozen=(), **kw):
    """One optimiser step: every parameter with a gradient against the restatement from its own pre-step state and its own
    step count; the `frozen` ones (no gradient, or skipped) bit-unchanged, state included."""
    before = {}
    for i, p in enumerate(params):
        st = opt.state[p]
        zeros = torch.zeros_like(p)
        before[i] = (p.detach().clone(), st["exp_avg"].clone() if st else zeros, st["exp_avg_sq"].clone() if st else zeros, st.get("step", 0) if st else 0)
    for p, g in zip(params, grads):
        p.grad = g
    opt.step(**kw)
    torch.cuda.synchronize()
    r = Report(name)
    for i, p in enumerate(params):
        st = opt.state[p]
        p0, m0, v0, s0 = before[i]
        if i in frozen:
            assert same_bits(p.detach(), p0) and same_bits(st["exp_avg"], m0) and same_bits(st["exp_avg_sq"], v0) and st["step"] == s0
            continue
        lr, (b1, b2), eps, wd = hps[i]
        hp = tuple(R.f32(x) for x in (lr, b1, b2, eps, wd))
        ref = R.adamw_ref(p0, grads[i], m0, v0, expect_steps[i], *hp)
        tf = adamw_t32(p0, grads[i], m0, v0, expect_steps[i], *hp, gscale=t32(1.0))
        zero = bool((p0 == 0).all())
        r.tensor("dp" if zero else "p", "p%d" % i, p.detach(), ref[0], tf[0])
        r.tensor("m", "p%d" % i, st["exp_avg"], ref[1], tf[1])
        r.tensor("v", "p%d" % i, st["exp_avg_sq"], ref[2], tf[2])
    r.done()


def test_optimizer_class_eager_skips_then_device_state_then_eager(HF, Lb):
    from hero_amd.optim import AdamW
    gen = torch.Generator().manual_seed(77)
    sizes = (5, 16385, 40000)
    params = [torch.nn.Parameter(torch.randn(5, generator=gen).cuda()), torch.nn.Parameter(torch.zeros(16385, device="cuda")),
              torch.nn.Parameter(torch.randn(200, 200, generator=gen).cuda())]
    opt = AdamW([{"params": params[:2], "lr": 1e-3, "weight_decay": 0.01, "betas": (0.9, 0.98)},
                 {"params": params[2:], "lr": 5e-3, "weight_decay": 0.0, "betas": (0.8, 0.999)}], eps=1e-6)
    hps = [(1e-3, (0.9, 0.98), 1e-6, 0.01)] * 2 + [(5e-3, (0.8, 0.999), 1e-6, 0.0)]

    def grads(missing=()):
        return [None if i in missing else R.log_uniform_grad(n, gen).cuda().view_as(params[i]) for i, n in enumerate(sizes)]

    _step_and_judge("class/eager1", opt, params, grads(), hps, [1, 1, 1])
    _step_and_judge("class/eager2 grad=None", opt, params, grads(missing=(1,)), hps, [2, None, 2], frozen=(1,))
    _step_and_judge("class/eager3 skip", opt, params, grads(), hps, [3, None, 3], frozen=(1,), skip={params[1]})
    _step_and_judge("class/eager4", opt, params, grads(), hps, [4, 2, 4])
    assert [opt.state[p]["step"] for p in params] == [4, 2, 4]
    # device-state mode: per-parameter counters and the rates live on the device (what a captured step uses)
    step_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    lr_t = torch.tensor([1e-3, 5e-3] + [float("nan")] * 6, dtype=torch.float32, device="cuda")
    for group in opt.param_groups:
        group["lr"] = 99.0                                                        # must not be read in this mode
    _step_and_judge("class/device5", opt, params, grads(), hps, [5, 3, 5], step_tensor=step_t, lr_tensor=lr_t)
    _step_and_judge("class/device6", opt, params, grads(), hps, [6, 4, 6], step_tensor=step_t, lr_tensor=lr_t)
    assert [opt.state[p]["step"] for p in params] == [4, 2, 4]                    # the host counts lag until they are synced
    assert opt._tsteps.tolist() == [6, 4, 6]
    opt.sync_steps_from_device()
    assert [opt.state[p]["step"] for p in params] == opt._tsteps.tolist() == [6, 4, 6]
    opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = 1e-3, 5e-3
    for p in params:
        opt.state[p]["step"] = -5                                                 # the eager step takes the device counters, not these
    _step_and_judge("class/eager7", opt, params, grads(), hps, [7, 5, 7])
    assert [opt.state[p]["step"] for p in params] == [7, 5, 7] and opt._tsteps is None


def test_optimizer_class_group_limit_and_misaligned_gradient(HF, Lb):
    from hero_amd.optim import AdamW
    with pytest.raises(ValueError, match="8 parameter groups"):
        AdamW([{"params": [torch.nn.Parameter(torch.zeros(4))]} for _ in range(9)])
    AdamW([{"params": [torch.nn.Parameter(torch.zeros(4))]} for _ in range(8)])
    # grad_sumsq() over per-parameter gradients: one that is a misaligned view is copied, not handed to hero_sumsq as it is
    gen = torch.Generator().manual_seed(78)
    p = [torch.nn.Parameter(torch.zeros(1001, device="cuda")), torch.nn.Parameter(torch.zeros(7, device="cuda"))]
    buf = torch.randn(1100, generator=gen).cuda()
    p[0].grad, p[1].grad = buf[1:1002], buf[1024:1031]
    assert p[0].grad.data_ptr() % 16 == 4 and p[1].grad.data_ptr() % 16 == 0
    got = AdamW(p).grad_sumsq()
    ref = torch.tensor([R.sumsq_ref(p[0].grad) + R.sumsq_ref(p[1].grad)], dtype=torch.float64)
    r = Report("class/grad_sumsq misaligned")
    r.tensor("sumsq", "sum", got, ref, (p[0].grad.pow(2).sum() + p[1].grad.pow(2).sum()).reshape(1))
    r.done()
