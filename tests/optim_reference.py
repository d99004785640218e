"""float64 restatement of the optimiser step (hero_sumsq + hero_adamw / hero_adamw_multi, hero_amd/csrc/rows.hip): plain torch
on CPU tensors, float64 throughout, nothing from hero_amd.  The order of operations is the reference's (optim/adamw.py:43-106,
clipping as torch.nn.utils.clip_grad_norm_ does it, train_vcmr.py:257-260); tests/test_cpu_optim_reference.py holds it against
oracle.hero_oracle.adamw_step and clip_grad_norm_.

Hyper-parameters cross the C ABI as `float`: `f32(x)` is the value a kernel is handed, widened.  The tests give that value to
the restatement, like every other input, so that only the arithmetic is judged."""
import math

import torch


def f32(x):
    """The float32 nearest to the Python float `x`, as a Python float (what a C `float` field holds)."""
    return float(torch.tensor(x, dtype=torch.float32))


def adamw_ref(p, g, m, v, step, lr, beta1, beta2, eps, wd, gscale=1.0):
    """One AdamW step on float64 copies of p, g, m, v; returns the new (p, m, v).  `step` is the tensor's own 1-based count."""
    p, g, m, v = (t.detach().double().cpu().clone() for t in (p, g, m, v))
    g = g * gscale
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - lr * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step) * m / (v.sqrt() + eps)
    p = p - lr * wd * p
    return p, m, v


def clip_scale(sumsq, max_norm, grad_scale=1.0):
    """The multiplier on the raw gradients: grad_scale, times the clipping coefficient of the scaled gradients' norm."""
    norm = math.sqrt(float(sumsq)) * abs(grad_scale)
    return grad_scale * min(1.0, max_norm / (norm + 1e-6))


def sumsq_ref(g):
    return float(g.detach().double().cpu().pow(2).sum())


def gelu_grad_ref(u):
    """d/du [u * Phi(u)] = Phi(u) + u * phi(u), erf form (model/layers.py:16-25), float64."""
    u = u.detach().double().cpu()
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def log_uniform_grad(n, gen):
    """The optimiser tests' gradients: magnitudes log-uniform over [1e-8, 10], random sign, every 13th element exactly 0
    (fp32).  Shared by the CPU check that these inputs can tell a wrong eps / step and by the GPU tests."""
    mag = torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * (math.log(10.0) - math.log(1e-8)) + math.log(1e-8))
    sign = torch.randint(0, 2, (n,), generator=gen).double() * 2.0 - 1.0
    g = (mag * sign).float()
    g[::13] = 0.0
    return g


# ---- the multi-tensor case of tests/test_gpu_optim_kernels.py (inputs only; fp32 CPU tensors) -----------------------------
CHUNK = 16384
MULTI_SIZES = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, 33000, CHUNK + 6]
MISALIGNED = len(MULTI_SIZES) - 1                      # the last tensor starts one float past a 16-byte boundary
GROUPS = [(1e-3, 0.9, 0.98, 1e-6, 0.01), (5e-3, 0.8, 0.999, 1e-8, 0.0), (2e-4, 0.95, 0.9, 1e-4, 0.1)]   # lr, b1, b2, eps, wd
MULTI_STEP = 7
LAGS = (0, 3, 6)


def multi_case():
    """[{n, group, lag, step, fresh, p0, p, g, m, v}]: groups round-robin, the lags rotated against them so that every
    group has a fresh tensor (lag 6: tensor step 1, m = v = 0) and every fresh tensor starts from p = 0 (so do all even
    tensors).  Non-fresh moments: m ~ 0.1 N(0,1), v = m^2 * U(0.5, 2), as after real steps (|m| <~ sqrt(v))."""
    out = []
    for i, n in enumerate(MULTI_SIZES):
        gen = torch.Generator().manual_seed(7000 + i)
        lag = LAGS[(i // 3 + i) % 3]
        fresh = lag == MULTI_STEP - 1
        g = log_uniform_grad(n, gen)
        p = torch.zeros(n) if i % 2 == 0 else torch.randn(n, generator=gen)
        if fresh:
            m, v = torch.zeros(n), torch.zeros(n)
        else:
            m = 0.1 * torch.randn(n, generator=gen)
            v = m * m * (0.5 + 1.5 * torch.rand(n, generator=gen))
        out.append(dict(n=n, group=i % 3, lag=lag, step=MULTI_STEP - lag, fresh=fresh, p0=i % 2 == 0, p=p, g=g, m=m, v=v))
    assert all(t["p0"] for t in out if t["fresh"]) and {t["group"] for t in out if t["fresh"]} == {0, 1, 2}
    return out


def group_f32(gi):
    """A group's hyper-parameters as the kernel is handed them (C floats), widened."""
    return tuple(f32(x) for x in GROUPS[gi])
