"""tests/optim_reference.py, the float64 restatement the GPU optimiser tests judge against, held against what it restates:
oracle.hero_oracle.adamw_step (the reference's optim/adamw.py:43-106 on float64 tensors), torch.nn.utils.clip_grad_norm_
(train_vcmr.py:257-260) and tensor.to(torch.bfloat16); and the proof that the GPU tests' inputs can tell a right optimiser
from one with a wrong eps or a bias correction one step off."""
import math

import pytest
import torch

from oracle import hero_oracle as O
from tests import optim_reference as R
from tests.util import elem_rel_err

FLOOR = 16 * 2.0 ** -24            # the floor of every tolerance in tests/test_gpu_optim_kernels.py
GROUP_EPS = [g[3] for g in R.GROUPS]


@pytest.mark.parametrize("wd", [0.01, 0.0], ids=["decay", "no_decay"])
def test_restatement_equals_the_oracle_in_float64(wd):
    gen = torch.Generator().manual_seed(11)
    n = 1000
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    P, state = {"w": p0.clone()}, {}
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in (1, 2, 3):
        g = R.log_uniform_grad(n, gen).double() * step
        O.adamw_step(P, {"w": g.clone()}, state, lr=1e-3, step=step, betas=(0.9, 0.98), eps=1e-6, wd=wd)
        p, m, v = R.adamw_ref(p, g, m, v, step, 1e-3, 0.9, 0.98, 1e-6, wd)
        for got, want in ((p, P["w"]), (m, state["w"][0]), (v, state["w"][1])):
            assert got.dtype == torch.float64 and want.dtype == torch.float64
            assert elem_rel_err(got, want) <= 1e-12
    assert float((p - p0).abs().max()) > 1e-3                                     # three steps moved the weights


def test_gscale_is_a_multiplier_on_the_gradient():
    gen = torch.Generator().manual_seed(12)
    p, g = torch.randn(100, generator=gen), R.log_uniform_grad(100, gen)
    m, v = 0.1 * torch.randn(100, generator=gen), torch.rand(100, generator=gen)
    a = R.adamw_ref(p, g, m, v, 4, 1e-3, 0.9, 0.98, 1e-6, 0.01, gscale=0.125)
    b = R.adamw_ref(p, g.double() * 0.125, m, v, 4, 1e-3, 0.9, 0.98, 1e-6, 0.01)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("max_norm", [0.5, 1e4], ids=["clips", "does_not_clip"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_clip_scale_is_clip_grad_norm(max_norm, grad_scale):
    gen = torch.Generator().manual_seed(13)
    raw = [torch.randn(n, generator=gen, dtype=torch.float64) for n in (5, 1000, 33)]
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in raw]
    for q, g in zip(params, raw):
        q.grad = g * grad_scale                                                 # the averaged gradients are what is clipped
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    sumsq = sum(R.sumsq_ref(g) for g in raw)
    assert abs(math.sqrt(sumsq) * abs(grad_scale) - float(total)) <= 1e-12 * float(total)
    scale = R.clip_scale(sumsq, max_norm, grad_scale)
    assert (scale == grad_scale) == (float(total) + 1e-6 <= max_norm)
    for q, g in zip(params, raw):
        assert elem_rel_err(g * scale, q.grad) <= 1e-12


def test_bf16_rounding_is_tensor_to_bfloat16():
    """Round to nearest, ties to even, on the upper 16 bits: a hand-written rounding of the bit pattern equals .to(bfloat16)
    on random values, exact ties both ways, subnormals, +-0 and +-inf."""
    gen = torch.Generator().manual_seed(14)
    x = torch.cat([torch.randn(4096, generator=gen), R.log_uniform_grad(4096, gen),
                   torch.tensor([1.00390625, 1.01171875, -1.00390625, 1.0e-40, -1.0e-40, 0.0, -0.0, float("inf"), -float("inf")])])
    bits = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    rounded = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) & 0xFFFF
    got = x.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(got, rounded)
    assert x.to(torch.bfloat16)[8192:8195].tolist() == [1.0, 1.015625, -1.0]      # the ties went to the even neighbour


def test_inputs_tell_a_wrong_eps_and_a_wrong_step():
    """On the fresh-state tensors of the multi-tensor case (tensor step 1, m = v = 0, p = 0) the update of an element with
    |g| <~ eps is decided by eps, and the bias correction is at its largest: the restatement with eps = 1e-8 for 1e-6, or
    with step + 1, is off by far more than 100 x the floor of the tolerances - the GPU test would fail such a kernel."""
    case = R.multi_case()
    fresh = [t for t in case if t["fresh"]]
    assert len(fresh) == 3
    seen_eps = False
    for t in fresh:
        lr, b1, b2, eps, wd = R.group_f32(t["group"])
        assert t["step"] == 1 and not t["m"].any() and not t["v"].any() and not t["p"].any()
        right = R.adamw_ref(t["p"], t["g"], t["m"], t["v"], 1, lr, b1, b2, eps, wd)
        late = R.adamw_ref(t["p"], t["g"], t["m"], t["v"], 2, lr, b1, b2, eps, wd)
        e_step = elem_rel_err(late[0], right[0])
        print("\n[optim-ref] n %-6d group %d  step+1: %.3e" % (t["n"], t["group"], e_step), end="")
        assert e_step > 100 * FLOOR
        assert torch.equal(late[1], right[1]) and torch.equal(late[2], right[2])  # the step enters through p alone
        if GROUP_EPS[t["group"]] == 1e-6:
            wrong = R.adamw_ref(t["p"], t["g"], t["m"], t["v"], 1, lr, b1, b2, R.f32(1e-8), wd)
            # eps under the root: sqrt(v + eps^2)
            inside = (-lr * math.sqrt(1 - b2) / (1 - b1) * right[1] / (right[2] + eps * eps).sqrt()) * (1 - lr * wd)
            e_eps, e_in = elem_rel_err(wrong[0], right[0]), elem_rel_err(inside, right[0])
            print("  eps 1e-8: %.3e  eps inside the root: %.3e" % (e_eps, e_in), end="")
            assert e_eps > 100 * FLOOR and e_in > 100 * FLOOR
            seen_eps = True
    assert seen_eps
