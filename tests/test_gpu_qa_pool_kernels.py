"""hero_qa_pool_fwd / hero_qa_pool_bwd (hero_amd/csrc/qa_pool.hip) through hero_amd.qa.QaPoolFn against the float64
restatement of tests/qa_reference.py.  Shapes (Nv, A, L, Lqa, D) - the smallest that reach each failure mode:

    (2, 5, 7, 3, 128)       A no power of two, L below a wave
    (3, 4, 65, 0, 768)      L one past a wave, Lt == L (no tail rows), A a power of two: masked frames give exactly 1 / A
    (2, 5, 100, 20, 768)    the recipe's row geometry
    (1, 1, 1, 1, 64)        both softmaxes degenerate
    (2, 8, 256, 256, 1024)  the corner of the envelope

Every case but the degenerate one and `all_valid` masks the trailing frames of its last video (all answer copies alike, as the
collate does); `all_valid` = (2, 5, 7, 3, 128) with every frame valid.  Inputs are drawn once in the kernel's input dtype and the
same rounded values go to the reference, so only the arithmetic is judged.

Tolerance (the rule of tests/test_gpu_head_kernels.py; nothing is taken from a kernel's output): the element-wise error
(tests.util.elem_rel_err) of the fp32 PyTorch formulation (HeroForVideoQA.get_modularized_video's ops and autograd, fp32,
same inputs, on the GPU) against the float64 restatement, worst over this file's cases, times 4, floored at
16 * 2^-24 = 9.54e-7.  bf16-stored dX: per element |a - b| <= 2^-8 |b| + TOL * rms(b).  dw_qa / dw_se are sums of terms that
cancel; they are judged - kernel and PyTorch alike - against the size of what is summed (qa_reference `dw_*_scale`).
Every test prints the kernel's and PyTorch-fp32's figures (-s).

Measured on an AMD Instinct MI355X (gfx950), ROCm PyTorch, this file's inputs:

    output        worst PyTorch-fp32 error (case)                     x 4        TOL
    att (qa, se)  5.450e-06  (att_qa,    fp32 (2, 5, 100, 20, 768))                2.18e-05   2.18e-05
    pooled        1.096e-05  (se_pooled, fp32 (2, 8, 256, 256, 1024))              4.38e-05   4.38e-05
    dX            1.770e-05  (dX,        fp32 (2, 8, 256, 256, 1024))              7.08e-05   7.08e-05
    dw / scale    4.514e-07  (dw_qa,     bf16 (2, 8, 256, 256, 1024))              1.81e-06   1.81e-06

The kernels' own worst figures in the same run, for the record (they are not where the constants come from): att 4.9e-07,
pooled 1.6e-06, dX 4.1e-06 in fp32 (bf16-stored dX: 3.5e-03 = its rounding, inside the bf16 bound), dw / scale 2.5e-07.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import qa_reference as R
from tests.util import elem_rel_err

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
# worst PyTorch-fp32 figure per output over CASES x dtypes (the table above), times 4, floored
MEASURED = {"att": 5.450e-6, "pooled": 1.096e-5, "dX": 1.770e-5, "dw": 4.514e-7}
TOL = {k: max(FLOOR, 4 * v) for k, v in MEASURED.items()}

CASES = {
    "odd_A_short_L": (2, 5, 7, 3, 128, True),
    "all_valid": (2, 5, 7, 3, 128, False),
    "L65_no_tail": (3, 4, 65, 0, 768, True),
    "recipe": (2, 5, 100, 20, 768, True),
    "degenerate": (1, 1, 1, 1, 64, False),
    "corner": (2, 8, 256, 256, 1024, True),
}
_CACHE = {}


def mask_logits(s, m):
    return s * m + (1 - m) * -1e4


def torch_fp32(X, m, wq, ws, dqa, dse):
    """The PyTorch formulation (model/videoQA.py:36-59) in fp32 on the GPU, with autograd."""
    X = X.float().clone().requires_grad_(True)
    wq, ws = wq.clone().requires_grad_(True), ws.clone().requires_grad_(True)
    att_se = F.softmax(mask_logits(F.linear(X, ws), m.unsqueeze(-1)), dim=1)
    att_qa = F.softmax(mask_logits(F.linear(X, wq), m.unsqueeze(-1)), dim=2)
    se = torch.einsum("vqlm,vqld->vlmd", att_se, X).squeeze(2)
    qa = torch.einsum("vqlm,vqld->vqmd", att_qa, X).squeeze(2)
    ((qa * dqa).sum() + (se * dse).sum()).backward()
    return {"att_qa": att_qa.squeeze(-1), "att_se": att_se.squeeze(-1), "qa_pooled": qa, "se_pooled": se,
            "dX": X.grad, "dw_qa": wq.grad.reshape(-1), "dw_se": ws.grad.reshape(-1)}


def case_data(name, dtype):
    """Inputs, the float64 restatement and the PyTorch-fp32 results of a case: computed once, shared, never modified."""
    key = (name, dtype)
    if key not in _CACHE:
        Nv, A, L, Lqa, D, masked = CASES[name]
        g = torch.Generator().manual_seed(1000 + len(name) + L)
        seq = torch.randn(Nv * A, L + Lqa, D, generator=g).to(dtype).cuda()
        wq = (torch.randn(1, D, generator=g) * 2.0 / D ** 0.5).cuda()            # scores a few units apart
        ws = (torch.randn(1, D, generator=g) * 2.0 / D ** 0.5).cuda()
        dqa, dse = torch.randn(Nv, A, D, generator=g).cuda(), torch.randn(Nv, L, D, generator=g).cuda()
        m = torch.ones(Nv, A, L)
        if masked:
            m[-1, :, L - max(1, L // 3):] = 0
        m = m.cuda()
        X = seq[:, :L].float().view(Nv, A, L, D)
        ref = R.forward(X, m, wq, ws)
        ref.update(R.backward(X, m, wq, ws, dqa, dse))
        _CACHE[key] = dict(seq=seq, m=m, wq=wq, ws=ws, dqa=dqa, dse=dse, ref=ref, t32=torch_fp32(X, m, wq, ws, dqa, dse),
                           dims=(Nv, A, L, Lqa, D))
    return _CACHE[key]


def run_kernels(c):
    from hero_amd.qa import QaPoolFn
    Nv, A, L, Lqa, D = c["dims"]
    seq = c["seq"].clone().requires_grad_(True)
    wq, ws = c["wq"].clone().requires_grad_(True), c["ws"].clone().requires_grad_(True)
    qa, se = QaPoolFn.apply(seq, c["m"].view(Nv * A, L), wq, ws, A, L)
    torch.autograd.backward([qa, se], [c["dqa"], c["dse"]])
    return qa, se, seq.grad, wq.grad.reshape(-1), ws.grad.reshape(-1)


def raw_call(c, sentinel=None):
    """The two entry points through ctypes: also returns the attention tables; dX pre-filled with `sentinel`."""
    from hero_amd import _lib as Lb
    Nv, A, L, Lqa, D = c["dims"]
    seq, m = c["seq"], c["m"].view(Nv * A, L).contiguous()
    wq, ws = c["wq"].reshape(-1).contiguous(), c["ws"].reshape(-1).contiguous()
    qa, se = torch.empty(Nv, A, D, device="cuda"), torch.empty(Nv, L, D, device="cuda")
    att = torch.empty(2, Nv, A, L, device="cuda")
    Lb.check(Lb.lib().hero_qa_pool_fwd(Lb.ptr(seq), Lb.ptr(m), Lb.ptr(wq), Lb.ptr(ws), Lb.ptr(qa), Lb.ptr(se), Lb.ptr(att[0]), Lb.ptr(att[1]),
                                       Nv, A, L, L + Lqa, D, Lb.dt(seq), Lb.stream()))
    dx = torch.full_like(seq, sentinel if sentinel is not None else 0.0)
    dw = torch.full((2, Nv, D), 7.0, device="cuda")
    Lb.check(Lb.lib().hero_qa_pool_bwd(Lb.ptr(seq), Lb.ptr(m), Lb.ptr(wq), Lb.ptr(ws), Lb.ptr(att[0]), Lb.ptr(att[1]), Lb.ptr(c["dqa"]),
                                       Lb.ptr(c["dse"]), Lb.ptr(dx), Lb.ptr(dw[0]), Lb.ptr(dw[1]), Nv, A, L, L + Lqa, D, Lb.dt(seq), Lb.stream()))
    return qa, se, att, dx, dw


class Report:
    def __init__(self, case):
        self.case, self.bad = case, []

    def line(self, group, name, ek, et, ok):
        print("\n[qa-pool] %-22s %-10s kernel %.3e  torch-fp32 %.3e  tol %s %s"
              % (self.case, name, ek, et, "%.3e" % TOL[group], "" if ok else "MISS"), end="")
        if not ok:
            self.bad.append((name, ek, TOL[group]))

    def tensor(self, group, name, got, ref, t32):
        ek, et = elem_rel_err(got, ref), elem_rel_err(t32, ref)
        tol = TOL[group]
        if got.dtype == torch.bfloat16:
            a, b = got.detach().double().cpu(), ref.double().cpu()
            ok = bool(((a - b).abs() <= 2.0 ** -8 * b.abs() + tol * b.pow(2).mean().sqrt()).all())
        else:
            ok = ek <= tol
        self.line(group, name, ek, et, ok)

    def scaled(self, group, name, got, ref, scale, t32):
        err = lambda a: float(((a.detach().double().cpu() - ref.cpu()).abs() / scale.cpu().clamp_min(1e-300)).max())     # noqa: E731
        ek = err(got)
        self.line(group, name, ek, err(t32), ek <= TOL[group])

    def done(self):
        assert not self.bad, (self.case, self.bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_against_float64(name, dtype):
    c = case_data(name, dtype)
    Nv, A, L, Lqa, D = c["dims"]
    ref, t32 = c["ref"], c["t32"]
    qa, se, att, dx_raw, _ = raw_call(c, sentinel=123.0)
    qa2, se2, dx, dwq, dws = run_kernels(c)
    assert torch.equal(qa, qa2) and torch.equal(se, se2) and torch.equal(dx, dx_raw)      # the node is the two entry points
    r = Report("%s/%s" % (name, "bf16" if dtype == torch.bfloat16 else "fp32"))
    r.tensor("att", "att_qa", att[0], ref["att_qa"], t32["att_qa"])
    r.tensor("att", "att_se", att[1], ref["att_se"], t32["att_se"])
    r.tensor("pooled", "qa_pooled", qa, ref["qa_pooled"], t32["qa_pooled"])
    r.tensor("pooled", "se_pooled", se, ref["se_pooled"], t32["se_pooled"])
    assert dx.shape == (Nv * A, L + Lqa, D) and dx.dtype == dtype
    r.tensor("dX", "dX", dx[:, :L].reshape(Nv, A, L, D), ref["dX"], t32["dX"])
    # the rows behind the frames: exactly zero, over a buffer that held a sentinel
    assert int((dx_raw[:, L:] != 0).sum()) == 0
    r.scaled("dw", "dw_qa", dwq, ref["dw_qa"], ref["dw_qa_scale"], t32["dw_qa"])
    r.scaled("dw", "dw_se", dws, ref["dw_se"], ref["dw_se_scale"], t32["dw_se"])
    # masked frames: uniform over the answers - exactly 1 / A when A is a power of two
    masked = c["m"] == 0
    if bool(masked.any()):
        if A & (A - 1) == 0:
            assert bool((att[1][masked] == 1.0 / A).all())
        else:
            assert float((att[1][masked] - 1.0 / A).abs().max()) <= 2.0 ** -24
        assert float(att[0][masked].abs().max()) == 0.0                                    # exp(-1e4 - max) underflows to 0
    r.done()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["odd_A_short_L", "recipe", "corner"])
def test_two_runs_are_bitwise_equal(name, dtype):
    c = case_data(name, dtype)
    a, b = run_kernels(c), run_kernels(c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_outside_the_envelope_is_an_error():
    from hero_amd import _lib as Lb
    from hero_amd.qa import QaPoolFn
    z = torch.zeros(16, device="cuda")
    for Nv, A, L, Lt, D in ((1, 9, 4, 4, 64), (1, 2, 257, 257, 64), (1, 2, 4, 513, 64), (1, 2, 4, 3, 64), (1, 2, 4, 4, 1028), (1, 2, 4, 4, 6)):
        rc = Lb.lib().hero_qa_pool_fwd(*([Lb.ptr(z)] * 8), Nv, A, L, Lt, D, Lb.F32, Lb.stream())
        assert rc == -1, (A, L, Lt, D)
    with pytest.raises(ValueError, match="envelope"):
        QaPoolFn.apply(torch.zeros(9, 4, 64, device="cuda"), torch.ones(9, 4, device="cuda"), z[None, :1], z[None, :1], 9, 4)
