"""hero_frame_pool_fwd / _bwd and hero_bce_head_fwd / _bwd (hero_amd/csrc/violin.hip) through hero_amd.violin.FramePoolFn /
BceHeadFn and through the raw ctypes entry points, against the float64 restatement of tests/violin_reference.py.

Frame pool shapes (S, L, Lq, D) - the smallest that reach each failure mode:

    (3, 7, 3, 128)        L below a wave
    (2, 65, 0, 768)       L one past a wave, Lt == L (no tail rows)
    (8, 100, 30, 768)     the recipe: 4 videos x 2 statements, max_clip_len 100
    (1, 1, 1, 64)         degenerate
    (2, 256, 256, 1024)   the corner of the envelope
    (2, 7, 3, 128)        one sequence fully masked: uniform attention, pooled = row mean, dw and the score part of dX exactly 0

Every other non-degenerate case masks the trailing third of its last sequence.  Classifier tail shapes (S, K): (1, 8), (5, 256),
(8, 1536), (67, 2048), logits inside [-8, 8]; plus targets all 1 / all 0, a z == 0 row, accumulation into `acc`, and saturated
logits (+-30, +-200 against both labels).  Inputs are drawn once in the kernel's input dtype and the same rounded values go to the
reference, so only the arithmetic is judged.

Tolerance (the rule of tests/test_gpu_qa_pool_kernels.py; nothing is taken from a kernel's output): the element-wise error
(tests.util.elem_rel_err) of the fp32 PyTorch formulation (model/violin.py's ops and autograd, fp32, same inputs, on the GPU)
against the float64 restatement, worst over this file's cases, times 4, floored at 16 * 2^-24 = 9.54e-7.  bf16-stored outputs
(dX, dh): per element |a - b| <= 2^-8 |b| + TOL * rms(b).  dw and dw2 are sums of terms that cancel; they are judged - kernel and
PyTorch alike - against the size of what is summed (violin_reference `dw_scale`).  The saturation cases are judged against the
restatement at the floor, relative to max(1, |value|): there the PyTorch formulation is not a reference (its loss jumps to the
clamp and its gradient to 0).  Every test prints the kernel's and PyTorch-fp32's figures (-s).

Measured on an AMD Instinct MI355X (gfx950), ROCm PyTorch, this file's inputs:

    output        worst PyTorch-fp32 error (case)                     x 4        TOL
    att           3.702e-06  (corner,      fp32 (2, 256, 256, 1024))               1.48e-05   1.48e-05
    pooled        5.643e-06  (corner,      fp32 (2, 256, 256, 1024))               2.26e-05   2.26e-05
    dX            1.988e-05  (recipe,      bf16 (8, 100, 30, 768))                 7.95e-05   7.95e-05
    dw / scale    1.689e-06  (corner,      fp32 (2, 256, 256, 1024))               6.76e-06   6.76e-06
    logits        1.641e-06  (S67_K2048,   bf16 (67, 2048))                        6.56e-06   6.56e-06
    loss          2.332e-07  (recipe,      bf16 (8, 1536))                         9.33e-07   9.54e-07 (the floor)
    dh            2.862e-06  (S67_K2048,   bf16 (67, 2048))                        1.14e-05   1.14e-05
    dw2 / scale   1.507e-06  (S5_K256,     fp32 (5, 256))                          6.03e-06   6.03e-06
    db            1.459e-07  (recipe,      fp32 (8, 1536))                         5.84e-07   9.54e-07 (the floor)

The kernels' own worst figures in the same run, for the record (they are not where the constants come from): att 4.6e-07,
pooled 1.1e-06, dX 4.1e-06 in fp32 (bf16-stored dX: 3.5e-03 = its rounding, inside the bf16 bound), dw / scale 3.0e-07, logits
1.3e-07, loss 5.9e-08, dh 2.1e-07 in fp32 (bf16-stored dh: 3.1e-03), dw2 / scale 2.8e-07, db 1.2e-07; the saturation cases 2.4e-14.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import violin_reference as R
from tests.util import elem_rel_err

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
# worst PyTorch-fp32 figure per output over the cases x dtypes (the table above), times 4, floored
MEASURED = {"att": 3.702e-6, "pooled": 5.643e-6, "dX": 1.988e-5, "dw": 1.689e-6, "logits": 1.641e-6, "loss": 2.332e-7, "dh": 2.862e-6,
            "dw2": 1.507e-6, "db": 1.459e-7}
TOL = {k: max(FLOOR, 4 * v) for k, v in MEASURED.items()}

POOL_CASES = {  # (S, L, Lq, D, mask: "tail" = trailing third of the last sequence, "full" = last sequence fully masked, None)
    "short_L": (3, 7, 3, 128, "tail"),
    "L65_no_tail": (2, 65, 0, 768, "tail"),
    "recipe": (8, 100, 30, 768, "tail"),
    "degenerate": (1, 1, 1, 64, None),
    "corner": (2, 256, 256, 1024, "tail"),
    "fully_masked": (2, 7, 3, 128, "full"),
}
HEAD_CASES = {  # (S, K, targets: "mixed" | "ones" | "zeros")
    "S1_K8": (1, 8, "mixed"),
    "S5_K256": (5, 256, "mixed"),
    "recipe": (8, 1536, "mixed"),
    "S67_K2048": (67, 2048, "mixed"),
    "all_ones": (5, 256, "ones"),
    "all_zeros": (5, 256, "zeros"),
}
_CACHE = {}
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def mask_logits(s, m):
    return s * m + (1 - m) * -1e4


def torch_pool_fp32(X, m, w, dpooled):
    """The PyTorch formulation (model/violin.py:30-47) in fp32 on the GPU, with autograd."""
    X = X.float().clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    att = F.softmax(mask_logits(F.linear(X, w), m.unsqueeze(-1)), dim=1)
    pooled = torch.einsum("vlm,vld->vmd", att, X).squeeze(1)
    (pooled * dpooled).sum().backward()
    return {"att": att.squeeze(-1), "pooled": pooled, "dX": X.grad, "dw": w.grad.reshape(-1)}


def torch_head_fp32(h, w, b, t):
    """linear_2 -> sigmoid -> binary_cross_entropy (model/violin.py:73-81) in fp32 on the GPU, with autograd."""
    h = h.float().clone().requires_grad_(True)
    w, b = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    z = F.linear(h, w, b)
    loss = F.binary_cross_entropy(torch.sigmoid(z).squeeze(-1), t.float(), reduction="mean")
    loss.backward()
    return {"logits": z.squeeze(-1), "loss": loss.detach(), "dh": h.grad, "dw": w.grad.reshape(-1), "db": b.grad.reshape(())}


def pool_data(name, dtype):
    """Inputs, the float64 restatement and the PyTorch-fp32 results of a case: computed once, shared, never modified."""
    key = ("pool", name, dtype)
    if key not in _CACHE:
        S, L, Lq, D, how = POOL_CASES[name]
        g = torch.Generator().manual_seed(2000 + len(name) + L)
        seq = torch.randn(S, L + Lq, D, generator=g).to(dtype).cuda()
        w = (torch.randn(1, D, generator=g) * 2.0 / D ** 0.5).cuda()             # scores a few units apart
        dpooled = torch.randn(S, D, generator=g).cuda()
        m = torch.ones(S, L)
        if how == "tail":
            m[-1, L - max(1, L // 3):] = 0
        elif how == "full":
            m[-1] = 0
        m = m.cuda()
        X = seq[:, :L].float()
        ref = R.pool_forward(X, m, w)
        ref.update(R.pool_backward(X, m, w, dpooled))
        _CACHE[key] = dict(seq=seq, m=m, w=w, dpooled=dpooled, ref=ref, t32=torch_pool_fp32(X, m, w, dpooled), dims=(S, L, Lq, D))
    return _CACHE[key]


def head_data(name, dtype):
    key = ("head", name, dtype)
    if key not in _CACHE:
        S, K, how = HEAD_CASES[name]
        g = torch.Generator().manual_seed(3000 + len(name) + K)
        h = torch.randn(S, K, generator=g).to(dtype)
        w = torch.randn(1, K, generator=g) * 2.0 / K ** 0.5
        b = torch.randn(1, generator=g)
        z = (h.double() * w.double()).sum(-1) + b.double()
        if float(z.abs().max()) > 7.0:                                           # logits inside [-8, 8]
            w, b = w * (7.0 / float(z.abs().max())), b * (7.0 / float(z.abs().max()))
        t = {"mixed": torch.randint(0, 2, (S,), generator=g), "ones": torch.ones(S, dtype=torch.long),
             "zeros": torch.zeros(S, dtype=torch.long)}[how]
        if how == "mixed" and S > 1:
            t[0], t[1] = 1, 0
        h, w, b, t = h.cuda(), w.cuda(), b.cuda(), t.cuda()
        ref = R.head_forward(h, w, b, t)
        assert float(ref["logits"].abs().max()) < 8
        ref.update(R.head_backward(h, w, b, t))
        _CACHE[key] = dict(h=h, w=w, b=b, t=t, ref=ref, t32=torch_head_fp32(h, w, b, t), dims=(S, K))
    return _CACHE[key]


def run_pool(c):
    from hero_amd.violin import FramePoolFn
    S, L, Lq, D = c["dims"]
    seq, w = c["seq"].clone().requires_grad_(True), c["w"].clone().requires_grad_(True)
    pooled = FramePoolFn.apply(seq, c["m"], w, L)
    pooled.backward(c["dpooled"])
    return pooled, seq.grad, w.grad.reshape(-1)


def raw_pool(c, sentinel):
    """The two entry points through ctypes: also returns the attention table; dX and dw_part pre-filled with sentinels."""
    from hero_amd import _lib as Lb
    S, L, Lq, D = c["dims"]
    seq, m, w = c["seq"], c["m"], c["w"].reshape(-1).contiguous()
    pooled, att = torch.full((S, D), 5.0, device="cuda"), torch.full((S, L), 5.0, device="cuda")
    Lb.check(Lb.lib().hero_frame_pool_fwd(Lb.ptr(seq), Lb.ptr(m), Lb.ptr(w), Lb.ptr(pooled), Lb.ptr(att), S, L, L + Lq, D, Lb.dt(seq), Lb.stream()))
    dx = torch.full_like(seq, sentinel)
    part = torch.full((S, D), 7.0, device="cuda")
    Lb.check(Lb.lib().hero_frame_pool_bwd(Lb.ptr(seq), Lb.ptr(m), Lb.ptr(w), Lb.ptr(att), Lb.ptr(c["dpooled"]), Lb.ptr(dx), Lb.ptr(part),
                                          S, L, L + Lq, D, Lb.dt(seq), Lb.stream()))
    return pooled, att, dx, part


def run_head(c, dloss=None):
    from hero_amd.violin import BceHeadFn
    h, w, b = c["h"].clone().requires_grad_(True), c["w"].clone().requires_grad_(True), c["b"].clone().requires_grad_(True)
    loss, logits = BceHeadFn.apply(h, w, b, c["t"])
    loss.backward(dloss)
    return loss.detach(), logits, h.grad, w.grad.reshape(-1), b.grad.reshape(())


def raw_head(h, w, b, t, acc=None, dloss=1.0):
    from hero_amd import _lib as Lb
    S, K = h.shape
    w, b = w.reshape(-1).contiguous(), b.reshape(-1).contiguous()
    logits, loss = torch.full((S,), 5.0, device="cuda"), torch.full((1,), 5.0, device="cuda")
    Lb.check(Lb.lib().hero_bce_head_fwd(Lb.ptr(h), Lb.ptr(w), Lb.ptr(b), Lb.ptr(t), Lb.ptr(logits), Lb.ptr(loss), Lb.ptr(acc), S, K, Lb.dt(h), Lb.stream()))
    dh, dw, db = torch.full_like(h, 123.0), torch.full((K,), 7.0, device="cuda"), torch.full((1,), 7.0, device="cuda")
    dl = torch.full((1,), dloss, device="cuda")
    Lb.check(Lb.lib().hero_bce_head_bwd(Lb.ptr(h), Lb.ptr(w), Lb.ptr(logits), Lb.ptr(t), Lb.ptr(dl), Lb.ptr(dh), Lb.ptr(dw), Lb.ptr(db), S, K, Lb.dt(h), Lb.stream()))
    return logits, loss, dh, dw, db


class Report:
    def __init__(self, case):
        self.case, self.bad = case, []

    def line(self, group, name, ek, et, ok):
        print("\n[violin] %-22s %-8s kernel %.3e  torch-fp32 %.3e  tol %.3e %s" % (self.case, name, ek, et, TOL[group], "" if ok else "MISS"), end="")
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


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_frame_pool_against_float64(name, dtype):
    c = pool_data(name, dtype)
    S, L, Lq, D = c["dims"]
    ref, t32 = c["ref"], c["t32"]
    pooled_raw, att, dx_raw, part = raw_pool(c, sentinel=123.0)
    pooled, dx, dw = run_pool(c)
    assert torch.equal(pooled, pooled_raw) and torch.equal(dx, dx_raw)                     # the node is the two entry points
    r = Report("%s/%s" % (name, IDS[DTYPES.index(dtype)]))
    r.tensor("att", "att", att, ref["att"], t32["att"])
    r.tensor("pooled", "pooled", pooled, ref["pooled"], t32["pooled"])
    assert dx.shape == (S, L + Lq, D) and dx.dtype == dtype
    # every element was overwritten (the sentinel is 123; |dX| stays far below it) and the rows behind the frames are exactly zero
    assert int((dx_raw.float() == 123.0).sum()) == 0 and int((part == 7.0).sum()) == 0
    assert int((dx_raw[:, L:] != 0).sum()) == 0
    r.tensor("dX", "dX", dx[:, :L], ref["dX"], t32["dX"])
    r.scaled("dw", "dw", dw, ref["dw"], ref["dw_scale"], t32["dw"])
    masked = c["m"] == 0
    if POOL_CASES[name][4] == "tail":
        assert float(att[masked].abs().max()) == 0.0                                      # exp(-1e4 - max) underflows to 0
    if POOL_CASES[name][4] == "full":
        # the fully masked sequence: uniform attention, pooled = the row mean, no gradient through the scores
        X = c["seq"][-1, :L].double().cpu()
        assert float((att[-1] - 1.0 / L).abs().max()) <= 2.0 ** -24
        assert elem_rel_err(pooled[-1], X.mean(0)) <= TOL["pooled"]
        assert int((part[-1] != 0).sum()) == 0                                            # its share of dw: exactly zero
        want = (att[-1].cpu().unsqueeze(-1) * c["dpooled"][-1].cpu()).to(dtype)           # att * dpooled alone, one fp32 product
        assert torch.equal(dx[-1, :L].cpu(), want)
    r.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_bce_head_against_float64(name, dtype):
    c = head_data(name, dtype)
    ref, t32 = c["ref"], c["t32"]
    loss, logits, dh, dw, db = run_head(c)
    lg_raw, loss_raw, dh_raw, dw_raw, db_raw = raw_head(c["h"], c["w"], c["b"], c["t"])
    assert torch.equal(logits, lg_raw) and torch.equal(loss.reshape(1), loss_raw) and torch.equal(dh, dh_raw)
    assert torch.equal(dw, dw_raw) and torch.equal(db.reshape(1), db_raw)
    assert int((dh_raw.float() == 123.0).sum()) == 0
    r = Report("%s/%s" % (name, IDS[DTYPES.index(dtype)]))
    r.tensor("logits", "logits", logits, ref["logits"], t32["logits"])
    r.tensor("loss", "loss", loss.reshape(1), ref["loss"].reshape(1), t32["loss"].reshape(1))
    assert dh.dtype == dtype
    r.tensor("dh", "dh", dh, ref["dh"], t32["dh"])
    r.scaled("dw2", "dw2", dw, ref["dw"], ref["dw_scale"], t32["dw"])
    r.tensor("db", "db", db.reshape(1), ref["db"].reshape(1), t32["db"].reshape(1))
    r.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_upstream_gradient_is_read_from_the_device(dtype):
    """dloss = 0.25: every gradient scales with it (judged like the dloss = 1 case, against the restatement)."""
    c = head_data("S5_K256", dtype)
    ref = R.head_backward(c["h"], c["w"], c["b"], c["t"], dloss=0.25)
    _, _, dh, dw, db = run_head(c, torch.tensor(0.25, device="cuda"))
    r = Report("dloss/%s" % IDS[DTYPES.index(dtype)])
    r.tensor("dh", "dh", dh, ref["dh"], c["t32"]["dh"] * 0.25)
    r.scaled("dw2", "dw2", dw, ref["dw"], ref["dw_scale"], c["t32"]["dw"] * 0.25)
    r.tensor("db", "db", db.reshape(1), ref["db"].reshape(1), c["t32"]["db"].reshape(1) * 0.25)
    r.done()


def test_zero_logit_predicts_zero():
    """h = 0, b = 0: z is exactly 0, the prediction is 0 - right only for t = 0; loss term log 2; dz = +-0.5 / S."""
    h = torch.zeros(2, 8, device="cuda")
    h[1, 3] = 1.0                                                                 # against a zero weight: still z == 0
    w = torch.tensor([[1.0, 2.0, -1.0, 0.0, 0.5, 0.0, 0.0, 3.0]], device="cuda")
    b = torch.zeros(1, device="cuda")
    for t, right in ((torch.tensor([0, 0]), 2.0), (torch.tensor([1, 1]), 0.0), (torch.tensor([0, 1]), 1.0)):
        acc = torch.zeros(3, device="cuda")
        logits, loss, dh, dw, db = raw_head(h, w, b, t.cuda(), acc=acc)
        assert logits.tolist() == [0.0, 0.0]
        assert acc[1].item() == right and acc[2].item() == 2.0
        assert abs(loss.item() - 0.6931471805599453) <= FLOOR and abs(acc[0].item() - 2 * 0.6931471805599453) <= 2 * FLOOR
        assert torch.equal(dh[0].cpu(), (0.25 - 0.5 * t[0].float()) * w[0].cpu())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_acc_accumulates_over_two_calls(dtype):
    a, b = head_data("S67_K2048", dtype), head_data("recipe", dtype)
    acc = torch.zeros(3, device="cuda")
    for c in (a, b):
        raw_head(c["h"], c["w"], c["b"], c["t"], acc=acc)
    right = sum(float(c["ref"]["right"]) for c in (a, b))
    host = sum(int(((c["t32"]["logits"] > 0) == (c["t"] == 1)).sum()) for c in (a, b))   # the host count, from PyTorch's logits
    total = sum(float(c["ref"]["terms"].sum()) for c in (a, b))
    got = acc.tolist()
    print("\n[violin] acc/%s loss sum %.6f (float64 %.6f)  right %d  n %d" % (IDS[DTYPES.index(dtype)], got[0], total, got[1], got[2]), end="")
    assert got[1] == right == host and got[2] == 67 + 8
    assert abs(got[0] - total) <= TOL["loss"] * 2 * total                       # a sum of positive terms: the `loss` bound (elem_rel_err halves)
    from hero_amd.violin import ViolinMeter
    meter, host_meter = ViolinMeter(), ViolinMeter()
    for c in (a, b):
        meter.update(c["h"], c["w"], c["b"], c["t"])
        host_meter.update_host(c["t32"]["logits"], c["t"])
    m, hm = meter.compute(), host_meter.compute()
    assert m["acc"] == hm["acc"] == right / 75 and abs(m["loss"] - hm["loss"]) <= TOL["loss"] * 2 * hm["loss"]
    meter2 = ViolinMeter()                                                      # from logits: <(z, 0, 0, 0), (1, 0, 0, 0)> is z exactly
    for c in (a, b):
        z = meter2.update(c["t32"]["logits"], c["t"].view(-1, 1))
        assert torch.equal(z, c["t32"]["logits"])
    assert meter2.compute()["acc"] == hm["acc"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_saturated_logits_keep_a_finite_loss_and_the_stable_gradient(dtype):
    """z in {+-30, +-200} against both labels: the loss is min(softplus, 100), the gradient sigmoid(z) - t over S, no NaN / Inf.
    Judged against the restatement at the floor, relative to max(1, |value|)."""
    zs = [30.0, -30.0, 200.0, -200.0]
    h = torch.zeros(8, 8)
    h[:, 0] = torch.tensor(zs + zs)
    h = h.to(dtype).cuda()                                                        # 30 and 200 are bf16 numbers
    w = torch.tensor([[1.0, 0, 0, 0, 0, 0, 0, 0]], device="cuda")
    b = torch.zeros(1, device="cuda")
    t = torch.tensor([0] * 4 + [1] * 4, device="cuda")
    ref = R.head_forward(h, w, b, t)
    ref.update(R.head_backward(h, w, b, t))
    assert ref["terms"].tolist()[2] == 100.0 and ref["terms"].tolist()[7] == 100.0          # the clamp is reached
    acc = torch.zeros(3, device="cuda")
    logits, loss, dh, dw, db = raw_head(h, w, b, t, acc=acc)
    for x in (logits, loss, dh, dw, db, acc):
        assert bool(torch.isfinite(x.float()).all())
    assert logits.tolist() == zs + zs
    close = lambda got, want: float(((got.double().cpu() - want.cpu()).abs() / want.cpu().abs().clamp_min(1.0)).max())      # noqa: E731
    bf = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0                            # dh is stored in bf16
    e_loss, e_sum, e_dz = close(loss, ref["loss"].reshape(1)), close(acc[:1], ref["terms"].sum().reshape(1)), close(dh[:, 0].float(), ref["dz"])
    e_dw, e_db = close(dw, ref["dw"]), close(db, ref["db"].reshape(1))
    print("\n[violin] saturated/%s loss %.3e  sum %.3e  dz %.3e  dw %.3e  db %.3e  tol %.3e" % (IDS[DTYPES.index(dtype)], e_loss, e_sum, e_dz, e_dw, e_db, FLOOR), end="")
    assert e_loss <= FLOOR and e_sum <= FLOOR and e_dz <= FLOOR + bf and e_dw <= FLOOR and e_db <= FLOOR
    assert acc[1].item() == 4.0                                                   # z > 0 with t = 1, z < 0 with t = 0
    # confidently wrong examples keep their gradient: |dz| = 1 / S where the reference's is 0
    assert abs(dh[2, 0].item() - 1 / 8) <= 1e-6 and abs(dh[7, 0].item() + 1 / 8) <= 1e-6


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_runs_are_bitwise_equal(dtype):
    for name in ("short_L", "recipe", "corner"):
        c = pool_data(name, dtype)
        for x, y in zip(run_pool(c), run_pool(c)):
            assert torch.equal(x, y)
        for x, y in zip(raw_pool(c, 1.0), raw_pool(c, 2.0)):
            assert torch.equal(x, y)
    for name in ("recipe", "S67_K2048"):
        c = head_data(name, dtype)
        for x, y in zip(run_head(c), run_head(c)):
            assert torch.equal(x, y)


def test_outside_the_envelope_is_an_error():
    from hero_amd import _lib as Lb
    from hero_amd.violin import BceHeadFn, FramePoolFn
    z = torch.zeros(16, device="cuda")
    out = torch.full((16,), 9.0, device="cuda")
    p = Lb.ptr(z)
    for S, L, Lt, D in ((1, 257, 257, 64), (1, 4, 513, 64), (1, 4, 3, 64), (1, 4, 4, 1028), (1, 4, 4, 6), (1, 0, 4, 64), (-1, 4, 4, 64)):
        assert Lb.lib().hero_frame_pool_fwd(p, p, p, Lb.ptr(out), Lb.ptr(out), S, L, Lt, D, Lb.F32, Lb.stream()) == -1, (S, L, Lt, D)
        assert "envelope" in Lb.lib().hero_last_error().decode()
        assert Lb.lib().hero_frame_pool_bwd(p, p, p, p, p, Lb.ptr(out), Lb.ptr(out), S, L, Lt, D, Lb.F32, Lb.stream()) == -1, (S, L, Lt, D)
    for S, K in ((0, 8), (2, 6), (2, 2052), (2, 0)):
        assert Lb.lib().hero_bce_head_fwd(p, p, p, p, Lb.ptr(out), Lb.ptr(out), None, S, K, Lb.F32, Lb.stream()) == -1, (S, K)
        assert "envelope" in Lb.lib().hero_last_error().decode()
        assert Lb.lib().hero_bce_head_bwd(p, p, p, p, p, Lb.ptr(out), Lb.ptr(out), Lb.ptr(out), S, K, Lb.F32, Lb.stream()) == -1, (S, K)
    assert Lb.lib().hero_frame_pool_fwd(p, p, p, Lb.ptr(out), Lb.ptr(out), 1, 4, 4, 4, 7, Lb.stream()) == -1       # bad dtype
    assert Lb.lib().hero_frame_pool_fwd(p, p, p, Lb.ptr(out), Lb.ptr(out), 0, 4, 4, 4, Lb.F32, Lb.stream()) == 0    # S == 0: OK, no launch
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())                                               # nothing was launched
    with pytest.raises(ValueError, match="envelope"):
        FramePoolFn.apply(torch.zeros(2, 300, 64, device="cuda"), torch.ones(2, 257, device="cuda"), z[None, :64 // 4], 257)
    with pytest.raises(ValueError, match="envelope"):
        BceHeadFn.apply(torch.zeros(2, 6, device="cuda"), torch.zeros(1, 6, device="cuda"), z[:1], torch.zeros(2, dtype=torch.long, device="cuda"))
