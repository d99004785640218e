"""The device-gated entry points hero_st_ed_fwd_gated / hero_st_ed_bwd_gated (hero_amd/csrc/head.hip) and hero_adamw_multi_gated
(hero_amd/csrc/rows.hip) through the raw ctypes ABI.

Gate on: every output carries the bits of the ungated entry point on the same inputs, and agrees with the float64 statements
(tests/head_reference.st_ed_loss, tests/optim_reference.adamw_ref) under the tolerances that tests/test_gpu_head_kernels.py and
tests/test_gpu_optim_kernels.py carry for these kernels.  Gate off: exact zeros (or nothing at all) where the header says so, no
input read - NaN planted in the saved tensors, the frame embeddings and the upstream gradient reaches no output - and the arrival
ticket of the backward left at zero.  Captured launches follow the gate word of each replay.

Shapes: B in {1, 3, 65} (65: a second 64-share chunk in the last-arrival fold), L in {5, 61} (the 4-frame trip plus a tail),
D in {128, 1028} (1028: a second d += 1024 trip), K = 5, fp32 and bf16 frame embeddings; a -1 target wherever B leaves the
column another valid row (B >= 3).

Inputs: those of tests/test_gpu_head_kernels.py (_sted_inputs), with q2 scaled by sqrt(128 / D) so that the similarities keep
the magnitude they have at D = 128 whatever D is.  Unscaled, the lone pair of B = 1, L = 5, D = 1028 has an end softmax of
p = 0.99999152 at its target, and dw_ed = sum (p - 1) * sim starts from a p that was SAVED in fp32: 2^-24 / (1 - p) = 7e-3 of
relative error in the data the backward is handed, before any arithmetic (2.56e-3 in dw_ed, reproduced in float64 on the CPU from
the rounded p alone) - a statement about that input, not about a kernel, gated or not."""
import ctypes as C

import pytest
import torch

from tests import head_reference as HR
from tests import optim_reference as OR
from tests.test_gpu_head_kernels import Report, _sted_inputs, bits
from tests.test_gpu_optim_kernels import Guarded, adamw_t32
from tests.test_gpu_optim_kernels import Report as OptimReport
from tests.test_gpu_optim_kernels import same_bits

pytestmark = pytest.mark.gpu

K = 5
SENT = 7.25
G_UP, G_SCALE = 2.5, 0.7


@pytest.fixture(scope="module")
def Lb():
    from hero_amd import _lib
    _lib.lib()
    return _lib


def all_plus_zero(t):
    return bool((bits(t) == 0).all())


def word(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def sted_inputs(B, L, D, dtype):
    q2, ctx, mask, w_st, w_ed, tg = _sted_inputs(B, L, D, K, dtype)
    q2 = q2 * (128.0 / D) ** 0.5
    if B == 3:
        tg[1, 0] = -1                                          # rows 0 and 2 keep the start column valid
    assert B < 3 or bool((tg == -1).any())
    return q2, ctx, mask, w_st, w_ed, tg


class StEdRun:
    """One set of inputs on the device with its own output buffers and workspace; fwd() / bwd() launch the plain entry points
    (gate=None) or the gated ones."""

    INIT = torch.tensor([3.0, -1.0, 0.5, 0.0, 7.0])

    def __init__(self, Lb, cpu, ws=None, init=None):
        from hero_amd.head import StEdLossFn
        self.Lb = Lb
        self.q2, self.ctx, self.mask, self.w_st, self.w_ed, self.tg = [t.cuda() for t in cpu]
        B, L, D = self.ctx.shape
        self.rows = torch.full((B,), 9.0, device="cuda")
        self.saved = torch.full((3, B, L), SENT, device="cuda")
        self.dq2, self.dctx = torch.full_like(self.q2, 9.0), torch.full_like(self.ctx, 9.0)
        init = self.INIT if init is None else init              # dw_st / dw_ed accumulate: what they hold before the call
        self.dws, self.dwe = init.clone().cuda(), (-init).clone().cuda()
        self.g = torch.tensor([G_UP], device="cuda")
        self.ws = torch.zeros(Lb.lib().hero_st_ed_bwd_workspace_bytes(B) // 4, device="cuda") if ws is None else ws
        self.a = StEdLossFn._args(self.q2, self.ctx, self.mask, self.w_st, self.w_ed, self.tg, self.saved, K)
        a = self.a
        a.loss_rows, a.g, a.g_scale = Lb.ptr(self.rows), Lb.ptr(self.g), G_SCALE
        a.dq2, a.dctx, a.dw_st, a.dw_ed, a.ws = Lb.ptr(self.dq2), Lb.ptr(self.dctx), Lb.ptr(self.dws), Lb.ptr(self.dwe), Lb.ptr(self.ws)

    def fwd(self, gate=None):
        lib = self.Lb.lib()
        if gate is None:
            self.Lb.check(lib.hero_st_ed_fwd(C.byref(self.a), self.Lb.stream()))
        else:
            self.Lb.check(lib.hero_st_ed_fwd_gated(C.byref(self.a), self.Lb.ptr(gate), self.Lb.stream()))

    def bwd(self, gate=None):
        lib = self.Lb.lib()
        if gate is None:
            self.Lb.check(lib.hero_st_ed_bwd(C.byref(self.a), self.Lb.stream()))
        else:
            self.Lb.check(lib.hero_st_ed_bwd_gated(C.byref(self.a), self.Lb.ptr(gate), self.Lb.stream()))

    def outputs(self):
        return dict(loss_rows=self.rows, p_st=self.saved[0], p_ed=self.saved[1], sim=self.saved[2], dq2=self.dq2, dctx=self.dctx,
                    dw_st=self.dws, dw_ed=self.dwe)


SHAPES = [(B, L, D) for B in (1, 3, 65) for L in (5, 61) for D in (128, 1028)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,L,D", SHAPES)
def test_st_ed_gate_on_is_the_ungated_kernel(Lb, dtype, B, L, D):
    cpu = sted_inputs(B, L, D, dtype)
    plain, gated = StEdRun(Lb, cpu, init=torch.zeros(K)), StEdRun(Lb, cpu, init=torch.zeros(K))
    one = word(1)
    plain.fwd()
    plain.bwd()
    gated.fwd(one)
    gated.bwd(one)
    torch.cuda.synchronize()
    for (name, x), y in zip(plain.outputs().items(), gated.outputs().values()):
        assert torch.equal(bits(x), bits(y)), name
    assert bits(gated.ws[B * 32:]).tolist() == [0, 0, 0, 0]
    # the float64 statement
    q2, ctx, mask, w_st, w_ed, tg = cpu
    qr, cr, wsr, wer = HR.leaf(q2), HR.leaf(ctx), HR.leaf(w_st), HR.leaf(w_ed)
    ref, sim = HR.st_ed_loss(qr, cr, mask.double(), wsr, wer, tg)
    (G_UP * G_SCALE * ref).backward()
    m64 = mask.double()
    p_st = torch.softmax(HR.mask_logits(HR.conv1d_same(sim.detach(), wsr.detach().reshape(-1)), m64), 1)
    p_ed = torch.softmax(HR.mask_logits(HR.conv1d_same(sim.detach(), wer.detach().reshape(-1)), m64), 1)
    rep = Report("st_ed", "gated %s B=%d L=%d D=%d" % (str(dtype)[6:], B, L, D))
    rep.scalar("loss", gated.rows.double().sum().cpu(), ref.detach())
    rep.tensor("sim", gated.saved[2], sim)
    rep.tensor("p_st", gated.saved[0], p_st)
    rep.tensor("p_ed", gated.saved[1], p_ed)
    rep.tensor("dq2", gated.dq2, qr.grad)
    rep.tensor("dctx", gated.dctx, cr.grad)
    rep.tensor("dw_st", gated.dws, wsr.grad.reshape(-1))
    rep.tensor("dw_ed", gated.dwe, wer.grad.reshape(-1))
    rep.done()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,L,D", SHAPES)
def test_st_ed_gate_off_writes_zeros_reads_nothing_and_leaves_the_ticket(Lb, dtype, B, L, D):
    cpu = sted_inputs(B, L, D, dtype)
    off, one = word(0), word(1)
    run = StEdRun(Lb, cpu)
    run.fwd(off)
    torch.cuda.synchronize()
    assert bits(run.rows).tolist() == [0] * B                                     # +0.0f, every workgroup
    assert bool((run.saved == SENT).all())                                        # p_st / p_ed / sim keep their bytes
    # backward: NaN in everything it must not read
    run.saved.fill_(float("nan"))
    run.ctx.fill_(float("nan"))
    run.g.fill_(float("nan"))
    run.bwd(off)
    torch.cuda.synchronize()
    assert all_plus_zero(run.dq2) and all_plus_zero(run.dctx)                      # exact +0 in dctx's dtype
    assert torch.equal(bits(run.dws), bits(StEdRun.INIT)) and torch.equal(bits(run.dwe), bits(-StEdRun.INIT))
    assert all_plus_zero(run.ws)                                                  # shares and ticket untouched
    # a gate-on backward right behind it on the same workspace == one on a fresh workspace
    after, fresh = StEdRun(Lb, cpu, ws=run.ws), StEdRun(Lb, cpu)
    for r in (after, fresh):
        r.fwd(one)
        r.bwd(one)
    torch.cuda.synchronize()
    for (name, x), y in zip(after.outputs().items(), fresh.outputs().values()):
        assert torch.equal(bits(x), bits(y)), name
    assert float(after.dq2.abs().max()) > 0 and bool(torch.isfinite(after.dctx.float()).all())


@pytest.mark.parametrize("dtype,B,L,D", [(torch.float32, 65, 61, 128), (torch.bfloat16, 3, 5, 1028)], ids=["fp32", "bf16"])
def test_st_ed_one_captured_pair_follows_the_gate_word(Lb, dtype, B, L, D):
    cpu = sted_inputs(B, L, D, dtype)
    run = StEdRun(Lb, cpu)
    gate = word(1)
    run.fwd(gate)                                               # every lazy state of the launches exists before the capture
    run.bwd(gate)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run.fwd(gate)
        run.bwd(gate)
    seen = []
    for v in (1, 0, 1):
        gate.fill_(v)
        run.dws.copy_(StEdRun.INIT)                             # the accumulators start over; the rest is overwritten
        run.dwe.copy_(-StEdRun.INIT)
        graph.replay()
        torch.cuda.synchronize()
        seen.append({k: t.clone() for k, t in run.outputs().items()})
    for k in seen[0]:
        assert torch.equal(bits(seen[0][k]), bits(seen[2][k])), k
    assert float(seen[0]["loss_rows"].abs().sum()) > 0 and float(seen[0]["dq2"].abs().max()) > 0
    z = seen[1]
    assert bits(z["loss_rows"]).tolist() == [0] * B
    assert all_plus_zero(z["dq2"]) and all_plus_zero(z["dctx"])
    assert torch.equal(bits(z["dw_st"]), bits(StEdRun.INIT)) and torch.equal(bits(z["dw_ed"]), bits(-StEdRun.INIT))
    for k in ("p_st", "p_ed", "sim"):                           # what replay 1 left
        assert torch.equal(bits(z[k]), bits(seen[0][k])), k


# ---- hero_adamw_multi_gated ---------------------------------------------------------------------------------------------
SIZES = [5, OR.CHUNK + 7, 4096]                                 # two chunks for the second tensor, and the scalar tails
GROUP_OF = [0, 1, 0]
SLOT_OF = [4, 1, 6]
START = [100, 3, 102, 103, 0, 105, 11, 107]                     # slot 4: a fresh tensor (step 1); slots 1 and 6: steps 4 and 12


def adamw_case():
    out = []
    for i, n in enumerate(SIZES):
        gen = torch.Generator().manual_seed(8100 + i)
        g = OR.log_uniform_grad(n, gen)
        p = torch.randn(n, generator=gen)
        if START[SLOT_OF[i]] == 0:
            m, v = torch.zeros(n), torch.zeros(n)
        else:
            m = 0.1 * torch.randn(n, generator=gen)
            v = m * m * (0.5 + 1.5 * torch.rand(n, generator=gen))
        out.append(dict(n=n, group=GROUP_OF[i], p=p, g=g, m=m, v=v))
    return out


class AdamRun:
    def __init__(self, Lb, tensors):
        self.Lb, self.tensors = Lb, tensors
        self.dev = [{k: Guarded(t[k]) for k in "pgmv"} for t in tensors]
        descs = (Lb.TensorDesc * len(tensors))()
        chunks = []
        for i, (t, d) in enumerate(zip(tensors, self.dev)):
            descs[i] = Lb.TensorDesc(d["p"].ptr(), d["g"].ptr(), d["m"].ptr(), d["v"].ptr(), t["n"], t["group"], SLOT_OF[i])
            chunks += [(i, c) for c in range(-(-t["n"] // OR.CHUNK))]
        assert len(chunks) == 4
        self.descs = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
        self.ct = torch.tensor([c[0] for c in chunks], dtype=torch.int32).cuda()
        self.ci = torch.tensor([c[1] for c in chunks], dtype=torch.int32).cuda()
        self.counters = Guarded(torch.tensor(START, dtype=torch.int32), dtype=torch.int32)
        a = self.a = Lb.AdamWMulti()
        a.descs, a.chunk_tensor, a.chunk_index, a.n_chunks = self.descs.data_ptr(), self.ct.data_ptr(), self.ci.data_ptr(), len(chunks)
        for gi in range(8):
            a.groups[gi] = Lb.AdamWGroup(*(OR.GROUPS[gi] if gi < 2 else [float("nan")] * 5))
        a.step, a.grad_scale, a.max_grad_norm = 1, 1.0, 0.0
        a.tensor_steps, a.n_tensors = self.counters.ptr(), len(tensors)

    def launch(self, table="plain"):
        Lb = self.Lb
        if isinstance(table, str):
            rc = Lb.lib().hero_adamw_multi(C.byref(self.a), Lb.stream())
        else:
            rc = Lb.lib().hero_adamw_multi_gated(C.byref(self.a), Lb.ptr(table), Lb.stream())
        assert rc == 0, Lb.lib().hero_last_error()

    def out(self, i):
        return tuple(self.dev[i][k].t.clone() for k in "pmv")

    def guards_ok(self):
        for d in self.dev:
            assert all(d[k].intact() for k in "pgmv")
        assert self.counters.intact()


def check_pattern(run, plain, pattern, tensors, calls=1):
    """`run` after `calls` gated launches under `pattern` against the untouched inputs (gated-off tensors) and `plain` after as many
    ungated launches (gated-on tensors)."""
    want = list(START)
    for i, t in enumerate(tensors):
        if pattern[i]:
            want[SLOT_OF[i]] += calls
            for x, y in zip(run.out(i), plain.out(i)):
                assert same_bits(x, y), (pattern, i)
        else:
            for x, k in zip(run.out(i), "pmv"):
                assert same_bits(x.cpu(), t[k]), (pattern, i, k)
    assert run.counters.t.tolist() == want, pattern
    run.guards_ok()


@pytest.fixture(scope="module")
def adam_plain(Lb):
    """The ungated launch on the case's inputs, once: what every gated-on tensor must equal - itself held against float64."""
    tensors = adamw_case()
    plain = AdamRun(Lb, tensors)
    plain.launch()
    torch.cuda.synchronize()
    rep = OptimReport("gated/plain")
    for i, t in enumerate(tensors):
        step = START[SLOT_OF[i]] + 1
        hp = OR.group_f32(t["group"])
        ref = OR.adamw_ref(t["p"], t["g"], t["m"], t["v"], step, *hp)
        tf = adamw_t32(t["p"], t["g"], t["m"], t["v"], step, *hp, gscale=torch.tensor(1.0, device="cuda"))
        got = plain.out(i)
        for grp, x, r, f in zip(("p", "m", "v"), got, ref, tf):
            rep.tensor(grp, "n%d" % t["n"], x, r, f)
    rep.done()
    return tensors, plain


@pytest.mark.parametrize("pattern", [(1, 0, 1), (0, 0, 0), (1, 1, 1), None], ids=["101", "000", "111", "null"])
def test_adamw_multi_gated_skips_whole_tensors(Lb, adam_plain, pattern):
    tensors, plain = adam_plain
    run = AdamRun(Lb, tensors)
    if pattern is None:                                          # a NULL table is the ungated call
        rc = Lb.lib().hero_adamw_multi_gated(C.byref(run.a), None, Lb.stream())
        assert rc == 0
        pattern = (1, 1, 1)
    else:
        if not any(pattern):                                     # nothing may be read: NaN gradients and moments stay where they are
            for d in run.dev:
                d["g"].t.fill_(float("nan"))
            tensors = [dict(t, g=torch.full_like(t["g"], float("nan"))) for t in tensors]
        run.launch(torch.tensor(pattern, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    check_pattern(run, plain, pattern, tensors)


def test_adamw_multi_gated_needs_device_step_counts(Lb, adam_plain):
    run = AdamRun(Lb, adam_plain[0])
    run.a.tensor_steps = None
    assert Lb.lib().hero_adamw_multi_gated(C.byref(run.a), Lb.ptr(word(1)), Lb.stream()) != 0
    assert "tensor_steps" in Lb.lib().hero_last_error().decode()
    torch.cuda.synchronize()
    check_pattern(run, None, (0, 0, 0), adam_plain[0])


def test_adamw_multi_gated_captured_launch_follows_each_replay(Lb, adam_plain):
    tensors, plain = adam_plain
    table = torch.ones(3, dtype=torch.int32, device="cuda")
    warm = AdamRun(Lb, tensors)
    warm.launch(table)
    torch.cuda.synchronize()
    run = AdamRun(Lb, tensors)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run.launch(table)
    table.copy_(torch.tensor([0, 1, 0], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    check_pattern(run, plain, (0, 1, 0), tensors)
    # the second replay updates the others; tensor 1 stays at its one step
    table.copy_(torch.tensor([1, 0, 1], dtype=torch.int32))
    second = {1: run.out(1)}
    graph.replay()
    torch.cuda.synchronize()
    for i in (0, 2):
        for x, y in zip(run.out(i), plain.out(i)):
            assert same_bits(x, y), i
    for x, y in zip(run.out(1), second[1]):
        assert same_bits(x, y)
    assert run.counters.t.tolist() == [s + 1 if j in SLOT_OF else s for j, s in enumerate(START)]
    run.guards_ok()
