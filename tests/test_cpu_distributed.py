"""world_size-2 gloo tests (CPU) of the data-parallel plumbing that replaces Horovod:
gradient averaging, parameter broadcast, the flat gradient arena with bucketed async all-reduce
(sink interface + stock-autograd hooks) and the cross-GPU negative gather whose backward has no
collective (model/pretrain.py:427-447)."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(rank, world, port, fn, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = fn(rank, world)
    finally:
        dist.destroy_process_group()


def spawn(fn, world=2):
    ret = mp.Manager().dict()
    mp.spawn(_run, args=(world, _free_port(), fn, ret), nprocs=world, join=True)
    return [ret[r] for r in range(world)]


def _avg_and_broadcast(rank, world):
    from hero_amd.utils import distributed as D
    ts = [torch.full((3, 5), float(rank + 1)), torch.arange(7.0) * (rank + 1)]
    D.all_reduce_and_rescale_tensors(ts, 2.0)          # average over ranks, then / 2
    ok = torch.allclose(ts[0], torch.full((3, 5), 1.5 / 2)) and torch.allclose(ts[1], torch.arange(7.0) * 1.5 / 2)
    ps = [torch.full((4,), float(rank)), torch.full((300000,), float(rank) + 5)]
    D.broadcast_tensors(ps, 0, buffer_size=1024)
    ok = ok and float(ps[0].sum()) == 0.0 and float(ps[1][0]) == 5.0
    objs = D.all_gather_list({"r": rank})
    ok = ok and [o["r"] for o in objs] == [0, 1] and D.any_broadcast("x%d" % rank, 1) == "x1"
    return bool(ok)


def test_average_broadcast_objects():
    assert all(spawn(_avg_and_broadcast))


def _arena(rank, world):
    """Two-layer toy model: one parameter goes through stock autograd, one is accumulated by a fake
    'kernel' through the sink interface (two uses per step, like the shared cross-modal encoder)."""
    from hero_amd import functional as HF
    from hero_amd.utils import distributed as D
    torch.manual_seed(0)
    w1 = torch.nn.Parameter(torch.randn(6, 6))
    w2 = torch.nn.Parameter(torch.randn(6, 6))
    w3 = torch.nn.Parameter(torch.randn(5))           # never used -> stays zero, not 'touched'
    arena = D.GradArena([w1, w2, w3], bucket_bytes=64, overlap=True, static_usage=True)

    class SinkMul(torch.autograd.Function):          # y = x @ w2, grad of w2 written via the sink
        @staticmethod
        def forward(ctx, x, w):
            HF.SINK.use(w)
            ctx.save_for_backward(x)
            ctx.w = w
            return x @ w.detach()

        @staticmethod
        def backward(ctx, dy):
            (x,) = ctx.saved_tensors
            HF.SINK.dst(ctx.w).add_(x.t() @ dy)
            HF.SINK.done(ctx.w)
            return dy @ ctx.w.detach().t(), None

    def local_grads(r):
        g = torch.Generator().manual_seed(10 + r)
        x = torch.randn(4, 6, generator=g)
        a, b = w1.detach().clone().requires_grad_(), w2.detach().clone().requires_grad_()
        ((x @ a) @ b + (x @ b)).sum().backward()
        return a.grad, b.grad

    def cycle():
        for micro in range(2):                        # gradient accumulation: sync only on the 2nd
            arena.set_sync(micro == 1)
            g = torch.Generator().manual_seed(10 + rank)
            x = torch.randn(4, 6, generator=g)
            h = x @ w1
            y = SinkMul.apply(h, w2) + SinkMul.apply(x, w2)
            y.sum().backward()
        return sum(arena._launched)                   # buckets all-reduced from the hooks, before finish()

    # buckets: [w3, w2] and [w1].  First cycle: w1's bucket overlaps (the unsynchronised first
    # micro-step must not leave it marked final); the other waits for the never-used w3 until finish().
    overlapped = cycle()
    arena.finish()
    arena.zero()
    # static_usage: from the second optimiser step on, only parameters that got a gradient last step
    # are waited for -> both buckets overlap
    overlapped2 = cycle()
    arena.finish()
    arena.scale_(0.5)                                 # (two cycles' worth of identical gradients / 2 ... see below)
    arena.scale_(2.0 / world)                         # undo the 0.5 above, then average over ranks
    e1 = sum(local_grads(r)[0] for r in range(world)) * 2 / world
    e2 = sum(local_grads(r)[1] for r in range(world)) * 2 / world
    ok = torch.allclose(w1.grad, e1, atol=1e-5) and torch.allclose(w2.grad, e2, atol=1e-5)
    ok = ok and w1.grad.data_ptr() == arena.flat.data_ptr() + arena.slices[w1][0] * 4
    ok = ok and arena.touched == {w1, w2} and float(w3.grad.abs().sum()) == 0.0
    ok = ok and len(arena.buckets) == 2 and overlapped == 1 and overlapped2 == 2
    arena.zero()
    ok = ok and float(arena.flat.abs().sum()) == 0.0 and not arena.touched
    HF.set_grad_sink(None)
    return bool(ok)


def test_grad_arena_bucketed_allreduce():
    assert all(spawn(_arena))


def _arena_intermittent(rank, world):
    """static_usage with a parameter that only some steps use (the st/ed head under drop_svmr_prob,
    model/pretrain.py:74-75): its first appearance holds its bucket back for finish(); afterwards
    the bucket waits for it and falls back to finish() on the steps that skip it."""
    from hero_amd import functional as HF
    from hero_amd.utils import distributed as D
    torch.manual_seed(0)
    w1 = torch.nn.Parameter(torch.randn(6, 6))
    w2 = torch.nn.Parameter(torch.randn(6, 6))
    w3 = torch.nn.Parameter(torch.randn(6))
    arena = D.GradArena([w1, w2, w3], bucket_bytes=64, overlap=True, static_usage=True)
    x = torch.randn(4, 6, generator=torch.Generator().manual_seed(20 + rank))

    def step(use_w3):
        arena.set_sync(True)
        y = (x @ w1) @ w2
        if use_w3:
            y = y * w3                                  # used last in forward -> its gradient is final first
        y.sum().backward()
        launched = sum(arena._launched)
        arena.finish()
        got = [p.grad.clone() for p in (w1, w2, w3)]
        arena.zero()
        return launched, got

    def expect(use_w3):
        out = []
        for r in range(world):
            xr = torch.randn(4, 6, generator=torch.Generator().manual_seed(20 + r))
            a, b, c = (p.detach().clone().requires_grad_() for p in (w1, w2, w3))
            y = (xr @ a) @ b
            if use_w3:
                y = y * c
            y.sum().backward()
            out.append([a.grad, b.grad, c.grad if use_w3 else torch.zeros(6)])
        return [sum(o[i] for o in out) for i in range(3)]

    ok = True
    seen = []
    for use in (False, False, True, False, True):
        launched, got = step(use)
        seen.append(launched)
        ok = ok and all(torch.allclose(g, e, atol=1e-5) for g, e in zip(got, expect(use)))
    # buckets [w3, w2] and [w1]: step 1 nothing is expected yet (w3 never final -> only w1's bucket
    # overlaps); step 2 both; step 3 w3 appears first -> its bucket is held back; step 4 the bucket now
    # waits for w3 in vain; step 5 both overlap again
    ok = ok and seen == [1, 2, 1, 1, 2]
    HF.set_grad_sink(None)
    return bool(ok)


def test_grad_arena_intermittent_parameter():
    assert all(spawn(_arena_intermittent))


def _arena_deferred_done(rank, world):
    """Weight gradients of the HIP backward are queued and launched in groups AFTER their autograd node returned
    (functional.k_wgrad): the arena must take a sink parameter's finality from `done`, not from the AccumulateGrad
    hook that fires when the node returns (found by the 2-rank GPU test: buckets were reduced before the queued
    launch had run)."""
    from hero_amd import functional as HF
    from hero_amd.utils import distributed as D
    torch.manual_seed(0)
    w = torch.nn.Parameter(torch.randn(6, 6))
    v = torch.nn.Parameter(torch.randn(6))
    arena = D.GradArena([w, v], bucket_bytes=1 << 20, overlap=True)
    seen = {}

    class LateSink(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, wt):
            HF.SINK.use(wt)
            ctx.save_for_backward(x)
            ctx.w = wt
            return x @ wt.detach()

        @staticmethod
        def backward(ctx, dy):
            (x,) = ctx.saved_tensors
            wt = ctx.w

            def later():                                   # the "grouped launch" at the end of the backward pass
                seen["launched_before"] = list(arena._launched)
                HF.SINK.dst(wt).add_(x.t() @ dy)
                HF.SINK.done(wt)
            torch.autograd.Variable._execution_engine.queue_callback(later)
            return dy @ wt.detach().t(), None

    arena.set_sync(True)
    x = torch.randn(4, 6, generator=torch.Generator().manual_seed(40 + rank), requires_grad=True)
    (LateSink.apply(x, w) * v).sum().backward()
    launched_in_backward = sum(arena._launched)
    arena.finish()
    want = 0
    for r in range(world):
        xr = torch.randn(4, 6, generator=torch.Generator().manual_seed(40 + r))
        a = w.detach().clone().requires_grad_()
        ((xr @ a) * v.detach()).sum().backward()
        want = want + a.grad
    ok = seen["launched_before"] == [False] and launched_in_backward == 1 and torch.allclose(w.grad, want, atol=1e-5)
    HF.set_grad_sink(None)
    return bool(ok)


def test_grad_arena_finality_of_queued_weight_gradients():
    assert all(spawn(_arena_deferred_done))


def _arena_bf16_wire(rank, world):
    """compress='bf16': the buckets are summed in bf16 on the wire (the reference's fp16 payload) and widened
    back into the fp32 arena; the result is the bf16-rounded sum of the bf16-rounded local gradients."""
    from hero_amd import functional as HF
    from hero_amd.utils import distributed as D
    torch.manual_seed(0)
    w1 = torch.nn.Parameter(torch.randn(40, 6))
    w2 = torch.nn.Parameter(torch.randn(6, 6))
    arena = D.GradArena([w1, w2], bucket_bytes=64, overlap=True, compress="bf16")

    def local(r):
        x = torch.randn(4, 40, generator=torch.Generator().manual_seed(30 + r))
        a, b = w1.detach().clone().requires_grad_(), w2.detach().clone().requires_grad_()
        ((x @ a) @ b).sum().backward()
        return a.grad, b.grad

    arena.set_sync(True)
    x = torch.randn(4, 40, generator=torch.Generator().manual_seed(30 + rank))
    ((x @ w1) @ w2).sum().backward()
    arena.finish()
    ok = True
    for p, i in ((w1, 0), (w2, 1)):
        want = sum(local(r)[i].to(torch.bfloat16).float() for r in range(world))
        ok = ok and torch.allclose(p.grad, want, rtol=2 ** -7, atol=1e-3) and p.grad.dtype == torch.float32
    HF.set_grad_sink(None)
    return bool(ok)


def test_grad_arena_bf16_wire_format():
    assert all(spawn(_arena_bf16_wire))


def _arena_forced_one_rank(rank, world):
    """HERO_DP_FORCE_COLLECTIVES=1 with ONE rank (how the RCCL path is exercised on a 1-GPU box): the buckets go
    through the process group although world_size == 1, and the gradients equal the unsynchronised ones."""
    import os
    from hero_amd import functional as HF
    from hero_amd.utils import distributed as D
    assert world == 1 and not D.collectives_active()
    os.environ["HERO_DP_FORCE_COLLECTIVES"] = "1"
    try:
        assert D.collectives_active()
        torch.manual_seed(0)
        w1 = torch.nn.Parameter(torch.randn(40, 6))
        w2 = torch.nn.Parameter(torch.randn(6, 6))
        arena = D.GradArena([w1, w2], bucket_bytes=64, overlap=True, compress="bf16")
        x = torch.randn(4, 40)
        arena.set_sync(True)
        ((x @ w1) @ w2).sum().backward()
        launched = sum(arena._launched)
        arena.finish()
        a, b = w1.detach().clone().requires_grad_(), w2.detach().clone().requires_grad_()
        ((x @ a) @ b).sum().backward()
        ok = launched >= 1 and len(arena._wire) == len(arena.buckets)
        ok = ok and torch.allclose(w1.grad, a.grad.to(torch.bfloat16).float()) and torch.allclose(w2.grad, b.grad.to(torch.bfloat16).float())
    finally:
        del os.environ["HERO_DP_FORCE_COLLECTIVES"]
        HF.set_grad_sink(None)
    return bool(ok)


def test_forced_collectives_with_one_rank():
    assert all(spawn(_arena_forced_one_rank, world=1))


def _negatives(rank, world):
    from hero_amd.utils import distributed as D
    torch.manual_seed(rank)
    nq, nv, ln = 2 + rank, 2 + rank, 3 + 2 * rank      # different sizes per rank
    q = torch.randn(nq, 4, requires_grad=True)
    c = torch.randn(nv, ln, 4, requires_grad=True)
    m = torch.ones(nv, ln, dtype=torch.long)
    Q, Cx, M = D.gather_negatives(q, c, m)
    ok = Q.shape == (5, 4) and Cx.shape == (5, 5, 4) and M.shape == (5, 5)
    off = 0 if rank == 0 else 2
    ok = ok and torch.equal(Q[off:off + nq], q.detach()) and torch.equal(Cx[off:off + nv, :ln], c.detach())
    ok = ok and float(M[:2, 3:].sum()) == 0 and float(M[2:].sum()) == 15       # rank 0's clips padded
    w = torch.arange(5.0).view(5, 1)
    ((Q * w).sum() + (Cx * w.view(5, 1, 1)).sum()).backward()
    ok = ok and torch.allclose(q.grad, w[off:off + nq].expand(nq, 4))          # own slice only
    ok = ok and torch.allclose(c.grad, w[off:off + nv].view(nv, 1, 1).expand(nv, ln, 4))
    return bool(ok)


def test_gather_negatives_slice_backward():
    assert all(spawn(_negatives))


def _negatives_uniform(rank, world):
    """UNIFORM_SHAPES: every rank feeds the same padded shape, so the per-forward size exchange is skipped - the gather
    and its slice backward must equal the exchanging path's."""
    from hero_amd.utils import distributed as D
    torch.manual_seed(rank)
    q = torch.randn(3, 4, requires_grad=True)
    c = torch.randn(3, 5, 4, requires_grad=True)
    m = (torch.rand(3, 5) > 0.3).long()
    res = []
    for uniform in (False, True):
        D.UNIFORM_SHAPES[0] = uniform
        try:
            Q, Cx, M, own = D.gather_negatives(q, c, m, return_own=True)
        finally:
            D.UNIFORM_SHAPES[0] = False
        q.grad = c.grad = None
        w = torch.arange(6.0).view(6, 1)
        ((Q * w).sum() + (Cx * w.view(6, 1, 1)).sum()).backward()
        res.append((Q.detach().clone(), Cx.detach().clone(), M.clone(), own, q.grad.clone(), c.grad.clone()))
    a, b = res
    ok = all(torch.equal(x, y) for x, y in zip(a[:3] + a[4:], b[:3] + b[4:])) and a[3] == b[3] == (3 * rank, 3)
    return bool(ok)


def test_gather_negatives_uniform_shapes_skips_the_size_exchange():
    assert all(spawn(_negatives_uniform))


def _meta_loader(rank, world):
    """MetaLoader (data/loader.py:19-59): with distributed=True every rank follows rank 0's task draws although the
    ranks' own random streams differ; a window of accum_steps micro-steps stays on one task; loaders restart."""
    import random
    from hero_amd.loader import MetaLoader
    random.seed(100 + rank)                                     # different streams: only the broadcast can align them
    loaders = {"mlm": ([("mlm", rank, i) for i in range(3)], 2), "vsm": ([("vsm", rank, i) for i in range(5)], 1)}
    ml = MetaLoader(loaders, accum_steps=2, distributed=True)
    seq = []
    for k, (task, batch) in enumerate(ml):
        assert batch[0] == task and batch[1] == rank
        seq.append((task, batch[2]))
        if k == 39:
            break
    return seq


def test_meta_loader_ranks_follow_rank0():
    a, b = spawn(_meta_loader)
    assert a == b                                               # same tasks AND same positions inside each task's loader
    tasks = [t for t, _ in a]
    assert all(tasks[i] == tasks[i + 1] for i in range(0, 40, 2))          # accumulation windows are single-task
    assert {"mlm", "vsm"} == set(tasks)
    mlm_pos = [i for t, i in a if t == "mlm"]
    assert mlm_pos[:4] == [0, 1, 2, 0]                          # restarted after three batches


def test_meta_loader_single_process_contract():
    import random
    import pytest
    from torch.utils.data import DataLoader
    from hero_amd.loader import MetaLoader
    with pytest.raises(ValueError):
        MetaLoader({"a": [1, 2, 3]})                             # neither a DataLoader nor (loader, ratio)
    dl = DataLoader(list(range(4)), batch_size=2)
    ml = MetaLoader({"a": dl, "b": (["x"], 3)}, accum_steps=1)
    assert ml.sampling_pools == ["a", "b", "b", "b"] and ml.step == 0
    random.seed(0)
    got = []
    for task, batch in ml:
        got.append(task)
        if len(got) == 400:
            break
    assert ml.step == 400 and 0.65 < got.count("b") / 400 < 0.85           # ratio 3 : 1


def test_bench_launch_command_for_a_plain_gpus_n():
    """`python bench.py --gpus N` without a launcher runs the driver's own N > 1 command line as a child process (VERDICT r4
    next #1): one process per GPU under torch.distributed.run on 127.0.0.1; with fewer devices than ranks the ranks share
    device 0 over gloo (a plumbing run)."""
    import importlib
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in _sys.path:
        _sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    cmd, env = bench.launch_command(8, ["--gpus", "8", "--steps", "20"], n_devices=8, port=29500)
    assert cmd[:3] == [_sys.executable, "-m", "torch.distributed.run"] and "--nnodes=1" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-5].endswith("bench.py") and cmd[-4:] == ["--gpus", "8", "--steps", "20"]
    assert env["MASTER_ADDR"] == "127.0.0.1" and "HERO_BENCH_ONE_DEVICE" not in env and env["HSA_ENABLE_IPC_MODE_LEGACY"]
    cmd, env = bench.launch_command(2, ["--gpus", "2"], n_devices=1)
    assert env["HERO_BENCH_ONE_DEVICE"] == "1" and env["HERO_BENCH_BACKEND"] == "gloo"
    assert int(cmd[cmd.index("--master-port") + 1]) > 0
    # under a launcher (WORLD_SIZE set) or with one GPU asked for, nothing is launched
    import argparse
    old = dict(os.environ)
    try:
        os.environ["WORLD_SIZE"] = "2"
        assert bench.self_launch(argparse.Namespace(gpus=2)) is None
        os.environ.pop("WORLD_SIZE")
        os.environ.pop("RANK", None)
        assert bench.self_launch(argparse.Namespace(gpus=1)) is None
    finally:
        os.environ.clear()
        os.environ.update(old)


def test_bench_dump_outputs_writes_a_fixed_float_sample(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR`: the last micro-step's loss and a seeded sample of the parameters and of their gradients,
    float .npy files only, the same positions in every run, a parameter without a gradient sampled as zeros."""
    import importlib
    import sys as _sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in _sys.path:
        _sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 20, bias=False))
    model(torch.randn(5, 40)).sum().backward()
    model[1].weight.grad = None
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, torch.tensor(1.25))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grads_sample.npy", "loss.npy", "params_sample.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == 1.25
    p, g = np.load(tmp_path / "a" / "params_sample.npy"), np.load(tmp_path / "a" / "grads_sample.npy")
    flat_p = torch.cat([q.detach().reshape(-1) for q in model.parameters()]).numpy()
    n_first = 40 * 30 + 30                                    # the second layer (no gradient) starts here
    idx = torch.randint(0, flat_p.size, (1000,), generator=torch.Generator().manual_seed(0)).sort().values.numpy()
    assert p.shape == (1000,) and np.array_equal(p, flat_p[idx])
    assert (g[idx >= n_first] == 0).all() and (g[idx < n_first] != 0).any()
