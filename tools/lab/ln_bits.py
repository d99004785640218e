#!/usr/bin/env python3
"""Raw bits of the LayerNorm and column-sum kernels (layernorm.hip) on a fixed list of small cases, to compare two library
builds - a refactor of the kernels must not move one bit.

  python tools/lab/ln_bits.py save OUT.pt        run every case, torch.save the results
  python tools/lab/ln_bits.py compare A.pt B.pt   torch.equal on the raw bytes, per case and tensor; exit status 1 on a difference

One `save` process per build (HERO_HIP_LIB selects the library), then `compare`.

Cases: every (x dtype, y / dy dtype) pair x {straight-line (cols % 256 == 0), general (a partial last chunk), wide (cols > 1024:
dx kernel + two-stage column reduction)} through HF.k_ln_fwd and HF.k_ln_bwd, with and without each dropout, grad_beta 0 and 1,
with and without dbias_in, more than 4096 rows (second grid-stride trip of the fused backward); the forward with embedding
tables and want_pre; hero_layernorm_bwd with defer_fold = 1 and the hero_colsum_multi that folds its partials; HF.k_colsum
(no rows, fewer rows than row-lanes, a column offset, both dtypes) and hero_colsum_multi with mixed problems.

Every tensor the kernels write (the results k_ln_fwd / k_ln_bwd allocate included) is the middle of a larger buffer
pre-filled with a bit pattern, and the whole buffer is saved: what the kernels must leave alone is compared too."""
import ctypes as C
import os, sys
sys.path.insert(0, os.getcwd())
import torch

F32, BF16 = torch.float32, torch.bfloat16
SENT = 0x5A
G = 1024                                  # guard elements on either side


def guarded(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    big = _EMPTY(n + 2 * G, dtype=dtype, device="cuda")
    big.view(torch.uint8).fill_(SENT)
    return big, big[G:G + n].view(*shape)


_EMPTY, _EMPTY_LIKE = torch.empty, torch.empty_like


class Guard:
    """While active, torch.empty / torch.empty_like of GPU tensors hand out guarded buffers (the 1M-float workspaces of
    functional.py excepted); .bufs holds the whole buffers in allocation order."""

    def __enter__(self):
        self.bufs = []

        def empty(*size, dtype=None, device=None, **kw):
            shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
            if device is None or torch.device(device).type != "cuda" or (len(shape) == 1 and shape[0] >= (1 << 20)):
                return _EMPTY(*size, dtype=dtype, device=device, **kw)
            big, view = guarded(shape, dtype or F32)
            self.bufs.append(big)
            return view

        torch.empty = empty
        torch.empty_like = lambda t, **kw: empty(tuple(t.shape), dtype=t.dtype, device=t.device)
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like = _EMPTY, _EMPTY_LIKE

    def add(self, shape, dtype, fill):
        big, view = guarded(shape, dtype)
        view.fill_(fill)
        self.bufs.append(big)
        return view

    def result(self):
        torch.cuda.synchronize()
        return {"buf%02d" % i: b.view(torch.uint8).cpu() for i, b in enumerate(self.bufs)}


def rnd(*shape, dtype=F32, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16)]                      # (x, y / dy)
FORMS = [("line", 37, 768), ("line", 4101, 256), ("general", 37, 516), ("general", 9, 132), ("wide", 21, 1028), ("wide", 70, 1540)]
NAME = {F32: "f32", BF16: "bf16"}


def run_all(HF, Lb):
    res = {}
    dev = torch.device("cuda:0")
    HF.manual_seed(1234, "cuda:0")
    mk = lambda on: HF.RNG.make(0.1, True, dev) if on else None      # noqa: E731
    for xd, yd in PAIRS:
        for form, rows, cols in FORMS:
            tag = "%s/%s %s %dx%d" % (NAME[xd], NAME[yd], form, rows, cols)
            x = rnd(rows, cols, dtype=xd, seed=1) * 2 + 0.5
            g, b = rnd(cols, seed=2) * 0.1 + 1, rnd(cols, seed=3) * 0.1
            dy = rnd(rows, cols, dtype=yd, seed=4)
            for drop in (0, 1):
                with Guard() as gd:
                    _, mean, rstd, _ = HF.k_ln_fwd(x, g, b, 1e-12, yd, rows, cols, drop=mk(drop))
                    res["%s fwd drop%d" % (tag, drop)] = gd.result()
            for d_out in (0, 1):
                for d_in in (0, 1):
                    for gb in (0, 1):
                        with Guard() as gd:
                            kw = {}
                            if gb:
                                kw = dict(dgamma=gd.add((cols,), F32, 1.0), dbeta=gd.add((cols,), F32, 2.0), grad_beta=1.0)
                                if cols <= 1024 and d_in:
                                    kw["dbias_in"] = gd.add((cols,), F32, 3.0)
                            HF.k_ln_bwd(x, dy, g, mean, rstd, drop_out=mk(d_out), drop_in=mk(d_in), **kw)
                            res["%s bwd out%d in%d beta%d" % (tag, d_out, d_in, gb)] = gd.result()
            if cols <= 1024 and rows < 100:                          # defer_fold = 1, then the multi-fold of the partials
                with Guard() as gd:
                    nblk = Lb.lib().hero_layernorm_bwd_blocks(rows)
                    part = gd.add((nblk, 3 * cols), F32, 0.0)
                    dst = [gd.add((cols,), F32, 1.0 + k) for k in range(3)]
                    a = Lb.LnBwd()
                    a.x, a.dy, a.gamma, a.mean, a.rstd = x.data_ptr(), dy.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr()
                    a.dx = gd.add((rows, cols), yd, 0.0).data_ptr()
                    a.dgamma, a.dbeta, a.dbias_in = [t.data_ptr() for t in dst]
                    a.grad_beta, a.workspace, a.rows, a.cols, a.defer_fold = 1.0, part.data_ptr(), rows, cols, 1
                    a.x_dtype, a.dtype = Lb.dt(x), Lb.dt(dy)
                    a.dropout_out, a.dropout_in = Lb.no_dropout(), Lb.no_dropout()
                    Lb.check(Lb.lib().hero_layernorm_bwd(C.byref(a), Lb.stream()))
                    p3 = (Lb.Colsum * 3)(*[Lb.Colsum(part.data_ptr() + 4 * k * cols, t.data_ptr(), nblk, cols, 3 * cols, Lb.F32, 1.0)
                                           for k, t in enumerate(dst)])
                    w3 = _EMPTY(Lb.lib().hero_colsum_multi_workspace_bytes(p3, 3) // 4 + 1, device="cuda")
                    Lb.check(Lb.lib().hero_colsum_multi(p3, 3, w3.data_ptr(), Lb.stream()))
                    res["%s bwd defer_fold" % tag] = gd.result()
    # forward with embedding tables, with and without x, the sum kept (want_pre)
    for cols in (768, 516):
        rows = 37
        t0, t1 = rnd(50, cols, seed=4), rnd(7, cols, seed=5)
        i0 = torch.randint(0, 50, (rows,), generator=torch.Generator().manual_seed(6)).int().cuda()
        i1 = torch.randint(0, 7, (rows,), generator=torch.Generator().manual_seed(7)).int().cuda()
        g, b = rnd(cols, seed=2) * 0.1 + 1, rnd(cols, seed=3) * 0.1
        for xd, yd in PAIRS:
            for with_x in (0, 1):
                if not with_x and xd != yd:
                    continue
                with Guard() as gd:
                    HF.k_ln_fwd(rnd(rows, cols, dtype=xd, seed=1) if with_x else None, g, b, 1e-5, yd, rows, cols, tabs=[t0, t1, t1[3:4]],
                                idxs=[i0, i1, None], want_pre=True, drop=mk(with_x), device=dev)
                    res["%s/%s tables %dx%d x%d" % (NAME[xd], NAME[yd], rows, cols, with_x)] = gd.result()
    # plain column sums
    for dt in (F32, BF16):
        for rows, cols, ld, col0 in ((0, 8, 16, 0), (3, 8, 16, 8), (70, 132, 132, 0), (1000, 768, 2304, 768), (5000, 260, 264, 4)):
            for beta in (0.0, 1.0):
                with Guard() as gd:
                    src, out = rnd(max(rows, 1), ld, dtype=dt, seed=8), gd.add((cols,), F32, 0.5)
                    if rows:
                        HF.k_colsum(src, out=out, beta=beta, col0=col0, ncols=cols)
                    else:                                            # (an empty tensor has no device pointer to hand to k_colsum)
                        ws = _EMPTY(Lb.lib().hero_colsum_workspace_bytes(rows, cols) // 4, device="cuda")
                        Lb.check(Lb.lib().hero_colsum(src.data_ptr(), out.data_ptr(), 0, cols, ld, Lb.dt(src), beta, ws.data_ptr(), Lb.stream()))
                    res["%s colsum %dx%d ld%d beta%d" % (NAME[dt], rows, cols, ld, int(beta))] = gd.result()
    with Guard() as gd:
        srcs = [rnd(3000, 2304, dtype=BF16, seed=1), rnd(1920, 768, dtype=BF16, seed=2), rnd(1000, 3 * 768, seed=3), rnd(37, 16, seed=4), rnd(70, 4 * 64, seed=5)]
        specs = [(srcs[0], 768, 1536, 1.0), (srcs[1], 0, 768, 0.0), (srcs[2], 768, 768, 1.0), (srcs[3], 0, 16, 1.0)]
        probs = [Lb.Colsum(t.data_ptr() + c0 * t.element_size(), gd.add((n,), F32, 0.5).data_ptr(), t.shape[0], n, t.shape[1], Lb.dt(t), beta)
                 for t, c0, n, beta in specs]
        ids = torch.tensor([5, -1, 0, 2], dtype=torch.int32).cuda()  # indexed destination rows: 4 groups of 64 columns -> rows of a table
        probs.append(Lb.Colsum(srcs[4].data_ptr(), gd.add((6, 64), F32, 0.25).data_ptr(), 70, 256, 256, Lb.F32, 1.0, 64, ids.data_ptr()))
        arr = (Lb.Colsum * len(probs))(*probs)
        ws = _EMPTY(Lb.lib().hero_colsum_multi_workspace_bytes(arr, len(probs)) // 4 + 1, device="cuda")
        Lb.check(Lb.lib().hero_colsum_multi(arr, len(probs), ws.data_ptr(), Lb.stream()))
        res["colsum_multi"] = gd.result()
    return res


def save(path):
    from hero_amd import functional as HF, _lib as Lb
    res = run_all(HF, Lb)
    torch.save(res, path)
    print("%d cases, %d tensors from %s -> %s" % (len(res), sum(len(v) for v in res.values()), Lb.LIB_PATH, path))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%-44s only in one file" % name)
            bad += 1
            continue
        diff = [t for t in sorted(set(a[name]) | set(b[name]))
                if a[name].get(t) is None or b[name].get(t) is None or a[name][t].shape != b[name][t].shape or not torch.equal(a[name][t], b[name][t])]
        bad += len(diff)
        print("%-44s %d tensors %s" % (name, len(a[name]), "equal" if not diff else "DIFFERENT: " + " ".join(diff)))
    print("%d cases, %d differences" % (len(a), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "save":
        save(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
