#!/usr/bin/env python3
"""Raw bits of the GEMM family (gemm_ws.hip: wave-specialised K,K / O,O / stream-K group / batched wgrad kernels; gemm.hip:
the 4-wave kernels behind one launch helper) on a fixed list of cases, to compare two library builds - a refactor of the
kernels must not move one bit.

  python tools/lab/gemm_bits.py save OUT.pt        run every case, torch.save the results
  python tools/lab/gemm_bits.py compare A.pt B.pt   torch.equal on the raw bytes, per case and buffer; exit status 1 on a difference

One `save` process per build (HERO_HIP_LIB selects the library), then `compare`.  The smallest hero_wgrad_batch case runs
first.

Only cases whose result is deterministic BY CONSTRUCTION (every output element is written once, or receives one fp32 add, or
its adds are ordered by the kernel):
  K,K      forced geometries 9 / 10 (192 x 192, 128 x 192) at (385, 192, 64), (1000, 200, 128), (700, 776, 768); 13 (64 x 128)
           at (130, 136, 64), (333, 264, 640); 14 (64 x 192) at (1000, 392, 640).  Epilogues: bias; bias + residual + dropout;
           bias + GELU with the saved pre-activation; bias + GELU_DG; none; residual; GELU_BWD and MUL_AUX, each also with
           column sums in the PARTIAL-TABLE mode (atomic column sums from several tile rows are order-dependent: left to the
           suite's tolerance); for 13 / 14 ReLU with aux, with and without a residual.
  O,O      hero_gemm, forced 9, outputs 384 x 200 and 3264 x 3264 (289 tiles: 33 workgroups take a second item), beta 0 and 1.
           The split is min(CUs / tiles, k-steps / 4): 1 for 3264 x 3264 at 320 and 500 rows and for 384 x 200 up to 448 rows
           (one add per element).  384 x 200 at 500 rows has 8 k-steps -> TWO splits: exact on beta = 0 (0 + p1 + p2 in
           either order), order-dependent on beta = 1 - so that output runs 320 / 500 rows with beta 0 and 320 / 448 with beta 1.
  group    hero_wgrad_group, four 1536 x 1536 problems = 256 tiles: on 256 workgroups every stream-K range is one whole tile
           (one add per element); 1024 and 1064 rows.  Skipped, and said so, on a device without 256 CUs.
  batch    hero_wgrad_batch (ordered by design): one layer of the four BertLayer shapes at 1920 rows (whole-tile tail) and 8200
           rows (big slices + packed remainders), the ragged set (768 x 4352, 1000 x 776, a column-sliced dY) at 1920 rows;
           dbias on all but the first problem.
  4-wave   one case per launcher: direct-to-LDS K,K at (700, 776, 768) for cfg 0..3 (bias / generic ReLU epilogue),
           register-staged (cfg 4) K,O and O,K, gemm_glds_tr_kernel (O,O) at rows 520, 200 x 136, and the slab split-K path.

Every tensor a kernel writes is the middle of a larger buffer pre-filled with a bit pattern, and the whole buffer is saved:
what the kernels must leave alone is compared too."""
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import torch

F32, BF16 = torch.float32, torch.bfloat16
SENT = 0x5A
G = 4096                                  # guard elements on either side


class Bufs:
    def __init__(self):
        self.bufs = []

    def add(self, shape, dtype, fill=None):
        """A contiguous tensor of `shape` in the middle of a guarded buffer; fill None leaves the pattern in it too."""
        n = int(np.prod(shape))
        big = torch.empty(n + 2 * G, dtype=dtype, device="cuda")
        big.view(torch.uint8).fill_(SENT)
        view = big[G:G + n].view(*shape)
        if fill is not None:
            view.fill_(fill)
        self.bufs.append(big)
        return view

    def result(self):
        torch.cuda.synchronize()
        return {"buf%02d" % i: b.view(torch.uint8).cpu() for i, b in enumerate(self.bufs)}


def rnd(*shape, dtype=BF16, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).cuda()


def forced(Lb, cfg):
    class _F:
        def __enter__(self):
            Lb.check(Lb.lib().hero_gemm_force_config(cfg))

        def __exit__(self, *exc):
            Lb.lib().hero_gemm_force_config(-1)
    return _F()


def run_batch(Lb, probs, n, rows):
    buf = np.zeros(8 + 8 * 256 * 16, dtype=np.int32)
    words = Lb.lib().hero_wgrad_batch_plan(probs, n, rows, buf.ctypes.data, buf.size)
    assert words > 8, words
    plan = torch.from_numpy(buf[:words].copy()).cuda()
    Lb.check(Lb.lib().hero_wgrad_batch(probs, n, rows, Lb.BF16, plan.data_ptr(), words, Lb.stream()))
    torch.cuda.synchronize()


def batch_case(Lb, rows, shapes, sliced=None):
    """shapes: (n_out, n_in) per problem; sliced = (index, wide columns, first column): that problem's dY is a column slice."""
    bf = Bufs()
    keep = []
    probs = (Lb.WgradProblem * len(shapes))()
    for i, (n, k) in enumerate(shapes):
        dy, x = rnd(rows, n, seed=100 + i), rnd(rows, k, seed=200 + i)
        dw = bf.add((n, k), F32, 0.25)
        probs[i] = Lb.WgradProblem(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), n, k, n, k, k, 4)
        if sliced and sliced[0] == i:
            wide = rnd(rows, sliced[1], seed=77)
            probs[i] = Lb.WgradProblem(wide.data_ptr() + sliced[2] * 2, x.data_ptr(), dw.data_ptr(), n, k, sliced[1], k, k, 4)
            keep.append(wide)
        if i:
            probs[i].dbias = bf.add((n,), F32, 0.125).data_ptr()
        keep += [dy, x]
    run_batch(Lb, probs, len(shapes), rows)
    return bf.result()


def kk_cases(HF, Lb, res):
    dev = torch.device("cuda:0")
    shapes = {9: [(385, 192, 64), (1000, 200, 128), (700, 776, 768)], 10: [(385, 192, 64), (1000, 200, 128), (700, 776, 768)],
              13: [(130, 136, 64), (333, 264, 640)], 14: [(1000, 392, 640)]}
    for cfg, lst in shapes.items():
        for M, N, K in lst:
            a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05)
            bias = rnd(N, dtype=F32, seed=3, scale=0.5)
            resid, saved = rnd(M, N, seed=4), rnd(M, N, seed=5)
            epis = [("bias", dict(bias=bias)), ("bias+res+drop", dict(bias=bias, residual=resid, drop=True)),
                    ("bias+gelu", dict(bias=bias, act=Lb.ACT_GELU, aux="out")), ("bias+gelu_dg", dict(bias=bias, act=Lb.ACT_GELU_DG, aux="out")),
                    ("none", dict()), ("res", dict(residual=resid)),
                    ("gelu_bwd", dict(act=Lb.ACT_GELU_BWD, aux=saved)), ("mul_aux", dict(act=Lb.ACT_MUL_AUX, aux=saved)),
                    ("gelu_bwd+colsum_partial", dict(act=Lb.ACT_GELU_BWD, aux=saved, colsum=True)),
                    ("mul_aux+colsum_partial", dict(act=Lb.ACT_MUL_AUX, aux=saved, colsum=True))]
            if cfg in (13, 14):
                epis += [("bias+relu_aux", dict(bias=bias, act=Lb.ACT_RELU, aux="out")),
                         ("bias+relu_aux+res", dict(bias=bias, act=Lb.ACT_RELU, aux="out", residual=resid))]
            for name, kw in epis:
                kw = dict(kw)
                bf = Bufs()
                out = bf.add((M, N), BF16)
                if kw.get("aux") == "out":
                    kw["aux"] = bf.add((M, N), BF16)
                if kw.pop("colsum", False):
                    kw["colsum"] = bf.add(((M + 63) // 64, N), F32)
                    kw["colsum_partial"] = True
                if kw.pop("drop", False):
                    HF.manual_seed(1234, "cuda:0")
                    kw["drop"] = HF.RNG.make(0.1, True, dev)
                with forced(Lb, cfg):
                    HF.k_gemm(a, w, out, M, N, K, K, K, N, Lb.LAYOUT_K, Lb.LAYOUT_K, Lb.BF16, **kw)
                res["K,K cfg%d %dx%dx%d %s" % (cfg, M, N, K, name)] = bf.result()


def oo_cases(HF, Lb, res):
    for n_out, n_in, runs in ((384, 200, ((320, 0.0), (500, 0.0), (320, 1.0), (448, 1.0))),
                              (3264, 3264, ((320, 0.0), (500, 0.0), (320, 1.0), (500, 1.0)))):
        for rows, beta in runs:
            dy, x = rnd(rows, n_out, seed=1), rnd(rows, n_in, seed=2)
            bf = Bufs()
            out = bf.add((n_out, n_in), F32, 0.75)
            with forced(Lb, 9):
                HF.k_gemm(dy, x, out, n_out, n_in, rows, n_out, n_in, n_in, Lb.LAYOUT_O, Lb.LAYOUT_O, Lb.BF16, out_f32=True, beta=beta, split_k=1)
            res["O,O cfg9 rows%d %dx%d beta%d" % (rows, n_out, n_in, int(beta))] = bf.result()


def group_cases(HF, Lb, res):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        print("hero_wgrad_group cases SKIPPED: the device reports %d CUs, whole-tile stream-K ranges need 256" % cus)
        return
    for rows in (1024, 1064):
        bf = Bufs()
        keep = []
        probs = (Lb.WgradProblem * 4)()
        for i in range(4):
            dy, x = rnd(rows, 1536, seed=10 + i), rnd(rows, 1536, seed=20 + i)
            probs[i] = Lb.WgradProblem(dy.data_ptr(), x.data_ptr(), bf.add((1536, 1536), F32, 0.5).data_ptr(), 1536, 1536, 1536, 1536, 1536, 4)
            keep += [dy, x]
        Lb.check(Lb.lib().hero_wgrad_group(probs, 4, rows, Lb.BF16, Lb.stream()))
        res["group 4 x 1536x1536 rows%d" % rows] = bf.result()


def four_wave_cases(HF, Lb, res):
    M, N, K = 700, 776, 768
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05)
    bias = rnd(N, dtype=F32, seed=3, scale=0.5)
    for cfg in (0, 1, 2, 3):
        for name, kw in (("bias", dict(bias=bias)), ("generic relu", dict(bias=bias, act=Lb.ACT_RELU))):
            bf = Bufs()
            out = bf.add((M, N), BF16)
            with forced(Lb, cfg):
                HF.k_gemm(a, w, out, M, N, K, K, K, N, Lb.LAYOUT_K, Lb.LAYOUT_K, Lb.BF16, **kw)
            res["4-wave K,K cfg%d %dx%dx%d %s" % (cfg, M, N, K, name)] = bf.result()
    M, N, K = 520, 200, 136                                          # register-staged: K,O and O,K
    bt, at = rnd(K, N, seed=4, scale=0.05), rnd(K, M, seed=5)
    a2, w2 = rnd(M, K, seed=6), rnd(N, K, seed=7, scale=0.05)
    for name, args in (("K,O", (a2, bt, K, N, Lb.LAYOUT_K, Lb.LAYOUT_O)), ("O,K", (at, w2, M, K, Lb.LAYOUT_O, Lb.LAYOUT_K))):
        bf = Bufs()
        out = bf.add((M, N), BF16)
        A, B, lda, ldb, al, bl = args
        with forced(Lb, 4):
            HF.k_gemm(A, B, out, M, N, K, lda, ldb, N, al, bl, Lb.BF16)
        res["4-wave cfg4 %s %dx%dx%d" % (name, M, N, K)] = bf.result()
    rows, n_out, n_in = 520, 200, 136                                # gemm_glds_tr_kernel
    dy, x = rnd(rows, n_out, seed=1), rnd(rows, n_in, seed=2)
    for beta in (0.0, 1.0):
        bf = Bufs()
        out = bf.add((n_out, n_in), F32, 0.75)
        with forced(Lb, 0):
            HF.k_gemm(dy, x, out, n_out, n_in, rows, n_out, n_in, n_in, Lb.LAYOUT_O, Lb.LAYOUT_O, Lb.BF16, out_f32=True, beta=beta, split_k=1)
        res["4-wave O,O glds_tr rows%d %dx%d beta%d" % (rows, n_out, n_in, int(beta))] = bf.result()
    M, N, K = 256, 512, 64 * 37                                      # slab split-K: 8 slabs, each written once
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05)
    n = Lb.lib().hero_gemm_splits(K, 8, Lb.BF16)
    bf = Bufs()
    slabs = bf.add((n, M, N), F32)
    HF.k_gemm(a, w, slabs, M, N, K, K, K, N, Lb.LAYOUT_K, Lb.LAYOUT_K, Lb.BF16, out_f32=True, split_k=8, split_stride=M * N)
    res["4-wave slab split-K %dx%dx%d, %d slabs" % (M, N, K, n)] = bf.result()


def run_all(HF, Lb):
    res = {}
    bert = [(768, 3072), (3072, 768), (768, 768), (2304, 768)]
    res["batch one layer rows1920"] = batch_case(Lb, 1920, bert)     # the smallest batched case first
    res["batch one layer rows8200"] = batch_case(Lb, 8200, bert)
    res["batch ragged rows1920"] = batch_case(Lb, 1920, [(768, 4352), (1000, 776), (768, 4352), (768, 768), (768, 3072), (3072, 768)],
                                              sliced=(3, 2304, 768))
    kk_cases(HF, Lb, res)
    oo_cases(HF, Lb, res)
    group_cases(HF, Lb, res)
    four_wave_cases(HF, Lb, res)
    return res


def save(path):
    from hero_amd import functional as HF, _lib as Lb
    res = run_all(HF, Lb)
    torch.save(res, path)
    print("%d cases, %d buffers from %s -> %s" % (len(res), sum(len(v) for v in res.values()), Lb.LIB_PATH, path))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%-56s only in one file" % name)
            bad += 1
            continue
        diff = [t for t in sorted(set(a[name]) | set(b[name]))
                if a[name].get(t) is None or b[name].get(t) is None or a[name][t].shape != b[name][t].shape or not torch.equal(a[name][t], b[name][t])]
        bad += len(diff)
        print("%-56s %d buffers %s" % (name, len(a[name]), "equal" if not diff else "DIFFERENT: " + " ".join(diff)))
    print("%d cases, %d differences" % (len(a), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "save":
        save(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
