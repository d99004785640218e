#!/usr/bin/env python3
"""Which kernel does hero_gemm launch for a problem?  A fixed list of cases (real shapes of the step: the routing rules
depend on them), recorded once from a kernel trace and pinned as tests/golden/gemm_routes.json, which
tests/test_cpu_gemm_route.py holds hero_gemm_route against without a GPU.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gemm_routes.py issue
        every case exactly once through hero_gemm under its forced configuration; a hero_fold_slabs launch in front of
        each case marks the case boundaries in the trace (no counters, no other tracing in that run)
  python tools/gemm_routes.py golden KERNEL_TRACE.csv COMMIT CUS OUT.json
        the trace -> per case the ordered (demangled kernel name, workgroups, workgroup size, LDS bytes); COMMIT is the
        commit whose library was traced, CUS its device's compute units.  `lds` is the tracer's LDS_Block_Size as it is
        (the recorded run's rocprofv3 reports 0 for dynamic LDS; the test then holds LDS to the kernels' own constants)
  python tools/gemm_routes.py list
        the cases

The golden table is the behaviour of the commit it names: it is recorded, never regenerated from newer code."""
import csv, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACT = dict(none=0, gelu=1, relu=2, gelu_bwd=3, relu_bwd=4, gelu_dg=5, mul_aux=6)
MARKER = "fold_slabs"                      # substring of the marker kernel's name
GEMM_KERNELS = ("gemm_", "scale_f32_kernel")


def _split_for(n_out, n_in, rows):
    from hero_amd.functional import _split_for as f
    return f(n_out, n_in, rows, 64)


def case(name, M, N, K, lay="KK", dt="bf16", force=-1, **epi):
    """epi: bias / residual / aux / drop (bool), act (name), out_f32, beta, split_k, colsum ("atomic" | "partial"), slabs (bool)."""
    bad = set(epi) - {"bias", "residual", "aux", "drop", "act", "out_f32", "beta", "split_k", "colsum", "slabs"}
    assert not bad, bad
    return dict(name=name, M=M, N=N, K=K, lay=lay, dt=dt, force=force, epi=epi)


def cases():
    out = []
    epilogues = [("bias", dict(bias=True)), ("bias+res+drop", dict(bias=True, residual=True, drop=True)),
                 ("bias+gelu+aux", dict(bias=True, act="gelu", aux=True)), ("none", dict()), ("res", dict(residual=True)),
                 ("gelu_bwd+aux", dict(act="gelu_bwd", aux=True)),
                 ("mul_aux+colsum", dict(act="mul_aux", aux=True, colsum="atomic")),
                 ("mul_aux+colsum_partial", dict(act="mul_aux", aux=True, colsum="partial")),
                 ("gelu_bwd+colsum_partial", dict(act="gelu_bwd", aux=True, colsum="partial"))]
    for M in (12000, 14450, 1920):                                   # 192 x 192, 128 x 192 and 64 x 128 tiles
        for en, e in epilogues:
            out.append(case("epi %s @%d" % (en, M), M, 768, 768, **e))
    for M, N, K in ((12000, 768, 768), (12000, 768, 3072), (12000, 2304, 768), (12000, 3072, 768), (24000, 3072, 768), (1440, 50272, 768),
                    (14450, 768, 768), (1920, 3072, 768), (1920, 2304, 768), (1920, 768, 768), (1920, 768, 3072), (3104, 768, 768),
                    (480, 768, 2304), (515, 768, 768), (700, 776, 768), (480, 768, 256), (131, 768, 4352), (385, 192, 64), (200, 136, 96)):
        out.append(case("shape %dx%dx%d" % (M, N, K), M, N, K, bias=True))
    # epilogues the wave-specialised family has no instantiation for
    for en, e in (("colsum act none", dict(colsum="atomic")), ("relu_bwd", dict(act="relu_bwd", aux=True)),
                  ("bias+gelu+res", dict(bias=True, act="gelu", aux=True, residual=True)), ("bias+drop", dict(bias=True, drop=True))):
        out.append(case("no-ws %s" % en, 12000, 768, 768, **e))
    for M in (1920, 12000):                                          # the residual form exists on the 64-row tiles only
        out.append(case("relu+aux+bias @%d" % M, M, 768, 768, bias=True, act="relu", aux=True))
        out.append(case("relu+aux+bias+res @%d" % M, M, 768, 768, bias=True, act="relu", aux=True, residual=True))
    # weight gradients: O,O with fp32 output, M x N = n_out x n_in, reduction over the rows
    for n_out, n_in in ((3072, 768), (768, 3072), (768, 768), (2304, 768)):
        for rows, betas in ((12000, (0.0, 1.0)), (12040, (1.0,))):
            for beta in betas:
                out.append(case("wgrad %dx%d rows%d beta%g" % (n_out, n_in, rows, beta), n_out, n_in, rows, lay="OO", out_f32=True, beta=beta,
                                split_k=_split_for(n_out, n_in, rows)))
    for M, N, K in ((1024, 200, 328), (4000, 768, 768)):
        out.append(case("K,O %dx%dx%d" % (M, N, K), M, N, K, lay="KO"))
        out.append(case("O,K %dx%dx%d" % (M, N, K), M, N, K, lay="OK", bias=True))
    out.append(case("slab split", 1440, 768, 50240, out_f32=True, split_k=16, slabs=True))
    out.append(case("atomic split beta0", 256, 512, 2368, out_f32=True, split_k=8, beta=0.0))
    out.append(case("atomic split beta1", 256, 512, 2368, out_f32=True, split_k=8, beta=1.0))
    # fp32
    for M, N, K in ((32, 768, 768), (5, 772, 260), (1, 8, 256)):
        out.append(case("f32 skinny %dx%dx%d" % (M, N, K), M, N, K, dt="f32", bias=True))
        out.append(case("f32 %dx%dx%d +res" % (M, N, K), M, N, K, dt="f32", bias=True, residual=True))
    out.append(case("f32 33 rows", 33, 768, 768, dt="f32", bias=True))
    out.append(case("f32 12000x768x768", 12000, 768, 768, dt="f32", bias=True))
    out.append(case("f32 12000x3072x768", 12000, 3072, 768, dt="f32", bias=True))
    out.append(case("f32 K,O", 1024, 200, 328, lay="KO", dt="f32"))
    out.append(case("f32 O,O", 768, 768, 1000, lay="OO", dt="f32", out_f32=True, beta=1.0))
    out.append(case("f32 split", 256, 512, 2048, dt="f32", out_f32=True, split_k=4, beta=0.0))
    # forced configurations
    for cfg in (0, 1, 2, 3, 4, 6, 8, 9, 10, 11, 12, 13, 14, 3 | (16 << 8)):
        out.append(case("force %d" % cfg, 700, 776, 768, force=cfg, bias=True))
    out.append(case("force 9 under half a round", 515, 768, 768, force=9, bias=True))
    for cfg in (9, 10, 13, 14):
        out.append(case("force %d wgrad 768x768" % cfg, 768, 768, 12000, lay="OO", force=cfg, out_f32=True, beta=1.0, split_k=_split_for(768, 768, 12000)))
    out.append(case("force 13 @130x136x64", 130, 136, 64, force=13, bias=True))
    assert len({c["name"] for c in out}) == len(out)
    return out


def issue():
    import torch
    from hero_amd import functional as HF, _lib as L
    dev = torch.device("cuda", 0)
    mark = torch.zeros(8, device=dev)
    for c in cases():
        M, N, K, e = c["M"], c["N"], c["K"], c["epi"]
        tdt = torch.bfloat16 if c["dt"] == "bf16" else torch.float32
        al, bl = (L.LAYOUT_K if ch == "K" else L.LAYOUT_O for ch in c["lay"])
        A = torch.zeros((M, K) if al == L.LAYOUT_K else (K, M), device=dev, dtype=tdt)
        B = torch.zeros((N, K) if bl == L.LAYOUT_K else (K, N), device=dev, dtype=tdt)
        out_f32 = bool(e.get("out_f32"))
        split = int(e.get("split_k", 1))
        n_slabs = L.lib().hero_gemm_splits(K, split, L.BF16 if c["dt"] == "bf16" else L.F32) if e.get("slabs") else 1
        Cm = torch.zeros((n_slabs, M, N), device=dev, dtype=torch.float32 if out_f32 else tdt)
        kw = dict(act=ACT[e.get("act", "none")], out_f32=out_f32, beta=float(e.get("beta", 0.0)), split_k=split)
        if e.get("bias"):
            kw["bias"] = torch.zeros(N, device=dev)
        if e.get("residual"):
            kw["residual"] = torch.zeros((M, N), device=dev, dtype=tdt)
        if e.get("aux"):
            kw["aux"] = torch.zeros((M, N), device=dev, dtype=tdt)
        if e.get("drop"):
            HF.manual_seed(1234, "cuda:0")
            kw["drop"] = HF.RNG.make(0.1, True, dev)
        if e.get("colsum"):
            partial = e["colsum"] == "partial"
            kw["colsum"] = torch.zeros(((M + 63) // 64 if partial else 1, N), device=dev)
            kw["colsum_partial"] = partial
        if e.get("slabs"):
            kw["split_stride"] = M * N
        torch.cuda.synchronize()
        L.check(L.lib().hero_fold_slabs(L.ptr(mark), 1, 4, L.ptr(mark) + 16, 4, L.F32, L.stream()))
        L.check(L.lib().hero_gemm_force_config(c["force"]))
        try:
            HF.k_gemm(A, B, Cm, M, N, K, A.shape[1], B.shape[1], N, al, bl, L.BF16 if c["dt"] == "bf16" else L.F32, **kw)
        finally:
            L.lib().hero_gemm_force_config(-1)
        torch.cuda.synchronize()
    print("issued %d cases on %s (%d CUs), library %s" % (len(cases()), torch.cuda.get_device_name(0),
                                                         torch.cuda.get_device_properties(0).multi_processor_count, L.LIB_PATH))


def golden(trace, commit, cus, out_path):
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_case, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if MARKER in name:
            cur = []
            per_case.append(cur)
        elif cur is not None and any(k in name for k in GEMM_KERNELS):
            wg = int(r["Workgroup_Size_X"])
            assert int(r["Grid_Size_X"]) % wg == 0 and int(r["Grid_Size_Y"]) == 1 and int(r["Grid_Size_Z"]) == 1, r
            cur.append(dict(kernel=name, grid=int(r["Grid_Size_X"]) // wg, threads=wg, lds=int(r["LDS_Block_Size"])))
    cs = cases()
    assert len(per_case) == len(cs), "%d markers in the trace, %d cases" % (len(per_case), len(cs))
    for c, launches in zip(cs, per_case):
        assert launches, "no GEMM kernel in the trace for case %r" % c["name"]
        c["launches"] = launches
    json.dump(dict(commit=commit, cus=int(cus), cases=cs), open(out_path, "w"), indent=1)
    print("%d cases, %d launches -> %s" % (len(cs), sum(len(c["launches"]) for c in cs), out_path))


if __name__ == "__main__":
    if sys.argv[1:] == ["issue"]:
        issue()
    elif len(sys.argv) == 6 and sys.argv[1] == "golden":
        golden(*sys.argv[2:])
    elif sys.argv[1:] == ["list"]:
        for c in cases():
            print(json.dumps(c))
    else:
        sys.exit(__doc__)
