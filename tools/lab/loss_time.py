#!/usr/bin/env python3
"""Device-event times of the loss entry points (hero_amd/csrc/loss.hip), direct C calls in bf16 at the shapes the bench tools use:
MLM (1368, 50265, 50272), FOM (1920, 100, 100) and features (288, 4352) of tools/bench_pretrain_eval.py, the captioning loss
(1000, 50272, 50272) of tools/bench_tvc_decoder.py (40 captions x 25 tokens); the counted pair at the MLM shape.

  python tools/lab/loss_time.py [--out FILE]      one JSON line: microseconds per call, per entry and shape

20 warm-up calls, then the median of 7 windows of back-to-back calls between two events (1000 calls; 200 at the vocabulary
shapes).  One process per library build (HERO_HIP_LIB selects it); compare the lines of several runs."""
import argparse
import ctypes as C
import json
import os, sys
import statistics
sys.path.insert(0, os.getcwd())
import torch

MLM, FOM, FEAT, TVC = (1368, 50265, 50272), (1920, 100, 100), (288, 4352), (1000, 50272, 50272)


def timed(fn, calls):
    if fn() != 0:
        raise RuntimeError("refused call")
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return round(statistics.median(out), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    from hero_amd import _lib as Lb
    lib, st = Lb.lib(), Lb.stream()
    g = torch.Generator(device="cuda").manual_seed(3)
    res = {"lib": Lb.LIB_PATH}
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device="cuda")      # noqa: E731
    for name, (rows, cols, ld), share in (("mlm", MLM, 1.0), ("fom", FOM, 0.15)):
        calls = 200 if cols > 10000 else 1000
        x = torch.randn(rows, ld, generator=g, device="cuda").bfloat16()
        y = torch.randint(0, cols, (rows,), generator=g, device="cuda")
        y[torch.rand(rows, generator=g, device="cuda") >= share] = -1
        loss, lse, dl, dx = f32(rows), f32(rows), torch.rand(rows, generator=g, device="cuda"), torch.empty_like(x)
        p = [t.data_ptr() for t in (x, y, loss, lse, dl, dx)]
        ce = Lb.CrossEntropy(p[0], p[1], p[2], p[3], p[4], p[5], rows, cols, ld, Lb.BF16, 1.0, -1)
        res["cross_entropy_fwd " + name] = timed(lambda: lib.hero_cross_entropy_fwd(C.byref(ce), st), calls)
        res["cross_entropy_bwd " + name] = timed(lambda: lib.hero_cross_entropy_bwd(C.byref(ce), st), calls)
        acc, ws, pred = torch.zeros(3, dtype=torch.float64, device="cuda"), f32(3 * rows), torch.empty(rows, dtype=torch.int32, device="cuda")
        res["ce_eval " + name] = timed(lambda: lib.hero_ce_eval(p[0], p[1], rows, cols, ld, Lb.BF16, 1.0, -1, acc.data_ptr(), pred.data_ptr(),
                                                               ws.data_ptr(), st), calls)
        if name == "mlm":
            cnt, mc = torch.tensor([rows - 100], dtype=torch.int32, device="cuda"), f32(2)
            res["ce_counted_fwd mlm"] = timed(lambda: lib.hero_ce_counted_fwd(p[0], p[1], cnt.data_ptr(), p[2], p[3], mc.data_ptr(), rows, cols, ld, Lb.BF16,
                                                                              1.0, -1, st), calls)
            res["ce_counted_bwd mlm"] = timed(lambda: lib.hero_ce_counted_bwd(p[0], p[1], cnt.data_ptr(), p[3], p[4], mc.data_ptr(), p[5], rows, cols, ld,
                                                                              Lb.BF16, 1.0, -1, st), calls)
        del x, dx
    rows, cols, ld = TVC
    x = torch.randn(rows, ld, generator=g, device="cuda").bfloat16()
    y = torch.randint(0, cols, (rows,), generator=g, device="cuda")
    y[::7] = -1
    loss, lse, sc, one, dx = f32(rows), f32(rows), f32(2), torch.ones(1, device="cuda"), torch.empty_like(x)
    res["smooth_ce_fwd tvc"] = timed(lambda: lib.hero_smooth_ce_fwd(x.data_ptr(), y.data_ptr(), loss.data_ptr(), lse.data_ptr(), sc.data_ptr(), rows, cols,
                                                                    ld, Lb.BF16, 0.1, -1, st), 200)
    res["smooth_ce_bwd tvc"] = timed(lambda: lib.hero_smooth_ce_bwd(x.data_ptr(), y.data_ptr(), lse.data_ptr(), one.data_ptr(), None, sc.data_ptr(),
                                                                    dx.data_ptr(), rows, cols, ld, Lb.BF16, 0.1, -1, st), 200)
    rows, cols = FEAT
    pr, tg = (torch.randn(rows, cols, generator=g, device="cuda").bfloat16() for _ in range(2))
    acc, ws = torch.zeros(3, dtype=torch.float64, device="cuda"), f32(2 * rows)
    res["feat_eval feat"] = timed(lambda: lib.hero_feat_eval(pr.data_ptr(), tg.data_ptr(), rows, cols, cols, cols, Lb.BF16, acc.data_ptr(), ws.data_ptr(), st), 1000)
    torch.cuda.synchronize()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
