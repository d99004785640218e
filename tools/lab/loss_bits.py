#!/usr/bin/env python3
"""Raw bits of the loss kernels (hero_amd/csrc/loss.hip) on a fixed list of small cases, to compare two library builds - a
refactor of the kernels must not move one bit.

  python tools/lab/loss_bits.py save OUT.pt         run every case on the GPU, torch.save the results
  python tools/lab/loss_bits.py compare A.pt B.pt    torch.equal on the raw bytes, per case and tensor; exit status 1 on a difference
  python tools/lab/loss_bits.py refused OUT.txt      no GPU: (return code, hero_last_error()) of every call that must be refused
                                                     before a launch, and of the rows == 0 returns; compare two files with diff

One `save` / `refused` process per build (HERO_HIP_LIB selects the library), then `compare` / diff.

Direct calls of the eight C entry points with seeded inputs, fp32 and bf16.  (cols, ld) = (7, 7) and (301, 301): the scalar walk,
first and second strided trip; (37, 40): 8-wide with only some threads loaded, a tail and padding; (2051, 2056): every thread
loads once, plus a tail; (4101, 4104): a second 8-wide trip for the low threads.
  plain, counted  rows 12 and 300 (the fold's second strided trip; at 300 rows the backward runs at the three narrow shapes only:
                  no kernel but the folds sees the row count), inv_temp 1.0 and 0.7, ignore_index -100 and 3, labels < 0 and
                  >= cols, counts None, 0, 1, 5, 12, 20, backward out of place and in place, the rows at and behind the count
                  filled with NaN / Inf, the ignored row 1 holding an Inf (a dead row of the plain kernel)
  smoothed        eps 0.1 and 1.0, with and without dloss_rows and mean_cnt, every row ignored, rows 0 and 300, logits of
                  magnitude 3e4
  ce_eval         rows 5 and 300: equal maxima planted (5.0 twice; -0 against +0 over negative values), a row of -inf, pred null
                  and not, acc pre-filled
  feat_eval       FEAT_ROWS x FEAT_COLS of tests/pretrain_eval_reference.py, and (ld_p, ld_t) unequal with one no multiple of 8
Every output is the middle of a larger buffer pre-filled with a byte pattern, and the whole buffer is saved: what the kernels must
leave alone is compared too (NaN by bit pattern: the comparison is on bytes)."""
import ctypes as C
import os, sys
sys.path.insert(0, os.getcwd())
import torch

F32, BF16 = torch.float32, torch.bfloat16
NAME = {F32: "f32", BF16: "bf16"}
SENT, G = 0x5A, 256                       # guard byte, guard elements on either side
SHAPES = ((7, 7), (301, 301), (37, 40), (2051, 2056), (4101, 4104))


class Case:
    """Guarded device buffers of one case, in allocation order."""

    def __init__(self):
        self.bufs = []

    def out(self, shape, dtype, fill=None, src=None):
        n = 1
        for s in shape:
            n *= s
        big = torch.empty(n + 2 * G, dtype=dtype, device="cuda")
        big.view(torch.uint8).fill_(SENT)
        view = big[G:G + n].view(*shape)
        if fill is not None:
            view.fill_(fill)
        if src is not None:
            view.copy_(src)
        self.bufs.append(big)
        return view

    def result(self):
        torch.cuda.synchronize()
        return {"buf%02d" % i: b.view(torch.uint8).cpu() for i, b in enumerate(self.bufs)}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def p(t):
    return None if t is None else t.data_ptr()


def logits_labels(rows, cols, ld, dtype, ignore, seed):
    x = (torch.randn(rows, ld, generator=gen(seed)) * 3).to(dtype)
    y = torch.randint(0, cols, (rows,), generator=gen(seed + 1))
    for r, v in ((1, ignore), (2, -5), (3, cols), (4, cols + 7)):
        if r < rows:
            y[r] = v
    if rows > 1:
        x[1, 2] = float("inf")
    return x.cuda(), y.cuda()


def plain_and_counted(Lb, res):
    lib = Lb.lib()
    for dtype in (F32, BF16):
        for cols, ld in SHAPES:
            for rows in (12, 300):
                for t in (1.0, 0.7):
                    for ignore in (-100, 3):
                        tag = "%s %dx%d/%d t%g ign%d" % (NAME[dtype], rows, cols, ld, t, ignore)
                        bwd = rows == 12 or ld <= 301
                        x, y = logits_labels(rows, cols, ld, dtype, ignore, 11)
                        g_rows = torch.randn(rows, generator=gen(5)).cuda()
                        c = Case()
                        loss, lse = c.out((rows,), F32), c.out((rows,), F32)
                        a = Lb.CrossEntropy(p(x), p(y), p(loss), p(lse), None, None, rows, cols, ld, Lb.dt(x), t, ignore)
                        Lb.check(lib.hero_cross_entropy_fwd(C.byref(a), Lb.stream()))
                        if bwd:
                            for inplace in (0, 1):
                                dx = c.out((rows, ld), dtype, src=x if inplace else None)
                                a = Lb.CrossEntropy(p(dx if inplace else x), p(y), None, p(lse), p(g_rows), p(dx), rows, cols, ld, Lb.dt(x), t, ignore)
                                Lb.check(lib.hero_cross_entropy_bwd(C.byref(a), Lb.stream()))
                        res["plain " + tag] = c.result()
                        g1 = torch.tensor([0.75]).cuda()
                        for count in (None, 0, 1, 5, 12, 20):
                            xc = x.clone()
                            if count is not None and count < rows:
                                xc[count::2] = float("nan")
                                xc[count + 1::2] = float("inf")
                            cnt = None if count is None else torch.tensor([count], dtype=torch.int32).cuda()
                            c = Case()
                            loss, lse, mc = c.out((rows,), F32), c.out((rows,), F32), c.out((2,), F32)
                            Lb.check(lib.hero_ce_counted_fwd(p(xc), p(y), p(cnt), p(loss), p(lse), p(mc), rows, cols, ld, Lb.dt(x), t, ignore, Lb.stream()))
                            if bwd:
                                for inplace in (0, 1):
                                    dx = c.out((rows, ld), dtype, src=xc if inplace else None)
                                    Lb.check(lib.hero_ce_counted_bwd(p(dx if inplace else xc), p(y), p(cnt), p(lse), p(g1), p(mc), p(dx), rows, cols, ld,
                                                                     Lb.dt(x), t, ignore, Lb.stream()))
                            res["counted %s count %s" % (tag, count)] = c.result()


def smoothed(Lb, res):
    lib = Lb.lib()

    def run(tag, x, y, cols, eps, ignore, bwd=True, rows=None):
        rows, ld = x.shape[0] if rows is None else rows, x.shape[1]
        c = Case()
        loss, lse, sc = c.out((max(rows, 1),), F32), c.out((max(rows, 1),), F32), c.out((2,), F32)
        Lb.check(lib.hero_smooth_ce_fwd(p(x), p(y), p(loss), p(lse), p(sc), rows, cols, ld, Lb.dt(x), eps, ignore, Lb.stream()))
        g1, g_rows = torch.tensor([0.75]).cuda(), torch.randn(max(rows, 1), generator=gen(5)).cuda()
        for with_rows in (0, 1) if bwd else ():
            for with_mean in (0, 1):
                for inplace in (0, 1):
                    dx = c.out((max(rows, 1), ld), x.dtype, src=x if inplace and rows else None)
                    Lb.check(lib.hero_smooth_ce_bwd(p(dx if inplace else x), p(y), p(lse), p(g1), p(g_rows) if with_rows else None,
                                                    p(sc) if with_mean else None, p(dx), rows, cols, ld, Lb.dt(x), eps, ignore, Lb.stream()))
        res["smooth " + tag] = c.result()

    for dtype in (F32, BF16):
        for cols, ld in SHAPES:
            for eps in (0.1, 1.0):
                tag = "%s 12x%d/%d eps%g" % (NAME[dtype], cols, ld, eps)
                x, y = logits_labels(12, cols, ld, dtype, 1, 21)
                x[1, 2] = 0.5                                            # finite: the smoothed loss reads every row
                run(tag, x, y, cols, eps, 1)
                run(tag + " all ignored", x, torch.full_like(y, 1), cols, eps, 1)
                run(tag + " 3e4", (x.float() * 1e4).to(dtype), y, cols, eps, 1)
            x, y = logits_labels(300, cols, ld, dtype, 1, 22)
            x[1, 2] = 0.5
            run("%s 300x%d/%d" % (NAME[dtype], cols, ld), x, y, cols, 0.1, 1, bwd=ld <= 301)
            run("%s 0x%d/%d" % (NAME[dtype], cols, ld), x, y, cols, 0.1, 1, rows=0)   # rows == 0: the pair is (0, 0), no row is touched


def evals(Lb, res):
    from tests import pretrain_eval_reference as R
    lib = Lb.lib()
    for dtype in (F32, BF16):
        for cols, ld in SHAPES:
            for rows in (5, 300):
                x = (torch.randn(rows, ld, generator=gen(31)) * 3).clamp_(max=4.5).to(dtype)
                y = torch.randint(0, cols, (rows,), generator=gen(32))
                a, b = cols // 3, cols - 1
                x[0, a] = x[0, b] = 5.0                                  # two equal maxima: the lower column, which is the label
                y[0] = a
                x[1] = -x[1].abs() - 1.0                                 # -0 at 2 against +0 at 5 over negative values: column 2
                x[1, 2], x[1, 5] = -0.0, 0.0
                y[1] = 5
                x[2] = float("-inf")
                y[3], y[4] = -1, cols
                x, y = x.cuda(), y.cuda()
                for t in (1.0, 0.7):
                    for with_pred in (0, 1):
                        c = Case()
                        acc = c.out((3,), torch.float64, src=torch.tensor([0.5, 3.0, 4.0], dtype=torch.float64))
                        ws = c.out((3 * rows,), F32)
                        pred = c.out((rows,), torch.int32) if with_pred else None
                        Lb.check(lib.hero_ce_eval(p(x), p(y), rows, cols, ld, Lb.dt(x), t, -1, p(acc), p(pred), p(ws), Lb.stream()))
                        res["ce_eval %s %dx%d/%d t%g pred%d" % (NAME[dtype], rows, cols, ld, t, with_pred)] = c.result()
        for rows in R.FEAT_ROWS:
            for cols in R.FEAT_COLS:
                up = (cols + 7) & ~7
                for ld_p, ld_t in ((up, up), (up + 8, up + 3)):
                    pr = torch.randn(rows, ld_p, generator=gen(41)).to(dtype).cuda()
                    tg = torch.randn(rows, ld_t, generator=gen(42)).to(dtype).cuda()
                    c = Case()
                    acc = c.out((3,), torch.float64, src=torch.tensor([0.5, 0.25, 7.0], dtype=torch.float64))
                    ws = c.out((2 * rows,), F32)
                    Lb.check(lib.hero_feat_eval(p(pr), p(tg), rows, cols, ld_p, ld_t, Lb.dt(pr), p(acc), p(ws), Lb.stream()))
                    res["feat_eval %s %dx%d/%d,%d" % (NAME[dtype], rows, cols, ld_p, ld_t)] = c.result()


def save(path):
    from hero_amd import _lib as Lb
    res = {}
    plain_and_counted(Lb, res)
    smoothed(Lb, res)
    evals(Lb, res)
    torch.save(res, path)
    print("%d cases, %d tensors from %s -> %s" % (len(res), sum(len(v) for v in res.values()), Lb.LIB_PATH, path))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = tensors = untouched = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%-60s only in one file" % name)
            bad += 1
            continue
        diff = [t for t in sorted(set(a[name]) | set(b[name]))
                if a[name].get(t) is None or b[name].get(t) is None or a[name][t].shape != b[name][t].shape or not torch.equal(a[name][t], b[name][t])]
        bad += len(diff)
        tensors += len(a[name])
        untouched += sum(bool((t == SENT).all()) for t in a[name].values())
        if diff:
            print("%-60s %d tensors DIFFERENT: %s" % (name, len(a[name]), " ".join(diff)))
    print("%d cases, %d tensors (%d of them all guard bytes: never written), %d differences" % (len(a), tensors, untouched, bad))
    return 1 if bad else 0


def refused(path):
    """Fake non-null pointers: every call here returns before it launches or reads anything (so: never on a machine with a GPU)."""
    if torch.cuda.is_available():
        sys.exit("loss_bits.py refused: fake pointers - run it without a GPU")
    from hero_amd import _lib as Lb
    lib = Lb.lib()
    P, A4, A2 = 0x10000, 0x10004, 0x10002                                # 16-byte aligned; 4-byte aligned only; 2-byte aligned only
    lines = []

    def variants(name, call, base, nulls, odd, cols1=False, rows0_returns=True):
        """The rows == 0 forms, bad dims, the dtype code 7, bad inv_temp / eps, each REQUIRED pointer null, each aligned one off."""
        v = [("rows = 0, all pointers null", dict({k: (None if k in nulls else x) for k, x in base.items()}, rows=0)),
             ("rows = 0 and dtype = 7", dict(base, rows=0, dtype=7))]
        if rows0_returns:                                                # (the two forwards with a fold launch it at rows == 0)
            v.append(("rows = 0", dict(base, rows=0)))
        v += [("%s = %d" % (k, x), dict(base, **{k: x})) for k, x in (("rows", -1), ("cols", 0), ("ld", base["cols"] - 1), ("dtype", 7))]
        if cols1:
            v.append(("cols = 1", dict(base, cols=1)))
        v += [("%s = %g" % (k, x), dict(base, **{k: x})) for k, xs in (("inv_temp", (0.0, -1.0)), ("eps", (0.0, 1.5))) if k in base for x in xs]
        v += [("%s null" % k, dict(base, **{k: None})) for k in nulls]
        v += [("%s = %d" % (k, x) if k.startswith("ld") else "%s misaligned" % k, dict(base, **{k: x})) for k, x in odd.items()]
        for label, a in v:
            rc = call(a)
            lines.append("%-58s rc %d  %s" % ("%s: %s" % (name, label), rc, lib.hero_last_error().decode() if rc else ""))

    def ce(fn):
        return lambda a: fn(C.byref(Lb.CrossEntropy(a["logits"], a["labels"], a["loss"], a["lse"], a["dloss"], a["dlogits"], a["rows"], a["cols"],
                                                    a["ld"], a["dtype"], 1.0, -100)), None)

    base = dict(logits=P, labels=P, loss=P, lse=P, dloss=P, dlogits=P, rows=4, cols=16, ld=16, dtype=0)
    variants("hero_cross_entropy_fwd", ce(lib.hero_cross_entropy_fwd), base, ("logits", "labels", "loss", "lse"), dict(logits=A4))
    variants("hero_cross_entropy_bwd", ce(lib.hero_cross_entropy_bwd), base, ("logits", "labels", "lse", "dloss", "dlogits"), dict(logits=A4, dlogits=A4))
    for fn in (lib.hero_cross_entropy_fwd, lib.hero_cross_entropy_bwd):
        lines.append("%-58s rc %d  %s" % ("hero_cross_entropy: struct null", fn(None, None), lib.hero_last_error().decode()))
    base = dict(logits=P, labels=P, count=P, loss=P, lse=P, mean_cnt=P, dloss=P, dlogits=P, rows=4, cols=16, ld=16, dtype=0, inv_temp=1.0)
    variants("hero_ce_counted_fwd", lambda a: lib.hero_ce_counted_fwd(a["logits"], a["labels"], a["count"], a["loss"], a["lse"], a["mean_cnt"], a["rows"],
                                                                      a["cols"], a["ld"], a["dtype"], a["inv_temp"], -100, None),
             base, ("logits", "labels", "loss", "lse", "mean_cnt"), dict(logits=A4, mean_cnt=A2), rows0_returns=False)
    variants("hero_ce_counted_bwd", lambda a: lib.hero_ce_counted_bwd(a["logits"], a["labels"], a["count"], a["lse"], a["dloss"], a["mean_cnt"], a["dlogits"],
                                                                      a["rows"], a["cols"], a["ld"], a["dtype"], a["inv_temp"], -100, None),
             base, ("logits", "labels", "lse", "dloss", "mean_cnt", "dlogits"), dict(logits=A4, mean_cnt=A2, dlogits=A4))
    base = dict(logits=P, labels=P, loss=P, lse=P, sum_cnt=P, dloss=P, dloss_rows=P, mean_cnt=P, dlogits=P, rows=4, cols=16, ld=16, dtype=0, eps=0.1)
    variants("hero_smooth_ce_fwd", lambda a: lib.hero_smooth_ce_fwd(a["logits"], a["labels"], a["loss"], a["lse"], a["sum_cnt"], a["rows"], a["cols"], a["ld"],
                                                                    a["dtype"], a["eps"], -100, None),
             base, ("logits", "labels", "loss", "lse", "sum_cnt"), dict(logits=A4), cols1=True, rows0_returns=False)
    variants("hero_smooth_ce_bwd", lambda a: lib.hero_smooth_ce_bwd(a["logits"], a["labels"], a["lse"], a["dloss"], a["dloss_rows"], a["mean_cnt"], a["dlogits"],
                                                                    a["rows"], a["cols"], a["ld"], a["dtype"], a["eps"], -100, None),
             base, ("logits", "labels", "lse", "dloss", "dlogits"), dict(logits=A4, dlogits=A4), cols1=True)
    base = dict(logits=P, labels=P, acc=P, pred=P, ws=P, rows=4, cols=16, ld=16, dtype=0, inv_temp=1.0)
    variants("hero_ce_eval", lambda a: lib.hero_ce_eval(a["logits"], a["labels"], a["rows"], a["cols"], a["ld"], a["dtype"], a["inv_temp"], -1, a["acc"],
                                                        a["pred"], a["ws"], None),
             base, ("logits", "labels", "acc", "ws"), dict(logits=A4, acc=A4, ws=A2, pred=A2))
    base = dict(pred=P, target=P, acc=P, ws=P, rows=4, cols=16, ld=16, ld_t=16, dtype=0)
    variants("hero_feat_eval", lambda a: lib.hero_feat_eval(a["pred"], a["target"], a["rows"], a["cols"], a["ld"], a["ld_t"], a["dtype"], a["acc"], a["ws"], None),
             base, ("pred", "target", "acc", "ws"), dict(pred=A4, target=A4, acc=A4, ws=A2, ld_t=15))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d calls, %d refused, from %s -> %s" % (len(lines), sum(" rc 0 " not in l for l in lines), Lb.LIB_PATH, path))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "save":
        save(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) == 3 and sys.argv[1] == "refused":
        refused(sys.argv[2])
    else:
        sys.exit(__doc__)
