"""The row-movement and index kernels of hero_amd/csrc/rows.hip through the raw ctypes ABI - hero_gather_rows,
hero_scatter_add_rows, hero_csr_gather_sum, hero_inverse_first, hero_segment_sort, hero_scatter_add_sorted (+ fold),
hero_transpose_cast, hero_copy_multi - against the host statements of tests/rows_reference.py (held against torch and the
project's host builders by tests/test_cpu_rows_reference.py).

Every comparison is exact: moved values bit for bit, sums through integer-valued operands whose every partial sum the
accumulator holds (rows_reference's docstring; the conditions are asserted on the CPU for every case used here).  The two
random-float cases of hero_scatter_add_sorted use the a-priori bound of a sum of n fp32 addends taken in any order,
|got - ref| <= n * 2^-24 * (|dst0| + sum |x|) per (destination, column) (n <= 1027: n (n - 1) 2^-24 < 1, so n 2^-24 bounds
gamma_(n-1)); the random-float case of hero_csr_gather_sum is compared bit for bit with the float32 sum in entry order.

Every destination and workspace lives inside a larger buffer between 64 guard elements and is pre-filled with NaN (floats) or
a sentinel (ints) unless the operation accumulates into it; after each call everything outside the contract's write set has the
bits it had before."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import rows_reference as R

pytestmark = pytest.mark.gpu

G = 64                                   # guard elements on each side of every buffer a kernel writes
ISENT = -77777                           # pre-fill of integer outputs: no index of this file
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
CODE = {"f32": 0, "bf16": 1}


@pytest.fixture(scope="module")
def Lb():
    from hero_amd import _lib
    _lib.lib()
    return _lib


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b.to(a.device)))


class Buf:
    """A device tensor inside a larger buffer: G guard elements before and after, `off` more elements in front (misalignment).
    Pre-filled with NaN / ISENT, or with `init`.  `before` is the pre-call image of the whole buffer."""

    def __init__(self, shape, dtype, init=None, off=0):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape))
        fill = float("nan") if dtype.is_floating_point else ISENT
        self.buf = torch.full((n + 2 * G + off,), fill, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.lo, self.n = G + off, n
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        if init is not None:
            self.t.copy_(init if torch.is_tensor(init) else torch.from_numpy(np.ascontiguousarray(init)))
        self.before = self.buf.clone()

    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.buf.element_size()       # (an empty view has no data_ptr of its own)

    def prefill(self):
        return self.before[self.lo:self.lo + self.n].view(self.t.shape)

    def guards_intact(self):
        b, a = bits(self.before), bits(self.buf)
        return torch.equal(a[:self.lo], b[:self.lo]) and torch.equal(a[self.lo + self.n:], b[self.lo + self.n:])

    def untouched(self):
        return torch.equal(bits(self.buf), bits(self.before))


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def equals_f64(got, ref):
    """The device tensor holds exactly the float64 values `ref` (integer-valued cases)."""
    return torch.equal(got.double().cpu(), torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float64)))


def sync():
    torch.cuda.synchronize()


# ---- hero_gather_rows ----------------------------------------------------------------------------------------------------------
GATHER_SHAPES = [(1, 4), (200, 4), (1, 8), (200, 8), (1, 132), (200, 132), (1, 768), (200, 768),
                 (2731, 768)]                    # 2731 * 768 / 4 = 524352 float4 > 2048 workgroups x 256 threads: a second grid-stride trip


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", GATHER_SHAPES)
def test_gather_rows(Lb, dtype, rows, cols):
    assert rows != 2731 or rows * cols // 4 > 2048 * 256
    rs = np.random.RandomState(rows + cols)
    a = dev(rs.randn(50, cols).astype(np.float32), TD[dtype])
    b = dev(rs.randn(30, cols).astype(np.float32), TD[dtype])
    an, bn = a.double().cpu().numpy(), b.double().cpu().numpy()
    if rows == 1:
        lists = [np.int32([49]), np.int32([-1]), np.int32([-31]), np.int32([0])]
    else:
        idx = rs.randint(-31, 50, size=rows).astype(np.int32)
        idx[::17], idx[1::19], idx[2::23], idx[3::29], idx[4::31] = -1, 0, 49, -2, -31          # zero rows, both ends of both tables
        lists = [idx, np.where(idx <= -2, -1, idx).astype(np.int32)]
    for k, idx in enumerate(lists):
        with_b = bool((idx <= -2).any())                                   # no index <= -2: b is NULL
        out = Buf((len(idx), cols), TD[dtype])
        di = dev(idx)
        Lb.check(Lb.lib().hero_gather_rows(a.data_ptr(), b.data_ptr() if with_b else None, di.data_ptr(), out.ptr(), len(idx), cols,
                                          CODE[dtype], Lb.stream()))
        sync()
        want = torch.from_numpy(R.gather_ref(an, bn, idx)).to(TD[dtype])
        assert same_bits(out.t, want), (k, int((bits(out.t).cpu() != bits(want)).sum()))
        assert out.guards_intact()


# ---- hero_scatter_add_rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [-1, 3])
@pytest.mark.parametrize("cols", R.SCATTER_COLS)
@pytest.mark.parametrize("sd,dd", R.SCATTER_COMBOS)
def test_scatter_add_rows(Lb, sd, dd, cols, skip):
    c = R.scatter_rows_case(cols, skip)
    src, idx = dev(c["src"], TD[sd]), dev(c["idx"])
    for with_b in (True, False):                                          # dst_b NULL: rows with negative ids are dropped, dst_a as before
        da = Buf((c["n_a"], cols), TD[dd], init=dev(c["a0"], TD[dd]))
        db = Buf((c["n_b"], cols), TD[dd], init=dev(c["b0"], TD[dd]))
        Lb.check(Lb.lib().hero_scatter_add_rows(src.data_ptr(), idx.data_ptr(), da.ptr(), db.ptr() if with_b else None, len(c["idx"]), cols,
                                               CODE[sd], CODE[dd], skip, Lb.stream()))
        sync()
        ra, rb = R.scatter_add_ref(c["src"].astype(np.float64), c["idx"], c["a0"], c["b0"] if with_b else None, skip)
        assert equals_f64(da.t, ra), ("dst_a", with_b, float((da.t.double().cpu() - torch.from_numpy(ra)).abs().max()))
        if with_b:
            assert equals_f64(db.t, rb), ("dst_b", float((db.t.double().cpu() - torch.from_numpy(rb)).abs().max()))
            assert db.guards_intact()
        else:
            assert db.untouched()
        if skip >= 0:
            assert same_bits(da.t[skip], da.prefill()[skip])
        assert da.guards_intact()


# ---- hero_csr_gather_sum -------------------------------------------------------------------------------------------------------
CSR_COUNTS = [0, 1, 2, 9, 1, 3, 0]                                           # entries per output row; the last row is empty


def csr_case(seed):
    rs = np.random.RandomState(seed)
    offs = np.concatenate([[0], np.cumsum(CSR_COUNTS)]).astype(np.int32)
    ent = rs.randint(0, 40, size=offs[-1]).astype(np.int32)
    ent[offs[5]:offs[6]] = [11, 39, 11]                                       # a repeated entry
    ent[offs[3]] = 0
    return offs, ent


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cols", [4, 132, 768])
def test_csr_gather_sum_integer_data(Lb, dtype, cols):
    offs, ent = csr_case(cols)
    srcn = np.random.RandomState(cols).randint(-8, 9, size=(40, cols)).astype(np.float32)          # |sum| <= 72: exact in bf16
    src, out = dev(srcn, TD[dtype]), Buf((len(CSR_COUNTS), cols), TD[dtype])
    do, de = dev(offs), dev(ent)
    Lb.check(Lb.lib().hero_csr_gather_sum(src.data_ptr(), do.data_ptr(), de.data_ptr(), out.ptr(), len(CSR_COUNTS), cols, CODE[dtype], Lb.stream()))
    sync()
    ref = R.csr_gather_sum_ref(srcn.astype(np.float64), offs, ent)
    assert np.abs(ref).max() <= 72 and equals_f64(out.t, ref)
    assert not out.t[0].any() and not out.t[-1].any() and out.guards_intact()


def test_csr_gather_sum_float_data_in_entry_order(Lb):
    cols = 132
    offs, ent = csr_case(1)
    srcn = np.random.RandomState(2).randn(40, cols).astype(np.float32)
    src, out = dev(srcn), Buf((len(CSR_COUNTS), cols), torch.float32)
    do, de = dev(offs), dev(ent)
    Lb.check(Lb.lib().hero_csr_gather_sum(src.data_ptr(), do.data_ptr(), de.data_ptr(), out.ptr(), len(CSR_COUNTS), cols, 0, Lb.stream()))
    sync()
    assert same_bits(out.t, torch.from_numpy(R.csr_gather_sum_f32_in_order(srcn, offs, ent)))
    assert out.guards_intact()


# ---- hero_inverse_first --------------------------------------------------------------------------------------------------------
def run_inverse_first(Lb, idx, na, nb):
    inv = Buf(na + nb, torch.int32)
    di = dev(idx if len(idx) else np.int32([ISENT]))
    rc = Lb.lib().hero_inverse_first(di.data_ptr(), len(idx), inv.ptr(), na, nb, Lb.stream())
    sync()
    return rc, inv


@pytest.mark.parametrize("tot", [1, 1024, 1025, 16384, 16385, 38400])      # 16384 ints = the 64 KiB default; 38400 = the 150 KiB opt-in
def test_inverse_first(Lb, tot):
    na = tot - tot // 3                                                       # tot = 1: nb = 0
    nb = tot - na
    assert nb > 0 or tot == 1
    for n in (0, 1, 5000):
        rs = np.random.RandomState(tot + n)
        idx = rs.randint(-nb - 2 - 40, na + 40, size=n).astype(np.int32)      # ids past the end of either table among them
        if n == 5000:
            idx[::50], idx[1::50], idx[2::50] = na + 7, -nb - 2, na - 1       # out of range on both sides; the last row of a
            if nb:
                idx[3::50] = -nb - 1                                          # the last row of b
        rc, inv = run_inverse_first(Lb, idx, na, nb)
        Lb.check(rc)
        want = R.inverse_first_ref(idx, na, nb)
        assert torch.equal(inv.t.cpu(), torch.from_numpy(want)), (n, int((inv.t.cpu() != torch.from_numpy(want)).sum()))
        assert inv.guards_intact()
        assert n < 5000 or want[na - 1] == 2


def test_inverse_first_every_source_named_many_times_and_no_b(Lb):
    for na, nb in ((20, 10), (30, 0)):
        rs = np.random.RandomState(na)
        idx = rs.randint(-nb - 1, na, size=5000).astype(np.int32)
        rc, inv = run_inverse_first(Lb, idx, na, nb)
        Lb.check(rc)
        want = R.inverse_first_ref(idx, na, nb)
        named = np.where(idx >= 0, idx, na - idx - 2)[idx != -1]
        assert (want >= 0).all() and np.bincount(named, minlength=na + nb).min() >= 50
        assert torch.equal(inv.t.cpu(), torch.from_numpy(want)) and inv.guards_intact()


def test_inverse_first_refuses_more_rows_than_the_lds_table(Lb):
    rc, inv = run_inverse_first(Lb, np.zeros(10, dtype=np.int32), 38000, 401)
    assert rc != 0 and inv.untouched()
    assert b"38400" in Lb.lib().hero_last_error()


# ---- hero_segment_sort ---------------------------------------------------------------------------------------------------------
def device_order(Lb, idx, n_dst, skip):
    rows = len(idx)
    order = Buf(rows, torch.int32)
    ws = Buf(max(Lb.lib().hero_segment_sort_workspace_bytes(rows) // 4, 1), torch.int32)
    di = dev(idx)
    Lb.check(Lb.lib().hero_segment_sort(di.data_ptr(), rows, n_dst, skip, order.ptr(), ws.ptr(), Lb.stream()))
    sync()
    assert order.guards_intact() and ws.guards_intact()
    return order.t.cpu().numpy()


@pytest.mark.parametrize("n_dst", R.SORT_NDST)
def test_segment_sort(Lb, n_dst):
    """The index holds ids up to n_dst - 1; no table of n_dst rows exists - the sort reads idx only.  n_dst >= 2^28 takes 32 key
    bits: the dropped rows' key must still sort behind id n_dst - 1 and not among id 0."""
    from hero_amd.functional import host_segment_order
    assert Lb.lib().hero_segment_sort_workspace_bytes(1000) == 16000
    for k, (rows, skip, pattern) in enumerate(R.sort_cases(n_dst)):
        idx = R.sort_ids(rows, n_dst, skip, pattern, seed=100 + k)
        got = device_order(Lb, idx, n_dst, skip)
        want = R.segment_order_ref(idx, skip)
        assert np.array_equal(want, host_segment_order(idx, skip))
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            dropped = (idx < 0) | (idx == skip)
            first_dropped = int(np.argmax(dropped[np.clip(got, 0, rows - 1)])) if dropped.any() else -1
            pytest.fail("n_dst %d (%d passes) rows %d skip %d %s: %d of %d positions differ, first at %d; the first dropped row stands at sorted "
                        "position %d, %d rows are kept; got[:8] %s want[:8] %s"
                        % (n_dst, R.sort_passes(n_dst), rows, skip, pattern, len(bad), rows, bad[0], first_dropped, int((~dropped).sum()),
                           got[:8].tolist(), want[:8].tolist()))


# ---- hero_scatter_add_sorted (+ fold) ------------------------------------------------------------------------------------------
def scatter_sorted(Lb, src, idx, order, table, skip):
    """One call on fresh guarded buffers; returns (dst Buf, workspace Buf)."""
    rows, cols = src.shape
    dst = Buf(tuple(table.shape), torch.float32, init=table)
    ws = Buf(max(Lb.lib().hero_scatter_add_sorted_workspace_bytes(rows, cols) // 4, 1), torch.float32)
    Lb.check(Lb.lib().hero_scatter_add_sorted(src.data_ptr(), idx.data_ptr(), order.data_ptr(), dst.ptr(), rows, cols,
                                             1 if src.dtype == torch.bfloat16 else 0, skip, ws.ptr(), Lb.stream()))
    sync()
    return dst, ws


def unnamed_rows(c):
    named = set(int(v) for v in c["idx"] if v >= 0 and v != c["skip"])
    return torch.tensor([r for r in range(c["n_dst"]) if r not in named], dtype=torch.long, device="cuda")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cols", [4, 8, 252, 256, 260, 768, 772, 1540])
def test_scatter_add_sorted_constructed_runs(Lb, dtype, cols):
    """Integer data: bit-exact against float64, for every constructed id list (tests/rows_reference.sorted_cases: every way a
    run can lie across the 16-position blocks).  Sorted by the host order the feeder copies in."""
    assert Lb.lib().hero_scatter_add_sorted_workspace_bytes(33, cols) == 3 * 2 * cols * 4
    for c in R.sorted_cases():
        rows = len(c["idx"])
        srcn, tabn = R.int_rows(rows, cols, seed=rows + cols), R.int_table(c["n_dst"], cols)
        order = dev(R.segment_order_ref(c["idx"], c["skip"]))
        dst, ws = scatter_sorted(Lb, dev(srcn, TD[dtype]), dev(c["idx"]), order, dev(tabn), c["skip"])
        ref = R.scatter_sorted_ref(srcn.astype(np.float64), c["idx"], tabn, c["skip"])
        diff = (dst.t.double().cpu() - torch.from_numpy(ref)).abs()
        assert equals_f64(dst.t, ref), (c["name"], "rows of the table that differ", torch.nonzero(diff.amax(1)).flatten().tolist()[:12], float(diff.max()))
        keep = unnamed_rows(c)
        assert same_bits(dst.t[keep], dst.prefill()[keep]), c["name"]
        assert dst.guards_intact() and ws.guards_intact(), c["name"]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_scatter_add_sorted_random_floats_within_the_summation_bound_and_reproducible(Lb, dtype):
    c = R.sorted_cases()[0]
    rows, cols = len(c["idx"]), 772
    rs = np.random.RandomState(9)
    srcn = dev(rs.randn(rows, cols).astype(np.float32), TD[dtype]).float().cpu().numpy()              # the values the kernel reads
    tabn = rs.randn(c["n_dst"], cols).astype(np.float32)
    src, idx, order, tab = dev(srcn, TD[dtype]), dev(c["idx"]), dev(R.segment_order_ref(c["idx"], c["skip"])), dev(tabn)
    outs = [scatter_sorted(Lb, src, idx, order, tab, c["skip"])[0] for _ in range(3)]
    ref = R.scatter_sorted_ref(srcn.astype(np.float64), c["idx"], tabn, c["skip"])
    keep = (c["idx"] >= 0) & (c["idx"] != c["skip"])
    n = 1.0 + np.bincount(c["idx"][keep], minlength=c["n_dst"])                                         # addends per destination: dst0 and its rows
    mag = np.abs(tabn).astype(np.float64)
    np.add.at(mag, c["idx"][keep], np.abs(srcn[keep]).astype(np.float64))
    bound = n[:, None] * 2.0 ** -24 * mag
    err = np.abs(outs[0].t.double().cpu().numpy() - ref)
    print("\n[rows] scatter_sorted %s random floats: worst error / bound %.3f (n up to %d)" % (dtype, float((err / bound).max()), int(n.max())), end="")
    assert n.max() == 1027 and (err <= bound).all(), float((err / bound).max())
    un = unnamed_rows(c)
    assert same_bits(outs[0].t[un], outs[0].prefill()[un]) and outs[0].guards_intact()
    assert same_bits(outs[0].t, outs[1].t) and same_bits(outs[0].t, outs[2].t)


def test_segment_sort_feeds_scatter_add_sorted(Lb):
    c = R.sorted_cases()[0]
    rows, cols = len(c["idx"]), 768
    got = device_order(Lb, c["idx"], c["n_dst"], c["skip"])
    assert np.array_equal(got, R.segment_order_ref(c["idx"], c["skip"]))
    srcn, tabn = R.int_rows(rows, cols, seed=5), R.int_table(c["n_dst"], cols)
    outs = [scatter_sorted(Lb, dev(srcn, torch.bfloat16), dev(c["idx"]), dev(got), dev(tabn), c["skip"])[0] for _ in range(3)]
    assert equals_f64(outs[0].t, R.scatter_sorted_ref(srcn.astype(np.float64), c["idx"], tabn, c["skip"]))
    assert same_bits(outs[0].t, outs[1].t) and same_bits(outs[0].t, outs[2].t)


# ---- hero_transpose_cast -------------------------------------------------------------------------------------------------------
TRANSPOSE_SHAPES = [(1, 1), (1, 33), (31, 32), (32, 31), (32, 32), (33, 65), (65, 33), (65, 1), (31, 65), (33, 31), (65, 65), (32, 1)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_transpose_cast(Lb, dtype):
    assert {s[0] for s in TRANSPOSE_SHAPES} == {s[1] for s in TRANSPOSE_SHAPES} == {1, 31, 32, 33, 65}
    for Rr, Cc in TRANSPOSE_SHAPES:
        for ldd in (Rr, Rr + 3):
            src = dev(np.random.RandomState(Rr * 100 + Cc).randn(Rr, Cc).astype(np.float32))
            dst = Buf((Cc, ldd), TD[dtype])
            Lb.check(Lb.lib().hero_transpose_cast(src.data_ptr(), dst.ptr(), Rr, Cc, ldd, CODE[dtype], Lb.stream()))
            sync()
            want = dst.prefill().clone()
            want[:, :Rr] = src.t().to(TD[dtype])
            assert same_bits(dst.t, want), (Rr, Cc, ldd)                      # the padding columns keep their pre-fill
            assert dst.guards_intact(), (Rr, Cc, ldd)


# ---- hero_copy_multi -----------------------------------------------------------------------------------------------------------
def test_copy_multi_one_launch_over_a_mixed_table(Lb):
    """Plain and transposed copies into fp32 and bf16, leading dimensions equal to and larger than the natural width (also not a
    multiple of 4), a source one float past a 16-byte boundary, destinations 2 / 4 / 8 bytes past one: every store path of the
    kernel (tests/test_cpu_rows_reference.py asserts the table reaches them).  The whole arenas are compared, so padding and the
    bytes between the tensors are held too."""
    L = Lb
    descs, n32, n16 = R.copy_table()
    SENT = -776.0                                                              # exact in fp32 and bf16
    arena = {0: torch.full((n32,), SENT, dtype=torch.float32, device="cuda"), 1: torch.full((n16,), SENT, dtype=torch.bfloat16, device="cuda")}
    image = {0: np.full(n32, SENT, dtype=np.float32), 1: np.full(n16, SENT, dtype=np.float32)}
    table, srcs = [], []
    for i, d in enumerate(descs):
        n = d["rows"] * d["cols"]
        alloc = torch.empty(n + 4, device="cuda")
        assert alloc.data_ptr() % 256 == 0 and arena[d["bf16"]].data_ptr() % 256 == 0
        s = alloc[d["src_off"]:d["src_off"] + n].view(d["rows"], d["cols"])
        sn = np.random.RandomState(i).randn(d["rows"], d["cols"]).astype(np.float32)
        s.copy_(torch.from_numpy(sn))
        srcs.append(s)
        esz = 2 if d["bf16"] else 4
        dptr = arena[d["bf16"]].data_ptr() + d["at"] * esz
        assert s.data_ptr() % 16 == 4 * d["src_off"] and dptr % 16 == d["dst_off"]
        table.append(L.CopyDesc(s.data_ptr(), dptr, d["rows"], d["cols"], d["ldd"], d["transpose"], d["bf16"], 0))
        R.copy_apply(image[d["bf16"]], d["at"], sn, d["ldd"], d["transpose"], d["bf16"])
    tdesc, tidx = R.copy_tiles(descs)
    raw = torch.frombuffer(bytearray(bytes((L.CopyDesc * len(table))(*table))), dtype=torch.uint8).cuda()
    dt_, di_ = dev(np.int32(tdesc)), dev(np.int32(tidx))
    L.check(L.lib().hero_copy_multi(raw.data_ptr(), dt_.data_ptr(), di_.data_ptr(), len(tdesc), L.stream()))
    sync()
    for i, (d, s) in enumerate(zip(descs, srcs)):                              # each copy = src.to(dtype) / src.t().to(dtype), bit for bit
        want = (s.t() if d["transpose"] else s).to(arena[d["bf16"]].dtype)
        got = torch.as_strided(arena[d["bf16"]], tuple(want.shape), (d["ldd"], 1), d["at"])
        assert same_bits(got, want.contiguous()), (i, d)
    for k in (0, 1):                                                           # ... and nothing else changed
        want = torch.from_numpy(image[k]).to(arena[k].dtype)
        assert same_bits(arena[k], want), (k, torch.nonzero(bits(arena[k]).cpu() != bits(want)).flatten().tolist()[:8])
