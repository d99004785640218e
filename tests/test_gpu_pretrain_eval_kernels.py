"""hero_ce_eval and hero_feat_eval (hero_amd/csrc/loss.hip) through hero_amd.pretrain_eval and the C ABI, against their float64 /
integer statement (tests/pretrain_eval_reference.py): predictions and counts exactly, the loss sum within the per-row tolerance
test_cross_entropy_matches_torch carries for the same arithmetic, the feature sums within the fp32 bound that
tests/test_cpu_pretrain_eval.py derives."""
import functools

import numpy as np
import pytest
import torch

from tests import pretrain_eval_reference as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float32]
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def _ce_case(shape):
    rows, cols, ld = shape
    x, y = R.ce_case(rows, cols, ld)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def _ce_want(shape, inv_temp):
    x, y = _ce_case(shape)
    acc, pred = R.ce_eval(x, y, shape[1], inv_temp, R.CE_IGNORE)
    return acc, pred, R.ce_loss_tolerance(x, y, shape[1], inv_temp, R.CE_IGNORE)


def _device_case(shape, dtype):
    x, y = _ce_case(shape)
    logits = torch.from_numpy(x.copy()).cuda().to(dtype)
    assert torch.equal(logits.float().cpu(), torch.from_numpy(x.copy()))             # the grid is exact in bf16
    return logits, torch.from_numpy(y.copy()).cuda()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64).clone()


@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("inv_temp", [1.0, 0.7])
def test_ce_eval_matches_the_statement(shape, dtype, inv_temp):
    from hero_amd import pretrain_eval as E
    rows, cols, ld = shape
    logits, labels = _device_case(shape, dtype)
    x_bits, y_bits = _bits(logits), labels.clone()
    want, want_pred, tol = _ce_want(shape, inv_temp)
    acc, pred = E.ce_eval(logits, labels, ncols=cols, ignore_index=R.CE_IGNORE, inv_temp=inv_temp, want_pred=True)
    assert acc.dtype == torch.float64 and pred.dtype == torch.int32
    got = acc.cpu()
    print("ce_eval", shape, dtype, inv_temp, "loss sum", got[0].item(), "statement", want[0], "tolerance", tol)
    assert torch.equal(pred.cpu().long(), torch.from_numpy(want_pred))              # planted ties, the padding never wins
    assert torch.equal(got[1:], torch.tensor([want[1], want[2]], dtype=torch.float64))
    assert abs(got[0].item() - want[0]) <= tol
    # the inputs (padding columns included) are read only
    assert torch.equal(_bits(logits), x_bits) and torch.equal(labels, y_bits)
    # a pre-filled triple is added to; a second run gives the same bits
    pre = torch.tensor([0.5, 3.0, 4.0], dtype=torch.float64)
    acc2 = E.ce_eval(logits, labels, ncols=cols, ignore_index=R.CE_IGNORE, inv_temp=inv_temp, acc=pre.cuda()).cpu()
    assert torch.equal(acc2[1:], got[1:] + pre[1:]) and acc2[0].item() == 0.5 + got[0].item()
    again = E.ce_eval(logits, labels, ncols=cols, ignore_index=R.CE_IGNORE, inv_temp=inv_temp).cpu()
    assert torch.equal(again.view(torch.int64), got.view(torch.int64))


def test_ce_eval_planted_rows():
    """What ce_case plants, spelled out on the vocabulary shape: 2047 before 2048 (one thread, neighbouring trips), 5 before 2053,
    the label on the first maximum counts and on the second does not, and 6.0 in the padding is never seen."""
    shape = (37, 50265, 50272)
    x, y = _ce_case(shape)
    _, pred, _ = _ce_want(shape, 1.0)
    assert x[0, 2047] == x[0, 2048] == 5.0 == x[0, :50265].max() and pred[0] == 2047 == y[0]
    assert x[1, 5] == x[1, 2053] == 5.0 and pred[1] == 5 and y[1] == 2053
    assert (x[:, 50265:] == 6.0).all() and x[:, :50265].max() == 5.0 and pred.max() < 50265
    assert list(y[-3:]) == [-1, 50265, 50271]
    xt, yt = _ce_case((64, 1931, 1936))
    assert xt[2, 8] == xt[2, 1930] == 5.0 and _ce_want((64, 1931, 1936), 1.0)[1][2] == 8


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_ce_eval_writes_only_its_outputs(dtype):
    """The C entry point with guard elements around pred, acc and the workspace; rows == 0 launches nothing."""
    from hero_amd import _lib as L
    shape = (64, 1931, 1936)
    rows, cols, ld = shape
    logits, labels = _device_case(shape, dtype)
    want, want_pred, tol = _ce_want(shape, 1.0)
    G = 8
    pred = torch.full((rows + 2 * G,), -77, dtype=torch.int32, device="cuda")
    acc = torch.full((3 + 2 * G,), SENTINEL, dtype=torch.float64, device="cuda")
    acc[G:G + 3] = 0
    ws = torch.full((3 * rows + 2 * G,), SENTINEL, dtype=torch.float32, device="cuda")
    rc = L.lib().hero_ce_eval(L.ptr(logits), L.ptr(labels), rows, cols, ld, L.dt(logits), 1.0, R.CE_IGNORE, acc.data_ptr() + 8 * G,
                              pred.data_ptr() + 4 * G, ws.data_ptr() + 4 * G, L.stream())
    L.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(pred[G:-G].cpu().long(), torch.from_numpy(want_pred))
    assert (pred[:G] == -77).all() and (pred[-G:] == -77).all()
    assert (acc[:G] == SENTINEL).all() and (acc[-G:] == SENTINEL).all() and acc[G + 2].item() == want[2]
    assert (ws[:G] == SENTINEL).all() and (ws[-G:] == SENTINEL).all()
    # rows == 0: acc untouched (no pointer is looked at); bad arguments are refused with a message
    before = acc.clone()
    L.check(L.lib().hero_ce_eval(None, None, 0, cols, ld, L.dt(logits), 1.0, -1, acc.data_ptr(), None, None, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(acc, before)
    p = L.ptr(logits)
    for bad in ((rows, cols, cols - 1, 1.0), (rows, 0, ld, 1.0), (rows, cols, ld, 0.0), (-1, cols, ld, 1.0)):
        assert L.lib().hero_ce_eval(p, L.ptr(labels), bad[0], bad[1], bad[2], L.dt(logits), bad[3], -1, acc.data_ptr(), None, ws.data_ptr(),
                                    L.stream()) == -1, bad
    assert b"hero_ce_eval" in L.lib().hero_last_error()


def test_ce_eval_wrapper_rows_zero_and_fallback():
    from hero_amd import pretrain_eval as E
    pre = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device="cuda")
    acc, pred = E.ce_eval(torch.zeros(0, 16, device="cuda"), torch.zeros(0, dtype=torch.long, device="cuda"), acc=pre.clone(), want_pred=True)
    assert torch.equal(acc, pre) and pred.numel() == 0
    # what the kernel refuses (a strided view) takes the float64 PyTorch statement, with the same answers
    logits, labels = _device_case((64, 1931, 1936), torch.float32)
    want, want_pred, _ = _ce_want((64, 1931, 1936), 1.0)
    acc, pred = E.ce_eval(logits[:, :1931], labels, ignore_index=R.CE_IGNORE, want_pred=True)
    assert torch.equal(pred.cpu().long(), torch.from_numpy(want_pred)) and acc[1].item() == want[1] and acc[2].item() == want[2]
    assert abs(acc[0].item() - want[0]) <= 1e-9 * want[0]


def test_ce_eval_captured_in_a_graph():
    """Two launches, nothing read on the host: captured once, replayed twice, the counters advance by exactly twice the eager
    amounts (0 + L and L + L are exact in float64)."""
    from hero_amd import pretrain_eval as E
    shape = (64, 1931, 1936)
    logits, labels = _device_case(shape, torch.bfloat16)
    eager = E.ce_eval(logits, labels, ncols=shape[1], ignore_index=R.CE_IGNORE).cpu()          # also loads the library
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gs = torch.cuda.Stream()
    gs.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(gs):
        with torch.cuda.graph(graph, stream=gs):
            E.ce_eval(logits, labels, ncols=shape[1], ignore_index=R.CE_IGNORE, acc=acc)
    torch.cuda.current_stream().wait_stream(gs)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), 2 * eager) and eager[2].item() == _ce_want(shape, 1.0)[0][2]


def _fold_f64(rows_f32):
    """The fold's documented order in float64: thread i adds rows i, i + 256, ... in order, then the halving tree w = 128 ... 1."""
    part = np.zeros(256, dtype=np.float64)
    for r, v in enumerate(np.asarray(rows_f32, dtype=np.float64)):
        part[r % 256] += v
    w = 128
    while w:
        part[:w] += part[w:2 * w]
        w >>= 1
    return part[0]


@pytest.mark.parametrize("shape", [(5, 7, 7), (5, 37, 40), (300, 2051, 2056), (5, 4101, 4104)], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("inv_temp", [1.0, 0.7])
def test_ce_eval_loss_is_the_training_loss_bit_for_bit(shape, dtype, inv_temp):
    """hero_ce_eval and hero_cross_entropy_fwd share one row scan: the loss counter is the float64 sum, in the fold's order, of the
    training kernel's per-row losses - the same int64 bit pattern - and the valid count is the number of live labels."""
    import ctypes as C
    from hero_amd import _lib as L
    from hero_amd import pretrain_eval as E
    rows, cols, ld = shape
    x, y = _ce_case(shape)
    y = y.copy()
    y[3], y[4] = R.CE_IGNORE, cols                                    # some ignored labels at every shape
    logits, labels = torch.from_numpy(x.copy()).cuda().to(dtype), torch.from_numpy(y).cuda()
    loss = torch.full((rows,), SENTINEL, dtype=torch.float32, device="cuda")
    lse = torch.empty((rows,), dtype=torch.float32, device="cuda")
    a = L.CrossEntropy(L.ptr(logits), L.ptr(labels), L.ptr(loss), L.ptr(lse), None, None, rows, cols, ld, L.dt(logits), inv_temp, R.CE_IGNORE)
    L.check(L.lib().hero_cross_entropy_fwd(C.byref(a), L.stream()))
    acc = E.ce_eval(logits, labels, ncols=cols, ignore_index=R.CE_IGNORE, inv_temp=inv_temp).cpu()
    live = (y != R.CE_IGNORE) & (y >= 0) & (y < cols)
    row_loss = loss.cpu().numpy()
    assert (row_loss[~live] == 0.0).all() and 0 < live.sum() < rows
    want = np.array([_fold_f64(row_loss)])
    print("ce_eval against cross_entropy_fwd", shape, dtype, inv_temp, "counter", acc[0].item(), "fold of the row losses", want[0])
    assert acc[:1].view(torch.int64).item() == want.view(np.int64)[0]
    assert acc[2].item() == live.sum()


# ---- hero_feat_eval ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _feat(rows, cols):
    p, t = R.feat_case(rows, cols)
    l2, cos = R.feat_eval_rows(p, t)
    return p, t, l2, cos


@pytest.mark.parametrize("rows", R.FEAT_ROWS)
@pytest.mark.parametrize("cols", R.FEAT_COLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_feat_eval_matches_the_statement(rows, cols, dtype):
    from hero_amd import _lib as L
    from hero_amd import pretrain_eval as E
    p, t, l2, cos = _feat(rows, cols)
    assert cos[rows - 1] == 0.0 and (rows == 1 or l2[0] == 0.0)                     # the zero target row; pred == target
    pd, td = torch.from_numpy(p.copy()).cuda().to(dtype), torch.from_numpy(t.copy()).cuda().to(dtype)
    got = E.feat_eval(pd, td).cpu()
    tol_l2, tol_cos = R.FEAT_L2_REL * float(l2.sum()), R.FEAT_COS_ABS * rows
    print("feat_eval", rows, cols, dtype, "l2", got[0].item(), l2.sum(), tol_l2, "cos", got[1].item(), cos.sum(), tol_cos)
    assert got[2].item() == rows
    assert abs(got[0].item() - l2.sum()) <= tol_l2 and abs(got[1].item() - cos.sum()) <= tol_cos
    # unequal leading dimensions (multiples of 8: the 16-byte loads; then not: the scalar form), guard columns untouched, a
    # pre-filled triple added to, two runs with the same bits
    for ld_p, ld_t in ((((cols + 7) & ~7) + 8, ((cols + 7) & ~7) + 24), (cols + 3, cols + 1)):
        wp = torch.full((rows, ld_p), SENTINEL, dtype=dtype, device="cuda")
        wt = torch.full((rows, ld_t), SENTINEL, dtype=dtype, device="cuda")
        wp[:, :cols], wt[:, :cols] = pd, td
        bp, bt = _bits(wp), _bits(wt)
        runs = []
        for _ in range(2):
            acc = torch.tensor([0.5, 0.25, 7.0], dtype=torch.float64, device="cuda")
            ws = torch.full((2 * rows + 8,), SENTINEL, dtype=torch.float32, device="cuda")
            L.check(L.lib().hero_feat_eval(L.ptr(wp), L.ptr(wt), rows, cols, ld_p, ld_t, L.dt(wp), L.ptr(acc), L.ptr(ws), L.stream()))
            runs.append(acc.cpu())
            assert (ws[2 * rows:] == SENTINEL).all()
        assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))
        assert runs[0][2].item() == rows + 7
        assert abs(runs[0][0].item() - 0.5 - l2.sum()) <= tol_l2 and abs(runs[0][1].item() - 0.25 - cos.sum()) <= tol_cos
        assert torch.equal(_bits(wp), bp) and torch.equal(_bits(wt), bt)
    if rows == 5 and cols == 132:
        one = torch.zeros(3, dtype=torch.float64, device="cuda")                   # the exact zero of the pred == target row
        E.feat_eval(pd[:1].contiguous(), td[:1].contiguous(), acc=one)
        assert one[0].item() == 0.0 and one[2].item() == 1


def test_feat_eval_rows_zero_and_bad_arguments():
    from hero_amd import _lib as L
    from hero_amd import pretrain_eval as E
    pre = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device="cuda")
    assert torch.equal(E.feat_eval(torch.zeros(0, 8, device="cuda"), torch.zeros(0, 8, device="cuda"), acc=pre.clone()), pre)
    x = torch.zeros(4, 16, device="cuda")
    ws = torch.zeros(8, device="cuda")
    for rows, cols, ld_p, ld_t in ((4, 16, 8, 16), (4, 16, 16, 8), (4, 0, 16, 16), (-1, 16, 16, 16)):
        assert L.lib().hero_feat_eval(L.ptr(x), L.ptr(x), rows, cols, ld_p, ld_t, L.F32, L.ptr(pre), L.ptr(ws), L.stream()) == -1
    assert b"hero_feat_eval" in L.lib().hero_last_error()
    with pytest.raises(ValueError):
        E.feat_eval(x, x[:, :8])
