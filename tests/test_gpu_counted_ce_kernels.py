"""The kernels behind the fixed-capacity pre-training heads, through the C ABI (include/hero_hip.h): hero_ce_counted_fwd / _bwd
against hero_cross_entropy_fwd / _bwd on the same buffer (bit for bit on the live rows, exact zeros everywhere else, NaN
behind the count never read), hero_mask_partition and hero_nce_pack_fwd / _bwd against their index statements.  Shapes are the
smallest at which the kernels take every path: a scalar-tail-only row (37 of 40 columns), a second trip of the 2048-column
vector loop plus a tail (2051 of 2056), partitions of less than a wave, more than a wave, more than one chunk of the workgroup
and several chunks with a ragged end, packed rows of three 16-byte segments and of 17 passes of a wavefront."""
import numpy as np
import pytest
import torch

from tests import pretrain_fixed_cases as C

pytestmark = pytest.mark.gpu

ROWS = 9
IGNORE = -100
DLOSS = 0.37


def _lib():
    from hero_amd import _lib as L
    return L, L.lib()


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _case(cols, ld, dtype, count, ignored):
    g = torch.Generator().manual_seed(cols * 31 + (0 if count is None else count))
    x = (torch.randn(ROWS, ld, generator=g) * 3).to(dtype)
    y = torch.randint(0, cols, (ROWS,), generator=g)
    if ignored:
        y[0], y[3] = IGNORE, IGNORE                               # below every count >= 4; row 0 below every count >= 1
    n = ROWS if count is None else min(count, ROWS)
    x[n:] = float("nan")                                          # rows at or behind the count must never be read
    live = torch.tensor([r < n and int(y[r]) != IGNORE for r in range(ROWS)])
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32).cuda()
    return x.cuda(), y.cuda(), cnt, n, live


def _plain_fwd(L, lib, x, y, cols, inv_temp):
    import ctypes
    rows, ld = x.shape
    loss, lse = torch.full((rows,), 7.0, device="cuda"), torch.full((rows,), 7.0, device="cuda")
    a = L.CrossEntropy(L.ptr(x), L.ptr(y), L.ptr(loss), L.ptr(lse), None, None, rows, cols, ld, L.dt(x), inv_temp, IGNORE)
    L.check(lib.hero_cross_entropy_fwd(ctypes.byref(a), L.stream()))
    return loss, lse


def _plain_bwd(L, lib, x, y, lse, dloss_rows, cols, inv_temp):
    import ctypes
    rows, ld = x.shape
    dx = torch.full_like(x, float("nan"))
    a = L.CrossEntropy(L.ptr(x), L.ptr(y), None, L.ptr(lse), L.ptr(dloss_rows), L.ptr(dx), rows, cols, ld, L.dt(x), inv_temp, IGNORE)
    L.check(lib.hero_cross_entropy_bwd(ctypes.byref(a), L.stream()))
    return dx


def _counted_fwd(L, lib, x, y, cnt, cols, inv_temp, out=None):
    rows, ld = x.shape
    loss, lse, mc = out or (torch.full((rows,), 7.0, device="cuda"), torch.full((rows,), 7.0, device="cuda"), torch.full((2,), 7.0, device="cuda"))
    L.check(lib.hero_ce_counted_fwd(L.ptr(x), L.ptr(y), L.ptr(cnt), L.ptr(loss), L.ptr(lse), L.ptr(mc), rows, cols, ld, L.dt(x), inv_temp, IGNORE,
                                    L.stream()))
    return loss, lse, mc


def _counted_bwd(L, lib, x, y, cnt, lse, dloss, mc, dx, cols, inv_temp):
    rows, ld = x.shape
    L.check(lib.hero_ce_counted_bwd(L.ptr(x), L.ptr(y), L.ptr(cnt), L.ptr(lse), L.ptr(dloss), L.ptr(mc), L.ptr(dx), rows, cols, ld, L.dt(x),
                                    inv_temp, IGNORE, L.stream()))
    return dx


def _check_fwd(loss, lse, mc, want_loss, want_lse, n, live):
    assert torch.equal(loss[:n], want_loss[:n]) and torch.equal(lse[:n], want_lse[:n])          # live AND ignored rows below the count
    assert torch.equal(_bits(loss[n:]), torch.zeros_like(_bits(loss[n:]))) and torch.equal(_bits(lse[n:]), torch.zeros_like(_bits(lse[n:])))
    assert not loss[:n][~live[:n].cuda()].any()
    n_live = int(live.sum())
    assert float(mc[1]) == float(n_live)
    mean = float(loss.double()[live.cuda()].sum() / max(n_live, 1))
    print("rows below the count", n, "live", n_live, "mean_cnt[0]", float(mc[0]), "float64 mean", mean)
    assert abs(float(mc[0]) - mean) <= float(np.spacing(np.float32(abs(mean))))                # one fp32 ulp
    if n_live == 0:
        assert mc.tolist() == [0.0, 0.0]


def _check_bwd(dx, want, live, cols):
    lv = live.cuda()
    assert torch.equal(_bits(dx[lv]), _bits(want[lv]))                                          # bit for bit (no NaN in live rows)
    assert torch.equal(_bits(dx[~lv]), torch.zeros_like(_bits(dx[~lv])))                        # exact +0 over all ld columns
    assert torch.equal(_bits(dx[:, cols:]), torch.zeros_like(_bits(dx[:, cols:])))              # padding columns


@pytest.mark.parametrize("ignored", [False, True])
@pytest.mark.parametrize("count", [None, 0, 1, 5, 9, 12])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cols, ld", [(37, 40), (2051, 2056)])
def test_counted_cross_entropy_equals_the_plain_kernels_on_the_live_rows(cols, ld, dtype, count, ignored):
    L, lib = _lib()
    inv_temp = 0.5 if cols == 37 else 1.0
    x, y, cnt, n, live = _case(cols, ld, dtype, count, ignored)
    want_loss, want_lse = _plain_fwd(L, lib, x, y, cols, inv_temp)
    loss, lse, mc = _counted_fwd(L, lib, x, y, cnt, cols, inv_temp)
    _check_fwd(loss, lse, mc, want_loss, want_lse, n, live)
    # backward: g = dloss[0] / max(n_live, 1) in fp32, as the kernel divides
    dloss = torch.tensor([DLOSS], dtype=torch.float32)
    g = dloss / torch.clamp(mc[1:2].cpu(), min=1.0)
    want = _plain_bwd(L, lib, x, y, want_lse, g.expand(ROWS).contiguous().cuda(), cols, inv_temp)
    dx = _counted_bwd(L, lib, x, y, cnt, lse, dloss.cuda(), mc, torch.full_like(x, float("nan")), cols, inv_temp)
    _check_bwd(dx, want, live, cols)
    # in place: the gradient over the logits themselves
    xi = x.clone()
    _counted_bwd(L, lib, xi, y, cnt, lse, dloss.cuda(), mc, xi, cols, inv_temp)
    assert torch.equal(_bits(xi), _bits(dx))
    torch.cuda.synchronize()


def test_counted_cross_entropy_without_rows_writes_the_zero_pair():
    L, lib = _lib()
    mc = torch.full((2,), 7.0, device="cuda")
    L.check(lib.hero_ce_counted_fwd(None, None, None, None, None, L.ptr(mc), 0, 8, 8, L.F32, 1.0, IGNORE, L.stream()))
    assert mc.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_captured_forward_backward_pair_replays_under_three_counts(dtype):
    L, lib = _lib()
    cols, ld, inv_temp = 2051, 2056, 1.0
    x, y, _, _, _ = _case(cols, ld, dtype, None, True)
    cnt = torch.tensor([4], dtype=torch.int32).cuda()
    dloss = torch.tensor([DLOSS]).cuda()
    out = (torch.zeros(ROWS, device="cuda"), torch.zeros(ROWS, device="cuda"), torch.zeros(2, device="cuda"))
    dx = torch.zeros_like(x)
    _counted_fwd(L, lib, x, y, cnt, cols, inv_temp, out)                     # eager once: everything is loaded before the capture
    torch.cuda.synchronize()
    gs = torch.cuda.Stream()
    gs.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(gs):
        with torch.cuda.graph(graph, stream=gs):
            _counted_fwd(L, lib, x, y, cnt, cols, inv_temp, out)
            _counted_bwd(L, lib, x, y, cnt, out[1], dloss, out[2], dx, cols, inv_temp)
    torch.cuda.current_stream().wait_stream(gs)
    seen = []
    for count in (2, 9, 5):
        cnt.fill_(count)
        x[count:] = float("nan")                                             # what lies behind THIS count is poison
        graph.replay()
        torch.cuda.synchronize()
        live = torch.tensor([r < count and int(y[r]) != IGNORE for r in range(ROWS)])
        want_loss, want_lse = _plain_fwd(L, lib, x, y, cols, inv_temp)
        _check_fwd(out[0], out[1], out[2], want_loss, want_lse, count, live)
        g = torch.tensor([DLOSS]) / torch.clamp(out[2][1:2].cpu(), min=1.0)
        _check_bwd(dx, _plain_bwd(L, lib, x, y, want_lse, g.expand(ROWS).contiguous().cuda(), cols, inv_temp), live, cols)
        seen.append(float(out[2][1]))
        x[count:] = torch.randn(ROWS - count, ld).to(dtype).cuda()           # finite again for a later, larger count
    assert seen == [1.0, 7.0, 3.0]                                           # rows 0 and 3 are ignored


@pytest.mark.parametrize("n", [1, 70, 1025, 4099])
def test_mask_partition_equals_the_statement(n):
    L, lib = _lib()
    g = torch.Generator().manual_seed(n)
    for mask in (torch.zeros(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool), torch.rand(n, generator=g) < 0.3):
        order, rank, count = (torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                              torch.full((1,), -7, dtype=torch.int32, device="cuda"))
        mask_d = mask.cuda()
        L.check(lib.hero_mask_partition(L.ptr(mask_d), n, L.ptr(order), L.ptr(rank), L.ptr(count), L.stream()))
        wo, wr, m = C.partition_statement(mask.numpy())
        assert torch.equal(order.cpu(), torch.from_numpy(wo)) and torch.equal(rank.cpu(), torch.from_numpy(wr)) and count.tolist() == [m]


@pytest.mark.parametrize("m", [0, 1, 17, 24, 30])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [12, 4352])
def test_nce_pack_equals_the_index_statement(D, dtype, m):
    L, lib = _lib()
    n, cap, n8 = 70, 24, 72
    g = torch.Generator().manual_seed(D + m)
    out, targets = torch.randn(n, D, generator=g), torch.randn(n, D, generator=g)
    count = torch.tensor([m], dtype=torch.int32).cuda()
    out_d, targets_d = out.cuda(), targets.cuda()
    cand = torch.full((n8, D), float("nan"), dtype=dtype, device="cuda")
    masked = torch.full((cap, D), float("nan"), dtype=dtype, device="cuda")
    L.check(lib.hero_nce_pack_fwd(L.ptr(out_d), L.ptr(targets_d), L.ptr(count), L.ptr(cand), L.ptr(masked), n, cap, D, L.dt(cand), L.stream()))
    r = torch.arange(n).unsqueeze(1)
    want = torch.zeros(n8, D, dtype=dtype)
    want[:n] = torch.where(r < m, targets, out).to(dtype)
    assert torch.equal(_bits(cand.cpu()), _bits(want))                       # the padding rows are zero
    assert torch.equal(_bits(masked.cpu()), _bits(out[:cap].to(dtype)))
    assert torch.equal(targets_d.cpu(), targets) and torch.equal(out_d.cpu(), out)              # inputs untouched
    d_cand, d_masked = torch.randn(n8, D, generator=g).to(dtype), torch.randn(cap, D, generator=g).to(dtype)
    d_out = torch.full((n, D), float("nan"), device="cuda")
    dc_d, dm_d = d_cand.cuda(), d_masked.cuda()                               # both alive across the launch
    L.check(lib.hero_nce_pack_bwd(L.ptr(dc_d), L.ptr(dm_d), L.ptr(count), L.ptr(d_out), n, cap, D, L.dt(cand), L.stream()))
    dm = torch.zeros(n, D)
    dm[:cap] = d_masked.float()
    want = dm + torch.where(r >= m, d_cand[:n].float(), torch.zeros(()))
    assert torch.equal(d_out.cpu(), want)
