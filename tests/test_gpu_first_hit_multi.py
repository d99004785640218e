"""hero_first_hit_multi through the C ABI against tests/didemo_reference.first_hit_multi (eval_by_task_type's fp32 arithmetic in
numpy with the reference's several-annotator rule).  Everything is compared with np.array_equal: the kernel does numpy's fp32
operations one by one, so its ranks are numpy's at exact ties too - no tolerance exists in this file."""
import numpy as np
import pytest
import torch

from hero_amd import retrieval as HR
from tests import didemo_reference as DR
from tests import postproc_reference as PR
from tests import uninit

pytestmark = pytest.mark.gpu
DEV = "cuda"
NQ = 9                                                            # not a multiple of the 4 queries of a workgroup
THD_SETS = ((0.5, 0.7), (0.5,), (0.1, 0.25, 0.3, 0.5, 0.6, 0.7, 0.9, 1.0))
GRID = [(1, 1, 0), (63, 63, 0), (64, 100, 3), (65, 40, 0), (130, 100, 56)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def wide(a, ld_extra):
    big = torch.full((a.shape[0], a.shape[1] + ld_extra), -7, dtype=torch.int32, device=DEV)
    big[:, :a.shape[1]] = dev(a)
    return big[:, :a.shape[1]]


def run(video, st, ed, gt_video, gt_ts, gt_n, interval, thds, n_pred, ld_extra=0):
    t = torch.tensor(thds, dtype=torch.float32, device=DEV) if len(thds) else None
    return HR.k_first_hit_multi(wide(video, ld_extra), dev(gt_video), wide(st, ld_extra), wide(ed, ld_extra), dev(gt_ts), dev(gt_n), interval, t,
                                n_pred)


def rows(p, G, interval, seed):
    """Nine rows on a 5 s grid of ground truth (frames of `interval` seconds, so that frame spans and annotators' spans meet in
    exact fractions: iou == thd occurs).  Planted, where the row is long enough: row 2 a vacant tail, row 3 never the
    ground-truth video, row 4 exactly one annotator overlapping (no hit), row 5 the second overlap only at a later prediction,
    row 6 the two thresholds first met at different ranks.  gt_n mixes 1 and >= 4 (G >= 4); rows 4-6 have >= 4 annotators."""
    rng = np.random.default_rng(seed)
    video = rng.integers(0, 3, size=(NQ, p)).astype(np.int32)
    st = rng.integers(0, 24, size=(NQ, p)).astype(np.int32)
    ed = (st + rng.integers(0, 8, size=(NQ, p))).astype(np.int32)
    gt_video = np.array([0, 1, 2, 1, 2, 0, 1, 2, 0], dtype=np.int32)
    if G >= 4:
        gt_n = np.array([1, 4, G, 1, G, 4, G, 4, 1], dtype=np.int32)
    else:
        gt_n = np.ones(NQ, dtype=np.int32)
    g0 = rng.integers(0, 7, size=(NQ, G)) * 5.0
    gt_ts = np.stack([g0, g0 + rng.integers(1, 3, size=(NQ, G)) * 5.0], axis=2).astype(np.float32)
    video[2, p // 2:], st[2, p // 2:], ed[2, p // 2:] = -1, -1, -1
    video[3] = 2
    f = lambda sec: int(round(sec / interval))                      # noqa: E731  (frame index of a time on both grids: 30 s = 20 / 15 frames)
    if G >= 4:
        far = [[90.0, 95.0]] * G
        # row 4: annotator 0 at [30, 60], the others far away; every prediction inside [30, 60]
        gt_ts[4, :] = far
        gt_ts[4, 0] = [30.0, 60.0]
        video[4], st[4], ed[4] = 2, f(30), f(60) - 1
        # row 5: annotators 0 and 1 at [0, 30] and [30, 60]; prediction 0 meets only the first, the last one spans both halves
        gt_ts[5, :] = far[:G]
        gt_ts[5, 0], gt_ts[5, 1] = [0.0, 30.0], [30.0, 60.0]
        video[5], st[5], ed[5] = 0, f(0), f(30) - 1
        st[5, p - 1], ed[5, p - 1] = f(0), f(60) - 1                # IoU 1/2 with each of the two: an exact tie at 0.5
        # row 6: annotators 0 and 1 both [0, 60]; prediction 0 covers 3/5 of it, the last one all of it
        gt_ts[6, :] = far[:G]
        gt_ts[6, 0], gt_ts[6, 1] = [0.0, 60.0], [0.0, 60.0]
        video[6], st[6], ed[6] = 1, f(0), f(36) - 1
        st[6, p - 1], ed[6, p - 1] = f(0), f(60) - 1
    return video, st, ed, gt_video, gt_ts, gt_n


@pytest.mark.parametrize("G", [1, 4, 5, 16])
@pytest.mark.parametrize("p,n_pred,ld_extra", GRID)
def test_first_hit_multi_grid(p, n_pred, ld_extra, G):
    seen_tie = False
    for interval in (1.5, 2.0):
        video, st, ed, gt_video, gt_ts, gt_n = rows(p, G, interval, 100 * p + G)
        P = min(p, n_pred)
        nan_pad, zero_pad = gt_ts.copy(), gt_ts.copy()
        for q in range(NQ):
            nan_pad[q, gt_n[q]:], zero_pad[q, gt_n[q]:] = np.nan, 0.0
        for thds in THD_SETS:
            want = DR.first_hit_multi(video, st, ed, gt_video, gt_ts, gt_n, interval, thds, n_pred)
            got = run(video, st, ed, gt_video, nan_pad, gt_n, interval, thds, n_pred, ld_extra)
            assert got.dtype == torch.int32 and tuple(got.shape) == (NQ, len(thds) + 1)
            assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy(), want)
            again = run(video, st, ed, gt_video, zero_pad, gt_n, interval, thds, n_pred, ld_extra)
            assert torch.equal(got, again)                          # the padding is never read; two runs, bit-identical
            assert (want[3] == P).all()                             # the video never matches
            if G >= 4 and thds == (0.5, 0.7):
                assert (want[4, 1:] == P).all() and want[4, 0] == 0           # one annotator alone is no hit
                if p > 1 and P == p:
                    assert want[5, 1] == p - 1                                # the second overlap arrives with the last prediction (IoU exactly 1/2)
                    assert want[6, 1] == 0 and want[6, 2] == p - 1             # 3/5 reaches 0.5 at once, 0.7 only at the end
                    seen_tie = True
                one = DR.first_hit_multi(video, st, ed, gt_video, gt_ts, gt_n, interval, thds, n_pred, need=1)
                assert not np.array_equal(one, want)                # the rule matters on these rows
        if G == 1:                                                  # the G = 1 path is hero_first_hit
            t = torch.tensor(THD_SETS[0], dtype=torch.float32, device=DEV)
            a = HR.k_first_hit(wide(video, ld_extra), dev(gt_video), wide(st, ld_extra), wide(ed, ld_extra), dev(gt_ts[:, 0]), interval, t, n_pred)
            b = run(video, st, ed, gt_video, gt_ts, gt_n, interval, THD_SETS[0], n_pred, ld_extra)
            assert torch.equal(a, b)
            assert np.array_equal(a.cpu().numpy(), PR.first_hit(video, st, ed, gt_video, gt_ts[:, 0], interval, THD_SETS[0], n_pred))
    assert seen_tie or G < 4 or p == 1 or n_pred < p


def test_first_hit_multi_no_thresholds():
    video, st, ed, gt_video, gt_ts, gt_n = rows(65, 4, 1.5, 7)
    got = HR.k_first_hit_multi(dev(video), dev(gt_video), dev(st), dev(ed), dev(gt_ts), dev(gt_n), 1.5, None, 65)
    assert np.array_equal(got.cpu().numpy(), DR.first_hit_multi(video, st, ed, gt_video, gt_ts, gt_n, 1.5, (), 65))
    got = HR.k_first_hit_multi(dev(video), dev(gt_video), None, None, None, None, 1.5, None, 65)        # VR: no st / ed, no ground-truth times
    assert np.array_equal(got.cpu().numpy(), PR.first_hit(video, None, None, gt_video, None, 1.5, (), 65))


def test_first_hit_multi_replays_in_a_graph():
    video, st, ed, gt_video, gt_ts, gt_n = rows(130, 5, 1.5, 11)
    args = (dev(video), dev(gt_video), dev(st), dev(ed), dev(gt_ts), dev(gt_n), 1.5, torch.tensor((0.5, 0.7), device=DEV), 100)
    eager = HR.k_first_hit_multi(*args).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        HR.k_first_hit_multi(*args)                                 # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = HR.k_first_hit_multi(*args)
    results = []
    for _ in range(2):
        out.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        results.append(out.clone())
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], eager)


def test_first_hit_multi_refuses_what_is_outside_the_envelope():
    z = torch.zeros((2, 8), dtype=torch.int32, device=DEV)
    g = torch.zeros((2,), dtype=torch.int32, device=DEV)
    n = torch.ones((2,), dtype=torch.int32, device=DEV)
    thd = torch.full((2,), 0.5, device=DEV)

    def ts(G):
        return torch.zeros((2, G, 2), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="hero_first_hit_multi"):
        HR.k_first_hit_multi(z, g, z, z, ts(17), n, 1.5, thd)                       # G > 16
    with pytest.raises(RuntimeError, match="hero_first_hit_multi"):
        HR.k_first_hit_multi(z, g, z, z, ts(0), n, 1.5, thd)                        # G < 1
    with pytest.raises(RuntimeError, match="hero_first_hit_multi"):
        HR.k_first_hit_multi(z, g, z, z, ts(4), n, 1.5, torch.zeros(9, device=DEV))  # T > 8
    with pytest.raises(RuntimeError, match="hero_first_hit_multi"):
        HR.k_first_hit_multi(z, g, z, z, ts(4), n, 1.5, thd, n_pred=0)              # P < 1
    from hero_amd import _lib as L
    first = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    call = L.lib().hero_first_hit_multi
    ok = (L.ptr(z), L.ptr(z), L.ptr(z), 2, 8, 8, L.ptr(g), L.ptr(ts(4)), L.ptr(n), 4, 1.5, L.ptr(thd), 2, L.ptr(first), L.stream())
    for at, bad in ((0, None), (6, None), (13, None),               # null video / gt_video / first
                    (5, 7),                                         # ld < P
                    (1, None), (7, None), (8, None), (11, None)):   # T > 0 without st / gt_ts / gt_n / thds
        a = list(ok)
        a[at] = bad
        with pytest.raises(RuntimeError, match="hero_first_hit_multi"):
            L.check(call(*a))
    with pytest.raises(ValueError):
        HR.k_first_hit_multi(z, g, z, None, ts(4), n)
    with pytest.raises(ValueError):
        HR.k_first_hit_multi(z, g, z, z, ts(4)[:, :, :1], n, 1.5, thd)
    with pytest.raises(ValueError):
        HR.k_first_hit_multi(z, g, z, z, ts(4), n.long(), 1.5, thd)
    with pytest.raises(ValueError):
        HR.k_first_hit_multi(z, g, z, z, None, None, 1.5, thd)
    with pytest.raises(ValueError):
        HR.k_first_hit_multi(z.long(), g, z, z, ts(4), n, 1.5, thd)


def test_first_hit_multi_does_not_read_its_output():
    """Through tests/uninit.py (float scratch under 0 and NaN; there is none), and with `first` itself pre-filled two ways."""
    video, st, ed, gt_video, gt_ts, gt_n = rows(65, 5, 1.5, 13)

    def build():
        return (dev(video), dev(gt_video), dev(st), dev(ed), dev(gt_ts), dev(gt_n), 1.5, torch.tensor((0.5, 0.7), device=DEV), 65)

    res = uninit.assert_fill_independent(build, lambda a: {"first": HR.k_first_hit_multi(*a)})
    want = DR.first_hit_multi(video, st, ed, gt_video, gt_ts, gt_n, 1.5, (0.5, 0.7), 65)
    assert np.array_equal(res["first"].cpu().numpy(), want)
    empty = torch.empty
    got = []
    for fill in (0, 0x7f7f7f7f):
        def alloc(*a, _fill=fill, **kw):
            return empty(*a, **kw).fill_(_fill)
        try:
            torch.empty = alloc
            got.append(HR.k_first_hit_multi(*build()))
        finally:
            torch.empty = empty
    assert torch.equal(got[0], got[1]) and np.array_equal(got[0].cpu().numpy(), want)


@pytest.mark.parametrize("name", DR.DIDEMO_CASES)
def test_recall_meter_on_didemo_fixture(name):
    """Every didemo.* case of case_vr.npz through RecallMeter.update reproduces the reference's eval_retrieval dictionaries."""
    case = DR.didemo_cases(DR.load_vr())[name]
    gt_ts, gt_n = HR.pack_gt_ts(case["ts_list"])
    assert np.array_equal(gt_ts.numpy(), case["gt_ts"]) and np.array_equal(gt_n.numpy(), case["gt_n"])
    meter = HR.RecallMeter(vfeat_interval=case["interval"])
    d = {"vcmr_video": dev(case["vcmr"][0]), "vcmr_st": dev(case["vcmr"][1]), "vcmr_ed": dev(case["vcmr"][2]),
         "svmr_st": dev(case["svmr"][1]), "svmr_ed": dev(case["svmr"][2])}
    meter.update(d, dev(case["gt_vidx"]), gt_ts.to(DEV), gt_n=gt_n.to(DEV))
    got = meter.compute()
    assert got["VCMR"] == case["metrics"]["VCMR"] and got["SVMR"] == case["metrics"]["SVMR"], (got, case["metrics"])
