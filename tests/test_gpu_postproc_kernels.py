"""hero_moment_nms and hero_first_hit through the C ABI against the host restatements (hero_amd.retrieval.nms_rows_host: the
reference's NMS in Python; tests/postproc_reference.first_hit: eval_by_task_type's fp32 arithmetic in numpy).  Everything is
integer-valued, so every comparison is exact - no tolerance exists in this file.  The NMS kernel divides frame counts in
float64 where the host divides seconds (frames * 1.5) in Python floats: the same rational, correctly rounded, exact ties
included (thresholds 0.5 and 0.6 meet many on integer moments); hero_first_hit does the fp32 operations of numpy one by one
(the build keeps fp32 division correctly rounded and contracts nothing), so its ranks are numpy's at ties as well."""
import numpy as np
import pytest
import torch

from hero_amd import retrieval as HR
from tests import postproc_reference as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = PR.load_cases()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nms_both(video, st, ed, thd, cap, max_after):
    keep, count = HR.k_moment_nms(dev(video), dev(st), dev(ed), thd, cap, max_after)
    again = HR.k_moment_nms(dev(video), dev(st), dev(ed), thd, cap, max_after)
    assert torch.equal(keep, again[0]) and torch.equal(count, again[1])                       # two runs, bit-identical
    assert keep.dtype == count.dtype == torch.int32 and tuple(keep.shape) == (len(st), max_after)
    want_keep, want_count = HR.nms_rows_host(video, st, ed, thd, cap, max_after)
    got_keep, got_count = keep.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(got_count, want_count), (got_count, want_count)
    assert np.array_equal(got_keep, want_keep)
    return got_keep, got_count


def rows(rng, n, length=100):
    """seven rows: three with a few videos and clustered moments, all vacant, one video, every candidate its own video, a vacant tail"""
    nq = 7
    centre = rng.integers(0, length, size=(nq, 8))
    video = rng.integers(0, 8, size=(nq, n))
    st = np.clip(np.take_along_axis(centre, video, 1) + rng.integers(-4, 5, size=(nq, n)), 0, length - 3)
    ed = np.minimum(st + rng.integers(0, 12, size=(nq, n)), length - 1)
    video[4] = 5
    video[5] = rng.permutation(max(n, 3000))[:n]
    for r, cut in ((3, 0), (6, n - n // 3)):
        video[r, cut:], st[r, cut:], ed[r, cut:] = -1, -1, -1
    return video.astype(np.int32), st.astype(np.int32), ed.astype(np.int32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 1024])
def test_nms_grid(n):
    rng = np.random.default_rng(1000 + n)
    video, st, ed = rows(rng, n)
    seen_cut = seen_suppressed = False
    for max_after in sorted({1, min(100, n), n}):
        for thd in (0.0, 0.5, 0.6, 1.0):
            keep, count = nms_both(video, st, ed, thd, 100, max_after)
            assert count[3] == 0 and (keep[3] == -1).all()                                   # all vacant
            assert (count[5] == min(max_after, n))                                            # separate videos: nothing falls
            seen_cut |= bool((count == max_after).any())
            seen_suppressed |= bool(count[4] < min(max_after, n, 100))
    assert seen_cut and (seen_suppressed or n == 1)
    if n == 1024:                                                                             # the per-video limit in a one-video row
        keep, count = nms_both(video[4:5], st[4:5], ed[4:5], 1.0, 7, n)
        assert count[0] == 7 and keep[0, :7].tolist() == list(range(7))
        keep, count = nms_both(video[:3], st[:3], ed[:3], 1.0, 100, n)                        # 8 videos x at most 100
        assert (count <= 800).all() and (count > 100).all()


@pytest.mark.parametrize("name", [c for c in PR.CASES if c != "f"])           # case f runs no NMS: it is covered through postprocess
def test_nms_fixture(name):
    case = CASES[name]
    cfg, out, ref = case["cfg"], case["out"], case["ref"]
    for task in ("vcmr", "svmr"):
        st, ed = out[task + "_st"].numpy(), out[task + "_ed"].numpy()
        video = out["vcmr_video"].numpy() if task == "vcmr" else np.clip(st, -1, 0)
        ma = min(cfg["max_after_nms"], st.shape[1])
        keep, count = nms_both(video, st, ed, cfg["nms_thd"], 100, ma)
        assert np.array_equal(count, ref[task + "_count"]) and np.array_equal(keep, ref[task + "_keep"][:, :ma])


def test_nms_refuses_what_is_outside_the_envelope():
    z = torch.zeros((2, 1025), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="hero_moment_nms"):
        HR.k_moment_nms(z, z, z, 0.5, 100, 100)
    z = torch.zeros((2, 8), dtype=torch.int32, device=DEV)
    for bad in (0, 9):
        with pytest.raises(RuntimeError, match="hero_moment_nms"):
            HR.k_moment_nms(z, z, z, 0.5, 100, bad)
    with pytest.raises(ValueError):
        HR.k_moment_nms(z.long(), z, z, 0.5)
    with pytest.raises(ValueError):
        HR.k_moment_nms(z[:, ::2], z[:, ::2], z[:, ::2], 0.5)


def first_both(video, st, ed, gt_video, gt_ts, interval, thds, n_pred, ld_extra=0):
    def wide(a):
        if a is None:
            return None
        big = torch.full((a.shape[0], a.shape[1] + ld_extra), -7, dtype=torch.int32, device=DEV)
        big[:, :a.shape[1]] = dev(a)
        return big[:, :a.shape[1]]
    t = torch.tensor(thds, dtype=torch.float32, device=DEV) if len(thds) else None
    got = HR.k_first_hit(wide(video), dev(gt_video), wide(st), wide(ed), None if gt_ts is None else dev(gt_ts), interval, t, n_pred)
    want = PR.first_hit(video, st, ed, gt_video, gt_ts, interval, thds, n_pred)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    return want


@pytest.mark.parametrize("p,n_pred,ld_extra", [(1, 1, 0), (63, 63, 0), (64, 100, 3), (65, 40, 0), (200, 100, 56), (1024, 1024, 0)])
def test_first_hit_grid(p, n_pred, ld_extra):
    rng = np.random.default_rng(p)
    nq = 9                                                        # not a multiple of the 4 queries of a workgroup
    video = rng.integers(0, 6, size=(nq, p)).astype(np.int32)
    st = rng.integers(0, 90, size=(nq, p)).astype(np.int32)
    ed = (st + rng.integers(0, 10, size=(nq, p))).astype(np.int32)
    video[2, p // 2:], st[2, p // 2:], ed[2, p // 2:] = -1, -1, -1
    video[3] = 4                                                  # never the ground-truth video
    gt_video = np.array([0, 1, 2, 3, 5, 0, 1, 2, 3], dtype=np.int32)
    g0 = rng.integers(0, 80, size=nq) * 1.5                       # ground truth on the frame grid: IoUs of 1/2 and the like occur
    gt_ts = np.stack([g0, g0 + rng.integers(1, 12, size=nq) * 1.5], axis=1).astype(np.float32)
    for interval in (1.5, 2.0):
        for thds in ((0.5, 0.7), (0.5,), (0.1, 0.25, 0.3, 0.5, 0.6, 0.7, 0.9, 1.0)):
            first = first_both(video, st, ed, gt_video, gt_ts, interval, thds, n_pred, ld_extra)
            assert (first[3] == min(p, n_pred)).all()
    first = first_both(video, None, None, gt_video, None, 1.5, (), n_pred, ld_extra)            # VR: T = 0, no st / ed
    assert first.shape == (nq, 1)
    first_both(video, st, ed, gt_video, gt_ts, 1.5, (), n_pred, ld_extra)                       # T = 0 with st / ed: vacancy through st


@pytest.mark.parametrize("name", PR.CASES)
def test_first_hit_fixture(name):
    case = CASES[name]
    cfg = case["cfg"]
    post = HR.postprocess_host(case["out"], vfeat_interval=cfg["vfeat_interval"], nms_thd=cfg["nms_thd"], max_after_nms=cfg["max_after_nms"])
    gt = case["gt_vidx"]
    for task in ("vcmr", "svmr"):
        st, ed = post[task + "_nms_st"].numpy(), post[task + "_nms_ed"].numpy()
        video = post["vcmr_nms_video"].numpy() if task == "vcmr" else np.where(st >= 0, gt.reshape(-1, 1), -1).astype(np.int32)
        first_both(video, st, ed, gt, case["gt_ts"], cfg["vfeat_interval"], (0.5, 0.7), 100)
    first_both(case["out"]["vr_indices"].numpy(), None, None, gt, None, 1.5, (), 100)


def test_first_hit_refuses_what_is_outside_the_envelope():
    z = torch.zeros((2, 8), dtype=torch.int32, device=DEV)
    g = torch.zeros((2,), dtype=torch.int32, device=DEV)
    ts = torch.zeros((2, 2), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="hero_first_hit"):
        HR.k_first_hit(z, g, z, z, ts, 1.5, torch.zeros(9, device=DEV))
    with pytest.raises(RuntimeError, match="hero_first_hit"):
        HR.k_first_hit(z, g, n_pred=0)
    with pytest.raises(ValueError):
        HR.k_first_hit(z, g, z, None)
    with pytest.raises(ValueError):
        HR.k_first_hit(z, g, thds=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError):
        HR.k_first_hit(z.long(), g)
