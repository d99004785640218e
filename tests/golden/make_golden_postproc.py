#!/usr/bin/env python3
"""Golden vectors of what follows a full-corpus search - temporal NMS, truncation, recall - by running the *reference's*
post_processing_vcmr_nms, post_processing_svmr_nms, get_submission_top_n (utils/tvr_eval_utils.py) and eval_retrieval
(utils/tvr_standalone_eval.py) on synthetic candidate lists.

Container-only (needs the reference checkout), like make_golden_retrieval.py.  Writes tests/golden/case_postproc.npz; per case
<c> in a, b, c, d1, d2, e, f, g:

  <c>.vr_indices, vcmr_scores / video / st / ed, svmr_scores / st / ed    inputs in the result-dictionary layout of hero_amd.retrieval
  <c>.gt_vidx, gt_ts (fp32 seconds), desc_type (0 / 1 / 2 = v / t / vt)
  <c>.cfg      JSON: vfeat_interval, nms_thd, max_after_nms
  <c>.ref_vcmr_keep / ref_svmr_keep    [Nq, max_after_nms] positions in the input row of the reference's predictions after NMS and
               truncation (recovered through the row's unique scores), -1 beyond; ref_*_count; ref_*_st_sec / ref_*_ed_sec (fp32)
  <c>.metrics  JSON of eval_retrieval's dictionary (use_desc_type=True)

The lists are handed to the reference as eval_vcmr.py builds them (:339-414): VCMR seconds from float32 products, SVMR seconds
from float64 ones, [video, start, end, score] per prediction; vacant slots are simply absent.

The cases: (a) TVR-like - 80 queries x 200 candidates over 100 videos per query with a skewed video distribution and
clustered moments; (b) one video, 400 short moments on 256 frames, max_after_nms 150: the inner per-video limit of 100 decides;
(c) vacant slots at the end of the rows; (d1, d2) pairs whose IoU is exactly the threshold (3/5 at 0.6, 1/2 at 0.5); (e) one
candidate; (f) nms_thd -1; (g) vfeat_interval 2.  What the inputs must satisfy is asserted in `run_case` and `main`.

Run:  python tests/golden/make_golden_postproc.py
"""
import copy
import json
import os
import sys
import types

import numpy as np

np.bool = bool                # the reference's metric code predates numpy 1.24

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("HERO_REFERENCE", "/root/reference")
TYPES = ("v", "t", "vt")
IOU_THDS = (0.5, 0.7)


def reference_functions():
    try:
        import tqdm  # noqa: F401
    except ImportError:
        stub = types.ModuleType("tqdm")
        stub.tqdm = lambda it, **kw: it
        sys.modules["tqdm"] = stub
    sys.path.insert(0, os.path.join(REF, "utils"))             # the two files import nothing of their package
    import tvr_eval_utils as E                                   # noqa: reference import
    import tvr_standalone_eval as S                              # noqa: reference import
    return E.post_processing_vcmr_nms, E.post_processing_svmr_nms, E.get_submission_top_n, S.eval_retrieval


def decreasing_scores(rng, nq, n):
    s = np.sort(rng.uniform(0.0, 1.0, size=(nq, n)).astype(np.float32), axis=1)[:, ::-1].copy()
    assert (np.diff(s.astype(np.float64), axis=1) < 0).all(), "every row's scores must be strictly decreasing"
    return s


def clustered_moments(rng, shape, centers, length, spread=3, min_l=2, max_l=16):
    """start near the given centre, end = start + [min_l, max_l) inside the clip: the band of the search"""
    st = np.clip(centers + rng.integers(-spread, spread + 1, size=shape), 0, length - 1 - min_l)
    ed = np.minimum(st + rng.integers(min_l, max_l, size=shape), length - 1)
    return st.astype(np.int32), ed.astype(np.int32)


def ground_truth_near(rng, st, ed, interval, rank):
    """gt_ts [Nq, 2] fp32: the candidate of the given rank, moved by up to 1.5 s at each end"""
    q = np.arange(len(rank))
    g0 = st[q, rank] * interval + rng.uniform(-1.5, 1.5, size=len(rank))
    g1 = (ed[q, rank] + 1) * interval + rng.uniform(-1.5, 1.5, size=len(rank))
    g0 = np.maximum(g0, 0.0)
    return np.stack([g0, np.maximum(g1, g0 + 0.5)], axis=1).astype(np.float32)


def tvr_like(rng, nq=80, n=200, k=100, nv=2179, length=100, interval=1.5, vacant=0):
    d = {}
    vr = np.stack([rng.permutation(nv)[:k] for _ in range(nq)]).astype(np.int32)
    p = 1.0 / np.arange(1, k + 1) ** 0.8
    slot = rng.choice(k, size=(nq, n), p=p / p.sum())                                        # a few videos dominate
    centre = rng.integers(0, length, size=(nq, k))
    st, ed = clustered_moments(rng, (nq, n), np.take_along_axis(centre, slot, 1), length, spread=12)
    d["vr_indices"] = vr
    d["vr_scores"] = decreasing_scores(rng, nq, k)
    d["vcmr_scores"], d["vcmr_video"], d["vcmr_st"], d["vcmr_ed"] = decreasing_scores(rng, nq, n), np.take_along_axis(vr, slot, 1), st, ed
    rank = np.minimum(rng.geometric(0.08, size=nq) - 1, n - 1 - vacant)
    gt = d["vcmr_video"][np.arange(nq), rank].astype(np.int32)
    away = rng.uniform(size=nq) < 0.25                                                        # ground-truth video not retrieved at all
    gt[away] = nv + 7
    # SVMR: every candidate in the ground-truth video, three clusters
    c3 = rng.integers(0, length, size=(nq, 3))
    sst, sed = clustered_moments(rng, (nq, n), np.take_along_axis(c3, rng.integers(0, 3, size=(nq, n)), 1), length, spread=8)
    d["svmr_scores"], d["svmr_st"], d["svmr_ed"] = decreasing_scores(rng, nq, n), sst, sed
    srank = np.minimum(rng.geometric(0.05, size=nq) - 1, n - 1 - vacant)
    ts = ground_truth_near(rng, st, ed, interval, rank)
    ts_sv = ground_truth_near(rng, sst, sed, interval, srank)
    use_sv = rng.uniform(size=nq) < 0.5                    # one ground truth per query serves both tasks: half follow either list
    d["gt_ts"] = np.where(use_sv[:, None], ts_sv, ts).astype(np.float32)
    d["gt_vidx"] = gt
    d["desc_type"] = (rng.permutation(nq) % 3).astype(np.int32)                               # every type occurs
    if vacant:
        for q in range(nq):
            cut = n - int(rng.integers(0, vacant + 1))
            for key, fill in (("vcmr_scores", 0), ("vcmr_video", -1), ("vcmr_st", -1), ("vcmr_ed", -1)):
                d[key][q, cut:] = fill
            cut = n - int(rng.integers(0, vacant + 1))
            for key, fill in (("svmr_scores", 0), ("svmr_st", -1), ("svmr_ed", -1)):
                d[key][q, cut:] = fill
    return d


def one_video(rng, nq=6, n=400, length=256, interval=1.5):
    d = {}
    st = rng.integers(0, length - 3, size=(nq, n)).astype(np.int32)
    ed = (st + rng.integers(0, 3, size=(nq, n))).astype(np.int32)                             # short, well separated moments
    vid = np.full((nq, n), 11, dtype=np.int32)
    d["vr_indices"] = np.tile(np.array([[11, 3, 5]], dtype=np.int32), (nq, 1))
    d["vr_scores"] = decreasing_scores(rng, nq, 3)
    d["vcmr_scores"], d["vcmr_video"], d["vcmr_st"], d["vcmr_ed"] = decreasing_scores(rng, nq, n), vid, st, ed
    d["svmr_scores"], d["svmr_st"], d["svmr_ed"] = decreasing_scores(rng, nq, n), st.copy(), ed.copy()
    d["gt_vidx"] = np.full((nq,), 11, dtype=np.int32)
    d["gt_ts"] = ground_truth_near(rng, st, ed, interval, rng.integers(0, 150, size=nq))
    d["desc_type"] = (np.arange(nq) % 3).astype(np.int32)
    return d


def exact_ties(rng, pair, nq=6, n=16, length=12, interval=1.5):
    """rows of short integer moments in two videos; the first two candidates of every row are `pair`, whose IoU is the threshold"""
    d = {}
    st = rng.integers(0, length - 2, size=(nq, n)).astype(np.int32)
    ed = np.minimum(st + rng.integers(0, 6, size=(nq, n)), length - 1).astype(np.int32)
    vid = rng.integers(0, 2, size=(nq, n)).astype(np.int32)
    (st[:, 0], ed[:, 0]), (st[:, 1], ed[:, 1]) = pair
    vid[:, :2] = 0
    d["vr_indices"] = np.tile(np.array([[0, 1]], dtype=np.int32), (nq, 1))
    d["vr_scores"] = decreasing_scores(rng, nq, 2)
    d["vcmr_scores"], d["vcmr_video"], d["vcmr_st"], d["vcmr_ed"] = decreasing_scores(rng, nq, n), vid, st, ed
    d["svmr_scores"], d["svmr_st"], d["svmr_ed"] = decreasing_scores(rng, nq, n), st.copy(), ed.copy()
    d["gt_vidx"] = np.zeros((nq,), dtype=np.int32)
    d["gt_ts"] = ground_truth_near(rng, st, ed, interval, rng.integers(0, n, size=nq))
    d["desc_type"] = (np.arange(nq) % 3).astype(np.int32)
    return d


def lists_of(d, task, interval):
    """eval_vcmr.py:339-354 (SVMR, float64 products) and :396-414 (VCMR, float32 products); vacant slots are absent"""
    res = []
    for q in range(len(d["gt_vidx"])):
        st, ed, sc = d[task + "_st"][q], d[task + "_ed"][q], d[task + "_scores"][q]
        real = st >= 0
        if task == "vcmr":
            s0 = st.astype(np.float32) * interval
            s1 = ed.astype(np.float32) * interval + interval
            vid = d["vcmr_video"][q]
        else:
            s0 = st.astype(np.float64) * interval
            s1 = (ed.astype(np.float64) + 1) * interval
            vid = np.full_like(st, d["gt_vidx"][q])
        preds = [[int(vid[i]), float(s0[i]), float(s1[i]), float(sc[i])] for i in range(len(st)) if real[i]]
        res.append(dict(desc_id=q, desc="", predictions=preds))
    return res


def run_case(name, d, fns, interval=1.5, nms_thd=0.5, max_after=100):
    nms_vcmr, nms_svmr, top_n, eval_retrieval = fns
    nq, n = d["vcmr_st"].shape
    for task in ("vcmr", "svmr"):
        live = d[task + "_st"] >= 0
        assert (live[:, 0]).all(), "every query needs a first candidate"
        assert (live[:, :-1] >= live[:, 1:]).all(), "vacant slots are at the end"
        sc = np.where(live, d[task + "_scores"].astype(np.float64), -np.arange(n)[None, :] - 1.0)
        assert (np.diff(sc, axis=1) < 0).all(), "every row's scores must be strictly decreasing"
    res = {"VCMR": lists_of(d, "vcmr", interval), "SVMR": lists_of(d, "svmr", interval)}
    res["VR"] = [dict(desc_id=q, desc="", predictions=[[int(v), 0, 0, float(s)] for v, s in zip(d["vr_indices"][q][:100], d["vr_scores"][q][:100])])
                 for q in range(nq)]
    names = {"vid%d" % v: int(v) for v in set(d["vr_indices"].ravel().tolist()) | set(d["gt_vidx"].tolist()) | set(d["vcmr_video"].ravel().tolist()) if v >= 0}
    if nms_thd != -1:                                                       # eval_vcmr.py:458-478
        res["SVMR"] = nms_svmr(copy.deepcopy(res["SVMR"]), nms_thd=nms_thd, max_before_nms=n, max_after_nms=max_after)
        res["VCMR"] = nms_vcmr(copy.deepcopy(res["VCMR"]), nms_thd=nms_thd, max_before_nms=n, max_after_nms=max_after)
    res["video2idx"] = names
    sub = top_n(res, top_n=max_after)                                       # :420-421, 479-480
    gts = [dict(desc_id=q, desc="", type=TYPES[int(d["desc_type"][q])], vid_name="vid%d" % d["gt_vidx"][q],
                ts=[float(d["gt_ts"][q, 0]), float(d["gt_ts"][q, 1])]) for q in range(nq)]
    metrics = eval_retrieval(sub, gts, iou_thds=IOU_THDS, match_number=True, verbose=False, use_desc_type=True)
    metrics = json.loads(json.dumps(metrics))                               # plain floats
    o = {k: v for k, v in d.items()}
    for task in ("vcmr", "svmr"):
        keep = np.full((nq, max_after), -1, dtype=np.int32)
        s0, s1 = np.zeros((nq, max_after), dtype=np.float32), np.zeros((nq, max_after), dtype=np.float32)
        count = np.zeros((nq,), dtype=np.int32)
        for q, e in enumerate(sub[task.upper()]):
            where = {float(s): i for i, s in enumerate(d[task + "_scores"][q]) if d[task + "_st"][q, i] >= 0}
            assert e["desc_id"] == q and len(e["predictions"]) <= max_after
            for j, (vid, a, b, s) in enumerate(e["predictions"]):
                keep[q, j] = where[s]
                s0[q, j], s1[q, j] = a, b
                assert float(s0[q, j]) == a and float(s1[q, j]) == b, "seconds must be exact in float32"
                if task == "vcmr":
                    assert vid == d["vcmr_video"][q, keep[q, j]]
            count[q] = len(e["predictions"])
            assert (np.diff(keep[q, :count[q]]) > 0).all()
        o["ref_%s_keep" % task], o["ref_%s_count" % task], o["ref_%s_st_sec" % task], o["ref_%s_ed_sec" % task] = keep, count, s0, s1
    # no metric IoU within 1e-5 (relative) of a threshold: in float64 from the float32 inputs, for every prediction in the right video
    for task in ("vcmr", "svmr"):
        st, ed = d[task + "_st"].astype(np.float64), d[task + "_ed"].astype(np.float64)
        p0, p1 = st * interval, (ed + 1) * interval
        g0, g1 = d["gt_ts"][:, :1].astype(np.float64), d["gt_ts"][:, 1:].astype(np.float64)
        hull = np.maximum(p1, g1) - np.minimum(p0, g0)
        iou = np.maximum(0, np.minimum(p1, g1) - np.maximum(p0, g0)) / np.where(hull == 0, 1, hull)
        for thd in IOU_THDS:
            assert (np.abs(iou - thd) > 1e-5 * thd)[d[task + "_st"] >= 0].all(), "a metric IoU is too close to a threshold"
    o["cfg"] = np.array(json.dumps(dict(vfeat_interval=interval, nms_thd=nms_thd, max_after_nms=max_after)))
    o["metrics"] = np.array(json.dumps(metrics))
    print("%-3s Nq %3d N %4d  survivors vcmr %.1f svmr %.1f  VCMR %s" % (name, nq, n, o["ref_vcmr_count"].mean(), o["ref_svmr_count"].mean(), metrics["VCMR"]))
    return o, metrics


def iou_frames(a, b):
    return max(0, min(a[1], b[1]) + 1 - max(a[0], b[0])) / (max(a[1], b[1]) + 1 - min(a[0], b[0]))


def main():
    fns = reference_functions()
    rng = np.random.default_rng(20)
    out = {}

    def keep(name, o):
        for k, v in o.items():
            out["%s.%s" % (name, k)] = v

    a, m = run_case("a", tvr_like(rng), fns)
    n_live = 200 * 80
    assert a["ref_svmr_count"].sum() <= 0.75 * n_live, "NMS must bite in (a)"
    uncut = run_case("a'", {k: v for k, v in a.items() if not k.startswith("ref_") and k not in ("cfg", "metrics")}, fns, max_after=200)[0]
    assert (uncut["ref_vcmr_count"] > 100).any() and (a["ref_vcmr_count"] == 100).any(), "max_after_nms must cut a query of (a)"
    assert uncut["ref_vcmr_count"].sum() + uncut["ref_svmr_count"].sum() <= 0.75 * 2 * n_live, "a quarter of (a) must be suppressed"
    for task in ("VCMR", "SVMR", "VR"):
        groups = {}
        for key, val in m[task].items():
            groups.setdefault(key.rsplit("r", 1)[0], []).append(val)
        assert all(any(0 < x < 100 for x in vals) for vals in groups.values()), ("a recall figure of (a) is trivial", task, m[task])
    keep("a", a)
    b, _ = run_case("b", one_video(rng), fns, max_after=150)
    assert (b["ref_vcmr_count"] == 100).all() and (b["ref_svmr_count"] == 100).all(), "the per-video limit must decide (b)"
    keep("b", b)
    keep("c", run_case("c", tvr_like(rng, nq=12, n=70, k=20, vacant=30), fns)[0])
    for name, pair, thd in (("d1", ((0, 4), (2, 4)), 0.6), ("d2", ((0, 3), (2, 3)), 0.5)):
        assert iou_frames(*pair) == thd
        d, _ = run_case(name, exact_ties(rng, pair), fns, nms_thd=thd)
        assert (d["ref_vcmr_keep"][:, :2] == [0, 1]).all() and (d["ref_svmr_keep"][:, :2] == [0, 1]).all(), "an exact tie must survive"
        keep(name, d)
    keep("e", run_case("e", tvr_like(rng, nq=5, n=1, k=4), fns)[0])
    keep("f", run_case("f", tvr_like(rng, nq=10, n=120, k=30), fns, nms_thd=-1)[0])
    keep("g", run_case("g", tvr_like(rng, nq=10, n=90, k=25, interval=2), fns, interval=2)[0])
    path = os.path.join(HERE, "case_postproc.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
