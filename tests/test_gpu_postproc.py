"""hero_amd.retrieval.postprocess and RecallMeter on the GPU: the fixture cases and a search at the TVR-val shape against
`postprocess_host` and the host metrics (exactly: everything downstream of the search's lists is integer-valued or exact in
fp32), the N > 1024 route, and one graph capture of postprocess + RecallMeter.update - a call that waited for the device
would fail the capture."""
import numpy as np
import pytest
import torch

import hero_amd
from hero_amd import retrieval as HR
from tests import postproc_reference as PR
from tests.test_gpu_retrieval import FixedQueries, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = PR.load_cases()


def same_post(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = a[k].cpu(), b[k].cpu()
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y), k     # bit for bit


def ground_truth(out, seed):
    """gt_ts near a candidate of the SVMR list (rank drawn low), gt video as searched; description types"""
    g = torch.Generator().manual_seed(seed)
    st, ed = out["svmr_st"].cpu(), out["svmr_ed"].cpu()
    nq, n = st.shape
    rank = torch.randint(0, min(n, 40), (nq,), generator=g)
    rows = torch.arange(nq)
    s, e = st[rows, rank].clamp(min=0).float() * 1.5, (ed[rows, rank].clamp(min=0) + 1).float() * 1.5
    ts = torch.stack([s + torch.rand(nq, generator=g) - 0.5, e + torch.rand(nq, generator=g) + 0.25], dim=1).clamp(min=0)
    return ts.to(DEV), torch.randint(0, 3, (nq,), generator=g).to(DEV)


@pytest.mark.parametrize("name", PR.CASES)
def test_fixture_cases_on_the_device(name):
    case = CASES[name]
    cfg = case["cfg"]
    kw = dict(vfeat_interval=cfg["vfeat_interval"], nms_thd=cfg["nms_thd"], max_after_nms=cfg["max_after_nms"])
    out = {k: v.to(DEV) for k, v in case["out"].items()}
    post = HR.postprocess(out, **kw)
    assert all(v.is_cuda for v in post.values())
    same_post(post, HR.postprocess_host(case["out"], **kw))
    ref = case["ref"]
    for task in ("vcmr", "svmr"):
        assert np.array_equal(post[task + "_nms_count"].cpu().numpy(), ref[task + "_count"])
        assert np.array_equal(post[task + "_nms_st_sec"].cpu().numpy().view(np.int32), ref[task + "_st_sec"].view(np.int32))
        assert np.array_equal(post[task + "_nms_ed_sec"].cpu().numpy().view(np.int32), ref[task + "_ed_sec"].view(np.int32))
    meter = hero_amd.RecallMeter(vfeat_interval=cfg["vfeat_interval"])
    gt, ts, ty = (torch.from_numpy(case[k]).to(DEV) for k in ("gt_vidx", "gt_ts", "desc_type"))
    lo = len(gt) // 3
    meter.update({k: v[:lo] for k, v in post.items()}, gt[:lo], ts[:lo], ty[:lo])          # two uneven chunks; row slices keep the row stride
    meter.update({k: v[lo:] for k, v in post.items()}, gt[lo:], ts[lo:], ty[lo:])
    assert meter.compute() == case["metrics"]


def test_tvr_shape_end_to_end():
    model, index, mod_q, gt = synthetic(80, 2179, 100, 768, seed=31, dtype=torch.float32)
    ids = torch.zeros(80, 4, dtype=torch.long, device=DEV)
    with FixedQueries(model, mod_q):
        out = index.search(model, ids, None, torch.ones_like(ids), gt_vidx=gt)
    assert out["vcmr_st"].shape == (80, 200)
    post = hero_amd.postprocess(out)
    host = hero_amd.postprocess_host({k: v.cpu() for k, v in out.items()})
    same_post(post, host)
    again = hero_amd.postprocess(out)
    same_post(post, again)
    n_sv, n_vc = post["svmr_nms_count"].cpu(), post["vcmr_nms_count"].cpu()
    print("\n[postproc] survivors of 200: svmr mean %.1f min %d max %d, vcmr mean %.1f min %d max %d" % (
        n_sv.float().mean(), n_sv.min(), n_sv.max(), n_vc.float().mean(), n_vc.min(), n_vc.max()), end="")
    assert int(n_sv.min()) >= 1 and int(n_sv.float().mean()) < 200, "the NMS must suppress something at this shape"
    ts, ty = ground_truth(out, 3)
    # the ground-truth video of half the queries: the best video of the search, so that VCMR and VR recall are not all zero
    gt2 = torch.where(torch.arange(80, device=DEV) % 2 == 0, out["vr_indices"][:, 0].long(), gt.long())
    meter = hero_amd.RecallMeter()
    meter.update(post, gt2, ts, ty)
    want = PR.meter_from_lists(hero_amd.RecallMeter(), host, gt2.cpu().numpy(), ts.cpu().numpy(), ty.cpu().numpy()).compute()
    got = meter.compute()
    assert got == want
    assert set(got) == {"VCMR", "SVMR", "VR", "VCMR_by_type", "SVMR_by_type", "VR_by_type"}
    assert got["VR"]["r1"] >= 50 and got["SVMR"]["0.5-r100"] > 0
    raw = hero_amd.RecallMeter()                                  # the search's own dictionary, no NMS keys
    raw.update(out, gt2, ts)
    assert raw.compute() == PR.meter_from_lists(hero_amd.RecallMeter(), {k: v.cpu() for k, v in out.items()}, gt2.cpu().numpy(), ts.cpu().numpy(),
                                                None).compute()


def test_more_than_1024_candidates_take_postprocess_host(monkeypatch):
    model, index, mod_q, gt = synthetic(3, 9, 20, 64, seed=5, dtype=torch.float32)
    calls = []
    real = HR.postprocess_host
    monkeypatch.setattr(HR, "postprocess_host", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ids = torch.zeros(3, 4, dtype=torch.long, device=DEV)
    with FixedQueries(model, mod_q):
        inside = index.search(model, ids, None, torch.ones_like(ids), gt_vidx=gt, max_vcmr_video=4, max_before_nms=1024)
        outside = index.search(model, ids, None, torch.ones_like(ids), gt_vidx=gt, max_vcmr_video=4, max_before_nms=1100)
    p_in = HR.postprocess(inside, max_after_nms=150)
    assert not calls
    p_out = HR.postprocess(outside, max_after_nms=150)
    assert calls == [1]
    assert set(p_in) == set(p_out) and all(v.is_cuda for v in p_out.values()) and p_out["vcmr_nms_st"].shape == (3, 150)
    same_post(p_in, real(inside, max_after_nms=150))
    same_post(p_out, real({k: v.cpu() for k, v in outside.items()}, max_after_nms=150))


def test_postprocess_and_update_capture_into_one_graph():
    model, index, mod_q, gt = synthetic(6, 40, 30, 64, seed=9, dtype=torch.float32)
    ids = torch.zeros(6, 4, dtype=torch.long, device=DEV)
    batches = []
    for seed in (0, 1):
        q = torch.randn(6, 64, generator=torch.Generator().manual_seed(seed)).to(DEV)
        with FixedQueries(model, q):
            out = index.search(model, ids, None, torch.ones_like(ids), gt_vidx=gt, max_vcmr_video=10, max_before_nms=120)
        ts, ty = ground_truth(out, seed)
        batches.append((out, out["vr_indices"][:, seed].contiguous(), ts, ty))
    assert not torch.equal(batches[0][0]["vcmr_st"], batches[1][0]["vcmr_st"])
    static = tuple({k: v.clone() for k, v in x.items()} if isinstance(x, dict) else x.clone() for x in batches[0])
    meter = hero_amd.RecallMeter(device=DEV)
    kw = dict(nms_thd=0.5, max_after_nms=100)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # warm-up outside the capture (library load, allocator)
        meter.update(HR.postprocess(static[0], **kw), *static[1:])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    meter.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        post = HR.postprocess(static[0], **kw)
        meter.update(post, *static[1:])
    for dst, src in zip(static, batches[1]):                      # the second batch into the static buffers, then one replay
        if isinstance(dst, dict):
            for k in dst:
                dst[k].copy_(src[k])
        else:
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    eager_post = HR.postprocess(batches[1][0], **kw)
    same_post(post, eager_post)
    eager = hero_amd.RecallMeter()
    eager.update(eager_post, *batches[1][1:])
    got = meter.compute()
    assert got == eager.compute() and got["VR"]["r5"] == 100.0
