"""The device collate of hero_amd/csrc/collate.hip through the raw ctypes ABI - hero_collate_subs, hero_collate_clip_mask,
hero_collate_frame_map (count pass, host exclusive scan, fill pass), hero_collate_gather_feats, hero_derive_multi - against the
host statements of tests/rows_reference.py, which tests/test_cpu_rows_reference.py holds against hero_amd.collate.video_collate,
hero_amd.model.model.build_frame_map and the torch expressions hero_derive_multi replaces.  Everything here is an index, a 0/1
mask or a moved value: all comparisons are exact.  Outputs are pre-filled with a sentinel / NaN between guard elements
(tests/test_gpu_rows_kernels.Buf); what a contract does not write keeps its bits."""
import numpy as np
import pytest
import torch

from tests import rows_reference as R
from tests.test_gpu_rows_kernels import ISENT, Buf, dev, same_bits, sync

pytestmark = pytest.mark.gpu

MAX_VL, MAX_SL = 5, 9                        # of rows_reference.collate_lists()


@pytest.fixture(scope="module")
def Lb():
    from hero_amd import _lib
    _lib.lib()
    return _lib


def dlen(ln):
    return {k: dev(v) for k, v in ln.items()}


# ---- hero_collate_subs ---------------------------------------------------------------------------------------------------------
def run_subs(Lb, nfrm, ntok, max_vl, out_size):
    T = len(nfrm)
    gidx, mask = Buf((T, out_size), torch.int64), Buf((T, out_size), torch.int64)
    a, b = dev(np.int32(nfrm)), dev(np.int32(ntok))
    Lb.check(Lb.lib().hero_collate_subs(a.data_ptr(), b.data_ptr(), gidx.ptr(), mask.ptr(), T, max_vl, out_size, Lb.stream()))
    sync()
    wg, wm = R.collate_subs_ref(nfrm, ntok, max_vl, out_size)
    assert torch.equal(gidx.t.cpu(), torch.from_numpy(wg)) and torch.equal(mask.t.cpu(), torch.from_numpy(wm))
    assert gidx.guards_intact() and mask.guards_intact()
    return gidx.t.cpu(), mask.t.cpu()


def test_collate_subs_small_rows(Lb):
    ln = R.lengths_of(R.collate_lists())
    assert set(ln["sub_nfrm"]) >= {0, MAX_VL} and set(ln["sub_ntok"]) >= {1, MAX_SL}
    need = int((np.maximum(ln["sub_nfrm"], 1) + ln["sub_ntok"]).max())
    for out_size in (need, need + 3, MAX_VL + MAX_SL):                       # the reference's width, and wider than any row needs
        gidx, mask = run_subs(Lb, ln["sub_nfrm"], ln["sub_ntok"], MAX_VL, out_size)
        assert int(mask.sum()) == int(ln["sub_nfrm"].sum() + ln["sub_ntok"].sum())
        assert int(gidx.max()) == MAX_VL + MAX_SL - 1


def test_collate_subs_grid_stride_second_trip(Lb):
    T, out_size, max_vl = 4100, 256, 100
    assert T * out_size > 4096 * 256
    rs = np.random.RandomState(1)
    nfrm, ntok = rs.randint(0, max_vl + 1, size=T), rs.randint(1, 151, size=T)
    nfrm[::7], nfrm[1::7], ntok[2::7], ntok[3::7] = 0, max_vl, 1, 150
    nfrm[-1], ntok[-1] = max_vl, 150                                           # the last row, handled on the second trip
    run_subs(Lb, nfrm, ntok, max_vl, out_size)


# ---- hero_collate_clip_mask ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,NF", [(3, 7), (7, 100), (1, 1)])
def test_collate_clip_mask(Lb, B, NF):
    assert (B * NF) % 256 != 0
    nfrm = np.int32(([0, 1, NF] + list(np.random.RandomState(B).randint(0, NF + 1, size=B)))[:B][::-1])
    mask = Buf((B, NF), torch.int64)
    a = dev(nfrm)
    Lb.check(Lb.lib().hero_collate_clip_mask(a.data_ptr(), mask.ptr(), B, NF, Lb.stream()))
    sync()
    assert torch.equal(mask.t.cpu(), torch.from_numpy(R.clip_mask_ref(nfrm, NF))) and mask.guards_intact()
    assert mask.t.sum(1).cpu().tolist() == nfrm.tolist()


# ---- hero_collate_frame_map ----------------------------------------------------------------------------------------------------
def run_frame_map(Lb, videos, NF, Lf):
    ln, B = R.lengths_of(videos), len(videos)
    d = dlen(ln)
    T = int(ln["vid_sub_off"][-1])
    lib, s = Lb.lib(), Lb.stream()
    counts = Buf(B * NF, torch.int32)
    Lb.check(lib.hero_collate_frame_map(d["vid_sub_off"].data_ptr(), d["sub_frm_off"].data_ptr(), d["sub_frm"].data_ptr(), None, counts.ptr(),
                                        None, None, B, NF, Lf, 0, s))
    sync()
    wc, wo, we, writes = R.frame_map_ref(ln["vid_sub_off"], ln["sub_frm_off"], ln["sub_frm"], B, NF, Lf)
    assert torch.equal(counts.t.cpu(), torch.from_numpy(wc)) and counts.guards_intact()
    offsets = dev(np.concatenate([[0], np.cumsum(counts.t.cpu().numpy())]).astype(np.int32))          # the caller's exclusive scan
    entries, inverse = Buf(len(we) + 5, torch.int32), Buf(T * Lf, torch.int32)
    Lb.check(lib.hero_collate_frame_map(d["vid_sub_off"].data_ptr(), d["sub_frm_off"].data_ptr(), d["sub_frm"].data_ptr(), offsets.data_ptr(),
                                        None, entries.ptr(), inverse.ptr(), B, NF, Lf, 1, s))
    sync()
    assert torch.equal(entries.t[:len(we)].cpu(), torch.from_numpy(we)) and bool((entries.t[len(we):] == ISENT).all())
    wi = np.full(T * Lf, ISENT, dtype=np.int32)                               # positions nothing writes keep the pre-fill
    for src_row, frame in writes.items():
        wi[src_row] = frame
    assert torch.equal(inverse.t.cpu(), torch.from_numpy(wi))
    assert entries.guards_intact() and inverse.guards_intact() and counts.guards_intact()
    return wc, wo, we, np.where(wi == ISENT, -1, wi)


def host_frame_map(videos, NF, Lf):
    from hero_amd.model.model import build_frame_map
    sub2frm = [[(sid, list(fr)) for sid, (fr, _) in enumerate(subs)] for _, subs in videos]
    o, e, inv = build_frame_map([len(subs) for _, subs in videos], sub2frm, len(videos), NF, Lf, "cpu")
    return o.numpy(), e.numpy(), inv.numpy()


def test_collate_frame_map_small_lists(Lb):
    NF, Lf = 6, 14
    videos = R.collate_lists()
    counts, _, _, _ = run_frame_map(Lb, videos, NF, Lf)                        # frames 7 and 40 of video 1 match nothing
    assert counts[2] == 3 and counts[4] == 2 and (counts[2 * NF:3 * NF] == 0).all()     # three subtitles; twice in one; a video without subtitles
    assert counts.sum() == sum(1 for _, subs in videos for fr, _ in subs for f in fr) - 2
    inside = [(nf, [([f for f in fr if f < NF], nt) for fr, nt in subs]) for nf, subs in videos]
    _, wo, we, winv = run_frame_map(Lb, inside, NF, Lf)
    o, e, inv = host_frame_map(inside, NF, Lf)
    assert np.array_equal(o, wo) and np.array_equal(e, we) and np.array_equal(inv, winv)


def test_collate_frame_map_several_workgroups(Lb):
    B, NF, Lf = 5, 60, 12
    videos = R.random_videos(B, NF, seed=1)
    assert B * NF > 2 * 128 and (B * NF) % 128 != 0
    counts, _, _, _ = run_frame_map(Lb, videos, NF, Lf)
    assert counts.max() >= 2
    inside = [(nf, [([f for f in fr if f < NF], nt) for fr, nt in subs]) for nf, subs in videos]
    _, wo, we, winv = run_frame_map(Lb, inside, NF, Lf)
    o, e, inv = host_frame_map(inside, NF, Lf)
    assert np.array_equal(o, wo) and np.array_equal(e, we) and np.array_equal(inv, winv)


# ---- hero_collate_gather_feats -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 768, 1028])                                  # 1028 / 4 = 257 float4 > 256 threads: a second column trip
def test_collate_gather_feats(Lb, D):
    videos = R.collate_lists()
    ln, B, NF = R.lengths_of(videos), len(videos), 6
    T = int(ln["vid_sub_off"][-1])
    cn = np.random.RandomState(D).randn(B, NF, D).astype(np.float32)
    c, d = dev(cn), dlen(ln)
    feats, row_vid = Buf((T, MAX_VL, D), torch.float32), Buf(T, torch.int32)
    Lb.check(Lb.lib().hero_collate_gather_feats(c.data_ptr(), feats.ptr(), d["vid_sub_off"].data_ptr(), d["vid_nfrm"].data_ptr(),
                                               d["sub_frm_off"].data_ptr(), d["sub_frm"].data_ptr(), row_vid.ptr(), T, MAX_VL, B, NF, D, Lb.stream()))
    sync()
    want, wv = R.gather_feats_ref(cn, ln["vid_sub_off"], ln["vid_nfrm"], ln["sub_frm_off"], ln["sub_frm"], MAX_VL)
    assert same_bits(feats.t, torch.from_numpy(want)) and torch.equal(row_vid.t.cpu(), torch.from_numpy(wv))
    assert feats.guards_intact() and row_vid.guards_intact()
    # video 1 has 3 frames: [1, 3, 2] keeps 1, 2 (2 shifts down), [7, 0, 40, 1] keeps 0, 1, [3] keeps nothing
    assert np.array_equal(want[5, :3], np.stack([cn[1, 1], cn[1, 2], np.zeros(D, np.float32)])) and not want[7].any()
    assert np.array_equal(want[6, :2], cn[1, :2]) and not want[6, 2:].any() and np.array_equal(want[3], cn[0, [2, 3, 4, 4, 5]])


# ---- hero_derive_multi ---------------------------------------------------------------------------------------------------------
P0, P1, P2 = 14, MAX_VL, MAX_SL
DERIVE_N = [255, 0, 300000, 1, 256, 300000, 0, 1, 0, 255, 1, 300000, 300000, 256, 0, 1]     # 300000 > 1024 workgroups x 256 threads
DERIVE_MODE = [0, 1, 2, 3, 1, 3, 2, 0, 3, 2, 1, 0, 1, 3, 0, 2]


def derive_source(mode, n, seed):
    rs = np.random.RandomState(seed)
    if mode == R.DERIVE_MASK_ADD:
        return rs.randint(0, 2, size=n).astype(np.int64)
    if mode == R.DERIVE_F32:
        x = rs.randint(-2 ** 24, 2 ** 24, size=n).astype(np.int64)
        x[::5] = rs.randint(-2 ** 40, 2 ** 40, size=len(x[::5]))             # not all representable: the cast rounds to nearest even
        return x
    if mode == R.DERIVE_I32:
        return rs.randint(-2 ** 31, 2 ** 31, size=n).astype(np.int64)
    return rs.randint(0, P1 + P2, size=n).astype(np.int64)                    # x on both sides of p1


def derive_descs(Lb, ns, modes):
    keep, descs, outs = [], [], []
    for i, (n, mode) in enumerate(zip(ns, modes)):
        x = derive_source(mode, n, seed=i)
        src = dev(x if n else np.int64([ISENT]))
        dst = Buf(n, torch.float32 if mode in (R.DERIVE_MASK_ADD, R.DERIVE_F32) else torch.int32)
        keep.append(src)
        outs.append((dst, R.derive_ref(mode, x, P0, P1, P2)))
        descs.append(Lb.Derive(src.data_ptr(), dst.ptr(), n, mode, P0, P1, P2))
    return keep, (Lb.Derive * len(descs))(*descs), outs


def test_derive_multi_sixteen_descriptors_of_different_lengths(Lb):
    assert len(DERIVE_N) == 16 and {(n, m) for n, m in zip(DERIVE_N, DERIVE_MODE)} >= {(300000, m) for m in range(4)}
    assert set(DERIVE_N) == {0, 1, 255, 256, 300000} and 300000 > 1024 * 256
    keep, arr, outs = derive_descs(Lb, DERIVE_N, DERIVE_MODE)
    Lb.check(Lb.lib().hero_derive_multi(arr, 16, Lb.stream()))
    sync()
    for i, (dst, want) in enumerate(outs):
        assert same_bits(dst.t, torch.from_numpy(want)), (i, DERIVE_N[i], DERIVE_MODE[i])
        assert dst.guards_intact(), i                                          # also: the element one past n
    flat = [w for (_, w), m, n in zip(outs, DERIVE_MODE, DERIVE_N) if m == R.DERIVE_FLAT_GATHER and n == 300000][0]
    assert (flat >= 0).any() and (flat <= -2).any() and not (flat == -1).any()


def test_derive_multi_one_descriptor_and_seventeen_refused(Lb):
    keep, arr, outs = derive_descs(Lb, [256], [R.DERIVE_FLAT_GATHER])
    Lb.check(Lb.lib().hero_derive_multi(arr, 1, Lb.stream()))
    sync()
    assert same_bits(outs[0][0].t, torch.from_numpy(outs[0][1])) and outs[0][0].guards_intact()
    keep, arr, outs = derive_descs(Lb, [255] * 17, [i % 4 for i in range(17)])
    rc = Lb.lib().hero_derive_multi(arr, 17, Lb.stream())
    sync()
    assert rc != 0 and all(dst.untouched() for dst, _ in outs)
