"""tests/pretrain_mask_reference.py - the integer statement of the device draw of the pre-training batches - is a sound
sampler: its rates are the binomial ones, its token range and its permutations are right, and it keeps the structural rules
of the reference's draws (data/mlm.py:21-58, data/mfm.py:19-25, data/fom.py:96-115).

Every bound is DERIVED: a count of n independent draws of probability q lies within 5 standard deviations sqrt(n q (1 - q))
of n q except with probability < 6e-7 per check; the seeds are fixed, so the tests are deterministic."""
import itertools
import math

import numpy as np

from tests import pretrain_mask_reference as R

MASK_ID, V_RANGE, CLS = 4, (5, 50265), 0


def _within(count, n, q, what):
    sd = math.sqrt(n * q * (1.0 - q))
    assert abs(count - n * q) <= 5.0 * sd, (what, count, n * q, sd)


def test_mlm_rates_shares_and_token_range():
    T, max_sl = 2500, 101                                             # 250 000 token draws (column 0 is never drawn)
    rng = np.random.default_rng(0)
    ids = rng.integers(V_RANGE[0], V_RANGE[1], size=(T, max_sl), dtype=np.int64)
    thr = R.threshold(0.15)
    out = R.mlm_mask(ids, np.full(T, 3), np.full(T, max_sl), 3 + max_sl, seed=0x1234567890ABCDEF, site=0x4D4C4D, thr=thr,
                     mask_id=MASK_ID, v_range=V_RANGE, first_token=CLS)
    kind = out["kind"]
    assert (kind != 4).all()                                          # 100 tokens per row: the at-least-one rule cannot matter here
    n = T * (max_sl - 1)
    assert n >= 200000
    m = int((kind > 0).sum())
    _within(m, n, thr / 2.0 ** 32, "selected")
    # given h < thr, h is uniform on [0, thr): the shares are thr80 / thr, (thr90 - thr80) / thr and the rest
    q_mask, q_rand = (thr * 4 // 5) / thr, (thr * 9 // 10 - thr * 4 // 5) / thr
    assert abs(q_mask - 0.8) < 1e-8 and abs(q_rand - 0.1) < 1e-8
    _within(int((kind == 1).sum()), m, 0.8, "mask share")
    _within(int((kind == 2).sum()), m, 0.1, "random share")
    _within(int((kind == 3).sum()), m, 0.1, "keep share")
    new = out["input_ids"]
    assert (new[kind == 1] == MASK_ID).all() and (new[kind == 3] == ids[kind == 3]).all()
    assert (new[:, 1:][kind[:, 1:] == 0] == ids[:, 1:][kind[:, 1:] == 0]).all()
    rand = new[kind == 2]
    assert rand.size > 1000 and rand.min() >= V_RANGE[0] and rand.max() < V_RANGE[1]
    # the random tokens spread over the range: the mean of k uniform draws on [lo, hi) has sd (hi - lo) / sqrt(12 k)
    width = V_RANGE[1] - V_RANGE[0]
    assert abs(rand.mean() - (V_RANGE[0] + (width - 1) / 2.0)) <= 5.0 * width / math.sqrt(12.0 * rand.size)
    assert (new[:, 0] == CLS).all() and not out["sel"][:, 0].any()    # column 0: the first token, never drawn
    assert out["count"] == m and (out["txt_labels"] == ids[out["sel"]]).all()
    assert np.array_equal(out["txt_mask_rows"], np.flatnonzero(out["txt_mask_tgt"].reshape(-1)))


def test_mlm_structural_rules():
    rng = np.random.default_rng(1)
    T, max_sl = 64, 9
    ids = rng.integers(5, 100, size=(T, max_sl), dtype=np.int64)
    ntok = rng.integers(1, max_sl + 1, size=T)
    ntok[:4] = (1, 2, 1, max_sl)
    nfrm = rng.integers(0, 4, size=T)
    nfrm[:4] = (2, 0, 0, 3)
    for c in range(T):
        ids[c, ntok[c]:] = 1
    Lf = int((np.maximum(nfrm, 1) + ntok).max())
    for p, need_forced in ((0.02, True), (0.0, True), (1.0, False)):
        out = R.mlm_mask(ids, nfrm, ntok, Lf, seed=77, site=3, thr=R.threshold(p), mask_id=MASK_ID, v_range=(5, 100), first_token=CLS)
        sel, kind = out["sel"], out["kind"]
        assert not sel[:, 0].any() and not sel[np.arange(max_sl)[None, :] >= ntok[:, None]].any()
        assert (sel.sum(1)[ntok >= 2] >= 1).all() and (sel.sum(1)[ntok <= 1] == 0).all()       # at least one; nothing to mask
        forced = (kind == 4).any(1)
        assert forced.any() == need_forced
        assert (sel[forced].sum(1) == 1).all() and sel[forced, 1].all() and (out["input_ids"][forced, 1] == MASK_ID).all()
        for r in range(T):                                            # the token mask, shifted right by the row's frame slots
            eff = max(int(nfrm[r]), 1)
            assert not out["txt_mask_tgt"][r, :eff + 1].any()
            assert np.array_equal(out["txt_mask_tgt"][r, eff:eff + ntok[r]], sel[r, :ntok[r]])
        assert (out["input_ids"][:, 1:][~sel[:, 1:]] == ids[:, 1:][~sel[:, 1:]]).all()
        if p == 1.0:
            assert out["count"] == int(np.maximum(ntok - 1, 0).sum())
        if p == 0.0:
            assert out["count"] == int((ntok >= 2).sum())


def test_mfm_rates_and_structural_rules():
    B, NF = 4000, 60
    vn = np.full(B, NF)
    vn[:3] = (1, 0, 7)
    lengths = {"vid_nfrm": vn, "vid_sub_off": np.arange(B + 1), "sub_frm_off": np.arange(B + 1) * 3,
               "sub_frm": np.tile(np.array([0, NF + 5, 2]), B)}                 # every row: frames 0, one past the clip, 2
    thr = R.threshold(0.15)
    out = R.mfm_mask(lengths, B, 4, NF, seed=(1 << 40) + 9, site=0x4D464D, thr=thr)
    c, f = out["c_v_masks"], out["f_v_masks"]
    assert not c[np.arange(NF)[None, :] >= vn[:, None]].any()
    assert (c.sum(1)[vn > 0] >= 1).all() and c[1].sum() == 0 and c[0, 0]              # at least one; no frame, nothing; one frame, that one
    natural = c.copy()
    natural[out["forced"] >= 0] = False
    n = int(vn.sum())
    _within(int(natural.sum()), n, thr / 2.0 ** 32, "selected frames")
    # at p = 0.02 a video of 60 frames has no selection of its own with probability 0.98^60 = 0.30: the at-least-one frames
    # are uniform on the video (mean (NF - 1) / 2, variance (NF^2 - 1) / 12)
    low = R.mfm_mask(lengths, B, 4, NF, seed=(1 << 40) + 9, site=0x4D464D, thr=R.threshold(0.02))
    forced = low["forced"][(low["forced"] >= 0) & (vn == NF)]
    _within(forced.size, int((vn == NF).sum()), (1.0 - R.threshold(0.02) / 2.0 ** 32) ** NF, "videos without a selection")
    assert forced.min() >= 0 and forced.max() < NF and (low["c_v_masks"].sum(1)[vn > 0] >= 1).all()
    assert abs(forced.mean() - (NF - 1) / 2.0) <= 5.0 * math.sqrt((NF * NF - 1) / 12.0 / forced.size)
    assert (low["c_v_masks"][low["forced"] >= 0].sum(1) == 1).all()
    # slots: frame 0, then frame 2 (the frame past the clip is dropped), then empty slots
    full = vn == NF
    assert np.array_equal(f[full, 0], c[full, 0]) and np.array_equal(f[full, 1], c[full, 2]) and not f[:, 2:].any()
    assert not f[1].any() and f[0, 0] and not f[0, 1:].any()                          # a row without a frame in its video: False


def test_fom_is_a_uniform_permutation_of_the_selected_frames():
    B, NF = 20000, 8
    vn = np.full(B, NF)
    vn[:2] = (0, 5)
    orders, targets = R.fom_shuffle(vn, NF, seed=0xFEDCBA9876543210, site=0x464F4D, thr=R.threshold(0.375))
    ident = np.arange(NF)[None, :]
    sel = targets != -1
    assert not sel[0].any() and not sel[1, 5:].any()
    assert (np.sort(orders, 1) == ident).all()                                        # a permutation of the positions
    assert (orders[~sel] == np.broadcast_to(ident, orders.shape)[~sel]).all()         # frames that were not drawn stay
    moved = orders != ident
    assert not (moved & ~np.take_along_axis(sel, orders, 1)).any()                    # only selected frames are shown elsewhere
    b, s = np.nonzero(sel)
    assert (orders[b, targets[b, s]] == s).all()                                      # targets is the inverse on the selected set
    b, p = np.nonzero(np.take_along_axis(sel, orders, 1) & sel)
    assert (targets[b, orders[b, p]] == p).all()
    n_sel = sel.sum(1)
    _within(int(sel[2:].sum()), (B - 2) * NF, R.threshold(0.375) / 2.0 ** 32, "selected frames")
    three = np.flatnonzero(n_sel == 3)
    assert three.size > 4000
    counts = dict.fromkeys(itertools.permutations(range(3)), 0)
    for v in three:
        P = np.flatnonzero(sel[v])
        counts[tuple(int(np.searchsorted(P, x)) for x in orders[v, P])] += 1
    assert len(counts) == 6
    for perm, k in counts.items():
        _within(k, three.size, 1.0 / 6.0, perm)


def test_seed_and_site_key_the_draw():
    vn = np.full(16, 40)
    a = R.fom_shuffle(vn, 40, seed=5, site=1, thr=R.threshold(0.5))[0]
    assert np.array_equal(a, R.fom_shuffle(vn, 40, seed=5, site=1, thr=R.threshold(0.5))[0])
    assert not np.array_equal(a, R.fom_shuffle(vn, 40, seed=R.advance(5), site=1, thr=R.threshold(0.5))[0])
    assert not np.array_equal(a, R.fom_shuffle(vn, 40, seed=5, site=2, thr=R.threshold(0.5))[0])
    assert not np.array_equal(a, R.fom_shuffle(vn, 40, seed=5 + (1 << 32), site=1, thr=R.threshold(0.5))[0])
    assert R.threshold(1.0) == 1 << 32 and R.threshold(0.0) == 0 and R.advance((1 << 64) - 1) == R.SEED_STEP - 1
