"""The device draw of the pre-training batches (hero_amd/csrc/pretrain_mask.hip: hero_mlm_mask, hero_mfm_mask,
hero_fom_shuffle) stated in numpy INTEGER arithmetic on tests/dropout_hash.py's hashes.  It is the one definition the GPU
tests compare against (tests/test_gpu_pretrain_mask.py); tests/test_cpu_pretrain_mask_reference.py checks that it is a sound
sampler.

    base = splitmix64(seed ^ site * 0xD6E8FEB86659FD93 mod 2^64),  k0 = low 32 bits, k1 = high 32 bits
    element e (index in the padded layout)  ->  h = mix32(e ^ k0),  h2 = mix32(e ^ k1);  selected iff h < thr
    thr = floor(p * 2^32) (p = 1: 2^32, everything);  thr80 = thr * 4 // 5,  thr90 = thr * 9 // 10
    a bounded integer from a hash x:  lo + (x * n >> 32)
    MLM  e = r * max_sl + c, 1 <= c < sub_ntok[r]; h < thr80 -> mask_id, else h < thr90 -> v_lo + (h2 * (v_hi - v_lo) >> 32),
         else kept; a row with sub_ntok >= 2 and nothing selected selects column 1 (mask_id); column 0 := first_token
    MFM  e = b * NF + f, f < vid_nfrm[b]; a video with frames and nothing selected selects (mix32(~b ^ k1) * vid_nfrm[b]) >> 32
    FOM  e = b * NF + f, f < vid_nfrm[b]; selected positions P (ascending) and S (the same, by (h2, position)):
         orders[b, P[i]] = S[i], targets[b, S[i]] = P[i]; identity and -1 elsewhere
    advance():  seed <- seed + 0x9E3779B97F4A7C15 mod 2^64
"""
import math

import numpy as np

from tests.dropout_hash import _mix32, _splitmix64

_M64 = (1 << 64) - 1
SITE_MUL = 0xD6E8FEB86659FD93
SEED_STEP = 0x9E3779B97F4A7C15


def threshold(p):
    assert 0.0 <= p <= 1.0
    return int(math.floor(p * 4294967296.0))          # exact: a scaling by a power of two


def keys(seed, site):
    base = _splitmix64((seed ^ ((site * SITE_MUL) & _M64)) & _M64)
    return base & 0xFFFFFFFF, base >> 32


def advance(seed):
    return (seed + SEED_STEP) & _M64


def _hash(e, k):
    return _mix32(np.asarray(e, dtype=np.uint64) ^ np.uint64(k))


def mlm_mask(ids, sub_nfrm, sub_ntok, Lf, seed, site, thr, mask_id, v_range, first_token):
    """ids [T, max_sl] int64 (clean).  Returns dict: input_ids, sel [T, max_sl] bool, kind [T, max_sl] (0 none, 1 mask, 2 random,
    3 kept, 4 the at-least-one rule), txt_mask_tgt [T, Lf] bool, txt_labels [n] int64, txt_mask_rows [n] int32, count."""
    ids = np.asarray(ids, dtype=np.int64)
    T, max_sl = ids.shape
    nfrm, ntok = np.asarray(sub_nfrm, dtype=np.int64), np.asarray(sub_ntok, dtype=np.int64)
    eff = np.maximum(nfrm, 1)
    assert (ntok <= max_sl).all() and (eff + ntok <= Lf).all(), "rows must fit their padded layout"
    k0, k1 = keys(seed, site)
    e = np.arange(T * max_sl, dtype=np.uint64).reshape(T, max_sl)
    h, h2 = _hash(e, k0), _hash(e, k1)
    col = np.arange(max_sl)[None, :]
    drawn = (col >= 1) & (col < ntok[:, None]) & (h < np.uint64(thr))
    n = int(v_range[1] - v_range[0])
    out = ids.copy()
    out[:, 0] = first_token
    kind = np.zeros((T, max_sl), dtype=np.int8)
    as_mask = drawn & (h < np.uint64(thr * 4 // 5))
    as_rand = drawn & ~as_mask & (h < np.uint64(thr * 9 // 10))
    kind[drawn], kind[as_rand], kind[as_mask] = 3, 2, 1
    out[as_mask] = mask_id
    out[as_rand] = (v_range[0] + ((h2 * np.uint64(n)) >> np.uint64(32)).astype(np.int64))[as_rand]
    sel = drawn.copy()
    forced = ~drawn.any(1) & (ntok >= 2)
    if forced.any():
        sel[forced, 1] = True
        kind[forced, 1] = 4
        out[forced, 1] = mask_id
    tgt = np.zeros((T, Lf), dtype=bool)
    for r in range(T):
        tgt[r, eff[r]:eff[r] + max_sl][:Lf - eff[r]] = sel[r][:Lf - eff[r]]
    assert int(tgt.sum()) == int(sel.sum())
    return {"input_ids": out, "sel": sel, "kind": kind, "txt_mask_tgt": tgt, "txt_labels": ids[sel],
            "txt_mask_rows": np.flatnonzero(tgt.reshape(-1)).astype(np.int32), "count": int(sel.sum())}


def slot_frames(lengths, T, max_vl):
    """[T, max_vl] frame (inside its video) behind every frame slot, -1 for an empty slot; [T] video of each row: the walk of
    hero_collate_gather_feats (frames outside [0, vid_nfrm) are dropped)."""
    off, frm = np.asarray(lengths["sub_frm_off"]), np.asarray(lengths["sub_frm"])
    vso, vn = np.asarray(lengths["vid_sub_off"]), np.asarray(lengths["vid_nfrm"])
    out = np.full((T, max_vl), -1, dtype=np.int64)
    vid = np.zeros(T, dtype=np.int64)
    for b in range(len(vn)):
        for r in range(vso[b], vso[b + 1]):
            vid[r] = b
            keep = [int(f) for f in frm[off[r]:off[r + 1]] if 0 <= f < vn[b]][:max_vl]
            out[r, :len(keep)] = keep
    return out, vid


def mfm_mask(lengths, T, max_vl, NF, seed, site, thr):
    """Returns dict: c_v_masks [B, NF] bool, f_v_masks [T, max_vl] bool, forced [B] (the at-least-one frame or -1), count."""
    vn = np.asarray(lengths["vid_nfrm"], dtype=np.int64)
    B = len(vn)
    k0, k1 = keys(seed, site)
    e = np.arange(B * NF, dtype=np.uint64).reshape(B, NF)
    c = (np.arange(NF)[None, :] < vn[:, None]) & (_hash(e, k0) < np.uint64(thr))
    forced = np.full(B, -1, dtype=np.int64)
    for b in range(B):
        if vn[b] > 0 and not c[b].any():
            forced[b] = (int(_hash(np.array([0xFFFFFFFF - b]), k1)[0]) * int(vn[b])) >> 32
            c[b, forced[b]] = True
    frames, vid = slot_frames(lengths, T, max_vl)
    ok = (frames >= 0) & (frames < NF)
    f = np.zeros((T, max_vl), dtype=bool)
    f[ok] = c[np.broadcast_to(vid[:, None], frames.shape)[ok], frames[ok]]
    return {"c_v_masks": c, "f_v_masks": f, "forced": forced, "count": int(c.sum())}


def fom_shuffle(vid_nfrm, NF, seed, site, thr):
    """Returns (shuffled_orders, targets) [B, NF] int64."""
    vn = np.asarray(vid_nfrm, dtype=np.int64)
    B = len(vn)
    k0, k1 = keys(seed, site)
    e = np.arange(B * NF, dtype=np.uint64).reshape(B, NF)
    sel = (np.arange(NF)[None, :] < vn[:, None]) & (_hash(e, k0) < np.uint64(thr))
    key = _hash(e, k1)
    orders = np.tile(np.arange(NF, dtype=np.int64), (B, 1))
    targets = np.full((B, NF), -1, dtype=np.int64)
    for b in range(B):
        P = np.flatnonzero(sel[b])
        S = np.array(sorted(P.tolist(), key=lambda f: (int(key[b, f]), f)), dtype=np.int64)
        orders[b, P] = S
        targets[b, S] = P
    return orders, targets
