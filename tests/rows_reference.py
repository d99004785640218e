"""Host statements of the row-movement and index operations (the first half of hero_amd/csrc/rows.hip, all of
hero_amd/csrc/collate.hip) and the case builders of tests/test_gpu_rows_kernels.py / tests/test_gpu_collate_kernels.py:
numpy, float64 / int64, plain loops, nothing from a kernel body - every statement is written from the comments of
include/hero_hip.h.  tests/test_cpu_rows_reference.py holds the statements against torch (stable sort, index_add_, .to(),
the mask arithmetic), against the project's host builders (functional.host_segment_order, collate.video_collate,
model.build_frame_map, CrossModalTrm's flat gather index) and checks the properties the GPU tests rely on.

Why the GPU tests need no tolerance.  Every one of these operations moves values or adds a few of them up.  Moved values are
compared bit for bit.  Sums are made exact by construction: the addends are small integers, so every partial sum, in whatever
order a kernel takes them, is an integer that the accumulator's format holds exactly -
    fp32 accumulator / destination:  |dst0| + sum |x| < 2^24 per (destination, column)        (`exact_f32`)
    bf16 destination of hero_scatter_add_rows:  x in {-1, 0, 1}, |dst0| + (number of non-zero x) <= 256 per (destination,
    column): 8 significand bits hold every integer up to 256                                     (`exact_bf16`)
and the float64 statement of the same sum is then the kernel's answer to the last bit."""
import numpy as np

SEG_B = 16                     # sorted positions per wave of hero_scatter_add_sorted (include/hero_hip.h: "blocks of 16 sorted rows")


# ---- number formats --------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32.  Finite inputs only."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


# ---- gathers / scatters -----------------------------------------------------------------------------------------------------
def gather_ref(a, b, idx):
    """out[r] = a[idx[r]] if idx[r] >= 0, zeros if idx[r] == -1, b[-idx[r] - 2] otherwise."""
    cols = a.shape[1]
    out = np.zeros((len(idx), cols), dtype=np.float64)
    for r, i in enumerate(idx):
        if i >= 0:
            out[r] = a[i]
        elif i <= -2:
            out[r] = b[-i - 2]
    return out


def scatter_add_ref(src, idx, dst_a, dst_b, skip):
    """dst_a[idx[r]] += src[r] (idx[r] >= 0), dst_b[-idx[r] - 2] += src[r] (idx[r] <= -2; dropped when there is no dst_b);
    rows with idx[r] == -1 or == skip are dropped.  float64 copies are returned."""
    da = np.array(dst_a, dtype=np.float64)
    db = None if dst_b is None else np.array(dst_b, dtype=np.float64)
    for r, i in enumerate(idx):
        if i == -1 or (skip >= 0 and i == skip):
            continue
        if i >= 0:
            da[i] += src[r]
        elif db is not None:
            db[-i - 2] += src[r]
    return da, db


def scatter_counts(src, idx, n_a, n_b, skip):
    """Per (destination, column): the number of non-zero addends and the sum of their magnitudes, for both destinations."""
    cols = src.shape[1]
    nz = [np.zeros((n_a, cols)), np.zeros((max(n_b, 1), cols))]
    mag = [np.zeros((n_a, cols)), np.zeros((max(n_b, 1), cols))]
    for r, i in enumerate(idx):
        if i == -1 or (skip >= 0 and i == skip):
            continue
        t, d = (0, i) if i >= 0 else (1, -i - 2)
        nz[t][d] += src[r] != 0
        mag[t][d] += np.abs(src[r])
    return nz, mag


def exact_f32(dst0, mag):
    return bool((np.abs(dst0) + mag < 2.0 ** 24).all())


def exact_bf16(src, dst0, nz):
    return bool(np.isin(src, (-1.0, 0.0, 1.0)).all() and (np.abs(dst0) + nz <= 256).all() and (dst0 == np.round(dst0)).all())


SCATTER_COMBOS = (("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16"))        # source -> destination
SCATTER_COLS = (2, 6, 128)
SCATTER_HOT = 7


def scatter_rows_case(cols, skip, seed=0):
    """600 rows of values in {-1, 0, 1} into 40 rows of dst_a and 12 of dst_b: destination 7 receives exactly 250 rows (the
    bf16 compare-and-swap loop under contention: 250 + |pre-fill| <= 256), every 9th row all zero, -1 and (if >= 0) the skip id
    present, both destinations pre-filled with non-zero integers of magnitude <= 3."""
    rs = np.random.RandomState(1000 + cols + seed)
    rows, n_a, n_b = 600, 40, 12
    src = rs.randint(-1, 2, size=(rows, cols)).astype(np.float32)
    src[::9] = 0.0
    idx = rs.randint(-n_b - 1, n_a, size=rows).astype(np.int32)         # -13 .. 39: -1 among them
    idx[idx == SCATTER_HOT] = SCATTER_HOT + 1
    idx[rs.permutation(rows)[:250]] = SCATTER_HOT
    return dict(src=src, idx=idx, n_a=n_a, n_b=n_b, hot=SCATTER_HOT, a0=int_table(n_a, cols), b0=-int_table(n_b, cols), skip=skip)


def csr_gather_sum_ref(src, offs, ent):
    """out[r] = sum of src[ent[e]] for e in [offs[r], offs[r + 1]); an empty row gives zeros."""
    out = np.zeros((len(offs) - 1, src.shape[1]), dtype=np.float64)
    for r in range(len(offs) - 1):
        for e in range(offs[r], offs[r + 1]):
            out[r] += src[ent[e]]
    return out


def csr_gather_sum_f32_in_order(src, offs, ent):
    """The same sum in float32, entries added one after the other in entry order ("pair order")."""
    out = np.zeros((len(offs) - 1, src.shape[1]), dtype=np.float32)
    for r in range(len(offs) - 1):
        for e in range(offs[r], offs[r + 1]):
            out[r] = out[r] + src[ent[e]].astype(np.float32)
    return out


def inverse_first_ref(idx, na, nb):
    """inv[s] (s < na) / inv[na + s] (rows of b): the smallest j with idx[j] naming that source row, -1 if none.  Ids that
    name no source row (>= na, or -idx - 2 >= nb) and -1 are ignored."""
    inv = np.full(na + nb, -1, dtype=np.int32)
    for j in range(len(idx) - 1, -1, -1):                 # backwards: the smallest j is written last
        v = int(idx[j])
        if 0 <= v < na:
            inv[v] = j
        elif v <= -2 and -v - 2 < nb:
            inv[na - v - 2] = j
    return inv


def segment_order_ref(idx, skip):
    """Row numbers sorted by (idx[row], row); rows with idx < 0 or == skip (skip >= 0) last, in row order."""
    kept = [r for r, v in enumerate(idx) if v >= 0 and not (skip >= 0 and v == skip)]
    dropped = [r for r, v in enumerate(idx) if not (v >= 0 and not (skip >= 0 and v == skip))]
    kept.sort(key=lambda r: int(idx[r]))                  # list.sort is stable
    return np.asarray(kept + dropped, dtype=np.int32)


def scatter_sorted_ref(src, idx, dst, skip):
    """dst[idx[r]] += src[r], rows with idx < 0 or == skip dropped; float64."""
    out = np.array(dst, dtype=np.float64)
    for r, v in enumerate(idx):
        if v >= 0 and not (skip >= 0 and v == skip):
            out[v] += src[r]
    return out


# ---- casts / transposes --------------------------------------------------------------------------------------------------------
def cast_ref(x, bf16):
    x = np.asarray(x, dtype=np.float32)
    return bf16_round(x) if bf16 else x


def copy_write_set(rows, cols, ldd, transpose):
    """Element offsets (from the descriptor's dst pointer, in destination elements) that the copy may change, in the order of
    src.reshape(-1): plain dst[r * ldd + c], transposed dst[c * ldd + r].  Everything else keeps its bytes."""
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return (c * ldd + r if transpose else r * ldd + c).reshape(-1)


def copy_apply(arena, at, src, ldd, transpose, bf16):
    """Apply one copy to a float32 host image of the destination arena (element offset `at`)."""
    rows, cols = src.shape
    arena[at + copy_write_set(rows, cols, ldd, transpose)] = cast_ref(src, bf16).reshape(-1)


# ---- scatter-sorted cases: constructed id sequences -------------------------------------------------------------------------------
SITUATIONS = (
    "run_of_1", "ends_at_15_next_starts_at_0", "whole_block_run", "whole_first_block", "whole_middle_block",
    "starts_at_last_position", "spans_2_blocks", "spans_9_blocks", "spans_66_blocks", "multi_block_runs_back_to_back",
    "two_partials_in_one_block", "multi_block_run_ends_at_15", "multi_block_run_before_dropped_tail", "multi_block_run_ends_list",
    "dropped_tail_crosses_block", "all_rows_dropped", "rows_1", "rows_15", "rows_16", "rows_17")

SKIP_ID = 1                                               # a valid table row that no run names: the padding id


def _runs_case(name, runs, tail):
    """runs: lengths of the runs in sorted order (ids increasing, with gaps so that some table rows are named by nothing);
    tail: dropped rows (-1 and the skip id in turn).  Returns idx in a fixed shuffled row order."""
    ids = [0 if k == 0 else 2 + 3 * k for k in range(len(runs))]         # 0, 5, 8, 11, ... (1 = skip, 2 - 4, 6, 7, ... unnamed)
    flat = [i for i, n in zip(ids, runs) for _ in range(n)] + [(-1 if t % 2 == 0 else SKIP_ID) for t in range(tail)]
    perm = np.random.RandomState(len(flat) * 7 + len(runs)).permutation(len(flat))
    idx = np.empty(len(flat), dtype=np.int32)
    idx[perm] = np.asarray(flat, dtype=np.int32)
    return {"name": name, "idx": idx, "skip": SKIP_ID, "n_dst": (ids[-1] if ids else SKIP_ID) + 3, "runs": list(runs), "tail": tail}


def sorted_cases():
    """The id lists of the scatter-sorted tests.  `main` (1373 rows), positions of the sorted list:
         0            run of 1                           1 - 15       ends at position 15 of block 0, next starts at 0 of block 1
         16 - 31      exactly block 1                    32 - 46      filler
         47 - 48      starts at the last position of block 2, 2 blocks
         49 - 191     9 blocks (3 - 11), ends at position 15
         192 - 244    starts aligned: block 12 whole and first, 13 - 14 whole and inside, ends in block 15
         245 - 274    back to back with it, blocks 15 - 17: block 15 holds the end of one crossing run and the start of the next
         275          run of 1                           276 - 286    filler
         287 - 1312   starts at the last position of block 17, 66 blocks (17 - 82): 65 continuation blocks, two probe steps
         1313 - 1352  3 blocks, the last kept rows       1353 - 1372  dropped tail over the boundary at 1360"""
    return [
        _runs_case("main", [1, 15, 16, 15, 2, 143, 53, 30, 1, 11, 1026, 40], 20),
        _runs_case("ends_list", [3, 39], 0),              # a crossing run ends the list inside a partial block
        _runs_case("ends_list_aligned", [16, 32], 0),     # ... and at the end of a full block, behind a one-block run
        _runs_case("all_dropped", [], 20),
        _runs_case("rows1", [1], 0),
        _runs_case("rows15", [7, 8], 0),
        _runs_case("rows16", [16], 0),
        _runs_case("rows17", [17], 0),
        _runs_case("rows17_tail", [1, 15], 1),
    ]


def sorted_keys(idx, skip):
    """The destination at every sorted position, -1 for dropped rows."""
    v = np.asarray(idx)[segment_order_ref(idx, skip)].astype(np.int64)
    return np.where((v < 0) | (v == skip), -1, v)


def situations(idx, skip):
    """Which of SITUATIONS the sorted id list contains; read off the list itself, not off the builder's arguments."""
    keys = sorted_keys(idx, skip)
    n, B = len(keys), SEG_B
    runs = []                                             # (key, first, last) of every run of kept rows
    i = 0
    while i < n and keys[i] >= 0:
        j = i
        while j + 1 < n and keys[j + 1] == keys[i]:
            j += 1
        runs.append((int(keys[i]), i, j))
        i = j + 1
    tail = n - i
    assert (keys[i:] == -1).all()
    found = set()
    span = lambda a, b: b // B - a // B + 1               # noqa: E731
    for k, (_, a, b) in enumerate(runs):
        nxt = runs[k + 1] if k + 1 < len(runs) else None
        if a == b:
            found.add("run_of_1")
        if b % B == B - 1 and nxt is not None:
            found.add("ends_at_15_next_starts_at_0")
        if a % B == 0 and b == a + B - 1:
            found.add("whole_block_run")
        if a % B == 0 and span(a, b) >= 2:
            found.add("whole_first_block")
        if any(a < blk * B and blk * B + B - 1 < b for blk in range(a // B + 1, b // B + 1)):
            found.add("whole_middle_block")
        if a % B == B - 1 and b > a:
            found.add("starts_at_last_position")
        for s in (2, 9, 66):
            if span(a, b) == s:
                found.add("spans_%d_blocks" % s)
        if span(a, b) >= 2 and nxt is not None and span(nxt[1], nxt[2]) >= 2:
            found.add("multi_block_runs_back_to_back")
            if nxt[1] % B != 0:
                found.add("two_partials_in_one_block")
        if span(a, b) >= 2 and b % B == B - 1:
            found.add("multi_block_run_ends_at_15")
        if span(a, b) >= 2 and nxt is None:
            found.add("multi_block_run_before_dropped_tail" if tail else "multi_block_run_ends_list")
    if tail and (n - tail) // B != (n - 1) // B:
        found.add("dropped_tail_crosses_block")
    if tail == n:
        found.add("all_rows_dropped")
    if n in (1, 15, 16, 17):
        found.add("rows_%d" % n)
    return found


def int_rows(rows, cols, seed, lo=-3, hi=3):
    """Integer-valued source rows in [lo, hi] (exact in bf16), every 5th row all zero."""
    x = np.random.RandomState(seed).randint(lo, hi + 1, size=(rows, cols)).astype(np.float32)
    x[::5] = 0.0
    return x


def int_table(n, cols):
    """A non-zero integer pre-fill, |value| <= 3, different in every row and column."""
    r, c = np.meshgrid(np.arange(n), np.arange(cols), indexing="ij")
    v = (r * 3 + c) % 6 - 3
    return np.where(v >= 0, v + 1, v).astype(np.float32)


# ---- segment-sort cases ---------------------------------------------------------------------------------------------------------
SORT_ROWS = (1, 5, 1023, 1024, 1025, 2049, 9601)
# 50272 (the vocabulary: 4 passes) and 2^24 + 1 (7 passes) fill the two pass counts the other sizes leave out
SORT_NDST = (1, 2, 15, 16, 17, 255, 256, 4095, 50272, 65536, 2 ** 20 + 3, 2 ** 24 + 1, 2 ** 28, 2 ** 30 - 1)


def sort_passes(n_dst):
    """4-bit passes of the radix sort: keys 0 .. n_dst - 1 and one more (the dropped rows') need bit_length(n_dst) bits."""
    return (int(n_dst).bit_length() + 3) // 4


def sort_ids(rows, n_dst, skip, pattern, seed):
    """int32 ids in [0, n_dst) with -1, the skip id, id 0 and id n_dst - 1 planted (rows >= 5: all of them present)."""
    rs = np.random.RandomState(seed)
    if pattern == "all_dropped":
        v = np.where(np.arange(rows) % 2 == 0, -1, skip if skip >= 0 else -1)
    elif pattern == "one_id":
        v = np.full(rows, (n_dst - 1) if skip != n_dst - 1 else 0)
    else:
        v = rs.randint(0, n_dst, size=rows, dtype=np.int64)
        v[rs.randint(0, 4, size=rows) == 0] = rs.randint(0, min(n_dst, 7))        # frequent small ids: long runs
        if rows >= 5:
            v[1::7] = -1
            v[2::11] = 0
            v[3::13] = n_dst - 1
            if skip >= 0:
                v[4::9] = skip
        if pattern == "sorted":
            v = np.sort(v)
        elif pattern == "reverse":
            v = np.sort(v)[::-1]
    return np.ascontiguousarray(v, dtype=np.int32)


def sort_cases(n_dst):
    """(rows, skip, pattern) for one n_dst: every row count with the three skip settings in turn, and the four special
    patterns at 1025 rows."""
    skips = (-1, 0, n_dst - 1)
    out = [(rows, skips[(k + n_dst) % 3], "random") for k, rows in enumerate(SORT_ROWS)]
    out += [(1025, skips[k % 3], p) for k, p in enumerate(("all_dropped", "one_id", "sorted", "reverse"))]
    out += [(2049, s, "random") for s in skips]
    return out


# ---- copy_multi table -----------------------------------------------------------------------------------------------------------
COPY_SHAPES = ((1, 768), (64, 64), (65, 129), (130, 96), (7, 5), (40, 98))


def copy_table():
    """The descriptors of the hero_copy_multi test: every shape plain and transposed into fp32 and bf16.  Per descriptor:
    rows, cols, transpose, bf16, ldd, src_off (fp32 elements past a 256-byte boundary), dst_off (BYTES past a 16-byte
    boundary), at (element offset of dst in its arena; set here so that write sets cannot meet)."""
    descs = []
    k = 0
    for rows, cols in COPY_SHAPES:
        for transpose in (0, 1):
            for bf16 in (0, 1):
                nat = rows if transpose else cols
                ldd = nat + (0, 4, 3, 0, 8, 1)[k % 6]
                dst_off = ((0, 2, 4, 8, 0, 0) if bf16 else (0, 4, 0, 8, 4, 0))[(k // 2) % 6]
                descs.append(dict(rows=rows, cols=cols, transpose=transpose, bf16=bf16, ldd=ldd, src_off=1 if k % 5 == 3 else 0, dst_off=dst_off))
                k += 1
    # the three aligned fast paths must be reachable: give the aligned shapes one descriptor each with nothing odd
    for rows, cols, transpose, bf16 in ((64, 64, 0, 1), (64, 64, 1, 0), (40, 98, 1, 1), (130, 96, 0, 0), (1, 768, 0, 1)):
        descs.append(dict(rows=rows, cols=cols, transpose=transpose, bf16=bf16, ldd=(rows if transpose else cols) + 4, src_off=0, dst_off=0))
    at = [0, 0]
    for d in descs:
        esz = 2 if d["bf16"] else 4
        extent = ((d["cols"] if d["transpose"] else d["rows"]) - 1) * d["ldd"] + (d["rows"] if d["transpose"] else d["cols"])
        start = (at[d["bf16"]] + 15) // 16 * 16 + 16       # a 16-element gap, then the next 16-element (>= 32-byte) boundary
        d["at"] = start + d["dst_off"] // esz
        at[d["bf16"]] = d["at"] + extent
    return descs, at[0] + 32, at[1] + 32


def copy_tiles(descs):
    """tile_desc / tile_index as hero_amd.functional._refresh_tables lists them: 64 x 64 tiles, row-major inside a tensor.
    (That helper itself only lays tensors back to back at their natural width, so it cannot build this table.)"""
    tdesc, tidx = [], []
    for i, d in enumerate(descs):
        nt = (-(-d["rows"] // 64)) * (-(-d["cols"] // 64))
        tdesc += [i] * nt
        tidx += list(range(nt))
    return tdesc, tidx


def copy_paths(d):
    """The alignment facts of one descriptor that decide how its elements are stored (16-byte alignment of both ends, widths
    that are multiples of 4)."""
    src_al = d["src_off"] % 4 == 0
    dst_al = d["dst_off"] % 16 == 0
    return dict(src_aligned=src_al, dst_aligned=dst_al, cols4=d["cols"] % 4 == 0, rows4=d["rows"] % 4 == 0, ldd4=d["ldd"] % 4 == 0)


# ---- collate ------------------------------------------------------------------------------------------------------------------------
def collate_subs_ref(sub_nfrm, sub_ntok, max_vl, out_size):
    """get_gather_index + the frame-level attention mask: a row has `eff` frame slots (its frames, or ONE masked zero slot if
    it has none) and then its tokens; gather_index sends token t to max_vl + t and every other position to itself."""
    nf, nt = np.asarray(sub_nfrm, dtype=np.int64)[:, None], np.asarray(sub_ntok, dtype=np.int64)[:, None]
    p = np.arange(out_size, dtype=np.int64)[None, :]
    eff = np.where(nf > 0, nf, 1)
    token = (p >= eff) & (p < eff + nt)
    gidx = np.where(token, max_vl + (p - eff), p)
    mask = ((p < eff + nt) & ((nf > 0) | (p >= 1))).astype(np.int64)
    return gidx, mask


def random_videos(B, NF, seed):
    """B videos of NF frames, six subtitles each with 0 - 4 frames drawn from [0, NF + 3) (some past the clip) and 1 - 8 tokens."""
    rs = np.random.RandomState(seed)
    return [(NF, [(rs.randint(0, NF + 3, size=rs.randint(0, 5)).tolist(), int(rs.randint(1, 9))) for _ in range(6)]) for _ in range(B)]


def lengths_of(videos):
    """The six int32 arrays the device collate reads, from `videos` = [(n_frames, [(frame list, n_tokens)])]: sub_nfrm counts the
    frames INSIDE the clipped video (what the mask sees), sub_frm lists all of them (what the frame map sees)."""
    i32 = lambda a: np.asarray(a, dtype=np.int32)          # noqa: E731
    subs = [(nf, fr, nt) for nf, rows in videos for fr, nt in rows]
    frm = [f for _, fr, _ in subs for f in fr]
    return {"sub_nfrm": i32([sum(1 for f in fr if 0 <= f < nf) for nf, fr, _ in subs]), "sub_ntok": i32([nt for _, _, nt in subs]),
            "sub_frm_off": i32(np.concatenate([[0], np.cumsum([len(fr) for _, fr, _ in subs])])), "sub_frm": i32(frm if frm else [0]),
            "vid_sub_off": i32(np.concatenate([[0], np.cumsum([len(rows) for _, rows in videos])])), "vid_nfrm": i32([nf for nf, _ in videos])}


def clip_mask_ref(vid_nfrm, NF):
    return np.asarray([[1 if f < n else 0 for f in range(NF)] for n in vid_nfrm], dtype=np.int64)


def frame_map_ref(vid_sub_off, sub_frm_off, sub_frm, B, NF, Lf):
    """counts [B * NF], offsets [B * NF + 1] (exclusive scan), entries (flat source rows subtitle row * Lf + slot, per
    frame in subtitle / slot order), writes {source row: output frame} of `inverse`.  Frames outside [0, NF) match nothing."""
    per = [[] for _ in range(B * NF)]
    writes = {}
    for b in range(B):
        for s in range(vid_sub_off[b], vid_sub_off[b + 1]):
            for slot, j in enumerate(range(sub_frm_off[s], sub_frm_off[s + 1])):
                f = int(sub_frm[j])
                if 0 <= f < NF:
                    per[b * NF + f].append(s * Lf + slot)
                    writes[s * Lf + slot] = b * NF + f
    counts = np.asarray([len(p) for p in per], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    entries = np.asarray([e for p in per for e in p], dtype=np.int32)
    return counts, offsets, entries, writes


def row_video_ref(vid_sub_off):
    return np.asarray([b for b in range(len(vid_sub_off) - 1) for _ in range(vid_sub_off[b], vid_sub_off[b + 1])], dtype=np.int32)


def gather_feats_ref(c_feats, vid_sub_off, vid_nfrm, sub_frm_off, sub_frm, max_vl):
    """f_v_feats[r, k] = c_v_feats[video(r), k-th frame of row r that lies inside [0, vid_nfrm[video(r)])], zero rows after
    the kept frames (and for kept frames past the padded clip length NF)."""
    B, NF, D = c_feats.shape
    row_vid = row_video_ref(vid_sub_off)
    out = np.zeros((len(row_vid), max_vl, D), dtype=np.float32)
    for r, b in enumerate(row_vid):
        keep = [int(f) for f in sub_frm[sub_frm_off[r]:sub_frm_off[r + 1]] if 0 <= f < vid_nfrm[b]]
        for k, f in enumerate(keep[:max_vl]):
            if f < NF:
                out[r, k] = c_feats[b, f]
    return out, row_vid


DERIVE_MASK_ADD, DERIVE_F32, DERIVE_I32, DERIVE_FLAT_GATHER = 0, 1, 2, 3


def derive_ref(mode, x, p0=0, p1=0, p2=0):
    """MASK_ADD: (1 - x) * -10000 in float32; F32 / I32: the cast; FLAT_GATHER (x [rows, p0] flattened, p1 = max_vl, p2 =
    max_sl): position p of a row names frame slot x (x < p1: image row row * p1 + x >= 0) or token x - p1 (text row
    row * p2 + x - p1, stored as -(that) - 2)."""
    x = np.asarray(x, dtype=np.int64)
    if mode == DERIVE_MASK_ADD:
        return (np.float32(1.0) - x.astype(np.float32)) * np.float32(-10000.0)
    if mode == DERIVE_F32:
        return x.astype(np.float32)
    if mode == DERIVE_I32:
        return x.astype(np.int32)
    row = np.arange(len(x), dtype=np.int64) // p0
    return np.where(x < p1, row * p1 + x, -(row * p2 + (x - p1)) - 2).astype(np.int32)


# ---- collate cases: python lists in the form hero_amd.collate.video_item takes ----------------------------------------------------
def collate_lists():
    """videos = [(n_frames, [(frame list, n_tokens incl. SEP)])]: subtitles without frames, with max_vl (= 5) frames, with one
    token and with max_sl (= 9) tokens; a video without subtitles; frame 2 of video 0 named by three subtitles; frame 4 twice in
    one subtitle; frames outside their clipped video (video 1: 3 frames; its subtitles name 3, 7 and 40 as well)."""
    return [
        (6, [([0, 1, 2], 4), ([2], 1), ([], 9), ([2, 3, 4, 4, 5], 2), ([], 1)]),
        (3, [([1, 3, 2], 3), ([7, 0, 40, 1], 5), ([3], 2)]),
        (4, []),
        (1, [([0], 9)]),
    ]
