"""tests/rows_reference.py, the host statements that tests/test_gpu_rows_kernels.py and tests/test_gpu_collate_kernels.py judge
against, held against what they restate - torch's stable sort, index_add_, .to(torch.bfloat16), the mask arithmetic, and the
project's own host builders (functional.host_segment_order, collate.video_collate, model.build_frame_map, the flat gather index
of model/encoder.py) - and the properties that make the GPU comparisons exact: integer sums that every accumulator holds, and
constructed id lists that contain every block-boundary situation of hero_scatter_add_sorted."""
import numpy as np
import pytest
import torch

from tests import rows_reference as R


# ---- segment order -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dst", R.SORT_NDST)
def test_segment_order_is_the_stable_sort_of_the_composed_key_and_the_feeders_host_order(n_dst):
    from hero_amd.functional import host_segment_order
    for k, (rows, skip, pattern) in enumerate(R.sort_cases(n_dst)):
        if rows > 2049:
            continue                                                  # the plain-loop statement is the slow side; 9601 runs on the GPU test
        idx = R.sort_ids(rows, n_dst, skip, pattern, seed=100 + k)
        want = R.segment_order_ref(idx, skip)
        v = torch.from_numpy(idx).long()
        key = torch.where((v < 0) | (v == skip), torch.full_like(v, 1 << 40), v)
        assert np.array_equal(want, torch.sort(key, stable=True)[1].int().numpy()), (rows, skip, pattern)
        assert np.array_equal(want, host_segment_order(idx, skip)), (rows, skip, pattern)
        assert idx.min() >= -1 and idx.max() < n_dst
        if rows >= 5 and pattern in ("random", "sorted", "reverse"):
            assert (idx == -1).any() and (idx == 0).any() and (idx == n_dst - 1).any()        # dropped rows AND id 0 AND the top id


def test_sort_cases_reach_every_pass_count_and_every_row_count():
    assert {R.sort_passes(n) for n in R.SORT_NDST} == set(range(1, 9))
    assert R.sort_passes(2 ** 28) == 8 and R.sort_passes(2 ** 28 - 1) == 7 and R.sort_passes(15) == 1 and R.sort_passes(16) == 2
    for n_dst in R.SORT_NDST:
        cases = R.sort_cases(n_dst)
        assert {c[0] for c in cases} == set(R.SORT_ROWS)
        assert {c[1] for c in cases} == {-1, 0, n_dst - 1}
        assert {c[2] for c in cases} == {"random", "all_dropped", "one_id", "sorted", "reverse"}


# ---- scatter-add -----------------------------------------------------------------------------------------------------------------
def test_scatter_add_is_index_add_in_float64():
    rs = np.random.RandomState(1)
    src = rs.randn(300, 6)
    idx = rs.randint(-12, 20, size=300).astype(np.int32)
    a0, b0 = rs.randn(20, 6), rs.randn(11, 6)
    for skip, with_b in ((-1, True), (5, True), (5, False)):
        da, db = R.scatter_add_ref(src, idx, a0, b0 if with_b else None, skip)
        li = torch.from_numpy(idx).long()
        ka = (li >= 0) & (li != skip)
        ta = torch.from_numpy(a0).clone().index_add_(0, li[ka], torch.from_numpy(src)[ka])
        assert np.allclose(da, ta.numpy(), rtol=0, atol=1e-12)
        if with_b:
            tb = torch.from_numpy(b0).clone().index_add_(0, (-li - 2)[li <= -2], torch.from_numpy(src)[li <= -2])
            assert np.allclose(db, tb.numpy(), rtol=0, atol=1e-12)
        else:
            assert db is None
    keep = (idx >= 0) & (idx != 5)
    t = torch.from_numpy(a0).clone().index_add_(0, torch.from_numpy(idx[keep]).long(), torch.from_numpy(src[keep]))
    assert np.allclose(R.scatter_sorted_ref(src, idx, a0, 5), t.numpy(), rtol=0, atol=1e-12)


def test_scatter_rows_cases_are_exact_by_construction():
    for sd, dd in R.SCATTER_COMBOS:
        for cols in R.SCATTER_COLS:
            for skip in (-1, 3):
                c = R.scatter_rows_case(cols, skip)
                nz, mag = R.scatter_counts(c["src"], c["idx"], c["n_a"], c["n_b"], skip)
                assert nz[0][c["hot"]].min() >= 100 and (c["idx"] == c["hot"]).sum() == 250          # the contended destination
                assert (c["idx"] <= -2).any() and (c["idx"] == -1).any() and (skip < 0 or (c["idx"] == skip).any())
                assert (np.abs(c["src"]).reshape(len(c["src"]), -1, 2).sum(2) == 0).any()   # all-zero source pairs
                assert (c["a0"] != 0).all() and (c["b0"] != 0).all()
                for t, d0 in enumerate((c["a0"], c["b0"])):
                    assert R.exact_f32(d0, mag[t])
                    if dd == "bf16":
                        assert R.exact_bf16(c["src"], d0, nz[t])


def test_exactness_conditions_reject_what_they_should():
    one = np.ones((300, 2), dtype=np.float32)
    idx = np.zeros(300, dtype=np.int32)
    nz, mag = R.scatter_counts(one, idx, 1, 0, -1)
    assert not R.exact_bf16(one, np.zeros((1, 2)), nz[0]) and R.exact_f32(np.zeros((1, 2)), mag[0])
    assert not R.exact_bf16(one[:256] * 2, np.zeros((1, 2)), nz[0] * 0) and not R.exact_f32(np.full((1, 2), 2.0 ** 24), mag[0])
    assert torch.tensor(256.0).bfloat16().item() == 256.0 and torch.tensor(257.0).bfloat16().item() != 257.0


# ---- scatter-sorted: the constructed id lists ----------------------------------------------------------------------------------------
def test_sorted_cases_contain_every_boundary_situation():
    seen = {}
    for c in R.sorted_cases():
        for s in R.situations(c["idx"], c["skip"]):
            seen.setdefault(s, []).append(c["name"])
        assert c["idx"].max() < c["n_dst"] and len(c["idx"]) == sum(c["runs"]) + c["tail"]
    assert set(seen) == set(R.SITUATIONS), sorted(set(R.SITUATIONS) - set(seen))
    main = R.situations(R.sorted_cases()[0]["idx"], R.SKIP_ID)
    assert main >= set(R.SITUATIONS) - {"multi_block_run_ends_list", "all_rows_dropped", "rows_1", "rows_15", "rows_16", "rows_17"}
    # the detector reads the list, not the builder: a list without crossings shows none
    plain = np.repeat(np.arange(7, dtype=np.int32) * 2, 2)
    assert R.situations(plain, -1) == set()
    assert R.situations(np.zeros(16 * 66, dtype=np.int32), -1) >= {"spans_66_blocks", "whole_first_block", "whole_middle_block", "multi_block_run_ends_list"}


def test_sorted_cases_are_exact_and_leave_table_rows_unnamed():
    for c in R.sorted_cases():
        rows = len(c["idx"])
        src = R.int_rows(rows, 8, seed=rows)
        tab = R.int_table(c["n_dst"], 8)
        assert (tab != 0).all() and np.abs(tab).max() <= 3 and np.abs(src).max() <= 3
        _, mag = R.scatter_counts(src, np.where(c["idx"] == c["skip"], -1, c["idx"]), c["n_dst"], 0, -1)
        assert R.exact_f32(tab, mag[0])
        named = set(int(v) for v in c["idx"] if v >= 0 and v != c["skip"])
        assert c["skip"] not in named and len(named) < c["n_dst"] - 1            # the skip row and some others stay as they are
        if c["runs"]:
            assert 0 in named                                                     # table row 0: also what dropped rows would hit


# ---- casts and copies -----------------------------------------------------------------------------------------------------------------
def test_bf16_round_is_torch_to_bfloat16():
    rs = np.random.RandomState(3)
    x = np.concatenate([rs.randn(5000).astype(np.float32) * 10.0 ** rs.randint(-20, 20, 5000),
                        np.float32([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 256.0, 257.0, 3.3895314e38, 1e-40])]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(R.bf16_round(x).view(np.uint32), want.view(np.uint32))


def test_copy_table_reaches_every_store_path_and_write_sets_are_disjoint():
    descs, n32, n16 = R.copy_table()
    assert {(d["rows"], d["cols"]) for d in descs} == set(R.COPY_SHAPES)
    for shape in R.COPY_SHAPES:
        assert {(d["transpose"], d["bf16"]) for d in descs if (d["rows"], d["cols"]) == shape} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {d["dst_off"] for d in descs if d["bf16"]} >= {0, 2, 4, 8} and any(d["src_off"] == 1 for d in descs)
    nat = lambda d: d["rows"] if d["transpose"] else d["cols"]            # noqa: E731
    assert any(d["ldd"] == nat(d) for d in descs) and any(d["ldd"] > nat(d) and d["ldd"] % 4 for d in descs)
    paths = [(d["transpose"], d["bf16"], R.copy_paths(d)) for d in descs]
    for bf16 in (0, 1):
        # plain: the 16-byte path, and the element path for each single reason
        assert any(t == 0 and b == bf16 and all(p[k] for k in ("src_aligned", "dst_aligned", "cols4", "ldd4")) for t, b, p in paths)
        for why in ("src_aligned", "dst_aligned", "cols4", "ldd4"):
            assert any(t == 0 and b == bf16 and not p[why] for t, b, p in paths), (bf16, why)
        # transposed: wide and narrow loads, wide and narrow stores
        assert any(t == 1 and b == bf16 and p["src_aligned"] and p["cols4"] for t, b, p in paths)
        assert any(t == 1 and b == bf16 and not p["cols4"] for t, b, p in paths)
        assert any(t == 1 and b == bf16 and p["dst_aligned"] and p["rows4"] and p["ldd4"] for t, b, p in paths)
        for why in ("dst_aligned", "rows4", "ldd4"):
            assert any(t == 1 and b == bf16 and not p[why] for t, b, p in paths), (bf16, why)
    for bf16, n in ((0, n32), (1, n16)):
        hit = np.zeros(n, dtype=np.int32)
        for d in descs:
            if d["bf16"] == bf16:
                ws = d["at"] + R.copy_write_set(d["rows"], d["cols"], d["ldd"], d["transpose"])
                assert len(np.unique(ws)) == d["rows"] * d["cols"] and ws.min() >= 16 and ws.max() < n - 16
                hit[ws] += 1
        assert hit.max() == 1 and (hit == 0).sum() > 16 * len(descs) // 2         # no overlap; gaps and padding to watch
    tdesc, tidx = R.copy_tiles(descs)
    assert len(tdesc) == sum(-(-d["rows"] // 64) * -(-d["cols"] // 64) for d in descs) and tidx[tdesc.index(8)] == 0


def test_copy_apply_is_to_dtype_of_the_source_or_its_transpose():
    rs = np.random.RandomState(4)
    src = rs.randn(7, 5).astype(np.float32)
    for transpose, bf16, ldd in ((0, 0, 5), (0, 1, 8), (1, 0, 7), (1, 1, 10)):
        arena = np.full(200, -776.0, dtype=np.float32)
        R.copy_apply(arena, 16, src, ldd, transpose, bf16)
        t = torch.from_numpy(src.T.copy() if transpose else src).to(torch.bfloat16 if bf16 else torch.float32).float().numpy()
        got = arena[16:16 + t.shape[0] * ldd].reshape(t.shape[0], ldd)
        assert np.array_equal(got[:, :t.shape[1]], t) and (got[:, t.shape[1]:] == -776.0).all() and (arena[:16] == -776.0).all()


# ---- gathers -------------------------------------------------------------------------------------------------------------------------
def test_gather_csr_and_inverse_first_statements():
    rs = np.random.RandomState(5)
    a, b = rs.randn(9, 4), rs.randn(6, 4)
    idx = np.int32([0, 8, -1, -2, -7, 3, 3, -1, 8, -2])
    li = torch.from_numpy(idx).long()
    cat = torch.cat([torch.from_numpy(a), torch.from_numpy(b), torch.zeros(1, 4, dtype=torch.float64)])
    flat = torch.where(li >= 0, li, torch.where(li == -1, torch.tensor(15), 9 + (-li - 2)))
    assert np.array_equal(R.gather_ref(a, b, idx), cat[flat].numpy())
    inv = R.inverse_first_ref(idx, 9, 6)
    assert inv.tolist() == [0, -1, -1, 5, -1, -1, -1, -1, 1] + [3, -1, -1, -1, -1, 4]
    assert R.inverse_first_ref(np.int32([9, -8, 4, -9]), 9, 6).tolist() == [-1] * 4 + [2] + [-1] * 10     # ids past either table
    offs, ent = np.int32([0, 0, 1, 3, 3]), np.int32([2, 2, 5])
    out = R.csr_gather_sum_ref(a, offs, ent)
    assert np.array_equal(out, np.stack([np.zeros(4), a[2], a[2] + a[5], np.zeros(4)]))
    assert np.array_equal(R.csr_gather_sum_f32_in_order(a, offs, ent)[2], a[2].astype(np.float32) + a[5].astype(np.float32))


# ---- collate ---------------------------------------------------------------------------------------------------------------------------
def _host_batch(videos, D=4):
    from hero_amd.collate import video_collate, video_item
    gen = torch.Generator().manual_seed(6)
    items = []
    for nf, subs in videos:
        toks = [list(range(3, 3 + nt - 1)) for _, nt in subs]
        items.append(video_item(torch.randn(nf, D, generator=gen), [(sid, list(fr)) for sid, (fr, _) in enumerate(subs)], toks))
    return video_collate(items)


def test_collate_statements_equal_the_host_collate():
    videos = R.collate_lists()
    batch = _host_batch(videos)
    ln = batch["lengths"]
    mine = R.lengths_of(videos)
    assert set(mine) == set(ln) and all(np.array_equal(mine[k], ln[k]) and mine[k].dtype == ln[k].dtype for k in ln)
    big = R.random_videos(5, 60, seed=1)
    host = _host_batch(big)["lengths"]
    assert all(np.array_equal(R.lengths_of(big)[k], host[k]) for k in host) and max(f for _, subs in big for fr, _ in subs for f in fr) >= 60
    T, max_vl = batch["f_v_feats"].shape[:2]
    out_size = batch["f_attn_masks"].shape[1]
    assert max_vl == 5 and batch["f_sub_input_ids"].shape[1] == 9 and (ln["sub_nfrm"] == 0).any() and (ln["sub_ntok"] == 1).any()
    for width in (out_size, out_size + 3):                                        # a wider buffer: more padding columns, same rule
        gidx, mask = R.collate_subs_ref(ln["sub_nfrm"], ln["sub_ntok"], max_vl, width)
        assert np.array_equal(gidx[:, :out_size], batch["f_gather_index"].numpy()) and np.array_equal(mask[:, :out_size], batch["f_attn_masks"].numpy())
        assert np.array_equal(gidx[:, out_size:], np.tile(np.arange(out_size, width), (T, 1))) and (mask[:, out_size:] == 0).all()
    NF = batch["c_v_feats"].shape[1]
    assert np.array_equal(R.clip_mask_ref(ln["vid_nfrm"], NF), batch["c_attn_masks"].numpy())
    feats, row_vid = R.gather_feats_ref(batch["c_v_feats"].numpy(), ln["vid_sub_off"], ln["vid_nfrm"], ln["sub_frm_off"], ln["sub_frm"], max_vl)
    assert np.array_equal(feats, batch["f_v_feats"].numpy())                     # frames past the clipped video dropped, later ones shifted
    assert row_vid.tolist() == [0] * 5 + [1] * 3 + [3]
    assert any(f >= n for (n, subs) in videos for fr, _ in subs for f in fr)


def test_frame_map_statement_equals_build_frame_map_where_that_accepts_the_case():
    from hero_amd.model.model import build_frame_map
    videos = R.collate_lists()
    NF, Lf = 6, 14
    inside = [(nf, [([f for f in fr if f < NF], nt) for fr, nt in subs]) for nf, subs in videos]
    for vs, accepted in ((inside, True), (videos, False)):
        batch = _host_batch(vs)
        ln = batch["lengths"]
        counts, offsets, entries, writes = R.frame_map_ref(ln["vid_sub_off"], ln["sub_frm_off"], ln["sub_frm"], len(vs), NF, Lf)
        assert counts.max() == 3 and (counts[2 * NF:3 * NF] == 0).all()          # three subtitles name one frame; a video without subtitles
        if not accepted:
            with pytest.raises(IndexError):
                build_frame_map(batch["num_subs"], batch["sub_idx2frame_idx"], len(vs), NF, Lf, "cpu")
            assert counts.sum() == sum(1 for _, subs in vs for fr, _ in subs for f in fr if f < NF)
            continue
        o, e, inv = build_frame_map(batch["num_subs"], batch["sub_idx2frame_idx"], len(vs), NF, Lf, "cpu")
        assert np.array_equal(o.numpy(), offsets) and np.array_equal(e.numpy(), entries)
        want = np.full(len(inv), -1, dtype=np.int32)
        for s, d in writes.items():
            want[s] = d
        assert np.array_equal(inv.numpy(), want)


def test_derive_statements_equal_the_torch_expressions_they_replace():
    rs = np.random.RandomState(7)
    m = torch.from_numpy(rs.randint(0, 2, size=500))
    assert np.array_equal(R.derive_ref(R.DERIVE_MASK_ADD, m.numpy()), ((1.0 - m.to(torch.float32)) * -10000.0).numpy())
    x = torch.from_numpy(rs.randint(-2 ** 31, 2 ** 31, size=500))
    assert np.array_equal(R.derive_ref(R.DERIVE_F32, x.numpy()), x.to(torch.float32).numpy())
    assert np.array_equal(R.derive_ref(R.DERIVE_I32, x.numpy()), x.to(torch.int32).numpy())
    T, p0, max_vl, max_sl = 37, 14, 5, 9
    g = torch.from_numpy(rs.randint(0, max_vl + max_sl, size=(T, p0)))
    row = torch.arange(T).unsqueeze(1)
    flat = torch.where(g < max_vl, row * max_vl + g, -(row * max_sl + (g - max_vl)) - 2).reshape(-1).to(torch.int32)      # model/encoder.py
    got = R.derive_ref(R.DERIVE_FLAT_GATHER, g.reshape(-1).numpy(), p0, max_vl, max_sl)
    assert np.array_equal(got, flat.numpy()) and (got >= 0).any() and (got <= -2).any()
