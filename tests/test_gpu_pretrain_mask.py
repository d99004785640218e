"""The device draw of the pre-training batches (hero_amd/csrc/pretrain_mask.hip through hero_amd.pretrain_data.PretrainMasker)
against its integer statement tests/pretrain_mask_reference.py: EVERY output of every kernel must be torch.equal to the
statement - own seed words (one above 2^32), explicit sites - at the smallest shapes at which the kernels can still go wrong:
more than one wavefront of columns / frames (70), rows with only the leading token, zero-frame rows, a one-frame video, frame
lists that run past the clip, probabilities 0, 0.02 (the at-least-one rules), 0.15 and 1 (count == capacity), both feature
widths (12 floats: three 16-byte segments; 4352: the bench width, 17 passes of a wavefront)."""
import numpy as np
import pytest
import torch

from tests import pretrain_mask_reference as R
from tests.util import load_tiny

pytestmark = pytest.mark.gpu

MASK_ID, V_RANGE, CLS = 4, (5, 128), 0
SITES = {"mlm": 11, "mfm": (1 << 33) + 5, "fom": 0x464F4D}
SEEDS = (7, (1 << 32) + 12345, 0xF123456789ABCDEF)


def _host_batch(subs, n_frames, D, seed=0):
    from hero_amd import synth
    return synth.video_batch(subs, n_frames, D, 128, torch.Generator().manual_seed(seed))


def _device(host):
    from hero_amd import synth
    dev = synth.to_device({k: v for k, v in host.items() if k != "lengths"}, "cuda")
    ln = {k: torch.as_tensor(v, dtype=torch.int32).cuda() for k, v in host["lengths"].items()}
    return dev, ln


def _masker(host, probs, seed):
    from hero_amd.pretrain_data import PretrainMasker
    m = PretrainMasker.for_batch(host, "cuda", MASK_ID, V_RANGE, CLS, mlm_prob=probs, mfm_prob=probs, fom_prob=probs, sites=SITES)
    return m.set_seed(seed)


# 9 rows, 70 token columns: a full row, a zero-frame row, a row with only the leading token, short rows (video 0: 5 rows, video 1: 4)
MLM_SUBS = [[([0, 1], 70), ([], 5), ([2], 1), ([3, 4, 5], 2), ([], 1)],
            [([0], 33), ([1, 2], 65), ([], 70), ([3], 7)]]
MLM_FRAMES = [8, 6]


def _check_mlm(host, m, st):
    cap = m.cap
    n = st["count"]
    assert int(m.counts[0]) == n
    assert torch.equal(m.input_ids.cpu(), torch.from_numpy(st["input_ids"]))
    assert torch.equal(m.txt_mask_tgt.cpu(), torch.from_numpy(st["txt_mask_tgt"]))
    labels = np.full(cap, -1, dtype=np.int64)
    labels[:n] = st["txt_labels"]
    rows = np.full(cap, -1, dtype=np.int32)
    rows[:n] = st["txt_mask_rows"]
    assert torch.equal(m.txt_labels[:cap].cpu(), torch.from_numpy(labels))
    assert torch.equal(m.txt_mask_rows[:cap].cpu(), torch.from_numpy(rows))
    # compaction order == torch.nonzero order
    assert torch.equal(m.txt_mask_rows[:n].long().cpu(), torch.nonzero(m.txt_mask_tgt.reshape(-1)).reshape(-1).cpu())


@pytest.mark.parametrize("p", [0.15, 0.02, 0.0, 1.0])
def test_mlm_mask_equals_the_statement(p):
    host = _host_batch(MLM_SUBS, MLM_FRAMES, 12)
    assert tuple(host["f_sub_input_ids"].shape) == (9, 70)
    dev, ln = _device(host)
    clean = dev["f_sub_input_ids"].clone()
    Lf = host["f_attn_masks"].shape[1]
    seen = []
    for seed in SEEDS:
        m = _masker(host, p, seed).draw(dev, ln, tasks=("mlm",))
        st = R.mlm_mask(host["f_sub_input_ids"].numpy(), host["lengths"]["sub_nfrm"], host["lengths"]["sub_ntok"], Lf, seed, SITES["mlm"],
                        R.threshold(p), MASK_ID, V_RANGE, CLS)
        _check_mlm(host, m, st)
        seen.append(st)
        b = m.mlm_batch()
        assert set(b) == {"input_ids", "position_ids", "v_feat", "attn_masks", "gather_index", "txt_mask_tgt", "txt_labels"}
        assert b["txt_labels"].shape == (st["count"],) and b["txt_mask_tgt"].dtype == torch.bool
    assert torch.equal(dev["f_sub_input_ids"], clean)                              # the clean batch stays clean
    if p == 0.02:
        assert any((s["kind"] == 4).any() for s in seen)                            # some row needs the at-least-one rule
    if p == 0.15:
        assert any((s["kind"] == 2).any() for s in seen) and any((s["kind"] == 3).any() for s in seen)
        assert not np.array_equal(seen[0]["sel"], seen[1]["sel"])
    if p == 1.0:
        assert all(s["count"] == int((host["lengths"]["sub_ntok"] - 1).sum()) for s in seen)


def test_mlm_mask_fills_its_capacity_when_every_token_is_selected():
    host = _host_batch([[([0], 70)] * 5, [([1, 2], 70)] * 4], [4, 4], 12)
    dev, ln = _device(host)
    m = _masker(host, 1.0, SEEDS[1]).draw(dev, ln, tasks=("mlm",))
    st = R.mlm_mask(host["f_sub_input_ids"].numpy(), host["lengths"]["sub_nfrm"], host["lengths"]["sub_ntok"], host["f_attn_masks"].shape[1],
                    SEEDS[1], SITES["mlm"], R.threshold(1.0), MASK_ID, V_RANGE, CLS)
    assert st["count"] == m.cap == 9 * 69
    _check_mlm(host, m, st)


# B = 3, NF = 70: a 70-frame video, a one-frame video, a 9-frame video with a subtitle whose frame list runs past the clip
MFM_SUBS = [[(list(range(0, 3)), 4), ([], 3), (list(range(3, 68)), 2), ([69], 2)],
            [([0], 3), ([], 2)],
            [([0, 1], 3), ([7, 8, 9, 10], 5), ([2, 30], 2)]]
MFM_FRAMES = [70, 1, 9]


@pytest.mark.parametrize("D, p", [(12, 0.15), (12, 0.02), (12, 0.0), (12, 1.0), (4352, 0.15)])
def test_mfm_mask_equals_the_statement(D, p):
    host = _host_batch(MFM_SUBS, MFM_FRAMES, D)
    T, max_vl = host["f_v_feats"].shape[:2]
    assert host["c_v_feats"].shape == (3, 70, D) and max_vl == 65
    dev, ln = _device(host)
    clean_c, clean_f = dev["c_v_feats"].clone(), dev["f_v_feats"].clone()
    forced_seen = False
    for seed in SEEDS:
        m = _masker(host, p, seed).draw(dev, ln, tasks=("mfm",))
        st = R.mfm_mask(host["lengths"], T, max_vl, 70, seed, SITES["mfm"], R.threshold(p))
        forced_seen |= bool((st["forced"] >= 0).any())
        c, f = torch.from_numpy(st["c_v_masks"]), torch.from_numpy(st["f_v_masks"])
        n = st["count"]
        assert int(m.counts[1]) == n and (p > 0 or n == 3) and (p < 1 or n == 80)
        assert torch.equal(m.c_v_masks.cpu(), c) and torch.equal(m.f_v_masks.cpu(), f)
        assert torch.equal(m.c_v_feats.cpu(), host["c_v_feats"].masked_fill(c.unsqueeze(-1), 0))
        assert torch.equal(m.f_v_feats.cpu(), host["f_v_feats"].masked_fill(f.unsqueeze(-1), 0))
        want = torch.zeros(3 * 70, D)
        want[:n] = host["c_v_feats"][c]
        assert torch.equal(m.feat_targets.cpu(), want)                              # compact in (b, f) order, zero rows behind the count
        b = m.mfm_batch()
        assert b["feat_targets"].shape == (n, D) and set(b) == set(dev) | {"f_v_masks", "c_v_masks", "feat_targets"}
    assert torch.equal(dev["c_v_feats"], clean_c) and torch.equal(dev["f_v_feats"], clean_f)      # bitwise unchanged
    if p == 0.02:
        assert forced_seen                                                          # a video with no selection of its own


@pytest.mark.parametrize("p", [1.0, 0.15, 0.5, 0.0])
def test_fom_shuffle_equals_the_statement(p):
    from hero_amd.pretrain_data import PretrainMasker
    vn = np.array([70, 1, 2, 0, 66, 33], dtype=np.int32)          # p = 1: more than 64, 1, 2 and 0 selected frames
    B, NF = len(vn), 70
    ln = {"vid_nfrm": torch.from_numpy(vn).cuda(), "vid_sub_off": torch.arange(B + 1, dtype=torch.int32).cuda(),
          "sub_frm_off": torch.zeros(B + 1, dtype=torch.int32).cuda(), "sub_frm": torch.zeros(1, dtype=torch.int32).cuda(),
          "sub_nfrm": torch.zeros(B, dtype=torch.int32).cuda(), "sub_ntok": torch.ones(B, dtype=torch.int32).cuda()}
    m = PretrainMasker(B, 2, 1, 3, B, NF, 4, "cuda", MASK_ID, V_RANGE, CLS, fom_prob=p, sites=SITES)
    got = []
    for seed in SEEDS:
        m.set_seed(seed).draw({}, ln, tasks=("fom",))
        orders, targets = R.fom_shuffle(vn, NF, seed, SITES["fom"], R.threshold(p))
        assert torch.equal(m.shuffled_orders.cpu(), torch.from_numpy(orders)) and torch.equal(m.targets.cpu(), torch.from_numpy(targets))
        pad = torch.arange(NF)[None, :] >= torch.from_numpy(vn.astype(np.int64))[:, None]
        assert (m.targets.cpu()[pad] == -1).all() and (m.shuffled_orders.cpu()[pad] == torch.arange(NF).repeat(B, 1)[pad]).all()
        got.append(orders)
        if p == 1.0:
            assert (targets[0] != -1).sum() == 70 and (targets[1] != -1).sum() == 1 and (targets[2] != -1).sum() == 2 \
                and (targets[3] != -1).sum() == 0 and (targets[4] != -1).sum() == 66
    if p >= 0.15:
        assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


def _ragged_host(seed=3):
    """Two small ragged videos at the tiny golden model's widths (vfeat 96, vocabulary 160)."""
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=gen))     # noqa: E731
    subs, n_frames = [], []
    for v in range(2):
        nf, cur, f0 = ri(18, 30), [], 0
        for _ in range(ri(4, 7)):
            fr = list(range(f0, min(f0 + ri(0, 4), nf)))
            f0 += len(fr)
            cur.append((fr, ri(2, 9)))
        subs.append(cur)
        n_frames.append(nf)
    return _host_batch(subs, n_frames, 96, seed)


def _statement_batches(host, dev, seed, p):
    """The three task batches assembled on the HOST from the statement's masks."""
    T, max_vl = host["f_v_feats"].shape[:2]
    NF = host["c_v_feats"].shape[1]
    ln = host["lengths"]
    s = R.mlm_mask(host["f_sub_input_ids"].numpy(), ln["sub_nfrm"], ln["sub_ntok"], host["f_attn_masks"].shape[1], seed, SITES["mlm"],
                   R.threshold(p), MASK_ID, V_RANGE, CLS)
    mlm = {"input_ids": torch.from_numpy(s["input_ids"]).cuda(), "position_ids": dev["f_sub_pos_ids"], "v_feat": dev["f_v_feats"],
           "attn_masks": dev["f_attn_masks"], "gather_index": dev["f_gather_index"],
           "txt_mask_tgt": torch.from_numpy(s["txt_mask_tgt"]).cuda(), "txt_labels": torch.from_numpy(s["txt_labels"]).cuda()}
    s = R.mfm_mask(ln, T, max_vl, NF, seed, SITES["mfm"], R.threshold(p))
    c, f = torch.from_numpy(s["c_v_masks"]), torch.from_numpy(s["f_v_masks"])
    mfm = dict(dev)
    mfm.update(f_v_feats=host["f_v_feats"].masked_fill(f.unsqueeze(-1), 0).cuda(), c_v_feats=host["c_v_feats"].masked_fill(c.unsqueeze(-1), 0).cuda(),
               f_v_masks=f.cuda(), c_v_masks=c.cuda(), feat_targets=host["c_v_feats"][c].cuda())
    orders, targets = R.fom_shuffle(ln["vid_nfrm"], NF, seed, SITES["fom"], R.threshold(p))
    fom = dict(dev)
    fom.update(shuffled_orders=torch.from_numpy(orders).cuda(), targets=torch.from_numpy(targets).cuda())
    return {"mlm": mlm, "mfm-nce": mfm, "fom": fom}


def test_captured_draw_replays_under_other_seed_words():
    """draw() for the three tasks under torch.cuda.graph ONCE; every replay equals the statement for the seed word that is on the
    device at that moment, and the draws of different seeds differ."""
    host = _ragged_host()
    dev, ln = _device(host)
    T, max_vl = host["f_v_feats"].shape[:2]
    NF, Lf = host["c_v_feats"].shape[1], host["f_attn_masks"].shape[1]
    p = 0.3
    m = _masker(host, p, 1).draw(dev, ln)                      # eager once: the library is loaded before the capture
    torch.cuda.synchronize()
    gs = torch.cuda.Stream()
    gs.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(gs):
        with torch.cuda.graph(graph, stream=gs):
            m.draw(dev, ln)
    torch.cuda.current_stream().wait_stream(gs)
    outs = []
    for seed in SEEDS:
        m.set_seed(seed)
        graph.replay()
        m.note_replay()
        torch.cuda.synchronize()
        s = R.mlm_mask(host["f_sub_input_ids"].numpy(), host["lengths"]["sub_nfrm"], host["lengths"]["sub_ntok"], Lf, seed, SITES["mlm"],
                       R.threshold(p), MASK_ID, V_RANGE, CLS)
        _check_mlm(host, m, s)
        f = R.mfm_mask(host["lengths"], T, max_vl, NF, seed, SITES["mfm"], R.threshold(p))
        c = torch.from_numpy(f["c_v_masks"])
        assert torch.equal(m.c_v_masks.cpu(), c) and torch.equal(m.f_v_masks.cpu(), torch.from_numpy(f["f_v_masks"]))
        assert torch.equal(m.c_v_feats.cpu(), host["c_v_feats"].masked_fill(c.unsqueeze(-1), 0))
        assert torch.equal(m.feat_targets[:f["count"]].cpu(), host["c_v_feats"][c]) and not m.feat_targets[f["count"]:].any()
        orders, targets = R.fom_shuffle(host["lengths"]["vid_nfrm"], NF, seed, SITES["fom"], R.threshold(p))
        assert torch.equal(m.shuffled_orders.cpu(), torch.from_numpy(orders)) and torch.equal(m.targets.cpu(), torch.from_numpy(targets))
        assert m._counts() == [s["count"], f["count"]]
        outs.append((s["sel"], f["c_v_masks"], orders))
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert all(not np.array_equal(x, y) for x, y in zip(outs[a], outs[b]))
    # advance() is a device op on the seed word: the statement's step
    m.set_seed(SEEDS[2]).advance()
    assert int(m.seed.item()) & ((1 << 64) - 1) == R.advance(SEEDS[2])


def test_model_on_masker_batches_equals_model_on_statement_batches_and_trains():
    """The tiny golden model, dropout off: model(batch, task) on the masker's batches == the same call on batches assembled on the
    host from the statement's masks, bit for bit; then one eager TrainStep micro-step per task gives a finite loss."""
    import hero_amd
    from hero_amd import functional as HF
    from hero_amd.model import HeroForPretraining
    from hero_amd.step import TrainStep
    from hero_amd.utils.misc import set_dropout
    hero_amd.set_compute_dtype(torch.float32)
    HF.set_grad_sink(None)
    HF.clear_weight_cache()
    model, _, _ = load_tiny("cuda", cls=HeroForPretraining)
    model.train()
    set_dropout(model, 0.0)
    host = _ragged_host()
    dev, ln = _device(host)
    seed, p = SEEDS[1], 0.2
    m = _masker(host, p, seed).draw(dev, ln)
    mine = {"mlm": m.mlm_batch(), "mfm-nce": m.mfm_batch(), "fom": m.fom_batch()}
    want = _statement_batches(host, dev, seed, p)
    # the pair keys of the reference's fom_collate (data/fom.py:64-92), restated as its loops over the statement's targets
    t, NF, idx, binary = want["fom"]["targets"].cpu().numpy(), host["c_v_feats"].shape[1], [], []
    for b in range(t.shape[0]):
        pos = np.flatnonzero(t[b] != -1)
        for x in range(len(pos)):
            for y in range(x + 1, len(pos)):
                i, j = int(pos[x]), int(pos[y])
                idx += [b * NF + i, b * NF + j, b * NF + j, b * NF + i]
                binary += [int(t[b, i] <= t[b, j]), int(t[b, j] <= t[b, i])]
    assert len(binary) >= 2
    assert mine["fom"]["reordered_frame_idx"].tolist() == idx and mine["fom"]["binary_targets"].tolist() == binary
    for task in ("mlm", "mfm-nce", "fom"):
        got = model(mine[task], task=task, compute_loss=True)
        ref = model(want[task], task=task, compute_loss=True)
        assert got.shape == ref.shape and torch.isfinite(ref).all()
        assert torch.equal(got, ref), task
    ts = TrainStep(model, opts=dict(learning_rate=1e-4, warmup_steps=2, num_train_steps=100), task="mlm")
    for task in ("mlm", "mfm-nce", "fom"):
        m.advance().draw(dev, ln)
        batch = {"mlm": m.mlm_batch, "mfm-nce": m.mfm_batch, "fom": m.fom_batch}[task]()
        loss = ts.micro_step(batch, task=task)
        assert torch.isfinite(loss).all(), task
    # every draw dropped what the models had memoised from the previous masks (row lists of another length): a refresh of
    # the whole memo table, as a feeder's commit runs it, finds only entries that still fit
    HF.refresh_memo()
    torch.cuda.synchronize()
    HF.reset_caches()
