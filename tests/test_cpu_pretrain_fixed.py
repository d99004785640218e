"""Host side of the fixed-capacity pre-training forms: the float64 statement of the counted
cross-entropy, the row capacities, the condition the GPU tests rely on (no overflow at their seeds and shapes), the partition
statement, and the C ABI additions."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from tests import pretrain_fixed_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hero_ce_counted_fwd", "hero_ce_counted_bwd", "hero_mask_partition", "hero_nce_pack_fwd", "hero_nce_pack_bwd")


@pytest.fixture(scope="module")
def built_lib():
    from hero_amd import build
    return build.build()


@pytest.mark.parametrize("count", [None, 0, 1, 9, 12])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_counted_cross_entropy_fallback_is_the_mean_over_the_live_rows(count, dtype):
    from hero_amd import functional as HF
    rows, cols, ld = 9, 37, 40
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(rows, ld, generator=g) * 3).to(dtype)
    y = torch.randint(0, cols, (rows,), generator=g)
    y[2], y[6] = -100, -100                                      # two ignored rows (one of them below every count >= 3)
    n = rows if count is None else min(count, rows)
    live = [r for r in range(n) if int(y[r]) != -100]
    x[n:] = float("nan")                                         # rows behind the count are never looked at
    x.requires_grad_(True)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32)
    got = HF.counted_cross_entropy(x, y, cnt, ncols=cols, inv_temp=0.5)
    assert got.dim() == 0 and got.dtype == torch.float32
    want = F.cross_entropy(x.detach()[live, :cols].double() * 0.5, y[live], reduction="sum") / max(len(live), 1) if live else torch.zeros((), dtype=torch.float64)
    assert abs(float(got.detach()) - float(want)) <= 2.0 ** -23 * max(abs(float(want)), 1.0)
    got.backward()
    dead = [r for r in range(rows) if r not in live]
    assert torch.equal(x.grad[dead], torch.zeros(len(dead), ld, dtype=dtype))          # exactly zero, NaN logits or not
    assert torch.equal(x.grad[:, cols:], torch.zeros(rows, ld - cols, dtype=dtype))    # padding columns
    if live:
        xr = x.detach()[live, :cols].double().requires_grad_(True)
        (F.cross_entropy(xr * 0.5, y[live], reduction="sum") / len(live)).backward()
        tol = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -22                      # one rounding to the logits' dtype
        assert float((x.grad[live, :cols].double() - xr.grad).abs().max()) <= tol * float(xr.grad.abs().max())


def test_counted_cross_entropy_fallback_without_live_rows_and_without_rows():
    from hero_amd import functional as HF
    x = torch.randn(4, 8, requires_grad=True)
    got = HF.counted_cross_entropy(x, torch.full((4,), -1), None, ignore_index=-1)
    got.backward()
    assert float(got.detach()) == 0.0 and not x.grad.any()
    assert float(HF.counted_cross_entropy(torch.zeros(0, 8), torch.zeros(0, dtype=torch.int64))) == 0.0


def test_row_capacity_values():
    from hero_amd.pretrain_data import PretrainMasker
    cap = PretrainMasker.row_capacity
    # ceil(150 + 6 sqrt(127.5)) = ceil(217.75) = 218, + 10 forced = 228 -> 232
    assert cap(1000, 0.15, 10) == 232
    assert cap(1000, 0.15, 10) == (int(math.ceil(1000 * 0.15 + 6 * math.sqrt(1000 * 0.15 * 0.85))) + 10 + 7) // 8 * 8
    assert cap(1000, 0.0, 3) == 8 and cap(1000, 0.0, 0) == 0 and cap(1000, 0.0, 9) == 16     # p = 0: only the forced selections
    assert cap(1000, 1.0, 7) == 1000 and cap(37, 1.0, 0) == 37                              # p = 1: everything, min(n, .) binds
    assert cap(10, 0.5, 4) == 10 and cap(20, 0.15, 3) == 16 and cap(5, 0.15, 2) == 5         # small n: min(n, .) binds
    assert cap(0, 0.3, 0) == 0
    # the D3 bench shape: 32 videos x 15 subtitles of 20 tokens, 60 frames
    assert cap(480 * 19, 0.15, 480) == 2056 and cap(32 * 60, 0.15, 32) == 416
    with pytest.raises(ValueError):
        cap(10, 1.5, 0)


def test_default_capacities_of_a_masker_follow_row_capacity():
    from hero_amd.pretrain_data import PretrainMasker
    m = PretrainMasker(9, 70, 65, 80, 3, 70, 12, "cpu", 4, (5, 128), 0, mlm_prob=0.15, mfm_prob=0.3)
    assert m.mlm_rows == PretrainMasker.row_capacity(9 * 69, 0.15, 9) and m.mfm_rows == PretrainMasker.row_capacity(210, 0.3, 3)
    assert m.mfm_order.shape == m.mfm_rank.shape == (210,) and m.mfm_order.dtype == torch.int32
    assert torch.equal(m.nce_labels, torch.arange(m.mfm_rows)) and m.overflow.tolist() == [0, 0] and m.overflow.dtype == torch.int64
    m = PretrainMasker(9, 70, 65, 80, 3, 70, 12, "cpu", 4, (5, 128), 0, mlm_rows=8, mfm_rows=24)
    assert (m.mlm_rows, m.mfm_rows) == (8, 24)
    assert set(m.static_entries()) == {"input_ids", "txt_mask_tgt", "txt_labels", "txt_mask_rows", "c_v_masks", "f_v_masks", "feat_targets",
                                       "c_v_feats", "f_v_feats", "shuffled_orders", "targets", "counts"}
    with pytest.raises(ValueError):
        PretrainMasker(9, 70, 65, 80, 3, 70, 12, "cpu", 4, (5, 128), 0, mfm_rows=211)


def test_no_draw_of_the_gpu_tests_overflows_the_default_capacities():
    from hero_amd.pretrain_data import PretrainMasker
    host = C.ragged_host()
    d = C.dims(host)
    draws = C.draws_without_overflow()
    assert len(draws) == 2 + C.STEP_DRAWS and len(set(draws)) == len(draws)
    worst = [0, 0]
    for seed, p in draws:
        mlm_rows = PretrainMasker.row_capacity(d["T"] * (d["max_sl"] - 1), p, d["T"])
        mfm_rows = PretrainMasker.row_capacity(d["B"] * d["NF"], p, d["B"])
        n_tok, n_frm = C.mlm_statement(host, seed, p)["count"], C.mfm_statement(host, seed, p)["count"]
        assert 1 <= n_tok <= mlm_rows and 1 <= n_frm <= mfm_rows, (seed, p, n_tok, mlm_rows, n_frm, mfm_rows)
        worst = [max(worst[0], n_tok), max(worst[1], n_frm)]
    print("largest counts", worst, "capacities", mlm_rows, mfm_rows)


@pytest.mark.parametrize("n", [1, 70, 1025])
def test_partition_statement_agrees_with_nonzero_order(n):
    from hero_amd import functional as HF
    g = torch.Generator().manual_seed(n)
    for mask in (torch.zeros(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool), torch.rand(n, generator=g) < 0.3):
        order, rank, m = C.partition_statement(mask.numpy())
        assert m == int(mask.sum())
        assert order[:m].tolist() == torch.nonzero(mask).reshape(-1).tolist()                 # masked first, nonzero order
        assert order[m:].tolist() == torch.nonzero(~mask).reshape(-1).tolist()                # then everything else, in order
        assert np.array_equal(rank[order], np.arange(n)) and np.array_equal(order[rank], np.arange(n))
        o, r, c = HF.mask_partition(mask)                                                     # the PyTorch fallback states the same
        assert o.dtype == r.dtype == c.dtype == torch.int32
        assert np.array_equal(o.numpy(), order) and np.array_equal(r.numpy(), rank) and c.tolist() == [m]


def test_nce_pack_fallback_is_the_index_statement():
    from hero_amd import functional as HF
    n, D, cap = 13, 8, 6
    g = torch.Generator().manual_seed(0)
    out, tg = torch.randn(n, D, generator=g, requires_grad=True), torch.randn(n, D, generator=g)
    for m in (0, 4, 6, 9):
        cand, masked = HF.nce_pack(out, tg, torch.tensor([m], dtype=torch.int32), cap, torch.float32)
        assert cand.shape == (16, D) and masked.shape == (cap, D)
        assert torch.equal(cand[:m], tg[:m]) and torch.equal(cand[m:n], out[m:].detach()) and not cand[n:].any()
        assert torch.equal(masked, out[:cap].detach())
        wc, wm = torch.randn(16, D, generator=g), torch.randn(cap, D, generator=g)
        (grad,) = torch.autograd.grad((cand * wc).sum() + (masked * wm).sum(), out)
        want = torch.zeros(n, D)
        want[:cap] += wm
        want[m:] += wc[m:n]
        assert torch.equal(grad, want)


def test_new_symbols_are_declared_bound_and_exported(built_lib):
    from hero_amd import _lib
    header = open(os.path.join(ROOT, "include", "hero_hip.h")).read()
    handle = ctypes.CDLL(built_lib)
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert hasattr(handle, name) and name in _lib.EXPORTS, name
    handle.hero_abi_version.restype = ctypes.c_int
    assert handle.hero_abi_version() == 3 == _lib.ABI_VERSION                # plain-argument additions: the version stays


def test_step_task_mapping():
    from hero_amd.step import mask_task_of
    assert [mask_task_of(t) for t in ("mlm", "mlm_how2", "mffr", "mfm-nce", "fom", "vsm", "tvr")] == ["mlm", "mlm", "mfm", "mfm", "fom", None, None]
