"""Host-side pieces of hero_amd.pretrain_data that need no GPU: the exact thresholds, the seed word's two's complement, and
functional.forget_memo - what PretrainMasker.draw() runs so that a later refresh_memo() does not meet row lists derived from
the previous masks."""
import pytest
import torch

from tests import pretrain_mask_reference as R


def test_thresholds_and_seed_words_are_exact():
    from hero_amd import pretrain_data as P
    for p in (0.0, 0.02, 0.15, 0.375, 0.5, 1.0):
        assert P.threshold(p) == R.threshold(p)
    assert P.threshold(1.0) == 1 << 32 and P.threshold(0.15) == 644245094        # floor(0.15 * 2^32)
    with pytest.raises(ValueError):
        P.threshold(1.5)
    assert P.SEED_STEP == R.SEED_STEP
    for s in (0, 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, 0xF123456789ABCDEF):
        assert P._signed(s) & ((1 << 64) - 1) == s and -(1 << 63) <= P._signed(s) < (1 << 63)
        word = torch.tensor([P._signed(s)], dtype=torch.int64)
        word.add_(P._signed(P.SEED_STEP))                                         # advance(): the sum mod 2^64
        assert int(word.item()) & ((1 << 64) - 1) == R.advance(s)


def test_forget_memo_drops_what_was_derived_from_a_rewritten_mask():
    from hero_amd import functional as HF
    HF.reset_caches()
    mask = torch.tensor([True, False, True, False, False])
    other = torch.arange(4)
    rows = HF.memo("mask_rows", (mask,), lambda: torch.nonzero(mask).reshape(-1))
    chained = HF.memo("rows_plus", (rows,), lambda: rows + 1)
    kept = HF.memo("twice", (other,), lambda: other * 2)
    mask.copy_(torch.tensor([True, True, True, False, False]))                     # another number of set rows
    with pytest.raises(RuntimeError):
        HF.refresh_memo()                                                          # the in-place redo cannot apply
    assert HF.forget_memo([mask]) == 2                                             # the entry and the one derived from it
    assert [e.tag for e in HF._MEMO.values()] == ["twice"]
    HF.refresh_memo()
    assert HF.memo("twice", (other,), lambda: None) is kept
    assert HF.memo("mask_rows", (mask,), lambda: torch.nonzero(mask).reshape(-1)).tolist() == [0, 1, 2]
    assert chained.tolist() == [1, 3]                                              # the old outputs are left alone
    HF.reset_caches()
