"""Host logic under the transformer block functions of hero_amd.functional (no GPU): the bounded cache whose entries a
captured graph may hold by address, and the row ranges of the sequence groups inside a row stack."""
import pytest
import torch

from hero_amd import functional as HF


@pytest.fixture
def capturing(monkeypatch):
    state = [False]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state[0])
    return state


def _fill(cache, keys):
    for k in keys:
        cache.get(k, lambda k=k: "v%s" % k)


def test_pinned_cache_drops_the_oldest_unpinned_entries_past_its_limit(capturing):
    c = HF._PinnedCache(4, 2)
    _fill(c, [0, 1])
    capturing[0] = True
    _fill(c, [2])                   # built under capture: pinned
    capturing[0] = False
    _fill(c, [3, 4])
    assert list(c.entries) == [0, 1, 2, 3, 4]           # `limit` is exceeded before anything is dropped
    _fill(c, [5])
    assert list(c.entries) == [2, 3, 4, 5]              # the two oldest went
    _fill(c, [6, 7])
    assert list(c.entries) == [2, 5, 6, 7]              # 3 and 4 went, never the pinned 2
    assert c.get(2, lambda: pytest.fail("a hit builds nothing")) == "v2"


def test_pinned_cache_grows_when_every_entry_is_pinned(capturing):
    c = HF._PinnedCache(2, 1)
    capturing[0] = True
    _fill(c, range(6))
    assert list(c.entries) == list(range(6)) and c.pinned == set(range(6))


def test_pinned_cache_pins_an_eager_entry_once_it_is_looked_up_under_capture(capturing):
    c = HF._PinnedCache(2, 2)
    _fill(c, [0, 1])
    capturing[0] = True
    assert c.get(0, None) == "v0"
    capturing[0] = False
    _fill(c, [2, 3, 4, 5])
    assert 0 in c.entries and 1 not in c.entries and len(c.entries) <= 4


def test_pinned_cache_keeps_none_as_a_value_and_never_pins_it(capturing):
    c = HF._PinnedCache(2, 1)
    built = []
    capturing[0] = True
    for _ in range(3):
        assert c.get("small", lambda: built.append(1)) is None
    assert built == [1] and c.pinned == set()
    capturing[0] = False
    _fill(c, [0, 1, 2])
    assert "small" not in c.entries                     # dropped like any unpinned entry


def test_pinned_cache_clear_keeps_the_pinned_entries_only_when_asked(capturing):
    c = HF._PinnedCache(8, 4)
    _fill(c, [0, 1])
    capturing[0] = True
    _fill(c, [2])
    c.get(0, None)
    capturing[0] = False
    c.clear(keep_pinned=True)
    assert list(c.entries) == [0, 2]
    _fill(c, [3])
    c.clear(keep_pinned=False)
    assert c.entries == {} and c.pinned == set()
    _fill(c, [2, 9])
    c.clear(keep_pinned=True)
    assert c.entries == {}                              # the pins went with the full clear


def test_segment_rows_of_padded_groups_follow_each_other():
    got = list(HF.segment_rows(((3, 24), (2, 15))))
    assert got == [(3, 24, slice(0, 72), None), (2, 15, slice(72, 102), None)]
    assert got == list(HF.segment_rows((HF.Segment(3, 24), HF.Segment(2, 15))))
    x = torch.zeros(102, 1)
    assert sum(x[rows].shape[0] for _, _, rows, _ in got) == x.shape[0]


def test_a_segment_with_sequence_offsets_covers_all_rows():
    off = torch.tensor([0, 24, 25, 40], dtype=torch.int32)
    (S, Lq, rows, seq_off), = HF.segment_rows((HF.Segment(3, 24, off),))
    assert (S, Lq, rows) == (3, 24, None) and seq_off is off
    x = torch.zeros(40, 2)
    assert HF._rows(x, rows) is x and HF._rows(x, slice(24, 25)).shape[0] == 1
