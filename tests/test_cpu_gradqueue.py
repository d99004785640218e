"""The deferred gradient queue of hero_amd.functional (host logic, no GPU): what goes into one weight-gradient / column-sum
launch, where a launch is cut so that no destination is in it twice, and the queue's bookkeeping across backward passes.
Jobs are built on stand-in tensors."""
import types

import pytest

from hero_amd import functional as HF

D = 768
BF16, F32 = "bf16", "f32"


def _t(ptr=0, shape=(1,), dtype=F32):
    n = 1
    for s in shape:
        n *= s
    size = 2 if dtype == BF16 else 4
    return types.SimpleNamespace(shape=shape, dtype=dtype, data_ptr=lambda: ptr, numel=lambda: n, element_size=lambda: size)


def _wjob(out, rows=1920, dtype=BF16, dbias=None, on_done=None):
    return HF.WgradJob(_t(shape=(rows, out.shape[0]), dtype=dtype), _t(shape=(rows, out.shape[1]), dtype=dtype), out, 0, out.shape[0],
                       on_done, dbias, None)


def _weights(n, base=1 << 20):
    """n disjoint [D, D] fp32 destinations, back to back (as in a flat gradient arena)."""
    return [_t(base + 4 * D * D * i, (D, D)) for i in range(n)]


def _groups(jobs, plan):
    out = []
    while jobs:
        n = plan(jobs)
        assert n >= 1
        out.append(n)
        jobs = jobs[n:]
    return out


def test_weight_gradient_launches_hold_at_most_32_jobs_of_equal_rows_and_dtype():
    assert _groups([_wjob(w) for w in _weights(40)], HF._next_wgrad_launch) == [32, 8]
    jobs = [_wjob(w, rows=1920 if i < 3 else 480) for i, w in enumerate(_weights(6))]
    assert _groups(jobs, HF._next_wgrad_launch) == [3, 3]
    jobs = [_wjob(w, dtype=BF16 if i < 2 else F32) for i, w in enumerate(_weights(5))]
    assert _groups(jobs, HF._next_wgrad_launch) == [2, 3]


def test_weight_gradient_launch_is_cut_before_a_destination_it_already_holds():
    w = _weights(4)
    assert _groups([_wjob(w[0]), _wjob(w[1]), _wjob(w[0]), _wjob(w[2])], HF._next_wgrad_launch) == [2, 2]
    bias = _t(1 << 12, (D,))
    assert _groups([_wjob(w[0], dbias=bias), _wjob(w[1], dbias=bias)], HF._next_wgrad_launch) == [1, 1]
    biases = [_t((1 << 12) + 4 * D * i, (D,)) for i in range(4)]                # adjacent, not overlapping
    assert _groups([_wjob(w[i], dbias=biases[i]) for i in range(4)], HF._next_wgrad_launch) == [4]
    # a grouped [Wq;Wk;Wv] destination and its middle third: another base pointer, the same memory
    qkv = _t(1 << 30, (3 * D, D))
    wk = _t((1 << 30) + 4 * D * D, (D, D))
    assert wk.data_ptr() != qkv.data_ptr()
    assert _groups([_wjob(qkv), _wjob(wk)], HF._next_wgrad_launch) == [1, 1]
    assert _groups([_wjob(wk), _wjob(qkv)], HF._next_wgrad_launch) == [1, 1]
    assert _groups([_wjob(wk), _wjob(_t((1 << 30) + 8 * D * D, (D, D)))], HF._next_wgrad_launch) == [2]     # Wk, then Wv


def _cjob(dst, on_done=None):
    return HF.ColsumJob(None, None, dst, on_done)


def test_column_sum_launches_hold_at_most_64_disjoint_destinations():
    assert _groups([_cjob(_t(4096 + 4 * D * i, (D,))) for i in range(70)], HF._next_colsum_launch) == [64, 6]
    base, rows = 1 << 24, 512
    table = _t(base, (rows, D))                                                 # indexed destination rows: the whole table
    row = lambda r: _t(base + 4 * r * D, (D,))                                  # noqa: E731
    assert _groups([_cjob(table), _cjob(row(3))], HF._next_colsum_launch) == [1, 1]
    assert _groups([_cjob(row(3)), _cjob(table)], HF._next_colsum_launch) == [1, 1]
    assert _groups([_cjob(row(0)), _cjob(row(1)), _cjob(row(rows - 1))], HF._next_colsum_launch) == [3]


@pytest.fixture
def queue(monkeypatch):
    """A queue whose end-of-backward hook is recorded instead of going to the autograd engine."""
    monkeypatch.setattr(HF._GradQueue, "flush_task", -1)
    requested = []
    q = HF._GradQueue(request_flush=lambda: requested.append(HF._GradQueue.flush_task))
    return q, requested


def test_queue_drops_what_a_backward_pass_that_raised_left_behind(queue):
    q, requested = queue
    ran = []
    for w in _weights(3):
        q.push(_wjob(w, on_done=lambda: ran.append(1)), 1, nbytes=100)
    assert (len(q.jobs), q.nbytes, q.task) == (3, 300, 1)
    fresh = _wjob(_weights(1)[0])
    q.push(fresh, 2, nbytes=7)                                                  # the next backward pass
    assert q.jobs == [fresh] and (q.nbytes, q.task) == (7, 2) and ran == []
    q.clear()
    assert q.jobs == [] and q.nbytes == 0


def test_queue_requests_one_flush_callback_per_backward_pass(queue):
    q, requested = queue
    other = HF._GradQueue(request_flush=q.request_flush)                        # the column sums of the same backward pass
    for task in (5, 5, 6):
        for w in _weights(2):
            q.push(_wjob(w), task)
            other.push(_cjob(w), task)
    assert requested == [5, 6]


def test_queue_byte_count_returns_to_zero_when_it_is_flushed(queue):
    q, _ = queue
    jobs = [_wjob(w) for w in _weights(40)]
    for j in jobs:
        q.push(j, 1, nbytes=j.dy.numel() * j.dy.element_size())
    assert q.nbytes == 40 * 1920 * D * 2
    taken = []
    while q.jobs:                                                               # as wgrad_flush drains it
        taken.append(q.take(HF._next_wgrad_launch(q.jobs)))
    assert [len(g) for g in taken] == [32, 8] and taken[0] + taken[1] == jobs
    assert q.nbytes == 0


def test_reset_caches_clears_both_queues(monkeypatch):
    monkeypatch.setattr(HF._GradQueue, "flush_task", -1)
    for q in (HF._WQ, HF._CQ):
        monkeypatch.setattr(q, "request_flush", lambda: None)
        q.push(_wjob(_weights(1)[0]), 3, nbytes=5)
    HF.reset_caches()
    assert HF._WQ.jobs == [] and HF._CQ.jobs == [] and HF._WQ.nbytes == 0
