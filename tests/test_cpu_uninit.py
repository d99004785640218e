"""The fill harness (tests/uninit.py) on the CPU: what it fills, that it restores the allocators, and - the proof that the GPU
tests built on it can fail - that assert_fill_independent rejects an op that reads a buffer it never wrote."""
import math

import pytest
import torch

from tests import uninit

FLOATS = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
OTHERS = [torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8, torch.bool]
ENTRY_POINTS = [(torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty")]


def _allocate(dtype):
    like = torch.ones(3, 5, dtype=dtype)
    return {
        "empty": torch.empty(3, 5, dtype=dtype),
        "empty-shape-tuple": torch.empty((7,), dtype=dtype, device="cpu"),
        "empty_like": torch.empty_like(like),
        "empty_strided": torch.empty_strided((3, 5), (5, 1), dtype=dtype),
        "new_empty": like.new_empty((2, 4)),
    }


@pytest.mark.parametrize("dtype", FLOATS, ids=str)
@pytest.mark.parametrize("value", [0.0, float("nan"), 3.5])
def test_floating_buffers_hold_the_fill(dtype, value):
    with uninit.filled(value):
        got = _allocate(dtype)
    for name, t in got.items():
        assert t.dtype == dtype, name
        if math.isnan(value):
            assert bool(torch.isnan(t).all()), name
        else:
            assert bool((t == value).all()), name


@pytest.mark.parametrize("dtype", OTHERS, ids=str)
def test_integer_and_bool_buffers_are_zero_under_both_fills(dtype):
    for value in uninit.FILLS:
        with uninit.filled(value):
            got = _allocate(dtype)
        for name, t in got.items():
            assert t.dtype == dtype and not bool(t.any()), (name, value)


def test_empty_tensors_and_torch_internals_keep_working():
    with uninit.filled(float("nan")):
        assert torch.empty(0).numel() == 0
        x = torch.randn(4, 6, requires_grad=True)
        y = torch.nn.functional.layer_norm(x, (6,))
        y.sum().backward()
        assert bool(torch.isfinite(x.grad).all())
        values, order = torch.sort(torch.tensor([3.0, 1.0, 2.0]))
        assert values.tolist() == [1.0, 2.0, 3.0] and order.tolist() == [1, 2, 0]
        lin = torch.nn.Linear(5, 3)
        assert bool(torch.isfinite(lin.weight).all())


def test_entry_points_are_restored():
    before = [getattr(owner, name) for owner, name in ENTRY_POINTS]
    with uninit.filled(0.0):
        inside = [getattr(owner, name) for owner, name in ENTRY_POINTS]
        assert all(a is not b for a, b in zip(before, inside))
    assert all(getattr(owner, name) is fn for (owner, name), fn in zip(ENTRY_POINTS, before))


def test_entry_points_are_restored_after_an_exception():
    before = [getattr(owner, name) for owner, name in ENTRY_POINTS]
    with pytest.raises(ZeroDivisionError):
        with uninit.filled(float("nan")):
            1 / 0
    assert all(getattr(owner, name) is fn for (owner, name), fn in zip(ENTRY_POINTS, before))
    with pytest.raises(AssertionError):          # assert_fill_independent leaves them restored when it fails, too
        uninit.assert_fill_independent(lambda: None, lambda _: {"y": torch.empty(3)})
    assert all(getattr(owner, name) is fn for (owner, name), fn in zip(ENTRY_POINTS, before))


def test_cached_scratch_is_filled_on_entry():
    from hero_amd import functional as HF
    key = ("cpu", None, "tests-uninit")
    HF._WS[key] = torch.ones(16)
    try:
        with uninit.filled(float("nan")):
            assert bool(torch.isnan(HF._WS[key]).all())
        with uninit.filled(0.0):
            assert not bool(HF._WS[key].any())
    finally:
        del HF._WS[key]


def _inputs():
    return torch.randn(33, generator=torch.Generator().manual_seed(5))


def test_a_dependent_op_fails_the_harness():
    """`empty * 0 + x` is x on benign memory and NaN where the buffer held one: exactly the masked-by-multiplication read."""
    def run(x):
        return {"y": torch.empty(x.numel()) * 0 + x}
    with pytest.raises(AssertionError) as err:
        uninit.assert_fill_independent(_inputs, run)
    msg = str(err.value)
    assert "y:" in msg and "33 of 33" in msg and "not finite under the NaN fill" in msg and "first at (0,)" in msg


def test_a_dependent_op_fails_through_every_entry_point():
    like = torch.ones(33)
    for alloc in (lambda: torch.empty_like(like), lambda: torch.empty_strided((33,), (1,)), lambda: like.new_empty((33,))):
        with pytest.raises(AssertionError):
            uninit.assert_fill_independent(_inputs, lambda x: {"y": alloc() * 0 + x})


def test_a_finite_difference_is_reported_with_count_and_first_index():
    def run(x):
        buf = torch.empty(x.numel())
        y = x.clone()
        y[7] = torch.where(torch.isnan(buf[7]), torch.tensor(1.0), torch.tensor(2.0))    # finite under both fills, differs
        return {"y": y}
    with pytest.raises(AssertionError) as err:
        uninit.assert_fill_independent(_inputs, run)
    assert "1 of 33 defined elements differ between the fills, first at (7,)" in str(err.value)


def test_an_independent_op_passes():
    def run(x):
        y = torch.empty(x.numel())
        torch.mul(x, 2.0, out=y)                 # writes every cell it returns
        idx = torch.empty(x.numel(), dtype=torch.int64)
        return {"y": y, "idx": idx}
    out = uninit.assert_fill_independent(_inputs, run)
    assert torch.equal(out["y"], _inputs() * 2)


def test_defined_excludes_exactly_the_masked_elements():
    def run(x):
        y = torch.empty(x.numel())
        y[:20] = x[:20]                          # contract: only the first 20 cells are defined
        return {"y": y}
    defined = torch.arange(33) < 20
    uninit.assert_fill_independent(_inputs, run, defined={"y": defined})
    with pytest.raises(AssertionError):
        uninit.assert_fill_independent(_inputs, run, defined={"y": torch.arange(33) < 21})
    with pytest.raises(AssertionError):          # a name no result carries is a mistake in the table, not an exclusion
        uninit.assert_fill_independent(_inputs, run, defined={"z": defined})
