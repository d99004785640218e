"""Fill harness: does a result depend on what an uninitialised buffer happened to hold?

`filled(value)` replaces the four allocators that hand out uninitialised memory - torch.empty, torch.empty_like,
torch.empty_strided, torch.Tensor.new_empty - with wrappers that call the original and then FILL the result: floating tensors
(fp32, bf16, fp16, fp64) with `value`, every other dtype with zero.  The patch reaches every caller that looks the name up
at call time, as hero_amd does (`torch.empty(...)`); torch's own Python-level users keep working, they only get defined memory.

`assert_fill_independent(build, run, defined)` runs an operation twice on identical inputs, once with every such buffer
pre-filled with 0.0 and once with NaN, and asserts that everything the operation defines is finite and BIT-IDENTICAL between
the two runs.  No tolerance is involved: a kernel that reads a cell it never wrote and "masks" it arithmetically (NaN * 0 is
NaN) fails, a kernel that writes what it reads or selects on what it loads passes.

Integer and bool buffers are zero-filled in BOTH runs, on purpose.  A poisoned index could send a load outside its buffer,
and these tests run on shared GPUs that one out-of-bounds access can take down: they must never make one fault.  What the
harness finds is therefore the arithmetic dependence on undefined FLOATING memory only.

Module-level caches of the library, on entry of `filled`:
  filled with `value` (scratch: created with torch.empty, every launch that reads a cell of it wrote that cell first)
    hero_amd.functional._WS        the fp32 workspaces of hero_colsum, hero_colsum_multi, hero_layernorm_bwd and
                                   hero_scatter_add_sorted, one per (device, slot)
  left alone (contract "zero between calls", or not scratch at all)
    hero_amd.head._STED_WS         created with torch.zeros: the partials and the ticket of hero_st_ed_bwd, which the kernel
                                   itself returns to zero (test_st_ed_bwd_bit_reproducible_and_leaves_its_ticket_at_zero)
    hero_amd.functional._WCACHE    compute copies of the weights: values, rebuilt after assert_fill_independent clears them
    hero_amd.functional._MEMO      derived batch tensors: values, cleared by assert_fill_independent
    hero_amd.functional._REFRESH, _WPLANS, _SEQ_OFF, hero_amd.model.embed._ARANGE    integer tables and plans built from
                                   host data (torch.tensor / from_numpy), never uninitialised
"""
import contextlib

import torch

FILLS = (0.0, float("nan"))
_NAMES = (("empty", torch), ("empty_like", torch), ("empty_strided", torch), ("new_empty", torch.Tensor))


def _fill(t, value):
    if isinstance(t, torch.Tensor) and t.numel():
        if t.dtype.is_floating_point:
            t.fill_(value)
        else:
            t.zero_()
    return t


def _wrap(orig, value):
    def alloc(*args, **kwargs):
        return _fill(orig(*args, **kwargs), value)
    alloc.__wrapped__ = orig
    return alloc


def scratch_caches():
    """The cached float scratch tensors of the library (see the module docstring)."""
    from hero_amd import functional as HF
    return list(HF._WS.values())


@contextlib.contextmanager
def filled(value):
    """Every tensor that torch.empty / empty_like / empty_strided / Tensor.new_empty returns inside the context holds `value`
    (floating dtypes) or zero (all others); the library's cached float scratch holds `value` too."""
    saved = [(owner, name, getattr(owner, name)) for name, owner in _NAMES]
    try:
        for owner, name, orig in saved:
            setattr(owner, name, _wrap(orig, value))
        for t in scratch_caches():
            _fill(t, value)
        yield
    finally:
        for owner, name, orig in saved:
            setattr(owner, name, orig)


def _clear_library_caches():
    from hero_amd import functional as HF
    HF.clear_weight_cache()
    HF._MEMO.clear()


def _first(mask):
    idx = mask.reshape(-1).nonzero()
    if not idx.numel():
        return None
    flat = int(idx[0])
    return tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), mask.shape)) if mask.dim() else ()


def assert_fill_independent(build, run, defined=None):
    """build() -> fresh inputs from fixed seeds; run(inputs) -> {name: tensor}.  Both are called once per fill, run inside
    filled(fill).  defined: {name: bool mask} - the elements of that result the operation's contract defines (default: all)."""
    results = []
    for fill in FILLS:
        _clear_library_caches()
        inputs = build()                    # outside the context: nothing allocated under the other fill is reused
        with filled(fill):
            out = run(inputs)
            if torch.cuda.is_available():
                torch.cuda.synchronize()
        results.append({k: v.detach().clone() for k, v in out.items()})
    zero, nan = results
    assert zero.keys() == nan.keys(), (sorted(zero), sorted(nan))
    unknown = set(defined or ()) - set(zero)
    assert not unknown, "defined names no result carries: %s" % sorted(unknown)
    problems = []
    for name in zero:
        a, b = zero[name], nan[name]
        if a.shape != b.shape or a.dtype != b.dtype:
            problems.append("%s: %s %s under the zero fill, %s %s under the NaN fill" % (name, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype))
            continue
        mask = torch.ones(a.shape, dtype=torch.bool, device=a.device)
        if defined is not None and name in defined:
            mask = defined[name].to(a.device).expand(a.shape)
        for tag, t in (("zero", a), ("NaN", b)):
            if t.dtype.is_floating_point:
                bad = ~torch.isfinite(t) & mask
                if bool(bad.any()):
                    problems.append("%s: %d of %d defined elements are not finite under the %s fill, first at %s" % (
                        name, int(bad.sum()), int(mask.sum()), tag, _first(bad)))
        if not torch.equal(a[mask], b[mask]):
            diff = (_bits(a) != _bits(b)) & mask
            i = _first(diff)
            if i is None:                   # the same NaN on both sides: reported above as not finite
                continue
            problems.append("%s: %d of %d defined elements differ between the fills, first at %s (%r under zero, %r under NaN)" % (
                name, int(diff.sum()), int(mask.sum()), i, a[i].item(), b[i].item()))
    assert not problems, "result depends on uninitialised memory:\n  " + "\n  ".join(problems)
    return zero


def _bits(t):
    """The bit pattern of a tensor as integers: a NaN equals itself, so only elements that really differ are counted."""
    if not t.dtype.is_floating_point:
        return t
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
