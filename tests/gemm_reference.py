"""Float64 restatement of hero_gemm's contract (include/hero_hip.h), written from the header and independent of the kernels'
code: operands on small dyadic grids, the epilogue in its documented order, the dropout draw by flat element index, the two
column-sum forms, split slabs and their fold, and bf16 rounding.

Why the grids: x / dy are integers in [-3, 3], w multiples of 1/32 in [-1/8, 1/8], so every product and every partial sum of
a reduction of length K is a multiple of 2^-7 (2^0 for weight gradients) bounded by K * 3 / 8.  Below 2^24 * 2^-7 = 131072
each such number is an fp32 value, so fp32 accumulation is EXACT in any order - MFMA blocks, split-K atomics, slab folds
and stream-K merges all give the same bits, and the float64 product below is the one correct answer."""
import math

import numpy as np
import torch

from tests.dropout_hash import _M64, _mix32, _splitmix64

ACT = dict(none=0, gelu=1, relu=2, gelu_bwd=3, relu_bwd=4, gelu_dg=5, mul_aux=6)
EXACT_ACTS = ("none", "relu", "relu_bwd", "mul_aux")
GRID_STEP = 2.0 ** -7                  # of an accumulator of x (integers) times w (multiples of 1/32) plus bias (1/8)
MAG_BOUND = 2.0 ** 24 * GRID_STEP      # partial sums below this are fp32 values


# ---- operand grids ---------------------------------------------------------------------------------------------------------
def _rng(seed, tag):
    return np.random.default_rng([seed, tag])


def grid_x(seed, shape):
    """x / dy: integers in [-3, 3]."""
    return _rng(seed, 1).integers(-3, 4, size=shape).astype(np.float64)


def grid_w(seed, shape):
    """w: multiples of 1/32 in [-4/32, 4/32]."""
    return _rng(seed, 2).integers(-4, 5, size=shape).astype(np.float64) / 32.0


def grid_bias(seed, n):
    """bias: multiples of 1/8 in [-1, 1]."""
    return _rng(seed, 3).integers(-8, 9, size=n).astype(np.float64) / 8.0


def grid_quarter(seed, shape, tag=4):
    """residual, aux of MUL_AUX / RELU_BWD, initial C / dw: multiples of 1/4 in [-2, 2]."""
    return _rng(seed, tag).integers(-8, 9, size=shape).astype(np.float64) / 4.0


def grid_preact(seed, shape):
    """aux of GELU_BWD (a saved pre-activation): multiples of 1/16 in [-4, 4] - bf16 values, on the grid E_as is measured on."""
    return _rng(seed, 5).integers(-64, 65, size=shape).astype(np.float64) / 16.0


# ---- number formats ----------------------------------------------------------------------------------------------------------
def _bf16_ulp(x64):
    x = np.abs(np.asarray(x64, dtype=np.float64))
    _, e = np.frexp(np.where(x == 0, 1.0, x))               # x = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e, -125) - 8)           # 8 significand bits


def bf16_rne(x64):
    """Round-to-nearest-even of float64 numbers to bfloat16 values (returned as float64), in ONE rounding."""
    x = np.asarray(x64, dtype=np.float64)
    ulp = _bf16_ulp(x)
    return np.rint(x / ulp) * ulp                           # rint: ties to even; x / ulp is exact (a power of two)


def bf16_half_ulp(x64):
    return 0.5 * _bf16_ulp(x64)


def _erf(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def gelu64(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    x = np.asarray(x, dtype=np.float64)
    cdf = 0.5 * (1.0 + _erf(x / math.sqrt(2.0)))
    return cdf + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_as_f32(x):
    """The DOCUMENTED fast GELU of the bf16 mode in float32 numpy: Phi(x) from the Abramowitz-Stegun 7.1.26 erfc form,
    erfc(z) = (a1 t + ... + a5 t^5) exp(-z^2), t = 1 / (1 + p z), z = |x| / sqrt 2.  -> (gelu, gelu') float32."""
    f = np.float32
    x = np.asarray(x, dtype=np.float32)
    ax = np.abs(x)
    q = np.exp(f(-0.5) * x * x).astype(np.float32)
    t = (f(1.0) / (f(1.0) + f(0.3275911) * f(math.sqrt(0.5)) * ax)).astype(np.float32)
    p = f(1.061405429)
    for a in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        p = (p * t + f(a)).astype(np.float32)
    half_erfc = (f(0.5) * p * t * q).astype(np.float32)
    cdf = np.where(x >= 0, f(1.0) - half_erfc, half_erfc).astype(np.float32)
    return (x * cdf).astype(np.float32), (cdf + x * f(1.0 / math.sqrt(2.0 * math.pi)) * q).astype(np.float32)


# ---- dropout -----------------------------------------------------------------------------------------------------------------
def dropout_keep(seed, site, threshold16, index):
    """keep = f(seed word, site, element index) of include/hero_hip.h for flat element indices (hero_gemm: index = m * N + n,
    below 2^34).  Four consecutive elements form a group; the group index is hashed twice, keyed by the low and the high half of
    splitmix64(seed ^ site * C); elements 0, 1 own the low / high 16 bits of the first hash, elements 2, 3 those of the second;
    an element is kept where its 16 bits are >= threshold16."""
    index = np.asarray(index, dtype=np.uint64)
    assert index.size == 0 or int(index.max()) < (1 << 34)
    base = _splitmix64((seed ^ ((site * 0xD6E8FEB86659FD93) & _M64)) & _M64)
    group, lane = index >> np.uint64(2), (index & np.uint64(3)).astype(np.int64)
    h = np.stack([_mix32(group ^ np.uint64(base & 0xFFFFFFFF)), _mix32(group ^ np.uint64(base >> 32))])     # [2, ...] 32-bit hashes
    u16 = np.stack([h[0] & np.uint64(0xFFFF), h[0] >> np.uint64(16), h[1] & np.uint64(0xFFFF), h[1] >> np.uint64(16)])
    return np.take_along_axis(u16, lane[None], axis=0)[0] >= np.uint64(threshold16)


def dropout_params(p):
    """(threshold16, fp32 scale) of a drop probability as hero_hip.h defines them."""
    return int(round(p * 65536)), float(np.float32(1.0 / (1.0 - p)))


# ---- the epilogue --------------------------------------------------------------------------------------------------------------
def epilogue_ref(acc64, bias=None, act="none", aux_in=None, drop=None, residual=None, beta=0.0, c0=None, tile_rows=0):
    """hero_gemm's epilogue on a float64 accumulator [M, N], in the header's order: bias, activation, dropout, residual,
    beta * C.  drop = (seed word, site, threshold16, scale).  -> dict:
      out      float64, BEFORE the rounding of the output dtype
      aux      what GELU (pre-activation), RELU (its output) and GELU_DG (gelu') save, else None
      colsum   [N] column sums of `out`
      partial  (tile_rows > 0) the [ceil(M / 64), N] table: an output tile of tile_rows rows writes its column sums to the
               row of its first 64-row block and zeros to the rows of its other blocks
      factor   for GELU_BWD: gelu'(aux_in), so that a caller can bound the error through the product."""
    v = np.array(acc64, dtype=np.float64)
    M, N = v.shape
    aux = factor = None
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float64).reshape(1, N)
    if act == "gelu":
        aux, v = v, gelu64(v)
    elif act == "relu":
        v = np.maximum(v, 0.0)
        aux = v
    elif act == "gelu_bwd":
        factor = gelu_grad64(aux_in)
        v = v * factor
    elif act == "relu_bwd":
        v = np.where(np.asarray(aux_in) > 0, v, 0.0)
    elif act == "gelu_dg":
        aux, v = gelu_grad64(v), gelu64(v)
    elif act == "mul_aux":
        v = v * np.asarray(aux_in, dtype=np.float64)
    else:
        assert act == "none", act
    if drop is not None and drop[2] != 0:
        seed, site, thr, scale = drop
        idx = np.arange(M, dtype=np.uint64).reshape(-1, 1) * np.uint64(N) + np.arange(N, dtype=np.uint64).reshape(1, -1)
        keep = dropout_keep(seed, site, thr, idx)
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), "the dropout scale is one fp32 multiply of an fp32 value"
        v = np.where(keep, (v.astype(np.float32) * np.float32(scale)).astype(np.float64), 0.0)
    if residual is not None:
        v = v + np.asarray(residual, dtype=np.float64)
        if not is_fp32(v):      # only behind a dropout scale that is no power of two: the epilogue's add is an fp32 add
            v = v.astype(np.float32).astype(np.float64)
    out = dict(aux=aux, factor=factor, colsum=v.sum(axis=0))
    if tile_rows:
        assert tile_rows % 64 == 0
        table = np.zeros(((M + 63) // 64, N))
        for m0 in range(0, M, tile_rows):
            table[m0 // 64] = v[m0:m0 + tile_rows].sum(axis=0)
        out["partial"] = table
    if beta != 0.0:
        v = v + float(beta) * np.asarray(c0, dtype=np.float64)
    out["out"] = v
    return out


def split_slabs(a64, b64, k_per_split, splits):
    """Per-split partial products of a [M, K] x [K, N] reduction cut into `splits` ranges of k_per_split: [splits, M, N]."""
    return np.stack([a64[:, s * k_per_split:(s + 1) * k_per_split] @ b64[s * k_per_split:(s + 1) * k_per_split] for s in range(splits)])


def fold_slabs(slabs):
    """hero_fold_slabs: the slabs added in slab order."""
    out = np.zeros_like(slabs[0])
    for s in slabs:
        out = out + s
    return out


def is_fp32(x64):
    return bool(np.array_equal(np.asarray(x64).astype(np.float32).astype(np.float64), x64))


# ---- the comparisons the GPU tests use -------------------------------------------------------------------------------------------
def same_bits(got, want64, bf16):
    """The exact comparison: `got` (torch tensor of the output dtype, cpu) against the one correct value - the float64
    number itself for fp32 outputs, its round-to-nearest-even for bf16 outputs."""
    want = torch.from_numpy(bf16_rne(want64) if bf16 else np.asarray(want64, dtype=np.float64))
    assert is_fp32(want.numpy()), "the expected value is no fp32 number: the exactness premise does not hold for this case"
    return torch.equal(got.double(), want)


def first_mismatches(got, want64, bf16, limit=8):
    want = bf16_rne(want64) if bf16 else np.asarray(want64, dtype=np.float64)
    g = got.double().numpy()
    bad = np.argwhere(~(g == want))
    return "%d of %d elements differ; first (row, col, got, want): %s" % (
        len(bad), want.size, [(int(r), int(c), float(g[r, c]), float(want[r, c])) for r, c in bad[:limit]])


def within(got, ref64, bound):
    """|got - ref64| <= bound element-wise (got: torch tensor, cpu) -> (ok, worst ratio)."""
    err = np.abs(got.double().numpy() - ref64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    live = bound > 0                                        # a zero bound (an exact zero factor) demands a zero error
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    return bool((err <= bound).all()), ratio
