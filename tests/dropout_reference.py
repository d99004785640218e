"""The dropout masks of the encoder attention and of LayerNorm, stated on the host, and what reads them off the kernels.

  keep      attention_keep / ln_keep: the counter-based draw (tests/gemm_reference.dropout_keep) on the element index that
            include/hero_hip.h documents - attention ((s*H + h)*Lm + i) * round_up(Lm, 4) + j with Lm the launch's maximum
            length (packed batches too), LayerNorm row * cols + c.
  read-out  inputs that make a kernel's OUTPUT show its mask element by element, and the decoders of those outputs.  Pure tensor
            functions: tests/test_cpu_dropout_reference.py feeds them from the float64 references below with a known random
            mask, tests/test_gpu_dropout_masks.py from the kernels.
              attention  q = k = 0 (every probability 1 / live keys), V row j = e_(j mod 64) in every head.  With the keys of one
                         64-key window live, ctx[i, d] != 0 <=> keep[i, w + d]; with dctx row i = e_(i mod 64) inside a 64-row
                         window and 0 outside, dV[j, d] != 0 <=> keep[w + d, j].
              LayerNorm  y == 0 <=> dropped (where the undropped output is not 0); dx_dropped == 0 <=> dropped (where dx is not
                         0); with p = 1/2 and dy[r, :] = 2^(r - r0) on at most 16 rows, dbeta[c] / 2 is the integer whose bit
                         r - r0 is keep[r, c].
  float64   attention and LayerNorm, forward and backward, with EXPLICIT multiplier tensors (0 or 1 / (1 - p)), in plain formulas.
"""
import math

import numpy as np
import torch

from tests.gemm_reference import dropout_keep

HEAD = 64
WINDOW = 64
MASKED = -10000.0


# ---- keep ------------------------------------------------------------------------------------------------------------------------
def attention_keep(seed, site, thr16, S, H, Lm):
    """bool [S, H, Lm, Lm]: keep of probability (s, h, i, j) of a launch of S sequences of at most Lm rows."""
    Lp = (Lm + 3) // 4 * 4
    assert (S * H * Lm - 1) * Lp + Lm - 1 < (1 << 34)                       # the largest index, before anything is allocated
    rows = np.arange(S * H * Lm, dtype=np.uint64).reshape(S, H, Lm, 1)
    index = rows * np.uint64(Lp) + np.arange(Lm, dtype=np.uint64).reshape(1, 1, 1, Lm)
    return torch.from_numpy(dropout_keep(seed, site, thr16, index))


def ln_keep(seed, site, thr16, rows, cols):
    """bool [rows, cols]: keep of element (row, c) of a [rows, cols] tensor."""
    assert rows * cols - 1 < (1 << 34)
    index = np.arange(rows, dtype=np.uint64).reshape(-1, 1) * np.uint64(cols) + np.arange(cols, dtype=np.uint64).reshape(1, -1)
    return torch.from_numpy(dropout_keep(seed, site, thr16, index))


# ---- batch geometry ----------------------------------------------------------------------------------------------------------------
class Geometry:
    """Rows of a batch of S sequences.  Padded: sequence s owns rows [s*Lm, (s+1)*Lm), all of them query rows, its first
    lens[s] keys live (the others masked additively).  Packed: sequence s owns lens[s] rows, all live."""

    def __init__(self, lens, Lm, packed):
        self.lens, self.Lm, self.packed, self.S = [int(n) for n in lens], int(Lm), bool(packed), len(lens)
        assert max(self.lens) <= Lm and min(self.lens) >= 1 and (not packed or max(self.lens) == Lm)
        self.nrows = list(self.lens) if packed else [self.Lm] * self.S
        self.row0 = [0]
        for n in self.nrows:
            self.row0.append(self.row0[-1] + n)
        self.rows = self.row0[-1]

    def seq_off(self):
        return torch.tensor(self.row0, dtype=torch.int32) if self.packed else None

    def positions(self):
        """[rows] position of every row inside its sequence."""
        return torch.cat([torch.arange(n) for n in self.nrows])

    def live(self):
        """bool [S, Lm, Lm]: (query row, key) pairs that exist."""
        m = torch.zeros(self.S, self.Lm, self.Lm, dtype=torch.bool)
        for s in range(self.S):
            m[s, :self.nrows[s], :self.lens[s]] = True
        return m

    def key_mask(self, w=None):
        """Additive key mask [S, Lm] float32: 0 on the live keys (of the window [w, w + 64) only, if given), else -10000."""
        m = torch.full((self.S, self.Lm), MASKED, dtype=torch.float32)
        for s, n in enumerate(self.lens):
            lo, hi = (0, n) if w is None else (min(w, n), min(w + WINDOW, n))
            m[s, lo:hi] = 0.0
        return m


def windows(n):
    return list(range(0, n, WINDOW))


# ---- attention read-out ----------------------------------------------------------------------------------------------------------------
def readout_qkv(geo, H, dtype=torch.float64):
    """[rows, 3*H*64]: q = k = 0, V row at position j = e_(j mod 64) in every head."""
    D = H * HEAD
    qkv = torch.zeros(geo.rows, 3 * D, dtype=dtype)
    pos = geo.positions()
    for h in range(H):
        qkv[torch.arange(geo.rows), 2 * D + h * HEAD + pos % HEAD] = 1.0
    return qkv


def readout_dctx(geo, H, w, dtype=torch.float64):
    """[rows, H*64]: row at position i = e_(i mod 64) in every head for w <= i < w + 64, else 0."""
    D = H * HEAD
    d = torch.zeros(geo.rows, D, dtype=dtype)
    pos = geo.positions()
    sel = torch.nonzero((pos >= w) & (pos < w + WINDOW)).reshape(-1)
    for h in range(H):
        d[sel, h * HEAD + pos[sel] % HEAD] = 1.0
    return d


class Pattern:
    """What the windows of one direction have shown so far: value [S, H, Lm, Lm] (the raw output entry that stands for
    probability (i, j)), seen [S, H, Lm, Lm] (how many windows covered it)."""

    def __init__(self, geo, H):
        self.geo, self.H = geo, H
        self.value = torch.zeros(geo.S, H, geo.Lm, geo.Lm, dtype=torch.float64)
        self.seen = torch.zeros(geo.S, H, geo.Lm, geo.Lm, dtype=torch.int32)

    def add_forward(self, ctx, w):
        """ctx [rows, H*64] of a forward whose live keys were those of window w: column d of head h is key w + d."""
        g = self.geo
        ctx = ctx.detach().double().cpu()
        for s in range(g.S):
            nk = min(WINDOW, g.lens[s] - w)
            if nk <= 0:
                continue                                   # no live key in this window: the row is a softmax over masked keys
            blk = ctx[g.row0[s]:g.row0[s + 1]].reshape(g.nrows[s], self.H, HEAD)[:, :, :nk]
            self.value[s, :, :g.nrows[s], w:w + nk] = blk.permute(1, 0, 2)
            self.seen[s, :, :g.nrows[s], w:w + nk] += 1

    def add_backward(self, dv, w):
        """dv [rows, H*64] (the V third of dqkv) of a backward whose dctx was readout_dctx(w): column d of key row j is
        query row w + d."""
        g = self.geo
        dv = dv.detach().double().cpu()
        for s in range(g.S):
            nq = min(WINDOW, g.nrows[s] - w)
            if nq <= 0:
                continue
            blk = dv[g.row0[s]:g.row0[s] + g.lens[s]].reshape(g.lens[s], self.H, HEAD)[:, :, :nq]
            self.value[s, :, w:w + nq, :g.lens[s]] = blk.permute(1, 2, 0)
            self.seen[s, :, w:w + nq, :g.lens[s]] += 1

    def complete(self):
        """Every live (i, j) was covered by exactly one window, nothing else by any."""
        return torch.equal(self.seen, self.geo.live()[:, None].expand_as(self.seen).to(torch.int32))

    def keep(self):
        return self.value != 0


# ---- attention, float64 ----------------------------------------------------------------------------------------------------------------
def attention_ref(qkv, mask_add, geo, H, mult=None, dctx=None):
    """Masked multi-head self-attention of a [rows, 3*H*64] projection (q | k | v), scores / 8 + additive key mask, softmax,
    probabilities times mult [S, H, Lm, Lm], context.  -> dict ctx [rows, H*64], probs [S, H, Lm, Lm] (undropped, 0 where
    no (row, key) exists) and, with dctx, dq / dk / dv [rows, H*64]: dP = (dctx V^T) * mult BEFORE the softmax Jacobian
    dS = P * (dP - sum_j dP P), dq = dS k / 8, dk = dS^T q / 8, dv = (P * mult)^T dctx."""
    D = H * HEAD
    qkv = qkv.detach().double().cpu()
    out = dict(ctx=torch.zeros(geo.rows, D, dtype=torch.float64), probs=torch.zeros(geo.S, H, geo.Lm, geo.Lm, dtype=torch.float64))
    if dctx is not None:
        dctx = dctx.detach().double().cpu()
        out.update(dq=torch.zeros(geo.rows, D, dtype=torch.float64), dk=torch.zeros(geo.rows, D, dtype=torch.float64),
                   dv=torch.zeros(geo.rows, D, dtype=torch.float64))
    for s in range(geo.S):
        r0, n = geo.row0[s], geo.nrows[s]
        q, k, v = (qkv[r0:r0 + n, t * D:(t + 1) * D].reshape(n, H, HEAD).permute(1, 0, 2) for t in range(3))     # [H, n, 64]
        sc = q @ k.transpose(-1, -2) / math.sqrt(HEAD)
        if mask_add is not None:
            sc = sc + mask_add[s, :n].detach().double().cpu().reshape(1, 1, n)
        P = torch.softmax(sc, dim=-1)
        m = mult[s, :, :n, :n].double() if mult is not None else torch.ones_like(P)
        out["probs"][s, :, :n, :n] = P
        out["ctx"][r0:r0 + n] = ((P * m) @ v).permute(1, 0, 2).reshape(n, D)
        if dctx is not None:
            do = dctx[r0:r0 + n].reshape(n, H, HEAD).permute(1, 0, 2)
            dP = (do @ v.transpose(-1, -2)) * m
            dS = P * (dP - (dP * P).sum(-1, keepdim=True))
            for key, val in (("dq", dS @ k / math.sqrt(HEAD)), ("dk", dS.transpose(-1, -2) @ q / math.sqrt(HEAD)),
                             ("dv", (P * m).transpose(-1, -2) @ do)):
                out[key][r0:r0 + n] = val.permute(1, 0, 2).reshape(n, D)
    return out


# ---- LayerNorm, float64 ----------------------------------------------------------------------------------------------------------------
def _ln_stats(x, eps):
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    return (x - mean) * rstd, rstd


def ln_ref(x, gamma, beta, eps, mult_out=None):
    """y = (xhat * gamma + beta) * mult_out."""
    xhat, _ = _ln_stats(x.detach().double().cpu(), eps)
    y = xhat * gamma.detach().double().cpu() + beta.detach().double().cpu()
    return y * mult_out.double() if mult_out is not None else y


def ln_bwd_ref(x, gamma, eps, dy, mult_out=None, mult_in=None):
    """The backward of y = LayerNorm(x) * mult_out where x = (the feeding linear's output + bias) * mult_in + residual:
    dy_eff = dy * mult_out; dgamma = sum_r dy_eff xhat; dbeta = sum_r dy_eff; g = dy_eff gamma;
    dx = rstd (g - mean_c g - xhat mean_c (g xhat)); dx_dropped = dx * mult_in; dbias_in = sum_r dx_dropped."""
    xhat, rstd = _ln_stats(x.detach().double().cpu(), eps)
    d = dy.detach().double().cpu()
    if mult_out is not None:
        d = d * mult_out.double()
    g = d * gamma.detach().double().cpu()
    dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    dxd = dx * mult_in.double() if mult_in is not None else dx
    return dict(dx=dx, dx_dropped=dxd, dgamma=(d * xhat).sum(0), dbeta=d.sum(0), dbias_in=dxd.sum(0), rstd=rstd)


# ---- LayerNorm read-out ----------------------------------------------------------------------------------------------------------------
COLSUM_WINDOW = 16          # rows per window of the column-sum read-out: a sum of <= 16 distinct powers of two < 2^16 is an fp32 value


def ln_forward_keep(y, y_undropped):
    """keep [rows, cols] off a dropped output; the undropped one must have no zero (else a zero of y says nothing)."""
    assert bool((y_undropped != 0).all())
    return y.detach().cpu() != 0


def ln_input_keep(dx, dx_dropped):
    """(keep, decided) off the two input gradients of one backward: where dx != 0, dx_dropped != 0 <=> kept."""
    dx, dxd = dx.detach().cpu(), dx_dropped.detach().cpu()
    return dxd != 0, dx != 0


def colsum_windows(rows):
    return [(r0, min(COLSUM_WINDOW, rows - r0)) for r0 in range(0, rows, COLSUM_WINDOW)]


def colsum_dy(rows, cols, r0, n, dtype=torch.float64):
    """dy [rows, cols]: 2^(r - r0) on rows r0 .. r0 + n - 1, 0 elsewhere (bf16 and fp32 values)."""
    assert 1 <= n <= COLSUM_WINDOW and r0 + n <= rows
    dy = torch.zeros(rows, cols, dtype=dtype)
    dy[r0:r0 + n] = (2.0 ** torch.arange(n, dtype=torch.float64)).to(dtype).reshape(n, 1)
    return dy


def colsum_decode(dbeta, n, scale=2.0):
    """bool [n, cols] off dbeta = sum_r dy[r] * (keep[r] ? scale : 0) of colsum_dy: bit k of dbeta / scale is keep[r0 + k].
    Asserts that dbeta / scale is such an integer."""
    v = dbeta.detach().double().cpu() / scale
    code = v.round().to(torch.int64)
    assert torch.equal(code.double(), v) and int(code.min()) >= 0 and int(code.max()) < (1 << n), "dbeta / scale is no n-bit integer"
    return ((code.reshape(1, -1) >> torch.arange(n, dtype=torch.int64).reshape(-1, 1)) & 1).bool()
