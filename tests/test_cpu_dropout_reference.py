"""What tests/test_gpu_dropout_masks.py rests on, checked without a GPU: the index builders of tests/dropout_reference.py against
the two older host statements of the draw, and every read-out decoder on the float64 emulation of what the kernel is asked to
compute - a KNOWN random mask goes in as multipliers and must come back bit for bit."""
import numpy as np
import pytest
import torch

from tests import dropout_reference as DR
from tests import gemm_reference as R
from tests import tvc_reference as TR

SEED63 = 0x7EDCBA9876543210                # a 63-bit seed word (the library keeps seeds below 2^63)
BIG_SITE = (1 << 33) + 5


# ---- the index builders ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lm", [9, 37, 64, 201])
@pytest.mark.parametrize("seed,site,thr", [(SEED63, BIG_SITE, 19661), (20240607, 7, 32768)])
def test_attention_keep_is_the_decoder_tests_draw(Lm, seed, site, thr):
    S, H = 3, 2
    keep = DR.attention_keep(seed, site, thr, S, H, Lm)
    mult = TR.dropout_multipliers(seed, site, thr, 2.0, S, H, Lm, Lm)
    assert keep.dtype == torch.bool and tuple(keep.shape) == (S, H, Lm, Lm)
    assert torch.equal(keep, mult > 0)
    rate = 1.0 - thr / 65536.0
    assert abs(float(keep.double().mean()) - rate) < 5 * (rate * (1 - rate) / keep.numel()) ** 0.5 + 1e-3
    # two heads, two sequences and two rows draw differently
    assert not torch.equal(keep[0, 0], keep[0, 1]) and not torch.equal(keep[0], keep[1]) and not torch.equal(keep[0, 0, 0], keep[0, 0, 1])


def test_attention_keep_refuses_indices_past_2_34():
    with pytest.raises(AssertionError):
        DR.attention_keep(1, 1, 100, 1 << 13, 16, 512)


@pytest.mark.parametrize("rows,cols", [(9, 132), (21, 1028), (5, 768)])
@pytest.mark.parametrize("seed,site,thr", [(SEED63, BIG_SITE, 19661), (3, 1, 32768)])
def test_ln_keep_is_the_flat_draw(rows, cols, seed, site, thr):
    keep = DR.ln_keep(seed, site, thr, rows, cols)
    assert keep.dtype == torch.bool and tuple(keep.shape) == (rows, cols)
    assert np.array_equal(keep.numpy().reshape(-1), R.dropout_keep(seed, site, thr, np.arange(rows * cols)))
    assert 0 < int(keep.sum()) < keep.numel()


# ---- the attention read-out ------------------------------------------------------------------------------------------------------------
def _random_keep(shape, seed, rate=0.7):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) < rate


@pytest.mark.parametrize("lens,packed", [([9, 6, 3], False), ([61, 58, 55], False), ([70, 67, 64], False), ([150, 147, 144], False),
                                         ([24, 9, 1, 17], True), ([201, 130, 31], True)])
def test_attention_read_out_recovers_a_known_mask(lens, packed):
    H, scale = 2, 1.0 / 0.7
    geo = DR.Geometry(lens, max(lens), packed)
    keep = _random_keep((geo.S, H, geo.Lm, geo.Lm), seed=geo.Lm)
    mult = keep.double() * scale
    qkv = DR.readout_qkv(geo, H)
    live = geo.live()[:, None].expand(-1, H, -1, -1)
    fwd, bwd = DR.Pattern(geo, H), DR.Pattern(geo, H)
    for w in DR.windows(geo.Lm):
        out = DR.attention_ref(qkv, geo.key_mask(w), geo, H, mult=mult)
        fwd.add_forward(out["ctx"], w)
        cnt = torch.tensor([max(0, min(DR.WINDOW, n - w)) for n in geo.lens], dtype=torch.float64).reshape(-1, 1, 1, 1)
        inwin = live & (torch.arange(geo.Lm).reshape(1, 1, 1, -1) >= w) & (torch.arange(geo.Lm).reshape(1, 1, 1, -1) < w + DR.WINDOW)
        assert torch.equal(out["probs"][inwin], (1.0 / cnt).expand_as(live)[inwin])              # every probability is 1 / live keys
        out = DR.attention_ref(qkv, geo.key_mask(), geo, H, mult=mult, dctx=DR.readout_dctx(geo, H, w))
        assert not out["dq"].any() and not out["dk"].any()
        bwd.add_backward(out["dv"], w)
    for pat in (fwd, bwd):
        assert pat.complete()
        assert torch.equal(pat.keep(), keep & live)
    n = torch.tensor(geo.lens, dtype=torch.float64).reshape(-1, 1, 1, 1).expand_as(live)
    torch.testing.assert_close(bwd.value[keep & live], (scale / n)[keep & live], rtol=1e-14, atol=0)


def test_attention_read_out_sees_one_flipped_element_and_a_shared_mask():
    """Decisive: a single flipped element, and a mask that two heads share, both come back as they went in."""
    H = 2
    geo = DR.Geometry([70, 67, 64], 70, False)
    keep = _random_keep((geo.S, H, 70, 70), seed=1)
    wrong = keep.clone()
    wrong[1, 1, 69, 65] = ~wrong[1, 1, 69, 65]
    shared = keep.clone()
    shared[:, 1] = shared[:, 0]
    qkv = DR.readout_qkv(geo, H)
    for m in (wrong, shared):
        fwd, bwd = DR.Pattern(geo, H), DR.Pattern(geo, H)
        for w in DR.windows(70):
            fwd.add_forward(DR.attention_ref(qkv, geo.key_mask(w), geo, H, mult=m.double())["ctx"], w)
            bwd.add_backward(DR.attention_ref(qkv, geo.key_mask(), geo, H, mult=m.double(), dctx=DR.readout_dctx(geo, H, w))["dv"], w)
        live = geo.live()[:, None].expand_as(m)
        for pat in (fwd, bwd):
            assert pat.complete() and torch.equal(pat.keep(), m & live) and not torch.equal(pat.keep(), keep & live)


def test_attention_ref_is_autograd_of_the_older_statement():
    """The plain formulas (dP masked before the softmax Jacobian) against float64 autograd through tvc_reference.attention."""
    S, L, H = 2, 11, 2
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(S * L, 3 * H * 64, generator=g, dtype=torch.float64)
    dctx = torch.randn(S * L, H * 64, generator=g, dtype=torch.float64)
    geo = DR.Geometry([11, 8], L, False)
    madd = geo.key_mask().double()
    madd[1, 0] = DR.MASKED
    mult = _random_keep((S, H, L, L), seed=4).double() / 0.7
    mine = DR.attention_ref(qkv, madd, geo, H, mult=mult, dctx=dctx)
    D = H * 64
    theirs = TR.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], S, L, L, H, key_mask_add=madd, mult=mult, dctx=dctx)
    for key in ("ctx", "dq", "dk", "dv"):
        torch.testing.assert_close(mine[key], theirs[key], rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(mine["probs"], theirs["P"], rtol=1e-12, atol=1e-15)


# ---- the LayerNorm read-outs -------------------------------------------------------------------------------------------------------------
def _ln_inputs(rows, cols, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma = torch.randn(cols, generator=g, dtype=torch.float64) * 0.1 + 1
    beta = torch.randn(cols, generator=g, dtype=torch.float64) * 0.1
    return x, gamma, beta


def test_layernorm_forward_and_input_read_outs_recover_known_masks():
    rows, cols, scale = 9, 132, 1.0 / 0.7
    x, gamma, beta = _ln_inputs(rows, cols)
    keep_out, keep_in = _random_keep((rows, cols), 5), _random_keep((rows, cols), 6)
    y0 = DR.ln_ref(x, gamma, beta, 1e-12)
    y = DR.ln_ref(x, gamma, beta, 1e-12, mult_out=keep_out.double() * scale)
    assert torch.equal(DR.ln_forward_keep(y, y0), keep_out)
    torch.testing.assert_close(y[keep_out], (y0 * scale)[keep_out], rtol=1e-15, atol=0)
    dy = torch.randn(rows, cols, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    b = DR.ln_bwd_ref(x, gamma, 1e-12, dy, mult_out=keep_out.double() * scale, mult_in=keep_in.double() * scale)
    got, decided = DR.ln_input_keep(b["dx"], b["dx_dropped"])
    assert bool(decided.all()) and torch.equal(got, keep_in)
    with pytest.raises(AssertionError):
        DR.ln_forward_keep(y, torch.zeros_like(y0))


def test_layernorm_ref_is_autograd_of_layer_norm():
    rows, cols, scale = 7, 36, 1.0 / 0.7
    x, gamma, beta = _ln_inputs(rows, cols)
    m_out, m_in = _random_keep((rows, cols), 8).double() * scale, _random_keep((rows, cols), 9).double() * scale
    dy = torch.randn(rows, cols, generator=torch.Generator().manual_seed(10), dtype=torch.float64)
    # x = u * m_in (u stands for the feeding linear's output plus its bias): d/du is dx_dropped, d/dbias its column sum
    u = torch.randn(rows, cols, generator=torch.Generator().manual_seed(11), dtype=torch.float64).requires_grad_(True)
    res = (x - (u * m_in)).detach()
    xin = u * m_in + res
    xin.retain_grad()
    gp, bp = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xin, (cols,), gp, bp, 1e-5) * m_out
    y.backward(dy)
    torch.testing.assert_close(DR.ln_ref(x, gamma, beta, 1e-5, mult_out=m_out), y.detach(), rtol=1e-12, atol=1e-13)
    b = DR.ln_bwd_ref(x, gamma, 1e-5, dy, mult_out=m_out, mult_in=m_in)
    for got, want in ((b["dx"], xin.grad), (b["dx_dropped"], u.grad), (b["dgamma"], gp.grad), (b["dbeta"], bp.grad), (b["dbias_in"], u.grad.sum(0))):
        torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("rows,cols", [(9, 132), (21, 1028), (70, 1028)])
def test_column_sum_read_out_recovers_a_known_mask(rows, cols):
    """p = 1/2: multipliers 0 or 2.  In fp32 arithmetic (the kernels' accumulators) the sum is exact in any order."""
    x, gamma, _ = _ln_inputs(rows, cols)
    keep = _random_keep((rows, cols), 12, rate=0.5)
    got = torch.zeros(rows, cols, dtype=torch.bool)
    wins = DR.colsum_windows(rows)
    assert len(wins) == (rows + 15) // 16 and sum(n for _, n in wins) == rows
    for r0, n in wins:
        dy = DR.colsum_dy(rows, cols, r0, n)
        assert torch.equal(dy.to(torch.bfloat16).double(), dy)                 # bf16 values
        dbeta = DR.ln_bwd_ref(x, gamma, 1e-12, dy, mult_out=keep.double() * 2.0)["dbeta"]
        # the same sum in fp32, rows added in reverse: the same number
        acc = torch.zeros(cols, dtype=torch.float32)
        for r in reversed(range(rows)):
            acc = acc + dy[r].float() * (keep[r].float() * 2.0)
        assert torch.equal(acc.double(), dbeta)
        got[r0:r0 + n] = DR.colsum_decode(dbeta, n)
    assert torch.equal(got, keep)
    with pytest.raises(AssertionError):
        DR.colsum_decode(torch.tensor([3.0]), 4)                               # 3 / 2 is no integer: no sum of doubled powers of two
