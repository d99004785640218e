"""The dropout masks of the encoder attention kernels and of LayerNorm against the HOST statement of the draw
(tests/dropout_reference.py: attention_keep, ln_keep), element for element.  Needs a real MI355X (-m gpu).

  Tier A  attention, exact: inputs that make ctx and dV show the mask (q = k = 0, one-hot V rows, one-hot dctx rows, one launch
          per 64-key / 64-row window); the boolean pattern of the forward and of the backward EQUALS attention_keep on every
          live (sequence, head, row, key).  One case per kernel of the dispatch table of hero_amd/csrc/attention.hip.
  Tier B  attention, values: ctx, probs, dq, dk, dv against float64 with the explicit multipliers, one shape per kernel family.
  Tier C  LayerNorm, exact: y == 0, dx_dropped == 0 and the bits of dbeta (dy = powers of two, p = 1/2) EQUAL ln_keep.
  Tier D  LayerNorm, values: y, dx, dx_dropped, dgamma, dbeta, dbias_in against float64 with both explicit masks.

Every mask is drawn from this file's own seed word and explicit sites (one of them above 2^32), independent of the library's
site counter.  tests/test_cpu_dropout_reference.py proves the read-outs on the float64 emulation of the same requests."""
import pytest
import torch

from tests import dropout_reference as DR

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB                      # 63 bits
SITES = (11, (1 << 32) + 7)
P = 0.3
S, H = 3, 2                                    # both s and h enter the pair index (s*H + h)
F32, BF16 = torch.float32, torch.bfloat16
# the tolerances tests/test_gpu_kernels.py carries for the same kernels without dropout (TOL, ptol, _ln_param_close)
TOL = {F32: dict(rtol=2e-5, atol=2e-5), BF16: dict(rtol=2e-2, atol=2e-2)}
PTOL = {F32: dict(rtol=1e-4, atol=1e-5), BF16: dict(rtol=2e-2, atol=2e-3)}
# Exact read-outs, kept VALUES: how far a kept entry may be from (undropped entry) * scale.  bf16: two roundings to 8 significand
# bits, half an ulp = 2^-8 relative each (attention: the dropped probability as a matrix-core operand and the stored output;
# LayerNorm: the undropped output the test compares with and the dropped one), and their product term.  fp32: the reciprocal of
# the row sum (1 ulp, 2^-23), the product with it and the product with the scale (2^-24 each); LayerNorm: one product.
VALUE_RTOL = {F32: 5 * 2.0 ** -24, BF16: 2.0 ** -7 + 2.0 ** -16}


@pytest.fixture(scope="module")
def HF():
    from hero_amd import functional
    return functional


@pytest.fixture(scope="module")
def Lb():
    from hero_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def seed_word():
    return torch.tensor([SEED], dtype=torch.int64, device="cuda")


def _drop(Lb, seed_word, site, p=P):
    """-> (HeroDropout, threshold16, scale as the kernels hold it)."""
    thr = max(1, int(round(p * 65536.0)))
    d = Lb.Dropout(seed_word.data_ptr(), site, thr, 1.0 / (1.0 - p))
    return d, thr, float(d.scale)


def rnd(*shape, dtype=F32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def _within(name, got, ref64, rtol, atol):
    """assert_close against a float64 reference, with the worst error / tolerance printed first."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    ratio = float(((got - ref64).abs() / (atol + rtol * ref64.abs())).max())
    print("\n[dropout] %-34s worst |err| / tolerance %.3f" % (name, ratio), end="")
    assert ratio <= 1.0, "%s: worst error is %.3f of the tolerance (rtol %g, atol %g)" % (name, ratio, rtol, atol)


def _lens(L):
    return [max(1, L - 3 * i) for i in range(S)]                   # as in test_attention_fwd_bwd


# ==== Tier A =========================================================================================================================
# (id, dtype, lens, packed, save_probs, ctx to the backward, backward, pairs per wave) and the kernels the case reaches
ATTN_CASES = [
    ("f32-9", F32, _lens(9), False, False, True, True, 0),              # attn_{fwd,bwd}_small_kernel<4>
    ("f32-23", F32, _lens(23), False, False, True, True, 0),            # attn_{fwd,bwd}_small_kernel<2>
    ("f32-61", F32, _lens(61), False, False, True, True, 0),            # attn_{fwd,bwd}_small_kernel<1>
    ("f32-70", F32, _lens(70), False, False, True, True, 0),            # attn_fwd_kernel<float>, attn_bwd_kernel<float, 32, staged>
    ("f32-130", F32, _lens(130), False, False, True, True, 0),          # attn_fwd_kernel<float>, attn_bwd_kernel<float, 64, staged>
    ("f32-150", F32, _lens(150), False, False, True, True, 0),          # attn_fwd_kernel<float>, attn_bwd_kernel<float, 64, QO_GLOBAL>
    ("f32-256", F32, _lens(256), False, False, True, True, 0),          # the same two at the longest backward
    ("f32-packed-24", F32, [24, 9, 1, 17], True, False, True, True, 0),  # attn_{fwd,bwd}_small_kernel<2>, seq_off
    # bf16, L <= 32: attn_mfma_fwd_kernel / attn_mfma_bwd_kernel<RC = true (row statistics) / false (saved probabilities)>
    ("bf16-15-stats", BF16, _lens(15), False, False, True, True, 0),
    ("bf16-15-probs", BF16, _lens(15), False, True, True, True, 0),
    ("bf16-31-stats", BF16, _lens(31), False, False, True, True, 0),
    ("bf16-31-probs", BF16, _lens(31), False, True, True, True, 0),
    # bf16, 32 < L <= 64: attn_mfma_fwd2_kernel / attn_mfma_bwd2_kernel<RC = true / false>
    ("bf16-37-stats", BF16, _lens(37), False, False, True, True, 0),
    ("bf16-37-probs", BF16, _lens(37), False, True, True, True, 0),
    ("bf16-64-stats", BF16, _lens(64), False, False, True, True, 0),
    ("bf16-64-probs", BF16, _lens(64), False, True, True, True, 0),
    # bf16, 64 < L <= 256 with ctx: attn_long_fwd_kernel, attn_long_bwd_dq_kernel, attn_long_bwd_dkv_kernel
    ("bf16-65-long", BF16, _lens(65), False, False, True, True, 0),
    ("bf16-130-long", BF16, _lens(130), False, False, True, True, 0),
    ("bf16-201-long", BF16, _lens(201), False, False, True, True, 0),
    ("bf16-256-long", BF16, _lens(256), False, False, True, True, 0),
    # bf16 backward without ctx: attn_bwd_kernel<bf16_t, 32 / 64, staged> (forward: attn_long_fwd_kernel)
    ("bf16-70-valu-bwd", BF16, _lens(70), False, False, False, True, 0),
    ("bf16-150-valu-bwd", BF16, _lens(150), False, False, False, True, 0),
    ("bf16-257-fwd", BF16, _lens(257), False, False, True, False, 0),   # attn_fwd_kernel<bf16_t>, forward only
    # packed bf16: one launch per length class (attn_mfma_*_kernel<CLS 1>, attn_mfma_*2_kernel<CLS 2>); the long kernels with seq_off
    ("bf16-packed-60", BF16, [60, 33, 5], True, False, True, True, 0),
    ("bf16-packed-201", BF16, [201, 130, 31], True, False, True, True, 0),
    ("bf16-31-ppw3", BF16, _lens(31), False, False, True, True, 3),     # attn_mfma_{fwd,bwd}_kernel<PPW = 3>
]


@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attention_mask_read_out(HF, Lb, seed_word, case):
    name, dtype, lens, packed, save_probs, give_ctx, backward, ppw = case
    site = SITES[ATTN_CASES.index(case) % 2]
    geo = DR.Geometry(lens, max(lens), packed)
    Lm, D, n_seq = geo.Lm, H * 64, geo.S
    drop, thr, scale = _drop(Lb, seed_word, site)
    keep = DR.attention_keep(SEED, site, thr, n_seq, H, Lm)
    live = geo.live()[:, None].expand(-1, H, -1, -1)
    assert 0.6 < float(keep[live].double().mean()) < 0.8
    qkv = DR.readout_qkv(geo, H, dtype).cuda()
    off = geo.seq_off().cuda() if packed else None
    key = torch.arange(Lm).reshape(1, 1, 1, -1)
    rtol = VALUE_RTOL[dtype]
    HF.ATTN_SAVE_PROBS = save_probs
    Lb.check(Lb.lib().hero_attention_force_ppw(ppw))
    try:
        # ---- forward: one launch per 64-key window, only that window's keys live
        fwd = DR.Pattern(geo, H)
        per_key = torch.zeros(n_seq, 1, 1, Lm, dtype=torch.float64)          # live keys of the window that key j is in
        for w in DR.windows(Lm):
            ctx, saved = HF.k_attn_fwd(qkv, geo.key_mask(w).cuda(), n_seq, Lm, H, drop=drop, seq_off=off)
            fwd.add_forward(ctx, w)
            cnt = torch.tensor([max(0, min(DR.WINDOW, n - w)) for n in geo.lens], dtype=torch.float64).reshape(-1, 1, 1, 1)
            inwin = live & (key >= w) & (key < w + DR.WINDOW)
            per_key = torch.where((key >= w) & (key < w + DR.WINDOW), cnt, per_key)
            assert (saved.dim() == 1) == (dtype == BF16 and Lm <= 64 and not save_probs)
            if saved.dim() == 4:                                             # the saved, UNDROPPED probabilities are 1 / live keys
                probs = saved.double().cpu()
                torch.testing.assert_close(probs[inwin], (1.0 / cnt).expand_as(live)[inwin], rtol=2.0 ** -22, atol=0)
                dead = live & ~inwin & (cnt > 0)
                assert not probs[dead].any()                                 # exp(-10000) is 0 in fp32
        assert fwd.complete()
        got = fwd.keep()
        assert torch.equal(got, keep & live), "forward: %d of %d live mask elements differ from the host draw" % (
            int((got != (keep & live)).sum()), int(live.sum()))
        want = (scale / per_key).expand_as(live)
        torch.testing.assert_close(fwd.value[keep & live], want[keep & live], rtol=rtol, atol=0)       # pins the 1 / (1 - p) scale
        if not backward:
            assert Lm > Lb.lib().hero_attention_max_len(Lb.dt(qkv), 1)
            return
        # ---- backward: all keys live, one launch per 64-row window of one-hot dctx rows
        madd = geo.key_mask().cuda()
        ctx, saved = HF.k_attn_fwd(qkv, madd, n_seq, Lm, H, drop=drop, seq_off=off)
        bwd = DR.Pattern(geo, H)
        for w in DR.windows(Lm):
            dctx = DR.readout_dctx(geo, H, w, dtype).cuda()
            dqkv = HF.k_attn_bwd(qkv, saved, dctx, n_seq, Lm, H, drop=drop, seq_off=off, ctx=ctx if give_ctx else None, mask_add=madd)
            assert not dqkv[:, :2 * D].any()                                 # q = k = 0: dq = dS k and dk = dS^T q are exact zeros
            bwd.add_backward(dqkv[:, 2 * D:], w)
        assert bwd.complete()
        got = bwd.keep()
        assert torch.equal(got, keep & live), "backward: %d of %d live mask elements differ from the host draw" % (
            int((got != (keep & live)).sum()), int(live.sum()))
        n = torch.tensor(geo.lens, dtype=torch.float64).reshape(-1, 1, 1, 1)
        torch.testing.assert_close(bwd.value[keep & live], (scale / n).expand_as(live)[keep & live], rtol=rtol, atol=0)
    finally:
        HF.ATTN_SAVE_PROBS = False
        Lb.check(Lb.lib().hero_attention_force_ppw(0))


# ==== Tier B =========================================================================================================================
VALUE_CASES = [
    ("f32-9", F32, _lens(9), False, True, True), ("f32-23", F32, _lens(23), False, True, True), ("f32-61", F32, _lens(61), False, True, True),
    ("f32-70", F32, _lens(70), False, True, True), ("f32-130", F32, _lens(130), False, True, True), ("f32-150", F32, _lens(150), False, True, True),
    ("f32-packed-24", F32, [24, 9, 1, 17], True, True, True),
    ("bf16-31", BF16, _lens(31), False, True, True), ("bf16-37", BF16, _lens(37), False, True, True),
    ("bf16-130-long", BF16, _lens(130), False, True, True), ("bf16-150-valu-bwd", BF16, _lens(150), False, False, True),
    ("bf16-257-fwd", BF16, _lens(257), False, True, False),
    ("bf16-packed-60", BF16, [60, 33, 5], True, True, True), ("bf16-packed-201", BF16, [201, 130, 31], True, True, True),
]


@pytest.mark.parametrize("case", VALUE_CASES, ids=[c[0] for c in VALUE_CASES])
def test_attention_values_against_float64(HF, Lb, seed_word, case):
    """Random q, k, v, dctx, the first key of sequence 1 masked: every output against tests/dropout_reference.attention_ref
    on the inputs as stored, the multipliers from the host draw.  bf16 lengths with row statistics run both ways."""
    name, dtype, lens, packed, give_ctx, backward = case
    site = SITES[(VALUE_CASES.index(case) + 1) % 2]
    geo = DR.Geometry(lens, max(lens), packed)
    Lm, D, n_seq = geo.Lm, H * 64, geo.S
    drop, thr, scale = _drop(Lb, seed_word, site)
    mult = DR.attention_keep(SEED, site, thr, n_seq, H, Lm).double() * scale
    qkv, dctx = rnd(geo.rows, 3 * D, dtype=dtype, seed=1), rnd(geo.rows, D, dtype=dtype, seed=2)
    madd = geo.key_mask()
    if lens[1] > 1:
        madd[1, 0] = DR.MASKED
    off = geo.seq_off().cuda() if packed else None
    written = geo.live()[:, None].expand(-1, H, -1, -1) if packed else torch.ones(n_seq, H, Lm, Lm, dtype=torch.bool)
    ref = DR.attention_ref(qkv, madd, geo, H, mult=mult, dctx=dctx)
    t = TOL[dtype]
    modes = (False, True) if Lb.lib().hero_attention_stats_ok(Lb.dt(qkv), Lm) else (False,)
    try:
        for save_probs in modes:
            HF.ATTN_SAVE_PROBS = save_probs
            tag = "%s%s " % (name, "/probs" if save_probs else "")
            ctx, saved = HF.k_attn_fwd(qkv, madd.cuda(), n_seq, Lm, H, drop=drop, seq_off=off)
            if saved.dim() == 4:                                     # (a packed batch writes only the rows and keys that exist)
                _within(tag + "probs", saved.cpu()[written], ref["probs"][written], **PTOL[dtype])
            _within(tag + "ctx", ctx, ref["ctx"], t["rtol"], t["atol"])
            if not backward:
                continue
            dqkv = HF.k_attn_bwd(qkv, saved, dctx, n_seq, Lm, H, drop=drop, seq_off=off, ctx=ctx if give_ctx else None, mask_add=madd.cuda())
            for k, key in enumerate(("dq", "dk", "dv")):
                _within(tag + key, dqkv[:, k * D:(k + 1) * D], ref[key], t["rtol"], 2 * t["atol"])       # close(..., scale=2)
    finally:
        HF.ATTN_SAVE_PROBS = False


# ==== Tier C =========================================================================================================================
LN_DTYPES = [(F32, F32), (F32, BF16), (BF16, BF16)]                 # (x, y / dy)
LN_IDS = ["f32-f32", "f32-bf16", "bf16-bf16"]


def _ln_inputs(rows, cols, xdt):
    x = rnd(rows, cols, dtype=xdt, seed=1) * 2 + 0.5
    return x, rnd(cols, seed=2) * 0.1 + 1, rnd(cols, seed=3) * 0.1


@pytest.mark.parametrize("dts", LN_DTYPES, ids=LN_IDS)
@pytest.mark.parametrize("cols", [132, 516, 4352, 1028, 256, 768])
def test_layernorm_forward_mask_read_out(HF, Lb, seed_word, dts, cols):
    """ln_fwd_kernel (132: VPL 1, 516: VPL 3, 1028: VPL 6, 4352: VPL 17, the last chunk partly past the row) and
    ln_fwd_full_kernel (256, 768).  9 rows: the last workgroup holds one row."""
    rows, (xdt, ydt) = 9, dts
    site = SITES[cols % 8 == 0]
    x, g, b = _ln_inputs(rows, cols, xdt)
    drop, thr, scale = _drop(Lb, seed_word, site)
    keep = DR.ln_keep(SEED, site, thr, rows, cols)
    y0, _, _, _ = HF.k_ln_fwd(x, g, b, 1e-12, ydt, rows, cols)
    y, _, _, _ = HF.k_ln_fwd(x, g, b, 1e-12, ydt, rows, cols, drop=drop)
    assert torch.equal(DR.ln_forward_keep(y, y0), keep)              # (asserts that y0 has no zero)
    y, want = y.double().cpu(), y0.double().cpu() * scale
    torch.testing.assert_close(y[keep], want[keep], rtol=VALUE_RTOL[ydt], atol=0)


@pytest.mark.parametrize("dts", LN_DTYPES, ids=LN_IDS)
@pytest.mark.parametrize("cols,params", [(132, True), (516, True), (256, True), (768, True), (132, False), (1028, True), (4352, False)])
def test_layernorm_input_mask_read_out(HF, Lb, seed_word, dts, cols, params):
    """The mask of the dropout in FRONT of the LayerNorm, replayed on dx: ln_bwd_fused_kernel (132, 516), ln_bwd_fused_full_kernel
    (256, 768), ln_bwd_dx_kernel (no parameter gradients, or more than 1024 columns)."""
    rows, (xdt, dt) = 9, dts
    site = SITES[cols % 8 != 0]
    x, g, b = _ln_inputs(rows, cols, xdt)
    dy = rnd(rows, cols, dtype=dt, seed=4)
    drop, thr, scale = _drop(Lb, seed_word, site)
    keep = DR.ln_keep(SEED, site, thr, rows, cols)
    _, mean, rstd, _ = HF.k_ln_fwd(x, g, b, 1e-12, dt, rows, cols)
    dx, dxd, _, _ = HF.k_ln_bwd(x, dy, g, mean, rstd, want_params=params, drop_in=drop)
    got, decided = DR.ln_input_keep(dx, dxd)
    assert bool(decided.all())                                       # no exact zero in dx: every element decides
    assert torch.equal(got, keep)
    dxd, want = dxd.double().cpu(), dx.double().cpu() * scale
    torch.testing.assert_close(dxd[keep], want[keep], rtol=VALUE_RTOL[dt], atol=0)


COLSUM_CASES = [(21, 1028, F32, None), (21, 1028, BF16, None), (70, 1028, F32, None)] + \
               [(9, c, d, None) for c in (132, 516, 256, 768) for d in (F32, BF16)] + \
               [(4 * 1024 + 5, 256, d, [(0, 16), (4096, 5)]) for d in (F32, BF16)]


@pytest.mark.parametrize("rows,cols,dtype,wins", COLSUM_CASES, ids=["%dx%d-%s" % (r, c, "f32" if d == F32 else "bf16") for r, c, d, _ in COLSUM_CASES])
def test_layernorm_output_mask_in_the_column_sums(HF, Lb, seed_word, rows, cols, dtype, wins):
    """The output mask as the COLUMN SUMS see it.  p = 1/2, dy[r, :] = 2^(r - r0) on a window of <= 16 rows: dbeta / 2 spells
    the window's mask in binary, exactly (fp32 sums of distinct powers of two below 2^16, in any order).
    1028 columns: colred_kernel (21 rows: a 16-row chunk in one 4-row trip and a 5-row chunk in the tail loop; 70: four trips
    and a 6-row tail); 132 / 516: ln_bwd_fused_kernel; 256 / 768: ln_bwd_fused_full_kernel; 4101 rows: the fused kernel's
    second grid-stride trip (rows 4096 .. 4100) must draw with the true row number."""
    site = SITES[rows % 2]
    x, g, b = _ln_inputs(rows, cols, dtype)
    drop, thr, scale = _drop(Lb, seed_word, site, p=0.5)
    assert thr == 32768 and scale == 2.0
    keep = DR.ln_keep(SEED, site, thr, rows, cols)
    _, mean, rstd, _ = HF.k_ln_fwd(x, g, b, 1e-12, dtype, rows, cols)
    for r0, n in (wins or DR.colsum_windows(rows)):
        dy = DR.colsum_dy(rows, cols, r0, n, dtype).cuda()
        _, _, _, dbeta = HF.k_ln_bwd(x, dy, g, mean, rstd, drop_out=drop)
        got = DR.colsum_decode(dbeta, n, scale)
        assert torch.equal(got, keep[r0:r0 + n]), "rows %d..%d: %d mask elements differ from the host draw" % (
            r0, r0 + n - 1, int((got != keep[r0:r0 + n]).sum()))


# ==== Tier D =========================================================================================================================
@pytest.mark.parametrize("cols,dtype", [(516, F32), (516, BF16), (768, F32), (768, BF16), (1028, F32)],
                         ids=["516-f32", "516-bf16", "768-f32", "768-bf16", "1028-f32"])
def test_layernorm_values_against_float64(HF, Lb, seed_word, cols, dtype):
    """Output and input dropout together, accumulating (grad_beta = 1), with the feeding linear's bias gradient where the
    library has it (up to 1024 columns): everything against float64 with the two masks from the host draw.
    dy = +-(0.5 + |randn|): one flipped output-mask element moves its own dx entry by |dy| scale gamma rstd (1 - (1 + xhat^2) /
    cols) >= 0.5 scale gamma rstd (1 - ...), which the test checks to be above the tolerance of that entry."""
    rows, eps = 21, 1e-12
    x, g, b = _ln_inputs(rows, cols, dtype)
    r = rnd(rows, cols, seed=4)
    dy = (torch.sign(r) * (0.5 + r.abs())).to(dtype)
    d_out, thr, scale = _drop(Lb, seed_word, SITES[1])
    d_in, _, _ = _drop(Lb, seed_word, SITES[0])
    m_out = DR.ln_keep(SEED, SITES[1], thr, rows, cols).double() * scale
    m_in = DR.ln_keep(SEED, SITES[0], thr, rows, cols).double() * scale
    ref = DR.ln_bwd_ref(x, g, eps, dy, mult_out=m_out, mult_in=m_in)
    t = TOL[dtype]
    tol_dx = 3 * t["atol"] + t["rtol"] * ref["dx"].abs()                         # close(..., scale=3)
    xhat = (x.double().cpu() - x.double().cpu().mean(-1, keepdim=True)) * ref["rstd"]
    shift = 0.5 * scale * g.double().cpu().abs() * ref["rstd"] * (1.0 - (1.0 + xhat ** 2) / cols)
    print("\n[dropout] ln %d: least shift of a flipped mask element / tolerance %.2f" % (cols, float((shift / tol_dx).min())), end="")
    assert bool((shift > tol_dx).all())
    y, mean, rstd, _ = HF.k_ln_fwd(x, g, b, eps, dtype, rows, cols, drop=d_out)
    _within("ln %d y" % cols, y, DR.ln_ref(x, g, b, eps, mult_out=m_out), t["rtol"], 3 * t["atol"])
    dg, db = torch.ones(cols, device="cuda"), torch.full((cols,), 2.0, device="cuda")
    dbias = torch.full((cols,), 3.0, device="cuda") if cols <= 1024 else None
    dx, dxd, _, _ = HF.k_ln_bwd(x, dy, g, mean, rstd, drop_out=d_out, drop_in=d_in, dgamma=dg, dbeta=db, grad_beta=1.0,
                                want_params=False, dbias_in=dbias)
    _within("ln %d dx" % cols, dx, ref["dx"], t["rtol"], 3 * t["atol"])
    _within("ln %d dx_dropped" % cols, dxd, ref["dx_dropped"], t["rtol"], 3 * t["atol"])
    bf = dtype == BF16
    _within("ln %d dgamma" % cols, dg, 1 + ref["dgamma"], 2e-2 if bf else 1e-4, 0.3 if bf else 1e-3)     # _ln_param_close
    _within("ln %d dbeta" % cols, db, 2 + ref["dbeta"], 1e-4, 1e-3)
    if dbias is not None:
        _within("ln %d dbias_in" % cols, dbias, 3 + ref["dbias_in"], 1e-4, 1e-3)
