"""The output stores of the bf16 matrix-core attention kernels (attention_mfma.hip, attention_mfma_long.hip): the tiles leave
through the LDS as 16-byte row segments.  Every case compares ctx and dQ | dK | dV with an fp32 torch restatement at the
tolerances of tests/test_gpu_kernels.py's attention tests, and checks what only a store path can break:

  guard rows      the outputs are views into larger buffers pre-filled with a bit pattern; every row outside the sequences (in
                  front of the first, behind the last, and in packed batches outside [seq_off[s], seq_off[s + 1])) still holds
                  it afterwards - a 32-row store tile must not write rows >= L
  column windows  head h's 64 columns of ctx and of each third of dqkv hold head h's data: V and dctx carry a different scale
                  per head, and the comparison is made window by window

Needs a real MI355X (-m gpu)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
TOL = dict(rtol=2e-2, atol=2e-2)          # tests/test_gpu_kernels.py: TOL[bfloat16]; dqkv is compared with atol x 2 there
SENT = 0x5A5A                             # bf16 1.5e16: no kernel output comes near it
G = 40                                    # guard rows on either side: more than one 32-row store tile


@pytest.fixture(scope="module")
def HF():
    from hero_amd import functional
    return functional


@pytest.fixture(scope="module")
def Lb():
    from hero_amd import _lib
    _lib.lib()
    return _lib


def guarded(rows, cols):
    big = torch.empty(rows + 2 * G, cols, dtype=BF16, device="cuda")
    big.view(torch.int16).fill_(SENT)
    return big, big[G:G + rows]


def assert_guards(big, written, what):
    """written: bool [rows] - the rows of the view (big[G : G + rows]) that belong to a sequence."""
    keep = torch.ones(big.shape[0], dtype=torch.bool, device="cuda")
    keep[G:G + written.numel()] = ~written
    raw = big.view(torch.int16)[keep]
    bad = (raw != SENT).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, "%s: %d guard rows were written (first: buffer row %d of the kept rows)" % (what, bad.numel(), int(bad[0]))


def keep_mask(HF, drop, lens, offs, rows, Lmax, H, off_t):
    """The dropout decisions of this site, [S, H, Lmax, Lmax] (1 = kept), read off the fp32 VALU kernels (attention.hip draws the
    same mask for the same site): q = k = 0 gives uniform probabilities, V = one key per head dim gives ctx[i, j] > 0 <=> kept."""
    D = H * 64
    x = torch.zeros(rows, 3 * D, device="cuda")
    for o, n in zip(offs, lens):
        for h in range(H):
            x[o:o + n, 2 * D + h * 64:2 * D + h * 64 + n] = torch.eye(n, device="cuda")
    c, _ = HF.k_attn_fwd(x, None, len(lens), Lmax, H, drop=drop, want_probs=False, seq_off=off_t)
    keep = torch.zeros(len(lens), H, Lmax, Lmax, device="cuda")
    for s, (o, n) in enumerate(zip(offs, lens)):
        keep[s, :, :n, :n] = (c[o:o + n].reshape(n, H, 64)[:, :, :n] > 0).permute(1, 0, 2).float()
    return keep


def run_case(HF, Lb, lens, Lmax, H, packed, use_mask, p_drop=0.0, ppw=(0,), lead=0, seed=0):
    """lens: rows per sequence; packed: through seq_off (first sequence at row `lead`), else all lens == Lmax."""
    D, S = H * 64, len(lens)
    offs = [lead]
    for n in lens:
        offs.append(offs[-1] + n)
    rows = offs[-1]
    offs = offs[:-1]
    off_t = torch.tensor(offs + [rows], dtype=torch.int32).cuda() if packed else None
    g = torch.Generator().manual_seed(1000 * seed + 7 * Lmax + S)
    head_scale = (0.4 + 0.6 * torch.arange(H).flip(0) / max(H - 1, 1)).repeat_interleave(64)      # <= 1: errors stay below the unit-scale case
    x = torch.randn(rows, 3 * D, generator=g)
    x[:, 2 * D:] *= head_scale
    qkv = x.to(BF16).cuda()
    dctx = (torch.randn(rows, D, generator=g) * head_scale).to(BF16).cuda()
    madd = None
    if use_mask:
        m = torch.ones(S, Lmax)
        for s, n in enumerate(lens):
            if n >= 3:
                m[s, s % n] = 0
        madd = ((1 - m) * -10000.0).cuda()
    written = torch.zeros(rows, dtype=torch.bool, device="cuda")
    for o, n in zip(offs, lens):
        written[o:o + n] = True
    drop = HF.RNG.make(p_drop, True, qkv.device) if p_drop > 0 else None
    if drop is not None:
        assert Lmax <= 64
        keep = keep_mask(HF, drop, lens, offs, rows, Lmax, H, off_t) / (1.0 - p_drop)

    # fp32 torch reference, sequence by sequence
    q = qkv.float().requires_grad_(True)
    ref = torch.zeros(rows, D, device="cuda")
    for s, (o, n) in enumerate(zip(offs, lens)):
        if n == 0:
            continue
        qq, kk, vv = [t.reshape(n, H, 64).permute(1, 0, 2) for t in q[o:o + n].split(D, dim=1)]
        sc = qq @ kk.transpose(-1, -2) / 8.0
        if madd is not None:
            sc = sc + madd[s, :n][None, None, :]
        pr = torch.softmax(sc, -1)
        if drop is not None:
            pr = pr * keep[s, :, :n, :n]
        ref[o:o + n] = (pr @ vv).permute(1, 0, 2).reshape(n, D)
    ref.backward(dctx.float())
    ref, gref = ref.detach(), q.grad

    def windows(got, want, cols0, atol_scale, what):
        for h in range(H):
            c0 = cols0 + h * 64
            try:
                torch.testing.assert_close(got[written][:, c0:c0 + 64].float(), want[written][:, c0:c0 + 64],
                                           rtol=TOL["rtol"], atol=TOL["atol"] * atol_scale)
            except AssertionError as e:
                raise AssertionError("%s, head %d (columns %d..%d): %s" % (what, h, c0, c0 + 63, e)) from None

    # forward, twice: same bits
    big_c, ctx = guarded(rows, D)
    _, saved = HF.k_attn_fwd(qkv, madd, S, Lmax, H, drop=drop, out=ctx, seq_off=off_t)
    big_c2, ctx2 = guarded(rows, D)
    HF.k_attn_fwd(qkv, madd, S, Lmax, H, drop=drop, out=ctx2, seq_off=off_t)
    assert torch.equal(big_c.view(torch.int16), big_c2.view(torch.int16)), "forward repeat: other bits"
    assert_guards(big_c, written, "ctx")
    windows(ctx, ref, 0, 1, "ctx")

    # backward, for every requested pairs-per-wave setting
    first = None
    for p in ppw:
        big_d, dqkv = guarded(rows, 3 * D)
        Lb.check(Lb.lib().hero_attention_force_ppw(p))
        try:
            HF.k_attn_bwd(qkv, saved, dctx, S, Lmax, H, drop=drop, out=dqkv, seq_off=off_t, ctx=ctx, mask_add=madd)
        finally:
            Lb.check(Lb.lib().hero_attention_force_ppw(0))
        assert_guards(big_d, written, "dqkv (ppw %d)" % p)
        for t, name in enumerate(("dQ", "dK", "dV")):
            windows(dqkv, gref, t * D, 2, "%s (ppw %d)" % (name, p))
        if first is None:
            first = big_d
        else:
            assert torch.equal(first.view(torch.int16), big_d.view(torch.int16)), "pairs per wave %d: other bits" % p


@pytest.mark.parametrize("S", [1, 3, 5])
@pytest.mark.parametrize("L", [1, 7, 8, 9, 15, 16, 17, 24, 31, 32])
def test_short_class_store_group_boundaries(HF, Lb, S, L):
    """One wave per (sequence, head) pair, four waves per workgroup: 12 / 36 / 60 pairs = fewer pairs than one workgroup's waves
    hold heads of one sequence only, a pair count that is no multiple of 4 x pairs-per-wave, L across the 8-row store groups."""
    run_case(HF, Lb, [L] * S, L, 12, packed=False, use_mask=True)


@pytest.mark.parametrize("L", [15, 24])
@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_short_class_mask_and_dropout(HF, Lb, L, use_mask, p_drop):
    """L = 24: mask rows by 16-byte loads (M4); L = 15: scalar mask loads; no mask: the select path."""
    run_case(HF, Lb, [L] * 3, L, 12, packed=False, use_mask=use_mask, p_drop=p_drop, seed=1)


@pytest.mark.parametrize("L", [9, 15, 24])
def test_backward_pairs_per_wave_restage_the_store_tiles(HF, Lb, L):
    """The staged dQ / dK / dV tiles are the K / Q / dO tiles the wave's NEXT pair restages: 1, 2 and 3 pairs per wave (60 pairs =
    60 / 30 / 20 waves) give the reference's values, untouched guards and the same bits."""
    run_case(HF, Lb, [L] * 5, L, 12, packed=False, use_mask=True, p_drop=0.1, ppw=(1, 2, 3), seed=2)


@pytest.mark.parametrize("L", [33, 40, 60, 64])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_64_row_class(HF, Lb, L, p_drop):
    """Two waves per pair: each stages rows [32 w, 32 w + 32) of the shared tiles."""
    run_case(HF, Lb, [L] * 2, L, 12, packed=False, use_mask=True, p_drop=p_drop, seed=3)


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_packed_batch_both_length_classes(HF, Lb, p_drop):
    """seq_off with an empty sequence, both launch classes (<= 32 rows: one wave per pair; longer: two), first sequence at row 5."""
    run_case(HF, Lb, [0, 5, 24, 32, 33, 48], 48, 12, packed=True, use_mask=True, p_drop=p_drop, lead=5, seed=4)
    run_case(HF, Lb, [24, 15, 0, 9], 24, 12, packed=True, use_mask=False, p_drop=p_drop, lead=0, ppw=(1, 2, 3), seed=5)


@pytest.mark.parametrize("L", [100, 256])
def test_long_class(HF, Lb, L):
    """One workgroup per pair, one wave per 32-row tile: dK / dV leave through the wave's P | dS tiles, ctx and dQ directly."""
    run_case(HF, Lb, [L], L, 12, packed=False, use_mask=True, seed=6)
