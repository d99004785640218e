#!/usr/bin/env python3
"""Isolated attention launches, one line per launch class, hipGraph timing (profiles/attn_store_ab.txt).  Run once per library
build (HERO_HIP_LIB), alternating the builds between processes:
  short    the bench batch's launch: 480 sequences x 24 rows + 32 x 15 rows as one packed launch, 12 heads, mask, dropout 0.1,
           row statistics (attn_mfma_fwd_kernel / attn_mfma_bwd_kernel)
  ragged   480 sequences of 8..48 rows (drawn once, fixed seed) as one packed launch: both length classes at once, the one-wave
           kernels on the sequences of <= 32 rows (CLS = 1) and the two-wave kernels on the longer ones (CLS = 2)
  64-row   the Temporal Transformer's: 32 x 60 rows (attn_mfma_fwd2_kernel / attn_mfma_bwd2_kernel)
  long     32 x 100 and 32 x 256 rows, saved probabilities (attn_long_*)"""
import os, sys, time
sys.path.insert(0, os.getcwd())
import torch
from hero_amd import functional as HF
dt = torch.bfloat16
H = 12
D = H * 64
drop = HF.RNG.make(0.1, True, torch.device("cuda", 0))


def t(fn, reps=10):
    end = time.time() + 0.25
    while time.time() < end:
        fn()
    torch.cuda.synchronize()
    gs = torch.cuda.Stream(); gs.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(gs):
        with torch.cuda.graph(gr, stream=gs):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(gs)
    gr.replay(); torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            gr.replay()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1000 / reps / 5)
    return best


def one(name, lens, Lmax, packed):
    S, M = len(lens), sum(lens)
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = torch.randn(M, 3 * D, device="cuda", generator=g).to(dt)
    dctx = torch.randn(M, D, device="cuda", generator=g).to(dt)
    madd = torch.zeros(S, Lmax, device="cuda")
    madd[:, -2:] = -10000.0
    off = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32).cuda() if packed else None
    ctx = torch.empty(M, D, device="cuda", dtype=dt)
    dq = torch.empty_like(qkv)
    _, saved = HF.k_attn_fwd(qkv, madd, S, Lmax, H, drop=drop, out=ctx, seq_off=off)
    f = t(lambda: HF.k_attn_fwd(qkv, madd, S, Lmax, H, drop=drop, out=ctx, seq_off=off))
    b = t(lambda: HF.k_attn_bwd(qkv, saved, dctx, S, Lmax, H, drop=drop, out=dq, seq_off=off, ctx=ctx, mask_add=madd))
    print("%-20s %-22s fwd %6.1f us  bwd %6.1f us" % (tag, name, f, b), flush=True)


tag = os.environ.get("HERO_HIP_LIB", "product").split("/")[-1]
one("short 480x24+32x15", [24] * 480 + [15] * 32, 24, True)
one("ragged 480x(8..48)", torch.randint(8, 49, (480,), generator=torch.Generator().manual_seed(5)).tolist(), 48, True)
one("64-row 32x60", [60] * 32, 60, False)
one("long 32x100", [100] * 32, 100, False)
one("long 32x256", [256] * 32, 256, False)
