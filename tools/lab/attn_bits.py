#!/usr/bin/env python3
"""Raw bits of the attention kernels - the bf16 matrix-core ones (attention_mfma.hip, attention_mfma_long.hip) and the fp32-VALU
ones (attention.hip, every row of the dispatch table in its header) - on a fixed list of small cases, to compare two library
builds: a refactor of the kernels must not move one bit.

  python tools/lab/attn_bits.py save OUT.pt       run every case through HF.k_attn_fwd / HF.k_attn_bwd, torch.save the results
  python tools/lab/attn_bits.py compare A.pt B.pt  torch.equal on the raw bits, per case and tensor; exit status 1 on a difference

One `save` process per build (HERO_HIP_LIB selects the library), then `compare`.

Every case: additive mask with one masked key per sequence, fixed seeds.  Saved per case: ctx and dqkv WITH their guard rows
(views into larger buffers pre-filled with a bit pattern, as in tests/test_gpu_attention_stores.py: the rows the kernels must
leave alone are compared too) and what the forward saves for the backward (row statistics or fp32 probabilities).
The long cases (L > 64) run with saved probabilities only: row statistics exist up to 64 rows (hero_attention_stats_ok), beyond
that k_attn_fwd saves the probabilities whatever ATTN_SAVE_PROBS says, so there is no second mode to cover.  The saved tensor
is allocated by k_attn_fwd: its entries outside the sequences (packed batches) are never written and are zeroed before saving.
The VALU cases: f32 on both sides of every length at which run<float>() changes kernels (16 | 17, 32 | 33, 64 | 65, 128 | 129,
144 | 145, up to 256) and one packed batch; bf16 backward WITHOUT ctx (the only bf16 backward that leaves the matrix cores);
the bf16 forward at 257 rows, which has no backward."""
import os, sys
sys.path.insert(0, os.getcwd())
import torch

BF16 = torch.bfloat16
F32 = torch.float32
SENT = 0x5A5A                             # per 16-bit half: the same pattern fills an f32 buffer
G = 40                                    # guard rows on either side: more than one 32-row store tile


def cases():
    """(name, lens, Lmax, H, packed, lead, ppw, save_probs, p_drop, dtype, bwd) - bwd: "ctx" (backward given the forward
    output), "noctx" or None (forward only)"""
    out = []
    for p in (0.0, 0.1):
        for probs in (False, True):
            for L in (1, 9, 24, 32):              # one wave per pair; 9: scalar mask / probability path, 24: the 16-byte one
                for ppw in (1, 2, 3):
                    out.append(("one-wave L%d ppw%d" % (L, ppw), [L] * 5, L, 3, False, 0, ppw, probs, p))
            for L in (33, 60, 64):                # two waves per pair
                out.append(("two-wave L%d" % L, [L] * 2, L, 2, False, 0, 0, probs, p))
            out.append(("packed", [24, 0, 40, 9, 64], 64, 2, True, 5, 0, probs, p))      # both length classes, an empty sequence
        for L in (65, 100, 129, 256):             # one workgroup per pair: both tile counts, partial last tiles
            out.append(("long L%d" % L, [L] * 2, L, 2, False, 0, 0, True, p))
    out = [c + (BF16, "ctx") for c in out]
    for p in (0.0, 0.1):
        for L in (1, 9, 16, 17, 32, 33, 64):      # small kernels: 4 / 2 / 1 lanes per key
            out.append(("f32 small L%d" % L, [L] * 3, L, 2, False, 0, 0, True, p, F32, "ctx"))
        out.append(("f32 packed", [24, 0, 40, 9, 64], 64, 2, True, 5, 0, True, p, F32, "ctx"))
        for L in (65, 128, 129, 144, 145, 256):   # backward: 32 | 64 keys per wave, Q and dO staged | read from global memory
            out.append(("f32 long L%d" % L, [L] * 2, L, 2, False, 0, 0, True, p, F32, "ctx"))
        for L in (65, 128, 129, 256):
            out.append(("bf16 valu bwd L%d" % L, [L] * 2, L, 2, False, 0, 0, True, p, BF16, "noctx"))
        out.append(("bf16 valu fwd L257", [257], 257, 2, False, 0, 0, True, p, BF16, None))
    return [(("%s %s drop%.1f" % (c[0], "probs" if c[7] else "stats", c[8])),) + c[1:] for c in out]


def guarded(rows, cols, dtype):
    big = torch.empty(rows + 2 * G, cols, dtype=dtype, device="cuda")
    big.view(torch.int16).fill_(SENT)
    return big, big[G:G + rows]


def run_case(HF, Lb, lens, Lmax, H, packed, lead, ppw, save_probs, p_drop, dtype, bwd):
    D, S = H * 64, len(lens)
    offs = [lead]
    for n in lens:
        offs.append(offs[-1] + n)
    rows = offs[-1]
    off_t = torch.tensor(offs, dtype=torch.int32).cuda() if packed else None
    g = torch.Generator().manual_seed(7 * Lmax + S)
    qkv = torch.randn(rows, 3 * D, generator=g).to(dtype).cuda()
    dctx = torch.randn(rows, D, generator=g).to(dtype).cuda()
    madd = torch.zeros(S, Lmax)
    for s, n in enumerate(lens):
        if n >= 3:
            madd[s, s % n] = -10000.0
    madd = madd.cuda()
    HF.manual_seed(1234, "cuda:0")
    drop = HF.RNG.make(p_drop, True, qkv.device)
    big_c, ctx = guarded(rows, D, dtype)
    big_d, dqkv = guarded(rows, 3 * D, dtype)
    probs_before = HF.ATTN_SAVE_PROBS
    try:
        HF.ATTN_SAVE_PROBS = save_probs
        Lb.check(Lb.lib().hero_attention_force_ppw(ppw))
        _, saved = HF.k_attn_fwd(qkv, madd, S, Lmax, H, drop=drop, out=ctx, seq_off=off_t)
        if bwd:
            HF.k_attn_bwd(qkv, saved, dctx, S, Lmax, H, drop=drop, out=dqkv, seq_off=off_t, ctx=ctx if bwd == "ctx" else None, mask_add=madd)
    finally:
        Lb.check(Lb.lib().hero_attention_force_ppw(0))
        HF.ATTN_SAVE_PROBS = probs_before
    torch.cuda.synchronize()
    is_stats = saved.dim() == 1
    sv = saved.view(S, H, Lmax, 2) if is_stats else saved
    valid = torch.zeros_like(sv, dtype=torch.bool)
    for s, n in enumerate(lens):
        if is_stats:
            valid[s, :, :n] = True
        else:
            valid[s, :, :n, :n] = True
    sv = torch.where(valid, sv, torch.zeros_like(sv))
    return {"ctx": big_c.view(torch.int16).cpu(), "stats" if is_stats else "probs": sv.view(torch.int32).cpu(),
            "dqkv": big_d.view(torch.int16).cpu()}


def save(path):
    from hero_amd import functional as HF, _lib as Lb
    res = {}
    for c in cases():
        res[c[0]] = run_case(HF, Lb, *c[1:])
    torch.save(res, path)
    print("%d cases from %s -> %s" % (len(res), Lb.LIB_PATH, path))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%-40s only in one file" % name)
            bad += 1
            continue
        line = []
        for t in sorted(set(a[name]) | set(b[name])):
            x, y = a[name].get(t), b[name].get(t)
            same = x is not None and y is not None and x.shape == y.shape and torch.equal(x, y)
            bad += not same
            line.append("%s %s" % (t, "equal" if same else "DIFFERENT"))
        print("%-40s %s" % (name, "  ".join(line)))
    print("%d cases, %d differences" % (len(a), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "save":
        save(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
