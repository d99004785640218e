#!/usr/bin/env python3
"""What the transformer block functions of hero_amd/functional.py LAUNCH and what comes out, to compare two source trees on one
library build (HERO_HIP_LIB): run from each tree's root (`cd .ab/<sha> && python <this file> [LOGDIR]`, tools/lab/ab_trees.sh).
Every call into the library is logged - export name, scalar arguments, struct fields; pointers as the ordinal of their first
appearance, so aliasing is compared and addresses are not.  Per case one line: calls, SHA-256 of that log, SHA-256 of the loss
and every parameter gradient's bits after two optimiser steps, torch.cuda.max_memory_allocated().  LOGDIR: keep the logs too."""
import ctypes as C, gc, hashlib, os, sys, types
sys.path.insert(0, os.getcwd())
import torch, hero_amd
from hero_amd import functional as HF, _lib as Lb
from hero_amd.model.layers import BertEncoder
from hero_amd.optim import AdamW

LOG, IDS = [], {}


def norm(v, kind=None):
    if isinstance(v, C.Structure):
        return [norm(getattr(v, f[0]), f[1]) for f in v._fields_]
    if isinstance(v, C.Array):
        return [norm(x, v._type_) for x in v]
    if hasattr(v, "_obj"):                                   # C.byref(struct)
        return norm(v._obj)
    if kind is C.c_void_p or (isinstance(v, int) and v >= 1 << 40):
        return "null" if not v else "p%d" % IDS.setdefault(v, len(IDS))
    return v.value if hasattr(v, "value") else v


class Recorder:
    def __init__(self, real):
        self.real = real

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        return lambda *a: (LOG.append("%s %r" % (name, [norm(x, k) for x, k in zip(a, fn.argtypes or [None] * len(a))])), fn(*a))[1]


def trainer(model, loss_fn):
    opt = AdamW(model.parameters(), lr=1e-3)

    def step():
        loss = loss_fn()
        loss.backward()
        opt.step()
        HF.refresh_weight_cache()
        return loss
    return model, step


def encoder(hidden, heads, layers, groups, packed=False, freeze=False, chain=False):
    cfg = types.SimpleNamespace(hidden_size=hidden, num_attention_heads=heads, num_hidden_layers=layers, intermediate_size=2 * hidden,
                                hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, layer_norm_eps=1e-12)
    torch.manual_seed(0)
    enc = BertEncoder(cfg).cuda().train()
    enc.pack_ragged = packed
    for layer in enc.layer if freeze else ():
        layer.attention.output.dense.bias.requires_grad = layer.intermediate.dense.bias.requires_grad = False
    hs = [torch.randn(S, Lq, hidden, device="cuda", requires_grad=True) for S, Lq in groups]
    masks = [torch.ones(S, Lq, dtype=torch.int64, device="cuda") for S, Lq in groups]
    for m in masks:                                          # ragged: sequence 0 full, sequence 1 one valid position, the rest short
        m[1, 1:] = 0
        m[2:, m.shape[1] // 2:] = 0

    def outputs():
        if chain:                                            # the unfused module chain: SelfAttentionFn, ProjResLnFn, LinearFn
            x, at, lay = HF.cast(hs[0], HF.compute_dtype()), enc.layer[0].attention, enc.layer[0]
            a = at.output(at.self(x, masks[0])[0], x)
            return [lay.output(lay.intermediate(a), a)]
        return enc.forward_multi(hs, masks)
    return trainer(enc, lambda: sum(o.float().pow(2).mean() for o in outputs()))


def tvc():
    from tests import test_gpu_tvc as T                      # the smallest TVC shape the suite has: its golden batch
    model, b = T.load_model(True, 0.1), T.load_batch()
    return trainer(model, lambda: model.caption_loss(b))


def train_step():
    from hero_amd.step import TrainStep
    from oracle import hero_oracle as O
    from tests.util import GOLDEN, load_tiny, to_dev
    model = load_tiny("cuda")[0].train()
    b = to_dev(O.load_npz_case(os.path.join(GOLDEN, "case_train.npz"))[0], "cuda")
    ts = TrainStep(model, opts=dict(learning_rate=1e-3, warmup_steps=2, num_train_steps=100), use_graph=True)
    it = iter([lambda: ts.micro_step(b)] * 4 + [lambda: (HF.clear_weight_cache(), ts.micro_step(b, eager=True))[1]])
    return model, lambda: next(it)()


AB = ((3, 24), (2, 15))
SINK = type("OverlapSink", (HF.GradSink,), {"wants_overlap": lambda self: True})
CASES = [("a two padded groups", torch.bfloat16, 2, lambda: encoder(128, 2, 2, AB)),
         ("b packed ragged", torch.bfloat16, 2, lambda: encoder(128, 2, 2, AB, packed=True)),
         ("c fp32 (3, 9) stats", torch.float32, 2, lambda: encoder(128, 2, 2, ((3, 9),))),
         ("c fp32 (3, 9) probs", torch.float32, 2, lambda: (setattr(HF, "ATTN_SAVE_PROBS", True), encoder(128, 2, 2, ((3, 9),)))[1]),
         ("d module chain", torch.bfloat16, 2, lambda: encoder(128, 2, 2, AB[:1], chain=True)),
         ("e frozen bo, b1", torch.bfloat16, 2, lambda: encoder(128, 2, 2, AB, freeze=True)),
         ("f overlap sink bf16", torch.bfloat16, 2, lambda: (HF.set_grad_sink(SINK()), encoder(128, 2, 2, AB))[1]),
         ("f overlap sink fp32", torch.float32, 2, lambda: (HF.set_grad_sink(SINK()), encoder(128, 2, 2, AB))[1]),
         ("g hidden 1088", torch.bfloat16, 2, lambda: encoder(1088, 17, 1, ((2, 8),))),
         ("h TVC decoder step", torch.float32, 1, tvc),
         ("i graph, 3 replays, eager", torch.bfloat16, 5, train_step)]

if __name__ == "__main__":
    Lb._lib = Recorder(Lb.lib())
    for name, dtype, steps, make in CASES:
        HF.reset_caches()
        HF.ATTN_SAVE_PROBS = False
        hero_amd.set_compute_dtype(dtype)
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        del LOG[:]
        IDS.clear()
        HF.manual_seed(1234, "cuda:0")
        model, step = make()
        h = hashlib.sha256()
        for _ in range(steps):
            h.update(step().detach().float().cpu().numpy().tobytes())
        torch.cuda.synchronize()
        for p in model.parameters():
            h.update(b"none" if p.grad is None else p.grad.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
        text = "\n".join(LOG)
        print("%-28s calls %5d  log %s  bits %s  peak %d" % (name, len(LOG), hashlib.sha256(text.encode()).hexdigest()[:16],
                                                            h.hexdigest()[:16], torch.cuda.max_memory_allocated()), flush=True)
        if len(sys.argv) > 1:
            open(os.path.join(sys.argv[1], name.split()[0] + "_" + "_".join(name.split()[1:]) + ".log"), "w").write(text)
        del model, step
