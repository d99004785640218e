"""Caption metrics on decoded captions, and the reward-weighted losses, on the GPU: the tiny TVC model of
tests/golden/case_tvc.npz in fp32, loaded as tests/test_gpu_tvc_sample.py loads it (8 steps, eos 30).

    as_tensor=True   the decoders' id rows as a device tensor: cut at eos they are the lists of the default call
    validate_tvc     over two batches with hand-made references equals tests/caption_reference.py on the decoded lists
    reward_weighted_loss   the kernels' route against fused_decoder = False for fixed ids and weights: the loss and the six
                     gradients tests/test_gpu_tvc.py checks, rel_err < 2e-4 (that file's fp32 tolerance between the two routes)
    self_critical_loss     top_k = 1 makes every sample the greedy caption: loss and gradients exactly 0; real sampling gives a
                     finite loss, and one seed gives equal bits twice"""
import pytest
import torch

from tests import caption_reference as R
from tests import test_gpu_tvc_sample as S
from tests.util import rel_err

pytestmark = pytest.mark.gpu
FP32_TOL = 2e-4
GRADS = sorted(k[len("grad."):] for k in S.Z.files if k.startswith("grad."))
EOS, STEPS = S.EOS, S.STEPS


@pytest.fixture(autouse=True)
def _fp32_default():
    import hero_amd
    from hero_amd import functional as HF
    hero_amd.set_compute_dtype(torch.float32)
    HF.clear_weight_cache()
    yield
    hero_amd.set_compute_dtype(torch.bfloat16)


def hand_refs(n, shift=0):
    """References over the tokens the tiny model emits (82, 81, 132, 110, ...) so that some n-grams match and some do not."""
    return [[[82, 81, 82, 82][:1 + (i + shift) % 4], [132, 132, 82, 82, 5 + i + shift], [110, 82]][:2 + (i + shift) % 2] for i in range(n)]


def cut_rows(rows):
    return [R.cut(r, EOS) for r in rows.tolist()]


def test_as_tensor_rows_cut_at_eos_are_the_default_lists():
    model, batch = S.load_model(), S.load_batch()
    for kw in (dict(kv_cache=False), dict(kv_cache=True), dict(kv_cache=True, use_graph=True)):
        from hero_amd.model import TvcGenerator
        gen = TvcGenerator(model, STEPS, S.DESC["bos"], EOS, **kw)
        lists = gen.greedy_decode(batch)
        rows = gen.greedy_decode(batch, as_tensor=True)
        assert torch.is_tensor(rows) and rows.is_cuda and tuple(rows.shape) == (len(lists), STEPS)
        assert cut_rows(rows) == lists
        if kw.get("use_graph"):                         # the rows are the caller's own: the next replay does not change them
            keep = rows.clone()
            gen.greedy_decode(S.shifted_batch(batch))
            assert torch.equal(rows, keep)
    gen = S.generator(model)
    assert any(len(c) < STEPS for c in lists) and any(len(c) > 0 for c in lists)
    lists, scores = gen.beam_decode(batch, 3, return_scores=True)
    rows, dev_scores = gen.beam_decode(batch, 3, return_scores=True, as_tensor=True)
    assert rows.is_cuda and tuple(rows.shape) == (len(lists), STEPS) and cut_rows(rows) == lists and dev_scores.tolist() == scores
    assert cut_rows(gen.beam_decode(batch, 3, as_tensor=True)) == lists
    for return_all in (False, True):
        kw = dict(n_samples=3, temperature=0.9, top_k=20, top_p=0.95, seed=5, return_all=return_all)
        lists = gen.sample_decode(batch, **kw)
        rows = gen.sample_decode(batch, as_tensor=True, **kw)
        assert rows.is_cuda and tuple(rows.shape) == (6 * (3 if return_all else 1), STEPS) and cut_rows(rows) == lists


@pytest.mark.parametrize("decode,args", [("greedy", {}), ("beam", dict(beam_size=3)),
                                          ("sample", dict(n_samples=2, temperature=0.8, top_k=10, seed=3))])
def test_validate_tvc_equals_the_python_reference_on_the_decoded_lists(decode, args):
    from hero_amd.caption import CaptionRefs, validate_tvc
    model, b0 = S.load_model(), S.load_batch()
    b0["clip_ids"] = ["a%d" % i for i in range(6)]
    b1 = dict(S.shifted_batch(b0), clip_ids=["b%d" % i for i in range(6)])
    by_name = dict(zip(b0["clip_ids"] + b1["clip_ids"], hand_refs(6) + hand_refs(6, shift=1)))
    names = b1["clip_ids"][:3] + b0["clip_ids"] + b1["clip_ids"][3:]          # the table's clip order is not the loader's
    refs = [by_name[c] for c in names]
    table = CaptionRefs(refs, clip_ids=names, device="cuda")
    gen = S.generator(model)
    got = validate_tvc(gen, [b0, b1], table, decode=decode, **args)
    lists = {}
    for b in (b0, b1):
        call = {"greedy": gen.greedy_decode, "beam": gen.beam_decode, "sample": gen.sample_decode}[decode]
        lists.update(zip(b["clip_ids"], call(b, **args)))
    hyps = [lists[c] for c in table.clip_ids]
    rows, want = R.score_corpus(hyps, refs)
    print("\n[caption] validate %s: %s" % (decode, {k: round(v, 4) for k, v in got.items()}), end="")
    assert sorted(got) == sorted(want) and any(r["correct"][0] > 0 for r in rows)
    for k in ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4"):
        assert abs(got[k] - want[k]) <= 1e-9 * max(1.0, want[k]), k
    assert abs(got["ROUGE_L"] - want["ROUGE_L"]) <= 100 * 1e-6
    assert abs(got["CIDEr"] - want["CIDEr"]) <= 100 * 1e-5 * max(1.0, max(r["cider"] for r in rows))
    assert model.training is False
    with pytest.raises(ValueError, match="never scored"):
        validate_tvc(gen, [b0], table, decode=decode, **args)


def fixed_rows():
    """12 caption rows (6 captions x 2 samples) of 8 ids: eos at different places, first, and nowhere; weights of both signs."""
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(31, 160, (12, STEPS), generator=g)
    for r, at in enumerate([2, 8, 0, 5, 7, 3, 8, 1, 4, 6, 8, 2]):
        if at < STEPS:
            ids[r, at] = EOS
    weights = torch.linspace(-1.5, 2.0, 12)
    return ids.to(torch.int32).cuda(), weights.cuda()


def loss_and_grads(fused):
    from hero_amd import functional as HF
    from hero_amd.caption import reward_weighted_loss
    HF.clear_weight_cache()
    model = S.load_model()
    model.fused_decoder = fused
    ids, weights = fixed_rows()
    loss = reward_weighted_loss(model, S.load_batch(), ids, weights, EOS, bos=S.DESC["bos"])
    loss.backward()
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    return float(loss.detach()), {n: params[n].grad.detach().clone() for n in GRADS}


def test_reward_weighted_loss_on_the_kernels_matches_the_pytorch_formulation():
    from hero_amd.caption import teacher_forcing_rows
    f_loss, f_grads = loss_and_grads(True)
    t_loss, t_grads = loss_and_grads(False)
    print("\n[caption] reward-weighted loss: fused %.6f  torch %.6f" % (f_loss, t_loss), end="")
    assert abs(f_loss - t_loss) < FP32_TOL * abs(t_loss) and abs(t_loss) > 1e-2
    for n in GRADS:
        e = rel_err(f_grads[n], t_grads[n])
        print("\n[caption] reward-weighted loss: grad %-60s %.3e" % (n, e), end="")
        assert e < FP32_TOL, (n, e)
        assert float(t_grads[n].abs().max()) > 0
    # the definition, from the PyTorch route's scores: sum_rows w_row * sum_t CE(row, t) / (number of valid tokens)
    model = S.load_model()
    model.fused_decoder = False
    ids, weights = fixed_rows()
    batch = S.load_batch()
    inputs, labels, pos = teacher_forcing_rows(ids, S.DESC["bos"], EOS, model.v_encoder.f_encoder.embeddings.padding_idx)
    with torch.no_grad():
        enc = model.encode(batch).repeat_interleave(2, dim=0)
        scores = model.decode(enc, batch["cap_attn_mask"].repeat_interleave(2, dim=0), inputs, pos, None, compute_loss=False)
        logp = torch.log_softmax(scores.double(), dim=-1)
        ce = -logp.gather(2, labels.clamp(min=0).unsqueeze(2)).squeeze(2) * (labels != -1)
        want = float((ce.sum(dim=1) * weights.double()).sum() / (labels != -1).sum())
    assert abs(t_loss - want) < FP32_TOL * abs(want)


def test_self_critical_loss_is_zero_under_top_k_1_and_reproducible_under_sampling():
    from hero_amd.caption import CaptionRefs, self_critical_loss
    model, batch = S.load_model(), S.load_batch()
    gen = S.generator(model)
    table = CaptionRefs(hand_refs(6), device="cuda")
    clip = torch.arange(6, dtype=torch.int32).cuda()
    loss = self_critical_loss(model, gen, batch, table, clip, n_samples=3, seed=1, top_k=1)
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert float(loss.detach()) == 0.0 and len(grads) > 10 and all(float(g.abs().max()) == 0.0 for g in grads)
    model.zero_grad(set_to_none=True)
    a = self_critical_loss(model, gen, batch, table, clip, n_samples=4, seed=9, temperature=1.3)
    a.backward()
    ga = {n: p.grad.detach().clone() for n, p in model.named_parameters() if n in GRADS}
    b = self_critical_loss(model, gen, batch, table, list(range(6)), n_samples=4, seed=9, temperature=1.3)
    print("\n[caption] self-critical loss, 4 samples at temperature 1.3: %.6f" % float(a.detach()), end="")
    assert bool(torch.isfinite(a.detach())) and float(a.detach()) != 0.0
    assert torch.equal(a.detach(), b.detach())
    assert all(bool(torch.isfinite(g).all()) for g in ga.values()) and any(float(g.abs().max()) > 0 for g in ga.values())
    assert model.training is False
