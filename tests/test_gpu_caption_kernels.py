"""hero_caption_score on the GPU: the rows of tests/golden/case_caption.npz against what the reference's scorers gave, and one
seeded random case of 257 rows with Tcap 128 against tests/caption_reference.py (plain Python, float64).

BLEU's integers and the LCS length are equal.  ROUGE-L within 1e-6 * max(1, |ref|): a handful of operations on ratios of
integers below 129, rounded to fp32 once.  CIDEr-D within 1e-5 * max(1, |ref|): every term is non-negative, sums and norms are
float64, the result is rounded to fp32 once - a few times 2^-24 relative; the bound leaves about 20x over that.

Measured on an MI355X (max |got - ref| / max(1, |ref|)): ROUGE-L 2.970e-08, CIDEr-D 5.307e-08, both below 2^-24 - the one
rounding of a float64 result to fp32; the figures per case are in the docstrings of the two value tests."""
import os

import numpy as np
import pytest
import torch

from tests import caption_reference as R
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
Z = np.load(os.path.join(GOLDEN, "case_caption.npz"))
C = int(Z["hyp_len"].shape[0])
HYPS = [Z["hyp"][i, :Z["hyp_len"][i]].tolist() for i in range(C)]
REFS = [[Z["ref"][r, :Z["ref_len"][r]].tolist() for r in range(Z["ref_off"][c], Z["ref_off"][c + 1])] for c in range(C)]
EOS, TCAP = 60000, 128
ROUGE_TOL, CIDER_TOL = 1e-6, 1e-5


def id_rows(hyps, ld, dtype=torch.int32, junk=True, tcap=TCAP):
    """The captions as a decoder leaves them: eos behind the caption where it fits into tcap, then junk that must not count."""
    g = torch.Generator().manual_seed(3)
    rows = torch.randint(0, 40, (len(hyps), ld), generator=g).to(dtype) if junk else torch.full((len(hyps), ld), EOS, dtype=dtype)
    for i, h in enumerate(hyps):
        rows[i, :len(h)] = torch.tensor(h, dtype=dtype)
        if len(h) < tcap:
            rows[i, len(h)] = EOS
    return rows.cuda()


def err(got, want):
    want = torch.as_tensor(want, dtype=torch.float64)
    return float(((got.double().cpu() - want).abs() / want.abs().clamp(min=1.0)).max())


_CASES = {}


def fixture_case():
    if "fixture" not in _CASES:
        from hero_amd.caption import CaptionRefs
        _CASES["fixture"] = CaptionRefs(REFS, device="cuda")
    return _CASES["fixture"]


def random_inputs():
    """257 rows over 41 clips, Tcap 128: captions of 0..128 tokens, most of them a reference of their clip with tokens replaced
    or repeated, over a small Pareto vocabulary plus ids around the sign bit of the packed key; the reference once, in Python."""
    if "inputs" not in _CASES:
        rng = np.random.RandomState(11)
        special = [32767, 32768, 50271, 65535]

        def sent(n):
            s = np.minimum(rng.pareto(1.1, n) * 2 + 1, 29).astype(np.int64)
            hot = rng.rand(n) < 0.1
            s[hot] = rng.choice(special, int(hot.sum()))
            return [int(t) for t in s]
        refs = []
        for c in range(41):
            n_ref = 32 if c == 7 else 1 if c == 8 else int(rng.randint(1, 7))
            refs.append([sent(128 if (c, i) in ((3, 0), (9, 1)) else int(rng.randint(1, 31))) for i in range(n_ref)])
        hyps, clip = [], []
        for m in range(257):
            c = int(rng.randint(41))
            kind = m % 8
            if m in (0, 1):
                c, h = 3, list(refs[3][0])                       # 128 tokens: no eos in the row
                if m == 1:
                    h[5::9] = [int(t) for t in rng.randint(300, 340, len(h[5::9]))]
            elif kind == 2:
                h = []
            elif kind == 3:
                h = sent(int(rng.randint(1, 50)))                # unrelated to the references
            elif kind == 4:
                r = refs[c][int(rng.randint(len(refs[c])))]
                h = (r + r + r)[:int(rng.randint(1, 100))]       # repeats: the clipping of the counts
            else:
                h = list(refs[c][int(rng.randint(len(refs[c])))])
                for i in rng.choice(len(h), len(h) // 4, replace=False):
                    h[i] = int(rng.randint(300, 340))
            hyps.append(h)
            clip.append(c)
        df, n = R.document_frequency(refs)
        want = [R.score_clip(h, refs[c], df, n) for h, c in zip(hyps, clip)]
        _CASES["inputs"] = (refs, hyps, clip, want)
    return _CASES["inputs"]


def random_case():
    if "random" not in _CASES:
        from hero_amd.caption import CaptionRefs
        refs, hyps, clip, want = random_inputs()
        _CASES["random"] = (CaptionRefs(refs, device="cuda"), hyps, torch.tensor(clip, dtype=torch.int32).cuda(), want)
    return _CASES["random"]


@pytest.mark.parametrize("dtype,ld", [(torch.int32, TCAP), (torch.int32, TCAP + 5), (torch.int64, TCAP + 3)], ids=["i32", "i32-ld133", "i64-ld131"])
def test_fixture_rows_match_the_reference_scorers(dtype, ld):
    """Measured on an MI355X, all three layouts: ROUGE-L 2.823e-08, CIDEr-D 5.307e-08 (the rounding of the results to fp32)."""
    from hero_amd.caption import k_caption_score
    refs = fixture_case()
    ids = id_rows(HYPS, ld, dtype)
    stats, rouge, cider, lcs = k_caption_score(ids, torch.arange(C, dtype=torch.int32).cuda(), refs, EOS, tcap=TCAP, want_lcs=True)
    e_r, e_c = err(rouge, Z["rouge"]), err(cider, Z["cider"])
    print("\n[caption] fixture %s ld %d: rouge %.3e  cider %.3e" % (dtype, ld, e_r, e_c), end="")
    assert torch.equal(stats.cpu(), torch.from_numpy(Z["stats"]))
    assert torch.equal(lcs.cpu(), torch.from_numpy(Z["lcs"]))
    assert e_r <= ROUGE_TOL and e_c <= CIDER_TOL


def test_random_rows_match_the_python_reference():
    """257 rows, Tcap 128, several rows per clip.  Measured on an MI355X: ROUGE-L 2.970e-08, CIDEr-D 5.133e-08."""
    from hero_amd.caption import caption_score_torch, k_caption_score
    refs, hyps, clip, want = random_case()
    ids = id_rows(hyps, TCAP)
    stats, rouge, cider, lcs = k_caption_score(ids, clip, refs, EOS, want_lcs=True)
    e_r, e_c = err(rouge, [w["rouge"] for w in want]), err(cider, [w["cider"] for w in want])
    print("\n[caption] random 257 x 128: rouge %.3e  cider %.3e" % (e_r, e_c), end="")
    assert torch.equal(stats.cpu(), torch.tensor([R.stats_row(w) for w in want], dtype=torch.int32))
    assert torch.equal(lcs.cpu(), torch.tensor([w["lcs"] for w in want], dtype=torch.int32))
    assert e_r <= ROUGE_TOL and e_c <= CIDER_TOL
    lens = [len(h) for h in hyps]
    assert 0 in lens and 128 in lens and sum(1 for w in want if w["correct"][3] > 0) > 60 and max(w["cider"] for w in want) > 4
    # the PyTorch route on the device gives the same integers, and floats within the same bounds
    t_stats, t_rouge, t_cider, t_lcs = caption_score_torch(ids, clip, refs, EOS)
    assert torch.equal(t_stats, stats) and torch.equal(t_lcs, lcs)
    assert err(t_rouge, [w["rouge"] for w in want]) <= ROUGE_TOL and err(t_cider, [w["cider"] for w in want]) <= CIDER_TOL


def test_junk_behind_eos_changes_nothing_and_two_runs_give_equal_bits():
    from hero_amd.caption import k_caption_score
    refs, hyps, clip, _ = random_case()
    a = k_caption_score(id_rows(hyps, TCAP + 2), clip, refs, EOS, tcap=TCAP, want_lcs=True)
    b = k_caption_score(id_rows(hyps, TCAP + 2), clip, refs, EOS, tcap=TCAP, want_lcs=True)
    c = k_caption_score(id_rows(hyps, TCAP + 2, junk=False), clip, refs, EOS, tcap=TCAP, want_lcs=True)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    # a smaller Tcap cuts the caption: the first 20 tokens, whatever follows
    short = k_caption_score(id_rows(hyps, TCAP), clip, refs, EOS, tcap=20)
    cut = k_caption_score(id_rows([h[:20] for h in hyps], 20, tcap=20), clip, refs, EOS)
    assert all(torch.equal(x, y) for x, y in zip(short, cut))


def test_guard_rows_and_pad_columns_stay_untouched():
    from hero_amd.caption import k_caption_score
    refs = fixture_case()
    ids, clip = id_rows(HYPS, TCAP), torch.arange(C, dtype=torch.int32).cuda()
    want = k_caption_score(ids, clip, refs, EOS, want_lcs=True)
    stats = torch.full((C + 2, 13), -77, dtype=torch.int32).cuda()
    rouge, cider = torch.full((C + 2,), -5.0).cuda(), torch.full((C + 2,), -6.0).cuda()
    lcs = torch.full((C + 2,), -9, dtype=torch.int32).cuda()
    k_caption_score(ids, clip, refs, EOS, out=(stats, rouge, cider, lcs))
    assert torch.equal(stats[:C, :10], want[0]) and bool((stats[:C, 10:] == -77).all()) and bool((stats[C:] == -77).all())
    assert torch.equal(rouge[:C], want[1]) and rouge[C:].tolist() == [-5.0, -5.0]
    assert torch.equal(cider[:C], want[2]) and cider[C:].tolist() == [-6.0, -6.0]
    assert torch.equal(lcs[:C], want[3]) and lcs[C:].tolist() == [-9, -9]
    # a clip index outside the table scores zeros, and no other row changes
    wild = clip.clone()
    wild[4], wild[9] = C, -1
    got = k_caption_score(ids, wild, refs, EOS, want_lcs=True)
    keep = torch.ones(C, dtype=torch.bool)
    keep[[4, 9]] = False
    for g, w in zip(got, want):
        assert torch.equal(g[keep.cuda()], w[keep.cuda()]) and float(g[~keep.cuda()].abs().sum()) == 0.0


def test_every_envelope_violation_is_refused_without_a_launch():
    from hero_amd import _lib as L
    from hero_amd import caption as CP
    refs = fixture_case()
    ids, clip = id_rows(HYPS, TCAP + 2), torch.arange(C, dtype=torch.int32).cuda()
    stats = torch.full((C, 10), -77, dtype=torch.int32).cuda()
    rouge, cider = torch.full((C,), -5.0).cuda(), torch.full((C,), -6.0).cuda()
    lib = L.lib()

    def call(M=C, ld=TCAP + 2, ld_stats=10, tcap=TCAP, eos=EOS, V=65536):
        return lib.hero_caption_score(ids.data_ptr(), 0, clip.data_ptr(), refs.blob.data_ptr(), stats.data_ptr(), rouge.data_ptr(),
                                      cider.data_ptr(), None, M, ld, ld_stats, tcap, eos, V, L.stream())
    for bad in (dict(M=0), dict(ld=TCAP - 1), dict(ld_stats=9), dict(tcap=0), dict(tcap=129, ld=200), dict(eos=-1), dict(eos=65536),
                dict(V=65537), dict(V=0), dict(V=100)):
        assert call(**bad) != 0 and b"hero_caption_score" in lib.hero_last_error(), bad
    torch.cuda.synchronize()
    assert bool((stats == -77).all()) and bool((rouge == -5.0).all()) and bool((cider == -6.0).all())
    for kw in (dict(tcap=129), dict(tcap=0), dict(vocab=65537), dict(vocab=100)):
        with pytest.raises(ValueError):
            CP.k_caption_score(torch.zeros((C, 140), dtype=torch.int32).cuda(), clip, refs, EOS, **kw)
    with pytest.raises(ValueError):
        CP.k_caption_score(ids[:, ::2], clip, refs, EOS)
    # outside the envelope the PyTorch route serves: 130 columns
    wide = id_rows([(h + h)[:130] for h in HYPS[:6]], 130, tcap=130)
    stats_t, rouge_t, cider_t = CP.caption_score(wide, clip[:6], refs, EOS)
    df, n = R.document_frequency(REFS)
    want = [R.score_clip((h + h)[:130], REFS[c], df, n) for c, h in enumerate(HYPS[:6])]
    assert stats_t.tolist() == [R.stats_row(w) for w in want] and err(cider_t, [w["cider"] for w in want]) <= CIDER_TOL


def test_the_launch_is_capturable_and_replays_on_new_ids():
    from hero_amd.caption import k_caption_score
    refs, hyps, clip, _ = random_case()
    first, second = id_rows(hyps, TCAP), id_rows(hyps[::-1], TCAP)
    rev = torch.flip(clip, dims=[0]).contiguous()
    want = k_caption_score(second, rev, refs, EOS, want_lcs=True)
    ids, cl = first.clone(), clip.clone()
    out = (torch.zeros((257, 10), dtype=torch.int32).cuda(), torch.zeros(257).cuda(), torch.zeros(257).cuda(),
           torch.zeros(257, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        k_caption_score(ids, cl, refs, EOS, out=out)
    ids.copy_(second)
    cl.copy_(rev)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(out, want))
