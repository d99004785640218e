"""Caption metrics without a GPU: tests/caption_reference.py (plain Python, float64) reproduces what the reference's scorers gave
for tests/golden/case_caption.npz - integers equal, floats within 1e-12 - and hero_amd.caption's table builder, its PyTorch
route, CaptionMeter and the teacher-forcing row builder are held to the fixture on CPU tensors.

Tolerances of the fp32 outputs against the float64 fixture, as for the kernel (tests/test_gpu_caption_kernels.py): ROUGE-L
1e-6 * max(1, |ref|), CIDEr-D 1e-5 * max(1, |ref|); the integers and the LCS length are equal."""
import os

import numpy as np
import pytest
import torch

from tests import caption_reference as R
from tests.util import GOLDEN

Z = np.load(os.path.join(GOLDEN, "case_caption.npz"))
C = int(Z["hyp_len"].shape[0])
HYPS = [Z["hyp"][i, :Z["hyp_len"][i]].tolist() for i in range(C)]
REFS = [[Z["ref"][r, :Z["ref_len"][r]].tolist() for r in range(Z["ref_off"][c], Z["ref_off"][c + 1])] for c in range(C)]
EOS, TCAP = 60000, 128          # an id that no sequence of the fixture holds
ROUGE_TOL, CIDER_TOL = 1e-6, 1e-5


def id_rows(hyps, ld=TCAP + 3, dtype=torch.int32, junk=True):
    """The hypotheses as a decoder leaves them: eos behind the caption (if it fits), then junk that must not count."""
    g = torch.Generator().manual_seed(3)
    rows = torch.randint(0, 40, (len(hyps), ld), generator=g).to(dtype) if junk else torch.full((len(hyps), ld), EOS, dtype=dtype)
    for i, h in enumerate(hyps):
        rows[i, :len(h)] = torch.tensor(h, dtype=dtype)
        if len(h) < ld:
            rows[i, len(h)] = EOS
    return rows


def within(got, want, tol):
    want = torch.as_tensor(want, dtype=torch.float64)
    return bool(((got.double() - want).abs() <= tol * want.abs().clamp(min=1.0)).all())


@pytest.fixture(scope="module")
def table():
    from hero_amd.caption import CaptionRefs
    return CaptionRefs(REFS, clip_ids=["clip%02d" % i for i in range(C)], device="cpu")


def test_fixture_is_what_the_issue_asks_for():
    lens = Z["hyp_len"].tolist()
    per_clip = np.diff(Z["ref_off"]).tolist()
    assert C == 48 and 0 in lens and 1 in lens and 128 in lens and 128 in Z["ref_len"].tolist()
    assert min(per_clip) == 1 and max(per_clip) == 32
    assert int((Z["stats"][:, 3] > 0).sum()) * 3 >= C
    assert any(t in Z["hyp"] for t in (32767, 32768, 50271, 65535))
    assert not (Z["hyp"] == EOS).any() and not (Z["ref"] == EOS).any()


def test_python_reference_reproduces_the_reference_scorers():
    rows, corpus = R.score_corpus(HYPS, REFS)
    assert np.array_equal(np.array([R.stats_row(r) for r in rows]), Z["stats"])
    assert [r["lcs"] for r in rows] == Z["lcs"].tolist()
    assert max(abs(r["rouge"] - x) for r, x in zip(rows, Z["rouge"])) <= 1e-12
    assert max(abs(r["cider"] - x) for r, x in zip(rows, Z["cider"])) <= 1e-12
    for k in range(4):
        assert abs(corpus["Bleu_%d" % (k + 1)] - 100 * Z["corpus_bleu"][k]) <= 1e-10
    assert abs(corpus["ROUGE_L"] - 100 * float(Z["corpus_rouge"])) <= 1e-10
    assert abs(corpus["CIDEr"] - 100 * float(Z["corpus_cider"])) <= 1e-10


def test_reference_cut_and_lcs():
    assert R.cut([5, 6, EOS, 7], EOS) == [5, 6] and R.cut([EOS, 1], EOS) == [] and R.cut([1, 2, 3], EOS, 2) == [1, 2]
    assert R.lcs([1, 2, 3, 4, 1], [3, 4, 1, 2, 1]) == 3 and R.lcs([], [1]) == 0 and R.lcs([1, 1], [1]) == 1


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_torch_route_matches_the_fixture(table, dtype):
    from hero_amd.caption import caption_score_torch
    ids = id_rows(HYPS, dtype=dtype)
    stats, rouge, cider, lcs = caption_score_torch(ids, torch.arange(C, dtype=torch.int32), table, EOS, tcap=TCAP)
    assert stats.dtype == torch.int32 and rouge.dtype == torch.float32 and cider.dtype == torch.float32
    assert torch.equal(stats, torch.from_numpy(Z["stats"]))
    assert torch.equal(lcs, torch.from_numpy(Z["lcs"]))
    assert within(rouge, Z["rouge"], ROUGE_TOL) and within(cider, Z["cider"], CIDER_TOL)
    # junk behind eos changes nothing, bit for bit; neither does the order of the rows
    clean = caption_score_torch(id_rows(HYPS, dtype=dtype, junk=False), torch.arange(C, dtype=torch.int32), table, EOS, tcap=TCAP)
    assert all(torch.equal(a, b) for a, b in zip((stats, rouge, cider, lcs), clean))
    perm = torch.randperm(C, generator=torch.Generator().manual_seed(1))
    mixed = caption_score_torch(ids[perm], perm.to(torch.int32), table, EOS, tcap=TCAP, block=7)
    assert all(torch.equal(a[perm], b) for a, b in zip((stats, rouge, cider, lcs), mixed))


def test_table_builder_answers_the_three_lookups(table):
    """The packed buffer's tables against dictionaries: the clipped maximum count of an n-gram in a clip, an n-gram's count in a
    reference with the reference's norms, an n-gram's idf - and signed order of the keys."""
    from hero_amd.caption import pack_keys
    df, n_clips = R.document_frequency(REFS)
    assert table.n_clips == n_clips == C and table.n_refs == int(Z["ref_len"].shape[0]) and table.max_refs == 32
    blob = table.blob.numpy().tobytes()
    hdr = np.frombuffer(blob, dtype=np.int64, count=48)
    assert hdr[1] == C and hdr[2] == table.n_refs and hdr[9] == len(blob) and len(blob) % 8 == 0
    assert abs(np.frombuffer(blob, dtype=np.float64, count=1, offset=32)[0] - np.log(float(C))) <= 1e-15
    flat = [r for rs in REFS for r in rs]
    norms = np.frombuffer(blob, dtype=np.float64, count=4 * len(flat), offset=hdr[7]).reshape(-1, 4)
    assert np.array_equal(np.frombuffer(blob, dtype=np.int32, count=len(flat), offset=hdr[6]), Z["ref_len"])
    negative = 0
    for n in range(1, 5):
        w = hdr[10 + 8 * (n - 1):18 + 8 * (n - 1)]
        cm_off = np.frombuffer(blob, dtype=np.int32, count=C + 1, offset=w[0])
        cm_key = np.frombuffer(blob, dtype=np.int64, count=cm_off[-1], offset=w[1])
        cm_cnt = np.frombuffer(blob, dtype=np.int32, count=cm_off[-1], offset=w[2])
        rw_off = np.frombuffer(blob, dtype=np.int32, count=len(flat) + 1, offset=w[3])
        rw_key = np.frombuffer(blob, dtype=np.int64, count=rw_off[-1], offset=w[4])
        rw_cnt = np.frombuffer(blob, dtype=np.int32, count=rw_off[-1], offset=w[5])
        idf_key = np.frombuffer(blob, dtype=np.int64, count=hdr[42 + n - 1], offset=w[6])
        idf_val = np.frombuffer(blob, dtype=np.float64, count=hdr[42 + n - 1], offset=w[7])
        key_of = lambda g: int(pack_keys(torch.tensor([list(g)], dtype=torch.long))[0])      # noqa: E731
        want_idf = {key_of(g): np.log(float(C)) - np.log(max(1.0, float(d))) for g, d in df.items() if len(g) == n}
        assert np.all(np.diff(idf_key) > 0) and dict(zip(idf_key.tolist(), idf_val.tolist())).keys() == want_idf.keys()
        assert max(abs(want_idf[k] - v) for k, v in zip(idf_key.tolist(), idf_val.tolist())) <= 1e-14
        negative += int((idf_key < 0).sum())
        for c, rs in enumerate(REFS):
            want = {}
            for r in rs:
                for g, k in R.ngrams(r).items():
                    if len(g) == n:
                        want[key_of(g)] = max(want.get(key_of(g), 0), k)
            seg = slice(cm_off[c], cm_off[c + 1])
            assert np.all(np.diff(cm_key[seg]) > 0) and dict(zip(cm_key[seg].tolist(), cm_cnt[seg].tolist())) == want
        for i, r in enumerate(flat):
            want = {key_of(g): k for g, k in R.ngrams(r).items() if len(g) == n}
            seg = slice(rw_off[i], rw_off[i + 1])
            assert dict(zip(rw_key[seg].tolist(), rw_cnt[seg].tolist())) == want
            norm = np.sqrt(sum((k * want_idf[g]) ** 2 for g, k in want.items()))
            assert abs(norms[i, n - 1] - norm) <= 1e-12 * max(1.0, norm)
        if n == 1:
            assert 0.0 in idf_val.tolist()                      # the n-gram of every clip: log C - log C, exactly
    assert negative >= 3                                        # 4-grams that start at or above 32768 sort as negative keys


def test_idf_from_a_second_corpus():
    from hero_amd.caption import CaptionRefs, caption_score_torch
    sub = list(range(5, 13))
    t = CaptionRefs([REFS[c] for c in sub], idf_refs=REFS, device="cpu")
    rows, _ = R.score_corpus([HYPS[c] for c in sub], [REFS[c] for c in sub], idf_refs=REFS)
    stats, rouge, cider, _ = caption_score_torch(id_rows([HYPS[c] for c in sub]), torch.arange(len(sub)), t, EOS, tcap=TCAP)
    assert stats.tolist() == [R.stats_row(r) for r in rows]
    assert within(cider, [r["cider"] for r in rows], CIDER_TOL) and within(rouge, [r["rouge"] for r in rows], ROUGE_TOL)
    own, _ = R.score_corpus([HYPS[c] for c in sub], [REFS[c] for c in sub])
    assert max(abs(a["cider"] - b["cider"]) for a, b in zip(rows, own)) > 0.1       # the idf corpus matters


def test_meter_is_independent_of_batch_order(table):
    from hero_amd.caption import CaptionMeter
    ids = id_rows(HYPS)
    results = []
    for seed, sizes in ((0, [48]), (1, [5, 20, 23]), (2, [1] * 48)):
        perm = torch.randperm(C, generator=torch.Generator().manual_seed(seed)).tolist()
        meter, at = CaptionMeter(table), 0
        for n in sizes:
            rows = perm[at:at + n]
            at += n
            meter.update(ids[rows], table.rows(["clip%02d" % r for r in rows]), EOS, tcap=TCAP)
        results.append(meter.compute())
    assert results[0] == results[1] == results[2]
    got = results[0]
    assert sorted(got) == ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "CIDEr", "ROUGE_L"]
    for k in range(4):                                          # BLEU comes from integers: float64 arithmetic only
        assert abs(got["Bleu_%d" % (k + 1)] - 100 * Z["corpus_bleu"][k]) <= 1e-10
    assert abs(got["ROUGE_L"] - 100 * float(Z["corpus_rouge"])) <= 100 * ROUGE_TOL
    assert abs(got["CIDEr"] - 100 * float(Z["corpus_cider"])) <= 100 * CIDER_TOL * max(1.0, float(Z["cider"].max()))


def test_meter_raises_on_a_missing_or_repeated_clip(table):
    from hero_amd.caption import CaptionMeter
    ids = id_rows(HYPS)
    with pytest.raises(ValueError, match="no eos"):
        CaptionMeter(table).update(ids[:40], list(range(40)))
    meter = CaptionMeter(table, eos=EOS).update(ids[:40], list(range(40)), tcap=TCAP)
    with pytest.raises(ValueError, match="never scored"):
        meter.compute()
    part = meter.compute(partial=True)
    rows, _ = R.score_corpus(HYPS[:40], REFS[:40], idf_refs=REFS)
    assert abs(part["CIDEr"] - 100 * sum(r["cider"] for r in rows) / 40) <= 100 * CIDER_TOL * 10
    meter.update(ids[39:], list(range(39, 48)), EOS, tcap=TCAP)
    with pytest.raises(ValueError, match="scored 2 times"):
        meter.compute()
    with pytest.raises(ValueError, match="scored 2 times"):
        meter.compute(partial=True)


@pytest.mark.parametrize("refs,what", [
    ([[[1, 2, 65536]]], "id"), ([[[1, -1]]], "id"), ([[[]]], "tokens"), ([[[1] * 129]], "tokens"), ([[]], "references"),
    ([[[1, 2]] * 33], "references"), ([], "non-empty")])
def test_builder_rejects_references_outside_the_envelope(refs, what):
    from hero_amd.caption import CaptionRefs
    with pytest.raises(ValueError, match=what):
        CaptionRefs(refs, device="cpu")
    with pytest.raises(ValueError, match=what):
        CaptionRefs([[[1, 2, 3]]], idf_refs=refs, device="cpu")


def test_builder_accepts_the_envelope_s_corners():
    from hero_amd.caption import CaptionRefs, caption_score_torch
    t = CaptionRefs([[[65535] * 128] * 32, [[0]]], clip_ids=["a", "b"], device="cpu")
    assert t.rows(["b", "a"]) == [1, 0]
    stats, rouge, cider, lcs = caption_score_torch(torch.tensor([[65535] * 128, [0] + [9] * 127]), torch.tensor([0, 1]), t, 9)
    assert stats.tolist() == [[128, 127, 126, 125, 128, 127, 126, 125, 128, 128], [1, 0, 0, 0, 1, 0, 0, 0, 1, 1]]
    assert lcs.tolist() == [128, 1] and rouge.tolist() == [1.0, 1.0]
    with pytest.raises(ValueError, match="every clip once"):
        CaptionRefs([[[1]], [[2]]], clip_ids=["a", "a"], device="cpu")


def test_wrapper_refuses_cpu_rows_and_bad_shapes(table):
    from hero_amd import caption as CP
    ids = id_rows(HYPS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CP.k_caption_score(ids, torch.arange(C, dtype=torch.int32), table, EOS, tcap=TCAP)
    with pytest.raises(ValueError):
        CP.caption_score_torch(ids, torch.arange(C - 1, dtype=torch.int32), table, EOS)
    with pytest.raises(ValueError):
        CP.caption_score_torch(ids.float(), torch.arange(C, dtype=torch.int32), table, EOS)
    with pytest.raises(ValueError, match="outside"):
        CP.caption_score_torch(ids, torch.full((C,), C, dtype=torch.int32), table, EOS, tcap=TCAP)


def test_envelope_query_and_argument_errors_need_no_gpu():
    """hero_caption_in_envelope is host code, and every violation is refused before anything is launched."""
    from hero_amd import _lib as L
    from hero_amd import build
    from hero_amd import caption as CP
    build.build()
    assert [CP.in_envelope(v, t) for v, t in ((65536, 128), (1, 1), (65537, 8), (0, 8), (100, 129), (100, 0))] == [True, True] + [False] * 4
    lib, one = L.lib(), 8                                        # a non-null, aligned stand-in: nothing dereferences it
    args = dict(M=4, ld=16, ld_stats=10, Tcap=16, eos=2, V=100)

    def call(**kw):
        a = dict(args, **kw)
        return lib.hero_caption_score(one, 0, one, one, one, one, one, None, a["M"], a["ld"], a["ld_stats"], a["Tcap"], a["eos"], a["V"], None)
    for bad in (dict(M=0), dict(ld=15), dict(ld_stats=9), dict(Tcap=0), dict(Tcap=129, ld=129), dict(eos=-1), dict(eos=100), dict(V=65537),
                dict(V=0)):
        assert call(**bad) != 0 and b"hero_caption_score" in lib.hero_last_error(), bad
    assert lib.hero_caption_score(None, 0, one, one, one, one, one, None, 4, 16, 10, 16, 2, 100, None) != 0
    assert lib.hero_caption_score(one, 0, one, 12, one, one, one, None, 4, 16, 10, 16, 2, 100, None) != 0     # tables not 8-byte aligned


def test_teacher_forcing_rows():
    """The label and input builder of reward_weighted_loss: junk after eos, no eos, eos first."""
    from hero_amd.caption import teacher_forcing_rows
    eos, bos, pad = 9, 0, 1
    rows = torch.tensor([[5, 6, eos, 7, eos], [5, 6, 7, 8, 4], [eos, 3, 3, 3, 3], [2, 3, 4, 5, eos]], dtype=torch.int32)
    inputs, labels, pos = teacher_forcing_rows(rows, bos, eos, pad)
    assert inputs.dtype == labels.dtype == torch.long and pos.tolist() == [[0, 1, 2, 3, 4]]
    assert labels.tolist() == [[5, 6, eos, -1, -1], [5, 6, 7, 8, 4], [eos, -1, -1, -1, -1], [2, 3, 4, 5, eos]]
    assert inputs.tolist() == [[bos, 5, 6, pad, pad], [bos, 5, 6, 7, 8], [bos, pad, pad, pad, pad], [bos, 2, 3, 4, 5]]
