#!/usr/bin/env python3
"""Golden vectors for the caption metrics by importing the *reference's* scorers (eval/pycocoevalcap: BleuScorer(n=4) with the
"closest" reference length, Rouge(), CiderScorer(n=4, sigma=6.0)) and feeding them integer token sequences as strings of
"w<id>" words.

Container-only (needs the reference checkout), like its siblings; never imported by a test.
Writes tests/golden/case_caption.npz:

  hyp [C, 128] int32, hyp_len [C]         the hypothesis of every clip, zero-padded
  ref [R, 128] int32, ref_len [R]         all references, clip after clip; ref_off [C + 1] the first reference of every clip
  stats [C, 10] int32                     BleuScorer's per-caption integers: correct[4], guess[4], testlen, reflen ("closest")
  lcs [C] int32                           the longest my_lcs of the hypothesis with a reference of its clip
  rouge [C], cider [C] float64            the per-clip scores of Rouge() and CiderScorer
  corpus_bleu [4], corpus_rouge, corpus_cider   the corpus values (not yet times 100)

48 clips.  Ids are Pareto-distributed over a small vocabulary, a general hypothesis is a reference with a quarter of its tokens
replaced by ids that no reference holds; the first clips are the edge cases listed in main(), and the maker asserts every one
of them, so the case is not vacuous.

Run:  python tests/golden/make_golden_caption.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G                                   # noqa: E402  (the reference's location)

CLIPS, TMAX, VOCAB, NOVEL, EVERYWHERE = 48, 128, 40, 900, 1
SPECIAL = (32767, 32768, 50271, 65535)


def words(seq):
    return " ".join("w%d" % t for t in seq)


def build():
    rng = np.random.RandomState(20)

    def sent(n):
        return [int(t) for t in np.minimum(rng.pareto(1.2, n) * 3 + 2, VOCAB - 1).astype(np.int64)]

    def corrupt(r):
        h = list(r)
        for i in rng.choice(len(h), max(1, len(h) // 4), replace=False):
            h[i] = NOVEL + int(rng.randint(0, 50))
        return h

    hyps, refs = [], []
    for c in range(CLIPS):
        rs = [sent(int(rng.randint(5, 26))) for _ in range(int(rng.randint(2, 7)))]
        hyps.append(corrupt(rs[int(rng.randint(len(rs)))]))
        refs.append(rs)
    for rs in refs:                                                       # one unigram in every clip: idf 0 (the edge cases below keep it)
        rs[0][0] = EVERYWHERE
    hyps[0] = []                                                          # an empty hypothesis
    hyps[1] = [refs[1][0][2]]                                             # one token
    hyps[2] = refs[2][0] + sent(30 - len(refs[2][0]))                     # longer than every reference of its clip
    refs[3][0] = [EVERYWHERE] + sent(TMAX - 1)                            # a reference and a hypothesis of 128 tokens
    hyps[3] = corrupt(refs[3][0])
    refs[4] = [sent(11) + [EVERYWHERE]]                                   # one reference, and the hypothesis equals it
    hyps[4] = list(refs[4][0])
    refs[5] = [sent(int(rng.randint(5, 26))) for _ in range(32)]          # 32 references
    refs[5][0][0] = EVERYWHERE
    hyps[5] = corrupt(refs[5][17])
    refs[6] = [[5, 7, 7, 9, 3, 4, EVERYWHERE], [7, 7, 2, 8, 6, 3, 4, 11]]  # the hypothesis repeats "7", "7 7", ... more often
    hyps[6] = [7, 7, 7, 7, 7, 7, 3, 4]
    refs[7] = [[EVERYWHERE] + sent(7), sent(12)]                          # equidistant reference lengths 8 and 12 around 10
    hyps[7] = corrupt(refs[7][1])[:10]
    a, b, c_, d = SPECIAL                                                 # 4-grams whose packed key starts / ends at the sign bit
    refs[8] = [[a, 4, 5, b, 6, b, 7, 8, d, 9, EVERYWHERE], [c_, 3, 4, a, 5, d, 6, 7, c_, 8, d, 2, 3, a]]
    hyps[8] = [a, 4, 5, b, 9, c_, 3, 4, a, 2, b, 7, 8, d, 3, d, 6, 7, c_, 6, d, 2, 3, a]
    assert all(EVERYWHERE in rs[0] for rs in refs)
    return hyps, refs


def main():
    sys.path.insert(0, G.REF)
    from eval.pycocoevalcap.bleu.bleu_scorer import BleuScorer          # noqa: reference import
    from eval.pycocoevalcap.cider.cider_scorer import CiderScorer       # noqa: reference import
    from eval.pycocoevalcap.rouge.rouge import Rouge, my_lcs            # noqa: reference import

    hyps, refs = build()
    bleu, cider, rouge = BleuScorer(n=4), CiderScorer(n=4, sigma=6.0), Rouge()
    rouge_rows, lcs_rows = [], []
    for h, rs in zip(hyps, refs):
        hs, rss = words(h), [words(r) for r in rs]
        bleu += (hs, rss)
        cider += (hs, rss)
        rouge_rows.append(rouge.calc_score([hs], rss))
        lcs_rows.append(max(my_lcs(r.split(" "), hs.split(" ")) for r in rss))
    corpus_bleu, _ = bleu.compute_score(option="closest", verbose=0)
    corpus_cider, cider_rows = cider.compute_score()
    stats = np.array([c["correct"] + c["guess"] + [c["testlen"], bleu._single_reflen(c["reflen"], "closest", c["testlen"])]
                      for c in bleu.ctest], dtype=np.int32)
    df = cider.document_frequency

    # ---- the case must not be vacuous ------------------------------------------------------------------------------------------
    lens = [len(h) for h in hyps]
    assert 0 in lens and 1 in lens and TMAX in lens and any(len(r) == TMAX for rs in refs for r in rs)
    assert any(len(h) > max(len(r) for r in rs) for h, rs in zip(hyps, refs)), "no hypothesis longer than its references"
    assert min(len(rs) for rs in refs) == 1 and max(len(rs) for rs in refs) == 32

    def counts(seq, n):
        out = {}
        for i in range(len(seq) - n + 1):
            out[tuple(seq[i:i + n])] = out.get(tuple(seq[i:i + n]), 0) + 1
        return out
    clipped = 0
    for h, rs in zip(hyps, refs):
        for n in (1, 2, 3):
            for g, k in counts(h, n).items():
                top = max(counts(r, n).get(g, 0) for r in rs)
                clipped += 1 if 0 < top < k else 0
    assert clipped >= 3, "the clipping of BLEU's counts is never live"
    ties = 0
    for h, rs in zip(hyps, refs):
        d = sorted((abs(len(r) - len(h)), len(r)) for r in rs)
        ties += 1 if len(d) > 1 and d[0][0] == d[1][0] and d[0][1] != d[1][1] else 0
    assert ties >= 1, "no two equidistant references of different length"
    assert df[("w%d" % EVERYWHERE,)] == CLIPS, "no n-gram in every clip"
    # (the scorer's table is a defaultdict: looking an unseen n-gram up has entered it with 0)
    assert any(df.get(tuple("w%d" % t for t in g), 0) == 0 for h in hyps for g in counts(h, 1)), "every hypothesis n-gram has df > 0"
    assert any(h in rs for h, rs in zip(hyps, refs)), "no hypothesis equals a reference"
    matched = set()
    for n in (4,):
        for g in counts(hyps[8], n):
            if any(g in counts(r, n) for r in refs[8]):
                matched.add((g[0], "first"))
                matched.add((g[-1], "last"))
    for t in SPECIAL:
        assert (t, "first") in matched and (t, "last") in matched, "token %d does not open and close a matching 4-gram" % t
    assert int((stats[:, 3] > 0).sum()) * 3 >= CLIPS, "correct[4] > 0 in fewer than a third of the rows"
    assert float(np.min(cider_rows)) == 0.0 and float(np.max(cider_rows)) > 5.0 and rouge_rows[4] == 1.0

    flat = [r for rs in refs for r in rs]
    hyp, ref = np.zeros((CLIPS, TMAX), np.int32), np.zeros((len(flat), TMAX), np.int32)
    for i, h in enumerate(hyps):
        hyp[i, :len(h)] = h
    for i, r in enumerate(flat):
        ref[i, :len(r)] = r
    out = dict(hyp=hyp, hyp_len=np.array(lens, np.int32), ref=ref, ref_len=np.array([len(r) for r in flat], np.int32),
               ref_off=np.cumsum([0] + [len(rs) for rs in refs]).astype(np.int32), stats=stats, lcs=np.array(lcs_rows, np.int32),
               rouge=np.array(rouge_rows, np.float64), cider=np.array(cider_rows, np.float64),
               corpus_bleu=np.array(corpus_bleu, np.float64), corpus_rouge=np.array(np.mean(np.array(rouge_rows))),
               corpus_cider=np.array(corpus_cider, np.float64))
    path = os.path.join(HERE, "case_caption.npz")
    np.savez_compressed(path, **out)
    print("wrote case_caption.npz", os.path.getsize(path), "bytes;", len(flat), "references; corpus BLEU", corpus_bleu,
          "ROUGE_L", float(out["corpus_rouge"]), "CIDEr", float(corpus_cider), "; rows with correct[4] > 0:", int((stats[:, 3] > 0).sum()))


if __name__ == "__main__":
    main()
