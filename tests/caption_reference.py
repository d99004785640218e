"""Caption metrics on integer token sequences in plain Python and float64: BLEU-1..4 (reference length "closest"), ROUGE-L and
CIDEr-D as the reference's eval/pycocoevalcap computes them on word strings (BleuScorer(n=4), Rouge(), CiderScorer(n=4,
sigma=6.0)), restated on lists of ints.  tests/golden/case_caption.npz holds what those scorers gave; tests/test_cpu_caption.py
holds this module to it (integers equal, floats within 1e-12), and the GPU tests hold the kernel to this module.

    document_frequency(refs)                -> (df {n-gram tuple: number of clips}, C)
    score_clip(hyp, refs, df, C)            -> dict(correct[4], guess[4], testlen, reflen, lcs, rouge, cider)
    score_corpus(hyps, refs, idf_refs=None) -> (list of per-clip dicts, corpus dict with the keys and scale of eval/tvc.py)
    cut(row, eos, tcap)                     -> the caption of a decoder's id row: everything before the first eos within tcap"""
import math
from collections import Counter

N_ORDERS, SIGMA, BETA2 = 4, 6.0, 1.44


def ngrams(seq):
    """Counter over the n-gram tuples of every order 1..4."""
    seq = list(seq)
    return Counter(tuple(seq[i:i + n]) for n in range(1, N_ORDERS + 1) for i in range(len(seq) - n + 1))


def document_frequency(refs):
    df = Counter()
    for clip in refs:
        df.update(set(g for r in clip for g in ngrams(r)))
    return df, len(refs)


def lcs(a, b):
    row = [0] * (len(b) + 1)
    for x in a:
        prev = 0
        for j, y in enumerate(b):
            cur = row[j + 1]
            row[j + 1] = prev + 1 if x == y else max(row[j + 1], row[j])
            prev = cur
    return row[len(b)]


def _weights(counts, df, log_c):
    vec = [dict() for _ in range(N_ORDERS)]
    for g, c in counts.items():
        vec[len(g) - 1][g] = float(c) * (log_c - math.log(max(1.0, float(df.get(g, 0)))))
    return vec, [math.sqrt(sum(w * w for w in v.values())) for v in vec]


def score_clip(hyp, refs, df, C):
    hyp = list(hyp)
    ch = ngrams(hyp)
    cr = [ngrams(r) for r in refs]
    # BLEU statistics
    correct = [0] * N_ORDERS
    for g, c in ch.items():
        correct[len(g) - 1] += min(c, max(r.get(g, 0) for r in cr))
    guess = [max(0, len(hyp) - n + 1) for n in range(1, N_ORDERS + 1)]
    reflen = min((abs(len(r) - len(hyp)), len(r)) for r in refs)[1]
    # ROUGE-L
    ls = [lcs(hyp, r) for r in refs]
    p = max(ls) / float(max(len(hyp), 1))
    q = max(l / float(len(r)) for l, r in zip(ls, refs))
    rouge = (1.0 + BETA2) * p * q / (q + BETA2 * p) if p != 0 and q != 0 else 0.0
    # CIDEr-D
    log_c = math.log(float(C))
    vh, nh = _weights(ch, df, log_c)
    total = [0.0] * N_ORDERS
    for r, counts in zip(refs, cr):
        vr, nr = _weights(counts, df, log_c)
        delta = float(max(len(hyp) - 1, 0) - max(len(r) - 1, 0))
        for n in range(N_ORDERS):
            val = sum(min(w, vr[n].get(g, 0.0)) * vr[n].get(g, 0.0) for g, w in vh[n].items())
            if nh[n] != 0 and nr[n] != 0:
                val /= nh[n] * nr[n]
            total[n] += val * math.exp(-(delta ** 2) / (2.0 * SIGMA ** 2))
    cider = sum(total) / N_ORDERS / len(refs) * 10.0
    return dict(correct=correct, guess=guess, testlen=len(hyp), reflen=reflen, lcs=max(ls), rouge=rouge, cider=cider)


def corpus_bleu(correct, guess, testlen, reflen):
    """bleu_scorer.py:252-261 on the summed statistics."""
    small, tiny = 1e-9, 1e-15
    out, bleu = [], 1.0
    for k in range(N_ORDERS):
        bleu *= float(correct[k] + tiny) / (guess[k] + small)
        out.append(bleu ** (1.0 / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out


def score_corpus(hyps, refs, idf_refs=None):
    df, C = document_frequency(refs if idf_refs is None else idf_refs)
    rows = [score_clip(h, r, df, C) for h, r in zip(hyps, refs)]
    bleu = corpus_bleu([sum(r["correct"][k] for r in rows) for k in range(N_ORDERS)],
                       [sum(r["guess"][k] for r in rows) for k in range(N_ORDERS)],
                       sum(r["testlen"] for r in rows), sum(r["reflen"] for r in rows))
    out = {"Bleu_%d" % (k + 1): bleu[k] * 100 for k in range(N_ORDERS)}
    out["ROUGE_L"] = sum(r["rouge"] for r in rows) / len(rows) * 100
    out["CIDEr"] = sum(r["cider"] for r in rows) / len(rows) * 100
    return rows, out


def cut(row, eos, tcap=None):
    row = list(row)[:tcap]
    return row[:row.index(eos)] if eos in row else row


def stats_row(s):
    """The kernel's ten integers of one row."""
    return list(s["correct"]) + list(s["guess"]) + [s["testlen"], s["reflen"]]
