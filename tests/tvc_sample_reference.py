"""Float64 restatement of sampled captioning, written from the rules (include/hero_hip.h "Sampled decoding",
TvcGenerator.sample_decode) in numpy - no library kernel, no torch.sort / multinomial, no code of the package; the two hashes come
from tests/dropout_hash.py:

    rows       R = N * S, row n * S + s = sample s of caption n
    finished   token = eos; cum, len unchanged; ids[r, t] = last[r] = eos; kept[r] = 0
    order      z_v = fp32(logit_v) * fp32(1 / temperature), ONE fp32 rounding (the input values of everything below); candidates by z
               descending, among equal z the lower token
    top-k      the first min(top_k, V) candidates (0 = off)
    top-p      masses exp(z_v - max z) over those; the shortest prefix whose mass is >= top_p * the mass of all of them, at least one
               candidate (top_p is the fp32 value; >= 1 = off)
    draw       the kept v that maximises z_v + g_v, among equals the lower token;  g = -log(-log1p(-u)),  u = (2h + 1) * 2^-24,
               h = mix32(v ^ (uint32)base) >> 9,  base = splitmix64(seed ^ (site * 0xD6E8FEB86659FD93)),  site = t * R + r
    update     cum += logit_v - lse (lse of the RAW row), len += 1, fin = (v == eos), ids[r, t] = last[r] = v, kept = the kept size
    pick       per caption the sample with the largest cum / max(len, 1) ** length_penalty, the lower sample among equals

What an fp32 implementation cannot be asked to reproduce is stated by two measured bounds (measure_bounds() below measures them
against this float64 statement, never against a kernel; tests/test_cpu_tvc_sample.py asserts that the recorded values cover it):

    DELTA   4 x the largest error of a numpy-float32 restatement of the normalised prefix mass (fp32 masses, numpy's pairwise
            np.sum(dtype=float32)) at the kept sizes around the nucleus boundary.  Every row comes with the bracket [j_lo, j_hi],
            the kept sizes at top_p -/+ DELTA; j_lo == j_hi: the kept size is determined.
    GAMMA   4 x the largest error of a float32 restatement of z + g.  A row whose two best perturbed scores (for a given kept
            size) are closer than GAMMA is a near-tie: either of the two tokens is admissible.

Measured over every case of this module (bf16-rounded normal logits, sigma 4): prefix-mass error 5.6e-7 at most, error of z + g
1.45e-6 at most."""
import numpy as np
import torch

from tests.dropout_hash import _mix32, _splitmix64

DELTA = 2.3e-6          # 4 x 5.6e-7, rounded up
GAMMA = 6.0e-6          # 4 x 1.45e-6, rounded up
_M64 = (1 << 64) - 1


def inv_temperature(temperature):
    return np.float32(1.0 / float(temperature))


def uniforms(seed, t, R, V):
    """u [R, V] float64, exact: (2h + 1) * 2^-24."""
    keys = np.array([_splitmix64((int(seed) & _M64) ^ (((t * R + r) * 0xD6E8FEB86659FD93) & _M64)) & 0xFFFFFFFF for r in range(R)],
                    dtype=np.uint64)
    h = _mix32(np.arange(V, dtype=np.uint64)[None, :] ^ keys[:, None]) >> np.uint64(9)
    return (2.0 * h.astype(np.float64) + 1.0) * 2.0 ** -24


def gumbel(u):
    return -np.log(-np.log1p(-u))


def _np(x):
    return x.detach().cpu().float().numpy() if torch.is_tensor(x) else np.asarray(x)


def _kept_size(csum, total, p, K):
    return np.minimum((csum < p * total).sum(axis=1) + 1, K)


def select_step(logits, tables, t, eos, seed, temperature, top_k, top_p, delta=DELTA):
    """logits [R, V] (a torch tensor of any float dtype or an array; widened, not re-derived); tables: cum, fin, len [R], ids
    [R, Tcap] (arrays or tensors) -> dict of float64 / int64 arrays: cum, fin, len, ids, last, kept after the step, and what the
    tests need to judge another implementation: j_lo, j_hi [R] (the bracket; 0 for finished rows), gap [R] (between the two best
    perturbed scores at the reference's kept size; inf with one candidate or a finished row), order [R, V] (tokens in candidate
    order), pert [R, V] (z + g by token), lse [R] of the raw rows, the inputs x, live [R], and frac [R, K] (the normalised prefix
    masses; None when top-p is off)."""
    x32 = _np(logits).astype(np.float32)
    R, V = x32.shape
    x = x32.astype(np.float64)
    z = (x32 * inv_temperature(temperature)).astype(np.float64)                   # the product is rounded to fp32 once
    order = np.argsort(-z, axis=1, kind="stable")                                   # -0.0 == 0.0: equal, the lower token first
    zs = np.take_along_axis(z, order, axis=1)
    K = min(int(top_k), V) if top_k > 0 else V
    p = float(np.float32(top_p))
    kept = np.full(R, K, dtype=np.int64)
    j_lo, j_hi = kept.copy(), kept.copy()
    frac = None
    if p < 1.0:
        csum = np.cumsum(np.exp(zs[:, :K] - zs[:, :1]), axis=1)
        total = csum[:, -1:]
        kept, j_lo, j_hi = (_kept_size(csum, total, q, K) for q in (p, p - delta, p + delta))
        frac = csum / total
    pert = z + gumbel(uniforms(seed, t, R, V))
    m = x.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]
    cum = np.asarray(_np(tables["cum"]), dtype=np.float64).copy()
    fin, length = (np.asarray(_np(tables[k])).astype(np.int64).copy() for k in ("fin", "len"))
    ids = np.asarray(_np(tables["ids"])).astype(np.int64).copy()
    out = {"x": x, "order": order, "pert": pert, "lse": lse, "frac": frac, "live": fin == 0, "zs": zs,
           "last": np.full(R, eos, dtype=np.int64), "gap": np.full(R, np.inf)}
    for r in range(R):
        if fin[r]:
            kept[r] = j_lo[r] = j_hi[r] = 0
            ids[r, t] = eos
            continue
        v, second, gap = draw(out, r, int(kept[r]))
        out["gap"][r] = gap
        out["last"][r] = v
        cum[r] += x[r, v] - lse[r]
        length[r] += 1
        fin[r] = int(v == eos)
        ids[r, t] = v
    out.update(cum=cum, fin=fin, len=length, ids=ids, kept=kept, j_lo=j_lo, j_hi=j_hi)
    return out


def draw(step, r, j):
    """The draw of row r if its kept set were the first j candidates -> (token, runner-up token or -1, the gap between them)."""
    cand = step["order"][r, :j]
    score = step["pert"][r, cand]
    rank = np.lexsort((cand, -score))                                               # score descending, then the lower token
    if j == 1:
        return int(cand[rank[0]]), -1, float("inf")
    return int(cand[rank[0]]), int(cand[rank[1]]), float(score[rank[0]] - score[rank[1]])


def admissible(step, r, j, gamma=GAMMA):
    """The tokens an fp32 implementation may draw in row r with kept size j: the float64 draw, and the runner-up in a near-tie."""
    v, second, gap = draw(step, r, j)
    return {v, second} if gap <= gamma else {v}


def cum_after(step, tables, r, v):
    return float(np.asarray(_np(tables["cum"]), dtype=np.float64)[r] + step["x"][r, v] - step["lse"][r])


def initial_tables(R, max_step):
    return {"cum": np.zeros(R), "fin": np.zeros(R, dtype=np.int64), "len": np.zeros(R, dtype=np.int64),
            "ids": np.zeros((R, max_step), dtype=np.int64)}


# ---- float32 restatements: what DELTA and GAMMA are measured on ---------------------------------------------------------------
def prefix_mass_error(step):
    """Largest |fp32 - float64| of the normalised prefix mass at the kept sizes j - 1, j, j + 1 around every live row's boundary:
    fp32 masses exp(z - max z) summed by numpy's pairwise np.sum(dtype=float32)."""
    if step["frac"] is None:
        return 0.0
    worst = 0.0
    K = step["frac"].shape[1]
    zs32 = step["zs"][:, :K].astype(np.float32)
    mass = np.exp(zs32 - zs32[:, :1]).astype(np.float32)
    for r in np.nonzero(step["live"])[0]:
        total = np.sum(mass[r], dtype=np.float32)
        for j in {max(int(step["kept"][r]) - 1, 1), int(step["kept"][r]), min(int(step["kept"][r]) + 1, K)}:
            got = np.float32(np.sum(mass[r, :j], dtype=np.float32) / total)
            worst = max(worst, abs(float(got) - float(step["frac"][r, j - 1])))
    return worst


def perturbed_error(logits, t, seed, temperature):
    """Largest |fp32 - float64| of z + g over the row set: g = -log(-log1p(-u)) evaluated in numpy float32."""
    x32 = _np(logits).astype(np.float32)
    R, V = x32.shape
    z32 = x32 * inv_temperature(temperature)
    u = uniforms(seed, t, R, V)
    u32 = u.astype(np.float32)
    g32 = -np.log(-np.log1p(-u32))
    return float(np.abs((z32 + g32).astype(np.float64) - (z32.astype(np.float64) + gumbel(u))).max())


# ---- cases -----------------------------------------------------------------------------------------------------------------
SELECT_SHAPES = [(1, 1), (1, 8), (5, 3), (3, 4)]                # (N, S)
SELECT_VOCABS = [160, 1000, 50272]
SELECT_PARAMS = [(1.0, 0, 1.0), (0.7, 0, 0.9), (1.3, 0, 0.5), (1.0, 50, 0.9), (1.0, 1, 1.0)]      # (temperature, top_k, top_p)
SMALL_V_PARAMS = (1.0, 5, 1.0)                                  # added at V = 160
ODD_VOCAB = 1003                                                # not a multiple of 4: the scalar row loop
SELECT_TCAP, SELECT_MID_T, SELECT_EOS, SELECT_SEED = 12, 5, 7, 0x5EED0123456789AB
MIN_DETERMINED, MIN_GAPPED = 0.95, 0.99
_SELECT = {}


def params_of(V):
    return SELECT_PARAMS + ([SMALL_V_PARAMS] if V == 160 else [])


def case_conditions(step):
    """(share of the live rows whose kept size is determined, share whose draw is no near-tie), from the reference alone."""
    live = step["live"]
    n = max(int(live.sum()), 1)
    return float(((step["j_lo"] == step["j_hi"]) & live).sum()) / n, float(((step["gap"] > GAMMA) & live).sum()) / n


def select_case(N, S, V, dtype, mid, params):
    """Inputs of one sampling step on the CPU, drawn once per case and never modified, with the float64 result:
    logits [R, ld] in `dtype`, bf16-rounded normal values of sigma 4 (ld = V + 8 for V = 1000, the padded vocabulary, else V; the
    columns behind V hold a large value that must not be read), and the tables - all rows alive at cum = 0 at t = 0, or (mid)
    random ones at t = SELECT_MID_T: cum in [-20, 0], a third of the rows finished, random lengths and ids.
    A draw of logits that leaves fewer than MIN_DETERMINED / MIN_GAPPED of its live rows determined is sharpened by drawing it
    again from the next seed (judged by this reference alone); tests/test_cpu_tvc_sample.py asserts the conditions."""
    key = (N, S, V, dtype, mid, params)
    if key not in _SELECT:
        temperature, top_k, top_p = params
        R, Tcap = N * S, SELECT_TCAP
        ld = V + 8 if V == 1000 else V
        base = 7000 + 101 * N + 17 * S + V + (5 if mid else 0) + (1 if dtype == torch.bfloat16 else 0) + 1009 * SELECT_PARAMS.index(params) \
            if params in SELECT_PARAMS else 99000 + 101 * N + 17 * S + V + (5 if mid else 0) + (1 if dtype == torch.bfloat16 else 0)
        for attempt in range(8):
            g = torch.Generator().manual_seed(base + 100003 * attempt)
            logits = torch.full((R, ld), 60.0)
            logits[:, :V] = (4.0 * torch.randn(R, V, generator=g)).bfloat16().float()
            logits = logits.to(dtype)
            tables = initial_tables(R, Tcap)
            t = 0
            if mid:
                t = SELECT_MID_T
                tables["cum"] = (-20.0 * torch.rand(R, generator=g, dtype=torch.float32)).numpy().astype(np.float64)
                tables["fin"] = (torch.rand(R, generator=g) < 0.34).long().numpy()
                tables["fin"][0] = 0                                                  # at least one live row in every case
                tables["len"] = torch.randint(1, t + 1, (R,), generator=g).numpy()
                tables["ids"] = torch.randint(0, V, (R, Tcap), generator=g).numpy()
            want = select_step(logits[:, :V], tables, t, SELECT_EOS, SELECT_SEED, temperature, top_k, top_p)
            determined, gapped = case_conditions(want)
            if determined >= MIN_DETERMINED and gapped >= MIN_GAPPED:
                break
        _SELECT[key] = dict(logits=logits, tables=tables, t=t, want=want, V=V, ld=ld, attempt=attempt, params=params)
    return _SELECT[key]


def all_cases():
    for N, S in SELECT_SHAPES:
        for V in SELECT_VOCABS:
            for dtype in (torch.float32, torch.bfloat16):
                for mid in (False, True):
                    for params in params_of(V):
                        yield N, S, V, dtype, mid, params


def measure_bounds(cases=None):
    """-> (largest prefix-mass error, largest error of z + g) of the float32 restatements over the cases."""
    mass = score = 0.0
    for N, S, V, dtype, mid, params in (cases or all_cases()):
        c = select_case(N, S, V, dtype, mid, params)
        mass = max(mass, prefix_mass_error(c["want"]))
        score = max(score, perturbed_error(c["logits"][:, :V], c["t"], SELECT_SEED, params[0]))
    return mass, score


def tie_case(top_p):
    """The tie rule: logits on the grid {-1, 0, 1, 2} at V = 160 with nine tokens at the maximum, top_k = 5.  top_p = 1: the five
    lowest-index maxima are kept.  top_p = 0.5: the five survivors have equal masses, so the boundary falls inside the equal-z
    run and exactly three are kept (0.4 < 0.5 <= 0.6).  20 rows: with 10 positions, 200 draws."""
    V, R = 160, 20
    g = torch.Generator().manual_seed(4242)
    row = torch.randint(-1, 2, (V,), generator=g).float()
    top = torch.randperm(V, generator=g)[:9].sort().values
    row[top] = 2.0
    return dict(logits=row.repeat(R, 1), V=V, R=R, top=top.tolist(), params=(1.0, 5, float(top_p)), positions=list(range(10)),
                kept=5 if top_p >= 1 else 3)


def distribution_case(top_k):
    """V = 16, 20 000 draws over distinct (t, r): 100 positions x 200 identical rows, fixed seed."""
    g = torch.Generator().manual_seed(1618)
    row = (1.5 * torch.randn(16, generator=g)).bfloat16().float()
    return dict(logits=row.repeat(200, 1), V=16, R=200, positions=list(range(100)), params=(1.0, int(top_k), 1.0), seed=20240607)


def chi_square(tokens, row, top_k):
    """Pearson's statistic of the drawn tokens against the softmax of `row` (renormalised over its top_k when top_k > 0)."""
    x = np.asarray(row, dtype=np.float64)
    p = np.exp(x - x.max())
    if top_k > 0:
        keep = np.argsort(-x, kind="stable")[:top_k]
        mask = np.zeros_like(p)
        mask[keep] = 1.0
        p = p * mask
    p = p / p.sum()
    counts = np.bincount(np.asarray(tokens, dtype=np.int64), minlength=x.size).astype(np.float64)
    assert counts[p == 0].sum() == 0, "a token outside the kept set was drawn"
    n = counts.sum()
    return float((((counts - n * p) ** 2)[p > 0] / (n * p[p > 0])).sum())


# ---- the whole decode ------------------------------------------------------------------------------------------------------
def pick(cum, length, N, S, length_penalty):
    norm = np.asarray(cum, dtype=np.float64).reshape(N, S) / np.maximum(np.asarray(length).reshape(N, S), 1).astype(np.float64) ** float(length_penalty)
    best = np.argsort(-norm, axis=1, kind="stable")[:, 0]
    srt = -np.sort(-norm, axis=1)
    margin = srt[:, 0] - srt[:, 1] if S > 1 else np.full(N, np.inf)
    return best, norm, margin


def cut_eos(ids, eos):
    out = []
    for i in ids:
        if i == eos:
            break
        out.append(int(i))
    return out


def decode(step_fn, N, S, max_step, bos, eos, seed, temperature=1.0, top_k=0, top_p=1.0, length_penalty=1.0, delta=DELTA, gamma=GAMMA):
    """The whole sampled decode.  step_fn(t, last [R] int64 torch tensor) -> logits [R, V] of step t.
    -> dict: all_ids (R lists cut at eos), all_scores [R], ids / scores of the picked samples, best [N], pick_margin [N],
    determined [R] (every step's kept size determined and no near-tie: the row's tokens are the only admissible ones), finished.
    delta / gamma: wider margins for a comparison between two routes whose step scores differ in their last bits."""
    R = N * S
    tables = initial_tables(R, max_step)
    last = torch.full((R,), bos, dtype=torch.long)
    determined = np.ones(R, dtype=bool)
    for t in range(max_step):
        step = select_step(step_fn(t, last), tables, t, eos, seed, temperature, top_k, top_p, delta=delta)
        determined &= ~step["live"] | ((step["j_lo"] == step["j_hi"]) & (step["gap"] > gamma))
        tables = {k: step[k] for k in ("cum", "fin", "len", "ids")}
        last = torch.from_numpy(step["last"])
    best, norm, margin = pick(tables["cum"], tables["len"], N, S, length_penalty)
    rows = np.arange(N) * S + best
    all_ids = [cut_eos(r, eos) for r in tables["ids"].tolist()]
    return {"all_ids": all_ids, "all_scores": norm.reshape(-1), "ids": [all_ids[r] for r in rows], "scores": norm[np.arange(N), best],
            "best": best, "pick_margin": margin, "determined": determined, "finished": int(tables["fin"].sum()), "tables": tables}
