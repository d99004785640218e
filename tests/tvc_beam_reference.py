"""Float64 restatement of beam-search captioning, written from the rules (include/hero_hip.h "Beam-search selection",
TvcGenerator.beam_decode) - no library kernel, no torch.topk, no code of the package:

    rows       R = N * B, row n * B + b = beam b of caption n
    live b     candidates (b, v): cum[b] + x[b, v] - lse_b,  lse_b = max_v x + log(sum_v exp(x - max))
    finished   exactly one candidate (b, eos) at cum[b]
    choice     the B best by score descending, among equal scores the lower flat index b * V + v; new beam i = the i-th best
    update     cum' = score, fin' = fin[p] | (v == eos), len' = len[p] + (fin[p] ? 0 : 1), ids'[i, :t] = ids[p, :t], ids'[i, t] = v,
               anc'[i, :t] = anc[p, :t], anc'[i, t] = n * B + p, last[i] = v
    pick       per caption the beam with the largest cum / max(len, 1) ** length_penalty, the lower beam among equals

The input values are used as they are given (a bf16 or fp32 tensor is widened, not re-derived).

The GAP of a caption at a step is the smallest difference between consecutive scores among its best B + 1 candidates: what
an fp32 implementation must resolve to choose the same candidates in the same order.  An exact tie inside one beam (equal
logits under one cum) is not counted - the index rule decides it on both sides.  A caption whose gap is below a test's
threshold at any step takes no part in that test's id comparison."""
import torch

DEAD = -1.0e30


def initial_tables(N, B, max_step):
    cum = torch.full((N, B), DEAD, dtype=torch.float64)
    cum[:, 0] = 0.0
    R = N * B
    return {"cum": cum.reshape(R), "fin": torch.zeros(R, dtype=torch.long), "len": torch.zeros(R, dtype=torch.long),
            "ids": torch.zeros((R, max_step), dtype=torch.long),
            "anc": torch.arange(R).unsqueeze(1).repeat(1, max_step)}


def select_step(logits, tables, t, B, eos):
    """logits [R, V]; tables: cum [R] (any float), fin, len [R], ids, anc [R, Tcap] (any integer dtype) -> (new tables with float64
    cum and int64 indices, plus "parent" [R] the parent BEAM and "last" [R] the token of every new beam; gap [N] float64)."""
    x = logits.detach().cpu().double()
    R, V = x.shape
    N = R // B
    cum = tables["cum"].detach().cpu().double()
    fin, length = tables["fin"].cpu().long(), tables["len"].cpu().long()
    ids, anc = tables["ids"].cpu().long().clone(), tables["anc"].cpu().long().clone()
    m = x.max(dim=1, keepdim=True).values
    lse = m + torch.log(torch.exp(x - m).sum(dim=1, keepdim=True))
    cand = cum.unsqueeze(1) + (x - lse)
    for r in range(R):
        if fin[r]:
            cand[r] = float("-inf")
            cand[r, eos] = cum[r]
    flat = cand.view(N, B * V)
    val, idx = torch.sort(flat, dim=1, descending=True, stable=True)            # stable: the lower flat index first among equals
    out = {"cum": torch.empty(R, dtype=torch.float64), "fin": torch.empty(R, dtype=torch.long), "len": torch.empty(R, dtype=torch.long),
           "ids": ids.clone(), "anc": anc.clone(), "parent": torch.empty(R, dtype=torch.long), "last": torch.empty(R, dtype=torch.long)}
    gap = torch.full((N,), float("inf"), dtype=torch.float64)
    for n in range(N):
        k = min(B + 1, B * V)
        best, where = val[n, :k], idx[n, :k]
        for a in range(k - 1):
            if best[a + 1] == float("-inf"):
                break
            d = float(best[a] - best[a + 1])
            if d == 0.0 and int(where[a]) // V == int(where[a + 1]) // V:
                continue                                                          # equal logits under one cum: the index rule
            gap[n] = min(float(gap[n]), d)
        for i in range(B):
            p, v, r = int(where[i]) // V, int(where[i]) % V, n * B + i
            pr = n * B + p
            out["cum"][r] = best[i]
            out["fin"][r] = int(bool(fin[pr]) or v == eos)
            out["len"][r] = int(length[pr]) + (0 if fin[pr] else 1)
            out["ids"][r, :t] = ids[pr, :t]
            out["ids"][r, t] = v
            out["anc"][r, :t] = anc[pr, :t]
            out["anc"][r, t] = pr
            out["parent"][r] = p
            out["last"][r] = v
    return out, gap


SELECT_SHAPES = [(1, 1), (1, 8), (5, 3), (3, 4)]                # (N, B)
SELECT_VOCABS = [160, 1000, 50272]
SELECT_TCAP, SELECT_MID_T, SELECT_EOS = 12, 5, 7
_SELECT = {}


def select_case(N, B, V, dtype, mid):
    """Inputs of one selection step on the CPU, drawn once per case and never modified, with the float64 result and gaps:
    logits [R, ld] in `dtype` (ld = V + 8 for V = 1000, else V; the columns behind V hold a large value that must not be read),
    and the tables - the initial ones at t = 0, or (mid) random ones at t = SELECT_MID_T: cum in [-20, 0], a third of the
    beams finished, random lengths, ids and in-caption ancestries.  |score| stays below 64."""
    key = (N, B, V, dtype, mid)
    if key not in _SELECT:
        g = torch.Generator().manual_seed(9000 + 101 * N + 17 * B + V + (5 if mid else 0) + (1 if dtype == torch.bfloat16 else 0))
        R, Tcap = N * B, SELECT_TCAP
        ld = V + 8 if V == 1000 else V
        logits = torch.full((R, ld), 60.0)
        logits[:, :V] = 3.0 * torch.randn(R, V, generator=g)
        logits = logits.to(dtype)
        tables = initial_tables(N, B, Tcap)
        t = 0
        if mid:
            t = SELECT_MID_T
            tables["cum"] = -20.0 * torch.rand(R, generator=g, dtype=torch.float32)
            tables["fin"] = (torch.rand(R, generator=g) < 0.34).long()
            tables["len"] = torch.randint(1, t + 1, (R,), generator=g)
            tables["ids"] = torch.randint(0, V, (R, Tcap), generator=g)
            tables["anc"] = (torch.arange(R).unsqueeze(1) // B) * B + torch.randint(0, B, (R, Tcap), generator=g)
        tables["cum"] = tables["cum"].float()
        want, gap = select_step(logits[:, :V], tables, t, B, SELECT_EOS)
        _SELECT[key] = dict(logits=logits, tables=tables, t=t, want=want, gap=gap, V=V, ld=ld)
    return _SELECT[key]


def pick(tables, N, B, length_penalty):
    """-> (best beam [N], its normalised score [N] float64, the distance to the second best [N]; inf with one beam)."""
    norm = tables["cum"].double().view(N, B) / tables["len"].view(N, B).clamp(min=1).double() ** float(length_penalty)
    val, idx = torch.sort(norm, dim=1, descending=True, stable=True)
    margin = val[:, 0] - val[:, 1] if B > 1 else torch.full((N,), float("inf"), dtype=torch.float64)
    return idx[:, 0], val[:, 0], margin


def cut_eos(ids, eos):
    out = []
    for i in ids:
        if i == eos:
            break
        out.append(i)
    return out


def search(step_fn, N, B, max_step, bos, eos, length_penalty=1.0):
    """The whole search.  step_fn(t, last [R] int64, parent_rows [R] int64 | None) -> logits [R, V] of step t, where row i
    continues row parent_rows[i] of the step before (None at t = 0).
    -> dict: ids (N lists cut at eos), scores [N], gaps [N, max_step], pick_margin [N], best [N], finished (count of finished
    beams), tables."""
    tables = initial_tables(N, B, max_step)
    last, parents, gaps = torch.full((N * B,), bos, dtype=torch.long), None, []
    for t in range(max_step):
        logits = step_fn(t, last, parents)
        tables, gap = select_step(logits, tables, t, B, eos)
        gaps.append(gap)
        last = tables["last"]
        parents = torch.arange(N).repeat_interleave(B) * B + tables["parent"]
    best, score, margin = pick(tables, N, B, length_penalty)
    rows = torch.arange(N) * B + best
    return {"ids": [cut_eos(r, eos) for r in tables["ids"][rows].tolist()], "scores": score, "gaps": torch.stack(gaps, dim=1),
            "pick_margin": margin, "best": best, "finished": int(tables["fin"].sum()), "tables": tables}
