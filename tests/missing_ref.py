"""Numpy restatement of the masked gather (bnpp_condition_batch_mv), the rule
that picks the factor carrying a partial variable's mask, the per-row masked
model, and a brute-force joint that sums over a row's missing variables.

masked_gather moves values or writes 0 and does no arithmetic, so the engine's
table must equal it bit for bit in both dtypes.

Brute force: the full joint by einsum in fp64 (models of at most 2^16 joint
states); a row conditions it on its OBSERVED entries only (MISSING = -1 leaves
the variable free) -- the definition of a row's result.
"""
import numpy as np

MISSING = -1


def masked_gather(T, cards, scope, ev_vars, partial, ev):
    """T: the source over `scope` (natural layout, flat).  ev: (len(ev_vars), R)
    integers.  partial: the ev_vars that stay dims of the output.  Returns the
    table over (scope minus hard evidence variables in scope order, b), flat,
    in T's dtype: out[rest][b] = T[hard values of row b, rest] where every
    partial variable of the scope is missing (< 0) in row b or equals its digit
    of rest, else 0.  A hard value is clamped into range; a partial value >=
    the card matches nothing."""
    ev_vars, partial = list(ev_vars), set(partial)
    ev = np.asarray(ev).reshape(len(ev_vars), -1)
    R = ev.shape[1]
    t = np.asarray(T).reshape([cards[v] for v in scope])
    rest = [v for v in scope if v not in ev_vars or v in partial]
    shape = [cards[v] for v in rest]
    n_rest = int(np.prod(shape, dtype=np.int64)) if rest else 1
    out = np.zeros((n_rest, R), dtype=t.dtype)
    for b in range(R):
        ix = []
        for v in scope:
            if v in ev_vars and v not in partial:
                ix.append(int(np.clip(ev[ev_vars.index(v), b], 0, cards[v] - 1)))
            else:
                ix.append(slice(None))
        sub = t[tuple(ix)].reshape(shape if rest else [1])
        keep = np.ones(shape if rest else [1], dtype=bool)
        for d, v in enumerate(rest):
            if v in partial:
                x = int(ev[ev_vars.index(v), b])
                if x >= 0:
                    sel = np.arange(cards[v]) == x
                    keep &= sel.reshape([-1 if i == d else 1 for i in range(len(rest))])
        out[:, b] = np.where(keep, sub, 0).reshape(-1)
    return out.reshape(-1)


def mask_factors(model_dict, ev_vars, partial):
    """Per evidence variable the factor that carries its mask (-1: hard, or in
    no factor): 1. a factor holding a hard evidence variable; 2. among those,
    else among all factors holding it, the fewest entries after conditioning on
    the hard variables; 3. the lowest factor index."""
    cards, scopes = model_dict["cards"], model_dict["scopes"]
    hard = [v for v in ev_vars if v not in partial]
    out = []
    for v in ev_vars:
        if v not in partial:
            out.append(-1)
            continue
        cand = []
        for f, s in enumerate(scopes):
            if v in s:
                size = int(np.prod([cards[x] for x in s if x not in hard], dtype=np.int64))
                cand.append((0 if any(x in hard for x in s) else 1, size, f))
        out.append(min(cand)[2] if cand else -1)
    return out


def masked_model(model_dict, ev_vars, mask_factor, row):
    """The model whose mask-carrying factors are multiplied by the row's
    indicator of its observed partial entries (cards and scopes unchanged)."""
    cards, scopes = model_dict["cards"], model_dict["scopes"]
    values = [np.array(v, dtype=np.float64).reshape([cards[x] for x in s]) for s, v in zip(scopes, model_dict["values"])]
    for v, f, x in zip(ev_vars, mask_factor, row):
        if f < 0 or x < 0:
            continue
        d = scopes[f].index(v)
        sel = (np.arange(cards[v]) == int(x)).reshape([-1 if i == d else 1 for i in range(len(scopes[f]))])
        values[f] = values[f] * sel
    return dict(model_dict, values=[v.reshape(-1).tolist() for v in values])


def joint(model_dict):
    cards, scopes = model_dict["cards"], model_dict["scopes"]
    assert np.prod([float(c) for c in cards]) <= 2 ** 16
    ops = []
    for s, v in zip(scopes, model_dict["values"]):
        ops += [np.asarray(v, dtype=np.float64).reshape([cards[x] for x in s]), list(s)]
    return np.einsum(*ops, list(range(len(cards))))


def condition(jt, ev_vars, row):
    """The joint with everything that contradicts the row's observed entries zeroed."""
    cond = np.zeros_like(jt)
    ix = [slice(None)] * jt.ndim
    for v, x in zip(ev_vars, row):
        if x >= 0:
            ix[v] = slice(int(x), int(x) + 1)
    cond[tuple(ix)] = jt[tuple(ix)]
    return cond


def brute(model_dict, ev_vars, rows, w=None):
    """-> (z[n], marginals: per variable an (n, card) array, NaN for Z = 0,
    counts: per factor the array over its scope, summed over the possible rows)."""
    cards, scopes = model_dict["cards"], model_dict["scopes"]
    nv = len(cards)
    jt = joint(model_dict)
    rows = np.asarray(rows).reshape(len(rows), len(ev_vars))
    w = np.ones(len(rows)) if w is None else np.asarray(w, dtype=np.float64)
    z = np.zeros(len(rows))
    marg = [np.full((len(rows), c), np.nan) for c in cards]
    counts = [np.zeros([cards[x] for x in s]) for s in scopes]
    for b, row in enumerate(rows):
        cond = condition(jt, ev_vars, row)
        z[b] = cond.sum()
        if z[b] == 0:
            continue
        post = cond / z[b]
        for v in range(nv):
            marg[v][b] = np.einsum(post, list(range(nv)), [v])
        for f, s in enumerate(scopes):
            counts[f] += w[b] * np.einsum(post, list(range(nv)), list(s))
    return z, marg, counts


def punch(rng, rows, frac, cols=None):
    """A copy of rows with about `frac` of the cells of `cols` (default: all) MISSING."""
    rows = np.array(rows, dtype=np.int64)
    cols = range(rows.shape[1]) if cols is None else cols
    for j in cols:
        rows[rng.random(rows.shape[0]) < frac, j] = MISSING
    return rows


# the sampling distribution tests (test_missing_host.py, test_gpu_missing.py): sample_batch_ref's case with the
# third evidence variable partial and missing in every other row.  The first candidate seed;
# test_missing_host.py asserts that the numpy restatement alone stays within sample_ref.bound under it
DIST_SEED = 20261020


def dist_case(model):
    """-> (ev_vars, rows, partial): sample_batch_ref.dist_case's 8 rows, the last evidence variable missing in rows 0, 2, 4, 6."""
    import sample_batch_ref as sbr
    ev_vars, rows = sbr.dist_case(model)
    rows = rows.copy()
    rows[::2, 2] = MISSING
    return ev_vars, rows, [ev_vars[2]]


def frequency_violations(model, ev_vars, rows, samples):
    """sample_batch_ref.frequency_violations with a row's observed entries as its evidence."""
    import sample_ref as sr
    bad = []
    for b, row in enumerate(rows):
        ev = {v: int(x) for v, x in zip(ev_vars, row) if x >= 0}
        for v in sr.check_frequencies(samples[b], model["cards"], joint_of=sr.joint(model, ev)):
            bad.append((b,) + tuple(v))
    return bad
