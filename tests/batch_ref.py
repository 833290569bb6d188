"""Numpy restatement of batched conditioning (bnpp_condition_batch) and a
helper that draws evidence row sets.

gather: out[rest][b] = src[ev values of row b, rest], by fancy indexing of the
source reshaped to its scope's cardinalities; the evidence row b is the last
(fastest) dimension.  Values are moved, never computed on, so the engine's
output must equal this one bit for bit in any dtype.
"""
import numpy as np


def gather(src, cards, scope, ev_vars, ev):
    """src: the table over `scope` (natural layout, last variable fastest);
    ev: an (len(ev_vars), n_rows) integer array, variable-major.  Evidence
    variables outside the scope are ignored.  Returns the flat table over
    (scope minus ev_vars, order preserved; then the row), row fastest."""
    ev = np.asarray(ev).reshape(len(ev_vars), -1)
    n_rows = ev.shape[1]
    ev_vars = list(ev_vars)
    t = np.asarray(src).reshape([cards[v] for v in scope])
    rest = [v for v in scope if v not in ev_vars]
    ix, k = [], 0
    for v in scope:
        if v in ev_vars:
            ix.append(ev[ev_vars.index(v)].reshape([1] * len(rest) + [n_rows]))
        else:
            shape = [1] * (len(rest) + 1)
            shape[k] = cards[v]
            ix.append(np.arange(cards[v]).reshape(shape))
            k += 1
    out = t[tuple(ix)] if ix else t
    return np.ascontiguousarray(np.broadcast_to(out, [cards[v] for v in rest] + [n_rows])).reshape(-1)


def draw_rows(cards, ev_vars, n, seed, samples=None):
    """n evidence rows over ev_vars as an (n, len(ev_vars)) int array: the
    first half (rounded up) uniform over each variable's range; the second
    half taken from the columns ev_vars of `samples` (an (m, n_vars) array of
    joint samples, so these rows are possible), or uniform too without it."""
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.integers(0, cards[v], n) for v in ev_vars], axis=1).astype(np.int64) if len(ev_vars) \
        else np.zeros((n, 0), dtype=np.int64)
    if samples is not None and len(ev_vars):
        h = (n + 1) // 2
        s = np.asarray(samples)
        rows[h:] = s[:n - h][:, list(ev_vars)]
    return rows
