"""Numpy restatement of the expected-counts accumulate step
(bnpp_bucket_counts) and a brute-force reference for whole runs.

accumulate: the contract of include/bnpp.h in the same order of operations --
sequential column sums, one division and one product per term, and np.add.at,
which adds in index order, over rows ascending -- so the engine's accumulator
must equal this one bit for bit.

brute_counts: the full joint by einsum in fp64 (models of at most 2^16 joint
states), conditioned per row, marginalised to every factor scope and summed.
"""
import numpy as np

# the evidence variables of the whole-run tests, per model
EV_VARS = {"asia": [0, 3, 6, 7], "cancer": [0, 3], "earthquake": [2, 4], "ising4x4": [0, 5, 10, 15],
           "alarm": [3, 10, 20], "ising6x6": [0, 7, 20, 35], "potts4x5k3": [1, 8, 19],
           "noisyor_30_40": [2, 35, 50, 65]}


def accumulate(acc, T, cards, scope, ev_vars, ev, w, rows_live, valid, has_b, n_rows):
    """Adds into acc (flat float64, the factor's natural layout over `scope`).

    T: the belief over (scope minus ev_vars in scope order, b), b fastest, as a
    flat array of R = n_rows rows (has_b False: no b dimension).  ev: an
    (len(ev_vars), R) integer array; w: R weights or None; valid: R entries or
    None.  Returns acc.
    """
    ev_vars = list(ev_vars)
    R = int(n_rows)
    ev = np.asarray(ev).reshape(len(ev_vars), R)
    rest = [v for v in scope if v not in ev_vars]
    n_rest = int(np.prod([cards[v] for v in rest], dtype=np.int64)) if rest else 1
    t = np.asarray(T, dtype=np.float64).reshape(n_rest, R if has_b else 1)
    if not has_b:
        t = np.broadcast_to(t, (n_rest, R))
    c = np.zeros(R)
    for r in range(n_rest):                                 # ascending rest index, sequentially from 0.0
        c = c + t[r]
    w = np.ones(R) if w is None else np.asarray(w, dtype=np.float64)
    keep = (np.arange(R) < rows_live) & (w != 0) & (c != 0) & ~np.isnan(c)
    if valid is not None:
        keep &= np.asarray(valid, dtype=np.float64).reshape(-1) != 0
    strides = {}
    st = 1
    for v in reversed(scope):
        strides[v] = st
        st *= cards[v]
    key = np.zeros(R, dtype=np.int64)
    for j, v in enumerate(ev_vars):
        if v in strides:
            key += np.clip(ev[j], 0, cards[v] - 1).astype(np.int64) * strides[v]
    rows = np.flatnonzero(keep)                             # ascending
    for r in range(n_rest):
        off, q = 0, r
        for v in reversed(rest):
            off += (q % cards[v]) * strides[v]
            q //= cards[v]
        with np.errstate(all="ignore"):
            term = w[rows] * (t[r][rows] / c[rows])
        np.add.at(acc, off + key[rows], term)
    return acc


def brute_counts(model_dict, ev_vars, rows, w=None):
    """Per factor (model order) the float64 array N_f over the factor's scope:
    sum over the possible rows b of w_b P(x_S | row b).  Also returns Z per row."""
    cards, scopes = model_dict["cards"], model_dict["scopes"]
    nv = len(cards)
    assert np.prod([float(c) for c in cards]) <= 2 ** 16
    ops = []
    for s, v in zip(scopes, model_dict["values"]):
        ops += [np.asarray(v, dtype=np.float64).reshape([cards[x] for x in s]), list(s)]
    joint = np.einsum(*ops, list(range(nv)))
    rows = np.asarray(rows).reshape(len(rows), len(ev_vars))
    w = np.ones(len(rows)) if w is None else np.asarray(w, dtype=np.float64)
    out = [np.zeros([cards[x] for x in s]) for s in scopes]
    z = np.zeros(len(rows))
    for b, row in enumerate(rows):
        cond = np.zeros_like(joint)
        ix = [slice(None)] * nv
        for v, x in zip(ev_vars, row):
            ix[v] = slice(int(x), int(x) + 1)
        cond[tuple(ix)] = joint[tuple(ix)]
        z[b] = cond.sum()
        if z[b] == 0 or w[b] == 0:
            continue
        post = cond / z[b]
        for f, s in enumerate(scopes):
            out[f] += w[b] * np.einsum(post, list(range(nv)), list(s))
    return out, z
