"""Numpy restatement of the batched-marginals emit step
(bnpp_bucket_marginal_rows) and a brute-force reference for whole runs.

emit_rows: the contract of include/bnpp.h in the same order of operations --
a sequential column sum from 0.0, ascending, then one division per entry, all
in fp64 on values converted from the table -- so the engine's array must equal
this one bit for bit, in fp64 and fp32.

brute_marginals: the full joint by einsum in fp64 (models of at most 2^16
joint states), conditioned per row and marginalised to every target.
"""
import numpy as np


def emit_rows(out, cards, tables, has_b, ev_row, n_rows, rows_live, ev):
    """Writes rows [0, rows_live) of out, an (R, W) float64 array, and returns it.

    tables[j]: target j's table over (x, b), b fastest, flat (has_b[j] False:
    no b dimension), or None: an evidence block (ev_row[j] >= 0, the row of ev,
    an (n_ev, R) integer array) or a free block.
    """
    R = int(n_rows)
    at = 0
    for j, k in enumerate(cards):
        blk = np.zeros((R, k))
        if tables[j] is not None:
            t = np.asarray(tables[j]).reshape(k, R if has_b[j] else 1).astype(np.float64)
            if not has_b[j]:
                t = np.broadcast_to(t, (k, R))
            c = np.zeros(R)
            for x in range(k):                              # ascending, sequentially from 0.0
                c = c + t[x]
            with np.errstate(all="ignore"):
                blk = (t / c).T                             # 0 / 0 = NaN, nothing special-cased
        elif ev_row[j] >= 0:
            val = np.clip(np.asarray(ev).reshape(-1, R)[ev_row[j]], 0, k - 1)
            blk[np.arange(R), val] = 1.0
        else:
            blk[:] = 1.0 / k
        out[:rows_live, at:at + k] = blk[:rows_live]
        at += k
    return out


def brute_marginals(model_dict, ev_vars, rows, targets=None):
    """(n, W) float64: per row the posterior marginal of every target, blocks in
    the targets' order (None: all variables); an evidence variable reads
    one-hot, an impossible row NaN in its other blocks.  Also returns Z per row."""
    cards, scopes = model_dict["cards"], model_dict["scopes"]
    nv = len(cards)
    assert np.prod([float(c) for c in cards]) <= 2 ** 16
    targets = list(range(nv)) if targets is None else list(targets)
    ops = []
    for s, v in zip(scopes, model_dict["values"]):
        ops += [np.asarray(v, dtype=np.float64).reshape([cards[x] for x in s]), list(s)]
    for v in range(nv):                                     # a variable in no factor: uniform, and Z leaves it out
        if not any(v in s for s in scopes):
            ops += [np.full(cards[v], 1.0 / cards[v]), [v]]
    joint = np.einsum(*ops, list(range(nv)))
    rows = np.asarray(rows).reshape(len(rows), len(ev_vars))
    out = np.zeros((len(rows), sum(cards[t] for t in targets)))
    z = np.zeros(len(rows))
    for b, row in enumerate(rows):
        cond = np.zeros_like(joint)
        ix = [slice(None)] * nv
        for v, x in zip(ev_vars, row):
            ix[v] = slice(int(x), int(x) + 1)
        cond[tuple(ix)] = joint[tuple(ix)]
        z[b] = cond.sum()
        at = 0
        for t in targets:
            if t in ev_vars:
                out[b, at + int(row[list(ev_vars).index(t)])] = 1.0
            else:
                with np.errstate(all="ignore"):
                    out[b, at:at + cards[t]] = np.einsum(cond, list(range(nv)), [t]) / z[b]
            at += cards[t]
    return out, z
