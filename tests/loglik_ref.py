"""Numpy restatements of the two steps of the log form of soft evidence
(rowio.cuh; include/bnpp.h states them with bnpp_stage_loglikelihoods and
bnpp_emit_row_logs), and a brute-force ln Z with the posteriors of the soft
variables, which are its gradient with respect to the log-likelihoods.

stage_loglik is given twice: explicitly, and as device_io_ref.stage_lik of
E = exp(l - top), the contract of the log form.  The two agree bit for bit
(tests/test_loglik_host.py).
"""
import numpy as np

import device_io_ref as dref
import soft_ref
from device_io_ref import NONE, launch_rows

LN_2 = float.fromhex("0x1.62e42fefa39efp-1")
LOG10_2 = float.fromhex("0x1.34413509f79ffp-2")
LOG10_E = float.fromhex("0x1.bcb7b1526e50ep-2")


def clean(loglik, rows):
    """The launch's rows widened to fp64 with invalid entries (NaN, +inf) replaced by -inf, and the bad mask."""
    v = np.asarray(loglik)[rows].astype(np.float64)
    bad = np.isnan(v) | (v == np.inf)
    return np.where(bad, -np.inf, v), bad


def tops(loglik, cards, row0, R):
    """top (n_soft, R): every block's largest entry (invalid ones count as -inf)."""
    loglik = np.asarray(loglik)
    v, _ = clean(loglik, launch_rows(loglik.shape[0], row0, R))
    out, w = np.empty((len(cards), R)), 0
    for i, k in enumerate(cards):
        out[i] = v[:, w:w + k].max(axis=1)
        w += k
    return out


def linear(loglik, cards):
    """E (n_rows, Ws) fp64 = exp(l - top) of every row, a block of nothing but -inf all zero; invalid entries 0."""
    loglik = np.asarray(loglik)
    v, _ = clean(loglik, np.arange(loglik.shape[0]))
    E, w = np.zeros(v.shape), 0
    for k in cards:
        blk = v[:, w:w + k]
        top = blk.max(axis=1)
        ok = top > -np.inf
        with np.errstate(under="ignore", invalid="ignore"):
            E[ok, w:w + k] = np.exp(blk[ok] - top[ok, None])
        w += k
    return E


def stage_loglik(loglik, cards, row0, R, out_dtype):
    """loglik (n_rows, Ws) float64 or float32 -> (T (Ws, R) of out_dtype, e_row int64 (R,), top (n_soft, R),
    status word 1).  The explicit restatement."""
    loglik = np.asarray(loglik)
    n_rows, ws = loglik.shape
    assert ws == sum(cards)
    rows = launch_rows(n_rows, row0, R)
    v, bad = clean(loglik, rows)
    cells = rows[:, None] * ws + np.arange(ws)[None, :]
    status = int(cells[bad].min()) if bad.any() else NONE
    out = np.zeros((ws, R), dtype=out_dtype)
    e_row = np.zeros(R, dtype=np.int64)
    top = np.empty((len(cards), R))
    w = 0
    for i, k in enumerate(cards):
        blk = v[:, w:w + k]
        top[i] = blk.max(axis=1)
        ok = top[i] > -np.inf
        e_row += ok
        with np.errstate(under="ignore"):
            out[w:w + k, ok] = np.ldexp(np.exp(blk[ok] - top[i][ok, None]), -1).astype(out_dtype).T
        w += k
    return out, e_row, top, status


def stage_loglik_via_linear(loglik, cards, row0, R, out_dtype):
    """The same through the contract: device_io_ref.stage_lik of E (its status word is the log form's own)."""
    loglik = np.asarray(loglik)
    out, e_row, st = dref.stage_lik(linear(loglik, cards), cards, row0, R, out_dtype)
    assert st == NONE
    return out, e_row, tops(loglik, cards, row0, R), stage_loglik(loglik, cards, row0, R, out_dtype)[3]


def shift_of(top):
    """The row's shift: its tops summed from 0.0 in the variables' order, every sum rounded once."""
    s = np.zeros(top.shape[1]) if len(top) else 0.0
    for t in top:
        s = s + t
    return s


def emit_row_logs(ln_z, log10_z, z, table, has_b, exp2, e_row, top, row0, rows_live):
    """Writes ln_z, log10_z and z at row0 + b (each may be None) for b < rows_live; table None: the constant 1;
    top (n_soft, R) or None."""
    for b in range(rows_live):
        p = 0.0 + (1.0 if table is None else float(table[b if has_b else 0]))
        ex = int(exp2) + (0 if e_row is None else int(e_row[b]))
        shift = 0.0
        for i in range(0 if top is None else len(top)):
            shift = shift + float(top[i][b])
        pm, pe = np.frexp(p)
        pw = float(ex + int(pe))
        ln = (np.log(pm) + pw * LN_2) + shift if p > 0 else -np.inf
        if ln_z is not None:
            ln_z[row0 + b] = ln
        if log10_z is not None:
            log10_z[row0 + b] = (np.log10(pm) + pw * LOG10_2) + shift * LOG10_E if p > 0 else -np.inf
        if z is not None:
            with np.errstate(over="ignore", under="ignore"):
                z[row0 + b] = np.exp(ln)
    return ln_z, log10_z, z


def brute_log(model_dict, ev_vars, rows, soft_vars, loglik):
    """-> (ln_z (n,), post (n, Ws)): soft_ref.brute on E plus the rows' shifts; post holds the marginals of the
    soft variables in the columns of loglik (NaN in an impossible row)."""
    cards = [model_dict["cards"][v] for v in soft_vars]
    loglik = np.asarray(loglik, dtype=np.float64)
    n = loglik.shape[0]
    z, marg, _ = soft_ref.brute(model_dict, ev_vars, rows, soft_vars, linear(loglik, cards))
    shift = shift_of(tops(loglik, cards, 0, n)) if len(cards) else np.zeros(n)
    with np.errstate(divide="ignore"):
        ln_z = np.where(z > 0, np.log(np.where(z > 0, z, 1.0)) + shift, -np.inf)
    post = np.concatenate([marg[v] for v in soft_vars], axis=1) if len(soft_vars) else np.zeros((n, 0))
    return ln_z, post


# ---- the cases of the staging step, shared by the host and the GPU tests ----

# several blocks per tile and more variables than waves; a block that fills the tile, one that does not fit it, the
# chunked two-pass path; nine mixed cards
CARDS = {"two": [2], "mixed": [2, 3, 2, 4, 5], "sixteen": [16], "seventeen": [17], "wide": [40, 2],
         "nine": [3, 2, 5, 2, 7, 4, 2, 6, 3]}


def loglik_case(rng, n, cards, dtype=np.float64):
    """Log-likelihoods with every special entry the log form names: -inf entries, blocks of nothing but -inf,
    entries 708.5, 744 and 746 below their top (the fp64 subnormal range and underflow), about 95 below (float
    subnormals once halved), and tops of +800 and -800."""
    ws = sum(cards)
    a = rng.uniform(-30.0, 3.0, (n, ws))
    a[rng.random((n, ws)) < 0.15] = -np.inf
    w = 0
    for i, k in enumerate(cards):
        top = np.where(np.arange(n) % 3 == 0, 800.0, np.where(np.arange(n) % 3 == 1, -800.0, rng.uniform(-5, 5, n)))
        at = w + rng.integers(0, k, n)
        a[np.arange(n), at] = top                           # the block's top, at a random place
        if k > 1:
            below = np.array([-708.5, -744.0, -746.0, -95.0, -88.0, -103.5])[(np.arange(n) + i) % 6]
            other = w + (at - w + 1 + rng.integers(0, k - 1, n)) % k
            a[np.arange(n), other] = top + below
        dead = (np.arange(n) + 2 * i) % 7 == 5
        a[dead, w:w + k] = -np.inf                          # an all -inf block: an impossible row
        w += k
    return a.astype(dtype)
