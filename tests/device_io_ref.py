"""Numpy restatements of the four device-resident row steps (rowio.cuh;
include/bnpp.h states them with bnpp_stage_evidence_rows, bnpp_stage_likelihoods,
bnpp_emit_row_scalars and bnpp_emit_row_states).

A launch of R rows starts at row row0 of the call's n_rows; its entry b is row
min(row0 + b, n_rows - 1); rows_live of its entries are the call's.
"""
import numpy as np

NONE = np.iinfo(np.int64).max            # a status word no invalid cell touched
LOG10_2 = float.fromhex("0x1.34413509f79ffp-2")


def launch_rows(n_rows, row0, R):
    """The call's row of every entry of the launch (the padding rule)."""
    return np.minimum(row0 + np.arange(R), n_rows - 1)


def stage_rows(ev, cards, partial, row0, R):
    """ev int32 (n_rows, n_ev) -> (the evidence table int32 (n_ev, R), status word 0)."""
    ev = np.asarray(ev, dtype=np.int32)
    n_rows, n_ev = ev.shape
    rows = launch_rows(n_rows, row0, R)
    x = ev[rows]                                                         # (R, n_ev)
    cards = np.asarray(cards, dtype=np.int64).reshape(1, n_ev)
    part = np.zeros((1, n_ev), dtype=bool) if partial is None else np.asarray(partial, dtype=bool).reshape(1, n_ev)
    ok = ((x >= 0) & (x < cards)) | ((x == -1) & part)
    cells = rows[:, None] * n_ev + np.arange(n_ev)[None, :]
    status = int(cells[~ok].min()) if (~ok).any() else NONE
    return np.ascontiguousarray(np.where(ok, x, 0).T.astype(np.int32)), status


def stage_lik(lik, cards, row0, R, out_dtype):
    """lik (n_rows, Ws) float64 or float32 -> (T (Ws, R) of out_dtype, e_row int64 (R,), status word 1)."""
    lik = np.asarray(lik)
    n_rows, ws = lik.shape
    assert ws == sum(cards)
    rows = launch_rows(n_rows, row0, R)
    v = lik[rows].astype(np.float64)                                    # fp32 widens exactly
    bad = ~(v >= 0) | np.isinf(v)
    cells = rows[:, None] * ws + np.arange(ws)[None, :]
    status = int(cells[bad].min()) if bad.any() else NONE
    v = np.where(bad, 0.0, v)
    out = np.empty((ws, R), dtype=out_dtype)
    e_row = np.zeros(R, dtype=np.int64)
    w = 0
    for k in cards:
        blk = v[:, w:w + k]
        top = blk.max(axis=1)
        _, e = np.frexp(top)                                            # frexp(0) = (0, 0)
        e = np.where(top > 0, e, 0).astype(np.int64)
        e_row += e
        with np.errstate(under="ignore"):
            out[w:w + k] = np.ldexp(blk, -e[:, None].astype(np.int32)).astype(out_dtype).T
        w += k
    return out, e_row, status


def emit_row_scalars(log10_z, z, table, has_b, exp2, e_row, row0, rows_live):
    """Writes log10_z[row0 + b] and z[row0 + b] (z may be None) for b < rows_live; table None: the constant 1."""
    for b in range(rows_live):
        p = 0.0 + (1.0 if table is None else float(table[b if has_b else 0]))
        ex = int(exp2) + (0 if e_row is None else int(e_row[b]))
        pm, pe = np.frexp(p)
        log10_z[row0 + b] = np.log10(pm) + float(ex + int(pe)) * LOG10_2 if p > 0 else -np.inf
        if z is not None:
            with np.errstate(over="ignore", under="ignore"):
                z[row0 + b] = np.ldexp(p, max(min(ex, 1 << 20), -(1 << 20)))
    return log10_z, z


def emit_row_states(out, n_degenerate, x, ev, ev_col, written, K, R, row0, rows_live, sampling, table=None, has_b=False,
                    deg=None, n_drawn=0):
    """x uint8 (n_vars, K, R), ev int32 (n_ev, R).  Writes out[row0 + b] ((n_vars,) int32, or (K, n_vars) uint8 when
    sampling) and, sampling, n_degenerate[row0 + b] for b < rows_live."""
    n_vars = len(ev_col)
    x = np.asarray(x).reshape(n_vars, K, R)
    for b in range(rows_live):
        impossible = False
        if sampling:
            p = 1.0 if table is None else float(table[b if has_b else 0])
            impossible = not (p > 0)
            if n_degenerate is not None:
                n_degenerate[row0 + b] = K * n_drawn if impossible else int(deg[b])
        for v in range(n_vars):
            val = int(ev[ev_col[v], b]) if ev_col[v] >= 0 else -1
            for s in range(K):
                cell = val if val >= 0 else int(x[v, s, b]) if written[v] and not impossible else 0
                if out is None:
                    continue
                if sampling:
                    out[row0 + b, s, v] = cell & 0xFF
                else:
                    out[row0 + b, v] = cell
    return out, n_degenerate
