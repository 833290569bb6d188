"""Numpy restatements of the steps of the device-resident model tables
(tables.cuh; include/bnpp.h states them with bnpp_stage_tables and
bnpp_mstep_dv), and a brute force for counts under log-form tables.

stage_tables: the linear form is what the engine makes of a model's values
when it uploads them (runtime.cpp upload_sources; tests/test_tables_host.py
restates that loop entry by entry and compares); the log form is the log form
of a likelihood block (loglik_ref.stage_loglik) with a factor for a block.
mstep: learn.m_step with the sum over the child taken in ascending order.
"""
import numpy as np

import counts_ref
from device_io_ref import NONE

# the factors of the staging tests: one entry; either side of a wave; 3 x 5 x 7; more than a workgroup's lanes
# sixteen times over, and odd; the last one is all zeros (linear) or all -inf (log).  Seven factors against a grid
# of at most three workgroups
SIZES = [1, 63, 64, 65, 105, 4097, 33]


# ---- the values of the staging tests, shared by the host and the GPU tests ----

def linear_case(rng, in_dtype):
    """Values of the staging tests' factors: a maximum that is subnormal, one near the top of the input's range, an
    all-zero factor, zeros among the entries."""
    tiny, huge = (5e-322, 1e300) if in_dtype == np.float64 else (1e-43, 3e38)
    parts = []
    for i, s in enumerate(SIZES):
        v = rng.uniform(0.0, 1.0, s) * 10.0 ** rng.integers(-12, 12)
        v[rng.random(s) < 0.1] = 0.0
        if i == 1:
            v = rng.integers(0, 9, s) * tiny                # every entry subnormal
            v[5] = 9 * tiny
        if i == 3:
            v[7] = huge
        if i == len(SIZES) - 1:
            v[:] = 0.0
        parts.append(v)
    with np.errstate(under="ignore"):
        return np.concatenate(parts).astype(in_dtype)


def log_case(rng, in_dtype):
    """Natural logs: -inf entries, entries far below their top (subnormal and zero once scaled), tops of +-700 (+-80
    for a float input), a factor of nothing but -inf."""
    big = 700.0 if in_dtype == np.float64 else 80.0
    parts = []
    for i, s in enumerate(SIZES):
        v = rng.uniform(-30.0, 3.0, s)
        v[rng.random(s) < 0.15] = -np.inf
        v[rng.integers(0, s)] = [0.5, big, -big, 2.0, -3.0, 1.25, 0.0][i]
        if s > 2:
            top = v.max()
            at = [j for j in range(s) if v[j] != top][:3]
            for j, below in zip(at, (-708.5, -744.0, -103.5)):
                v[j] = top + below
        if i == len(SIZES) - 1:
            v[:] = -np.inf
        parts.append(v)
    return np.concatenate(parts).astype(in_dtype)


def layout(sizes, out_dtype):
    """Byte offset of every factor in the buffer (each on a 256-byte line), and the buffer's bytes."""
    eb = np.dtype(out_dtype).itemsize
    off, at = [], 0
    for s in sizes:
        off.append(at)
        at += (s * eb + 255) // 256 * 256
    return off, max(at, 256)


def _bits(x, out_dtype):
    a = np.asarray([x], dtype=out_dtype)
    return int(a.view(np.uint32 if np.dtype(out_dtype).itemsize == 4 else np.uint64)[0])


def stage_tables(values, sizes, out_dtype, log=False):
    """values: flat float64 or float32 -> (tables: one out_dtype array per factor, maxbits, exp2, tops, shift,
    status: the flat index of the first invalid entry or NONE)."""
    values = np.asarray(values)
    assert values.ndim == 1 and values.shape[0] == sum(sizes)
    tables, maxbits, exp2, tops = [], [], [], []
    status, shift, at = NONE, 0.0, 0
    for s in sizes:
        v = values[at:at + s].astype(np.float64)            # a float is widened exactly
        if log:
            bad = np.isnan(v) | (v == np.inf)
            v = np.where(bad, -np.inf, v)
        else:
            bad = ~(v >= 0) | (v == np.inf)
            v = np.where(bad, 0.0, v)
        if bad.any():
            status = min(status, at + int(np.flatnonzero(bad)[0]))
        top = float(v.max())
        if log:
            if top == -np.inf:
                t, e = np.zeros(s, dtype=out_dtype), 0
            else:
                with np.errstate(under="ignore"):
                    t, e = np.ldexp(np.exp(v - top), -1).astype(out_dtype), 1
                shift = shift + top
        else:
            e = int(np.frexp(top)[1]) if top > 0 else 0
            with np.errstate(under="ignore"):
                t = np.ldexp(v, -e).astype(out_dtype)
        tables.append(t)
        maxbits.append(_bits(t.max(), out_dtype))
        exp2.append(e)
        tops.append(top)
        at += s
    return tables, maxbits, exp2, tops, (shift if log else 0.0), status


def child_cards(model_dict):
    return [model_dict["cards"][s[-1]] if len(s) else 1 for s in model_dict["scopes"]]


def mstep(counts, old, sizes, ks, prior):
    """counts, old: flat float64 -> new, flat.  Per parent configuration (k contiguous entries):
    num_i = counts_i + prior, tot = ((0.0 + num_0) + num_1) + ..., new_i = tot > 0 ? num_i / tot : old_i."""
    counts, old = np.asarray(counts, dtype=np.float64), np.asarray(old, dtype=np.float64)
    new, at = np.empty_like(old), 0
    for s, k in zip(sizes, ks):
        num = counts[at:at + s].reshape(-1, k) + float(prior)
        tot = np.zeros(num.shape[0])
        for i in range(k):
            tot = tot + num[:, i]
        ok = tot > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            new[at:at + s] = np.where(ok[:, None], num / np.where(ok, tot, 1.0)[:, None], old[at:at + s].reshape(-1, k)).reshape(-1)
        at += s
    return new


def with_values(model_dict, flat):
    """model_dict with the flat values split over its factors."""
    flat = np.asarray(flat, dtype=np.float64).reshape(-1)
    out, at = dict(model_dict), 0
    out["values"] = []
    for s in model_dict["scopes"]:
        size = int(np.prod([model_dict["cards"][v] for v in s], dtype=np.int64)) if len(s) else 1
        out["values"].append(flat[at:at + size].tolist())
        at += size
    assert at == flat.shape[0]
    return out


def flat_values(model_dict):
    return np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in model_dict["values"]])


def brute_counts_flat(model_dict, flat, ev_vars, rows, w=None):
    """counts_ref.brute_counts under the flat values -> (flat counts, z per row)."""
    per, z = counts_ref.brute_counts(with_values(model_dict, flat), ev_vars, rows, w)
    return np.concatenate([p.reshape(-1) for p in per]), z


def child_last(model_dict):
    """A golden BAYES model lists a CPT's child first; the M step wants it last (the UAI convention): every table
    transposed."""
    d = model_dict
    return dict(d, scopes=[list(s[1:]) + [s[0]] for s in d["scopes"]],
                values=[np.moveaxis(np.asarray(v).reshape([d["cards"][x] for x in s]), 0, -1).reshape(-1).tolist()
                        for s, v in zip(d["scopes"], d["values"])])
