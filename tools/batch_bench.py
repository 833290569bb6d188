#!/usr/bin/env python3
"""Batched-evidence measurements (warm calls, the sides alternating in one
process; medians of --reps with min-max; host clock around calls that end in a
device synchronise and the copy of the results to the host):

  rows   bnpp.partition_batch at n_rows = 2^10, 2^14, 2^16 (--ns), automatic
         rows per launch, beside the only way to get the same numbers without
         it: a loop of warm bnpp.partition calls over 256 of the rows (each row
         is another evidence assignment, so each call plans), scaled per row.
         Also the floor of that loop: an identical call relaunching its cached
         job.  rows/s and the ratio per model and dtype.
  sweep  the same call at n_rows = max(R, --n-min = 2^16) for rows per launch R = 2^8 ..
         2^18 (--rs), where the plan fits the memory budget: rows/s per R.
  gather the gather kernel alone (bnpp.condition_batch) at R = 2^16 on the
         model's largest evidence-bearing factor, timed with device events:
         GB/s over its algorithmic bytes (evidence read + entries gathered +
         output written).

Rows are drawn from joint samples of the model (bnpp.sample), so every row is
possible.  One JSON line per record; the script ends at the first failure.

    python tools/batch_bench.py rows --models alarm ising12x12 >> profiles/batch_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(REPO, "bn-pp_amd", "python"))
import bnpp  # noqa: E402
from bnpp import synth  # noqa: E402

MODELS = os.path.join(REPO, "tests", "golden", "models")
# evidence variables; None: those of the model's .evid file
EV_VARS = {"alarm": [3, 10, 20], "ising12x12": [0, 50, 100, 143], "noisyor_50_80": None, "Munin1": [10, 50, 100]}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
LOOP_ROWS = 256


def load(name):
    path = os.path.join(MODELS, name + ".uai")
    m = bnpp.Model.load(path)
    ev = EV_VARS[name]
    if ev is None:
        ev = sorted(synth.read_evidence(os.path.join(MODELS, name + ".uai.evid")))
    return m, synth.read_uai(path), ev


def draw(ctx, m, ev_vars, n):
    """n possible rows: the evidence columns of 4096 joint samples, repeated."""
    s, _, _ = bnpp.sample(ctx, m, 4096, seed=3)
    rows = np.ascontiguousarray(s[:, ev_vars].astype(np.int64))
    return rows[np.arange(n) % len(rows)]


def med(ts):
    return statistics.median(ts), [min(ts), max(ts)]


def rows_mode(name, dname, ns, reps):
    m, _, ev_vars = load(name)
    dt = DT[dname]
    cb, cl, cf = bnpp.Context(0), bnpp.Context(0), bnpp.Context(0)   # one cached job each
    rows = draw(cl, m, ev_vars, max(ns))
    evs = [dict(zip(ev_vars, (int(x) for x in r))) for r in rows[:LOOP_ROWS]]
    st, _, _ = bnpp.plan_batch(m, ev_vars, dtype=dt)
    z = {n: bnpp.partition_batch(cb, m, ev_vars, rows[:n], dtype=dt)[1] for n in ns}      # warm-up
    z1 = np.array([bnpp.partition(cl, m, e, dtype=dt)[1] for e in evs])
    same = bool(np.array_equal(z[ns[0]][:LOOP_ROWS].view(np.int64), z1.view(np.int64)))
    bnpp.partition(cf, m, evs[0], dtype=dt)
    t = {"loop": [], "floor": [], **{n: [] for n in ns}}
    for _ in range(reps):                                    # alternating
        for n in ns:
            t0 = time.perf_counter()
            bnpp.partition_batch(cb, m, ev_vars, rows[:n], dtype=dt)
            t[n].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for e in evs:
            bnpp.partition(cl, m, e, dtype=dt)
        t["loop"].append((time.perf_counter() - t0) * 1e3 / LOOP_ROWS)
        t0 = time.perf_counter()
        for _i in range(LOOP_ROWS):
            bnpp.partition(cf, m, evs[0], dtype=dt)
        assert bnpp.last_timing()["plan_ms"] == 0
        t["floor"].append((time.perf_counter() - t0) * 1e3 / LOOP_ROWS)
    for c in (cb, cl, cf):
        c.close()
    loop, loop_mm = med(t["loop"])
    floor, floor_mm = med(t["floor"])
    rec = {"mode": "rows", "case": name + " " + dname, "n_evidence_vars": len(ev_vars), "reps": reps,
           "rows_per_launch_planned_at_64GB": st["rows_per_launch"], "batch_bits_equal_single": same,
           "single_loop_ms_per_row": loop, "single_loop_ms_per_row_min_max": loop_mm,
           "single_relaunch_floor_ms_per_row": floor, "single_relaunch_floor_ms_per_row_min_max": floor_mm}
    for n in ns:
        b, mm = med(t[n])
        rec["batch_ms_n%d" % n] = b
        rec["batch_ms_min_max_n%d" % n] = mm
        rec["batch_rows_per_s_n%d" % n] = n / (b * 1e-3)
        rec["speedup_vs_loop_n%d" % n] = loop / (b / n)
        rec["speedup_vs_relaunch_floor_n%d" % n] = floor / (b / n)
    print(json.dumps(rec), flush=True)


def sweep_mode(name, dname, rs, reps, n_min):
    m, _, ev_vars = load(name)
    dt = DT[dname]
    c0 = bnpp.Context(0)
    rows_all = draw(c0, m, ev_vars, max(max(rs), n_min))
    c0.close()
    for R in rs:
        n = max(R, n_min)
        ctx = bnpp.Context(0)
        try:
            bnpp.partition_batch(ctx, m, ev_vars, rows_all[:n], dtype=dt, rows_per_launch=R)     # warm-up
        except bnpp.BnppError as e:
            if e.status != bnpp.ERR_OOM:
                raise
            print(json.dumps({"mode": "sweep", "case": name + " " + dname, "rows_per_launch": R, "fits": False,
                              "error": str(e)}), flush=True)
            ctx.close()
            continue
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            bnpp.partition_batch(ctx, m, ev_vars, rows_all[:n], dtype=dt, rows_per_launch=R)
            ts.append((time.perf_counter() - t0) * 1e3)
        tm = bnpp.last_timing()
        ctx.close()
        b, mm = med(ts)
        print(json.dumps({"mode": "sweep", "case": name + " " + dname, "rows_per_launch": R, "fits": True, "n_rows": n,
                          "reps": reps, "ms": b, "ms_min_max": mm, "rows_per_s": n / (b * 1e-3),
                          "launch_ms": tm["launch_ms"], "run_fetch_ms": tm["run_fetch_ms"]}), flush=True)


def gather_mode(name, dname, reps):
    import torch
    m, d, ev_vars = load(name)
    dt = DT[dname]
    td = torch.float64 if dname == "f64" else torch.float32
    eb = 8 if dname == "f64" else 4
    best = max((f for f in range(len(d["scopes"])) if set(d["scopes"][f]) & set(ev_vars)), key=lambda f: len(d["values"][f]))
    scope, R = d["scopes"][best], 1 << 16
    ctx = bnpp.Context(0)
    rows = draw(ctx, m, ev_vars, R)
    ev = torch.tensor(np.ascontiguousarray(rows.T).reshape(-1), dtype=torch.int32, device="cuda")
    src = torch.tensor(np.asarray(d["values"][best]), dtype=td, device="cuda")
    in_scope = [v for v in ev_vars if v in scope]
    rest = len(d["values"][best])
    for v in in_scope:
        rest //= d["cards"][v]
    out = torch.empty(rest * R, dtype=td, device="cuda")
    ts_ = torch.cuda.Stream()                                # the events and the kernel share this stream
    torch.cuda.set_stream(ts_)
    s = ts_.cuda_stream
    for _ in range(3):
        bnpp.condition_batch(ctx, dt, d["cards"], src.data_ptr(), scope, ev_vars, R, ev.data_ptr(), out.data_ptr(), stream=s)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts_)
        bnpp.condition_batch(ctx, dt, d["cards"], src.data_ptr(), scope, ev_vars, R, ev.data_ptr(), out.data_ptr(), stream=s)
        b.record(ts_)
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ctx.close()
    nbytes = len(in_scope) * R * 4 + 2 * rest * R * eb
    t, mm = med(ts)
    print(json.dumps({"mode": "gather", "case": name + " " + dname, "factor": best, "scope": scope,
                      "evidence_in_scope": in_scope, "rest_entries": rest, "rows": R, "reps": reps, "kernel_ms": t,
                      "kernel_ms_min_max": mm, "algorithmic_bytes": nbytes, "GBps": nbytes / (t * 1e6)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["rows", "sweep", "gather"])
    ap.add_argument("--models", nargs="+", default=list(EV_VARS))
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    ap.add_argument("--ns", nargs="+", type=int, default=[1 << 10, 1 << 14, 1 << 16])
    ap.add_argument("--rs", nargs="+", type=int, default=[1 << k for k in range(8, 19)])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n-min", type=int, default=1 << 16, help="sweep: rows per call (at least R)")
    a = ap.parse_args()
    for name in a.models:
        for dname in a.dtypes:
            if a.mode == "rows":
                rows_mode(name, dname, a.ns, a.reps)
            elif a.mode == "sweep":
                sweep_mode(name, dname, a.rs, a.reps, a.n_min)
            else:
                gather_mode(name, dname, a.reps)


if __name__ == "__main__":
    main()
