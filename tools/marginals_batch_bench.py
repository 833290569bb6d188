#!/usr/bin/env python3
"""Batched-marginals measurements (warm calls, the sides alternating in one
process; medians of --reps with min-max; host clock around calls that end in a
device synchronise and the copy of the results to the host):

  rows   bnpp.marginals_batch (all variables) at n_rows = 2^10 and 2^16 (--ns),
         automatic rows per launch, beside (a) the loop of bnpp.posterior_batch
         over the targets -- what a caller does without it: one context, so
         one plan and one forward elimination per target; timed on the first
         --loop-targets non-evidence variables and scaled to all of them, which
         the line says --, (b) bnpp.expected_counts and (c) bnpp.partition_batch
         over the same rows; marginals_batch also into a result array that is
         reused (out=), which leaves out the page faults of a fresh one.  One
         JSON line per model, dtype and n.
  split  the engine's own clocks of one warm call (BNPP_TIMING: staging, enqueue,
         wait, copy), read from its stderr line.
  host   one context, nothing alternating: the Python call with a fresh result
         array, and the library call (its own clock and the wall clock) into a
         reused and into a fresh array, beside the cost of allocating and freeing
         the array -- where the host time of a 2^16-row call goes.
  trace  one warm-up call and one more, nothing else on the device: run it under
             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o marg -- \
                 python tools/marginals_batch_bench.py trace --models alarm --dtypes f64 --ns 65536 --rows-file rows.npy
         (rows.npy written by `rows --save-rows`, so no sampling kernel is traced).
  share  reads DIR/**/*kernel_stats.csv of such a run: the emit kernel's
         (marg_rows_kernel) time and share of the device time of all kernels.

Rows are drawn from joint samples of the model (bnpp.sample), so every row is
possible.  The script ends at the first failure.

    python tools/marginals_batch_bench.py rows --models alarm ising12x12 >> profiles/marginals_batch_bench.jsonl
    python tools/marginals_batch_bench.py rows --models noisyor_50_80 --ns 64 >> profiles/marginals_batch_bench.jsonl
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(REPO, "bn-pp_amd", "python"))
import bnpp  # noqa: E402
from bnpp import synth  # noqa: E402

MODELS = os.path.join(REPO, "tests", "golden", "models")
# evidence variables; None: those of the model's .evid file (tools/batch_bench.py's)
EV_VARS = {"alarm": [3, 10, 20], "ising12x12": [0, 50, 100, 143], "noisyor_50_80": None}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}


def load(name):
    path = os.path.join(MODELS, name + ".uai")
    ev = EV_VARS[name]
    if ev is None:
        ev = sorted(synth.read_evidence(os.path.join(MODELS, name + ".uai.evid")))
    return bnpp.Model.load(path), ev


def draw(ctx, m, ev_vars, n):
    """n possible rows: the evidence columns of 4096 joint samples, repeated."""
    s, _, _ = bnpp.sample(ctx, m, 4096, seed=3)
    rows = np.ascontiguousarray(s[:, ev_vars].astype(np.int64))
    return rows[np.arange(n) % len(rows)]


def med(ts):
    return statistics.median(ts), [min(ts), max(ts)]


def clock(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def rows_mode(name, dname, ns, reps, loop_targets, save_rows):
    m, ev_vars = load(name)
    dt = DT[dname]
    cm, cc, cb = bnpp.Context(0), bnpp.Context(0), bnpp.Context(0)          # one cached job each
    loop = [t for t in range(m.n_vars) if t not in ev_vars]
    timed = loop[:loop_targets] if loop_targets > 0 else loop
    cp = bnpp.Context(0)                                                    # the loop's: it plans afresh per target, as a caller's does
    rows = draw(cb, m, ev_vars, max(ns))
    if save_rows:
        np.save(save_rows, rows)
    for n in ns:
        r = rows[:n]
        st, groups, kinds = bnpp.plan_marginals_batch(m, ev_vars, dtype=dt)
        sb, _, _ = bnpp.plan_batch(m, ev_vars, dtype=dt)
        out, lz = bnpp.marginals_batch(cm, m, ev_vars, r, dtype=dt)         # warm-up, all sides
        bnpp.expected_counts(cc, m, ev_vars, r, dtype=dt)
        lzb, _, _ = bnpp.partition_batch(cb, m, ev_vars, r, dtype=dt)
        worst = 0.0
        per = bnpp.split_marginals(m.cards, None, out)
        for t in timed:
            post, _ = bnpp.posterior_batch(cp, m, ev_vars, r, t, dtype=dt)
            worst = max(worst, float(np.abs(per[t] - post).max()))
        tm, tr, tc, tb, tp = [], [], [], [], []
        for _ in range(reps):                                               # alternating: the three cached jobs
            tm.append(clock(lambda: bnpp.marginals_batch(cm, m, ev_vars, r, dtype=dt)))
            tr.append(clock(lambda: bnpp.marginals_batch(cm, m, ev_vars, r, dtype=dt, out=out)))
            tc.append(clock(lambda: bnpp.expected_counts(cc, m, ev_vars, r, dtype=dt)))
            tb.append(clock(lambda: bnpp.partition_batch(cb, m, ev_vars, r, dtype=dt)))
        for _ in range(reps):                # the loop plans per target and frees the job before: kept apart from the others
            tp.append(clock(lambda: [bnpp.posterior_batch(cp, m, ev_vars, r, t, dtype=dt) for t in timed]))
        a, amm = med(tm)
        ar, armm = med(tr)
        c, cmm = med(tc)
        b, bmm = med(tb)
        p, pmm = med(tp)
        print(json.dumps({"mode": "rows", "case": name + " " + dname, "n_rows": n, "n_evidence_vars": len(ev_vars),
                          "reps": reps, "width": st["width"], "out_bytes_call": n * st["width"] * 8,
                          "belief_cols_b": st["belief_cols_b"], "belief_cols": st["belief_cols"],
                          "log10_z_bits_equal_partition_batch": bool(np.array_equal(lz.view(np.int64), lzb.view(np.int64))),
                          "worst_abs_diff_to_posterior_batch": worst,
                          "rows_per_launch_planned_at_64GB": st["rows_per_launch"],
                          "batch_rows_per_launch_planned_at_64GB": sb["rows_per_launch"], "launch_groups": len(groups),
                          "plan_bytes_moved": st["bytes_moved"], "batch_plan_bytes_moved": sb["bytes_moved"],
                          "marginals_batch_ms": a, "marginals_batch_ms_min_max": amm,
                          "marginals_batch_reused_out_ms": ar, "marginals_batch_reused_out_ms_min_max": armm,
                          "expected_counts_ms": c, "expected_counts_ms_min_max": cmm,
                          "partition_batch_ms": b, "partition_batch_ms_min_max": bmm,
                          "posterior_loop_targets_timed": len(timed), "posterior_loop_targets_all": len(loop),
                          "posterior_loop_timed_ms": p, "posterior_loop_timed_ms_min_max": pmm,
                          "posterior_loop_all_ms_scaled": p * len(loop) / max(len(timed), 1),
                          "ratio_to_partition_batch": a / b, "ratio_to_expected_counts": a / c,
                          "rows_per_s": n / (a * 1e-3)}), flush=True)
    for c in (cm, cc, cb, cp):
        c.close()


def split_mode(name, dname, n):
    """The engine's clocks of one warm call, from the line it prints under BNPP_TIMING
    (call_ms is that call's wall clock with the timing mode on, not a clean call's)."""
    m, ev_vars = load(name)
    ctx = bnpp.Context(0)
    rows = draw(ctx, m, ev_vars, n)
    bnpp.marginals_batch(ctx, m, ev_vars, rows, dtype=DT[dname])
    os.environ["BNPP_TIMING"] = "1"
    with tempfile.TemporaryFile() as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            total = clock(lambda: bnpp.marginals_batch(ctx, m, ev_vars, rows, dtype=DT[dname]))
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    del os.environ["BNPP_TIMING"]
    ctx.close()
    line = [ln for ln in text.split("\n") if "marginals_batch:" in ln][-1]
    parts = {k: float(v) for k, v in re.findall(r"(stage|enqueue|wait|copy) ([0-9.]+) ms", line)}
    print(json.dumps({"mode": "split", "case": name + " " + dname, "n_rows": n, "call_ms": total,
                      **{k + "_ms": v for k, v in parts.items()}}), flush=True)


def host_mode(name, dname, n, reps):
    import ctypes as C
    m, ev = load(name)
    dt = DT[dname]
    ctx = bnpp.Context(0)
    rows = draw(ctx, m, ev, n)
    W = sum(m.cards)
    for _ in range(2):
        bnpp.marginals_batch(ctx, m, ev, rows, dtype=dt)
    wall = [clock(lambda: bnpp.marginals_batch(ctx, m, ev, rows, dtype=dt)) for _ in range(reps)]
    ne, ev_v, n, keep, ev_x = bnpp._ev_rows(ev, rows)
    out, lz = np.zeros((n, W)), np.zeros(n)
    up = C.c_double()
    DP = C.POINTER(C.c_double)

    def raw(o):
        rc = bnpp._lib.bnpp_marginals_batch(ctx.handle, m.handle, ne, ev_v, n, ev_x, bnpp.MIN_FILL, None, 0, 0, None, dt, 0,
                                            o.ctypes.data_as(DP), lz.ctypes.data_as(DP), C.byref(up))
        if rc:
            raise SystemExit("bnpp_marginals_batch failed")
    reuse_wall, reuse_lib, fresh_wall, fresh_lib, alloc = [], [], [], [], []
    for _ in range(reps):
        reuse_wall.append(clock(lambda: raw(out)))
        reuse_lib.append(up.value)
    for _ in range(reps):
        t0 = time.perf_counter()
        o = np.zeros((n, W))
        alloc.append((time.perf_counter() - t0) * 1e3)
        fresh_wall.append(clock(lambda: raw(o)))
        fresh_lib.append(up.value)
        t0 = time.perf_counter()
        del o
        alloc[-1] += (time.perf_counter() - t0) * 1e3
    print(json.dumps({"mode": "host", "case": name + " " + dname, "n_rows": n, "reps": reps, "out_bytes_call": n * W * 8,
                      "python_call_fresh_array_ms": med(wall)[0], "library_call_reused_array_wall_ms": med(reuse_wall)[0],
                      "library_call_reused_array_own_clock_ms": med(reuse_lib)[0],
                      "library_call_fresh_array_wall_ms": med(fresh_wall)[0],
                      "library_call_fresh_array_own_clock_ms": med(fresh_lib)[0],
                      "alloc_and_free_ms": med(alloc)[0]}), flush=True)
    ctx.close()


def trace_mode(name, dname, n, rows_file):
    m, ev_vars = load(name)
    rows = np.load(rows_file)[:n]
    ctx = bnpp.Context(0)
    for _ in range(2):
        bnpp.marginals_batch(ctx, m, ev_vars, rows, dtype=DT[dname])
    ctx.close()


def share_mode(case, directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under " + directory)
    total = emit = gather = 0.0
    calls = 0
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                ns = float(row["TotalDurationNs"])
                total += ns
                if "marg_rows" in row["Name"]:
                    emit += ns
                    calls += int(row["Calls"])
                if "cond_batch_kernel" in row["Name"]:
                    gather += ns
    print(json.dumps({"mode": "share", "case": case, "kernel_ns_total": total, "emit_kernel_ns": emit,
                      "emit_kernel_calls": calls, "emit_ns_per_call": emit / calls if calls else None,
                      "emit_share_of_kernel_time": emit / total if total else None,
                      "gather_share_of_kernel_time": gather / total if total else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["rows", "split", "host", "trace", "share"])
    ap.add_argument("--models", nargs="+", default=["alarm", "ising12x12"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    ap.add_argument("--ns", nargs="+", type=int, default=[1 << 10, 1 << 16])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-targets", type=int, default=8, help="rows: targets the posterior_batch loop is timed on (0: all)")
    ap.add_argument("--save-rows", default=None, help="rows: also write the drawn rows (npy) for a trace run")
    ap.add_argument("--rows-file", default=None, help="trace: rows written by --save-rows")
    ap.add_argument("--dir", default=None, help="share: the profiler's output directory")
    a = ap.parse_args()
    if a.mode == "share":
        share_mode(" ".join(a.models + a.dtypes + [str(n) for n in a.ns]), a.dir)
        return
    for name in a.models:
        for dname in a.dtypes:
            if a.mode == "rows":
                rows_mode(name, dname, a.ns, a.reps, a.loop_targets, a.save_rows)
            elif a.mode == "split":
                split_mode(name, dname, a.ns[-1])
            elif a.mode == "host":
                host_mode(name, dname, a.ns[-1], a.reps)
            else:
                trace_mode(name, dname, a.ns[0], a.rows_file)


if __name__ == "__main__":
    main()
