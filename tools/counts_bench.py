#!/usr/bin/env python3
"""Expected-counts measurements (warm calls, the two sides alternating in one
process; medians of --reps with min-max; host clock around calls that end in a
device synchronise and the copy of the results to the host):

  rows   bnpp.expected_counts at n_rows = 2^10 and 2^16 (--ns), automatic rows
         per launch, beside bnpp.partition_batch over the same rows: the ratio
         is what DESIGN 5's "3-4.5 PR passes" of a bucket tree should be read
         against.  One JSON line per model, dtype and n.
  trace  one warm-up call and one more, nothing else on the device: run it under
             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o counts -- \
                 python tools/counts_bench.py trace --models alarm --dtypes f64 --ns 65536 --rows-file rows.npy
         (rows.npy written by `rows --save-rows`, so no sampling kernel is traced).
  share  reads DIR/**/*kernel_stats.csv of such a run: the share of the
         accumulate kernels (counts_rows_*, counts_fold_*) and of the
         gather kernel in the device time of all kernels.

Rows are drawn from joint samples of the model (bnpp.sample), so every row is
possible.  The script ends at the first failure.

    python tools/counts_bench.py rows --models alarm ising12x12 >> profiles/counts_bench.jsonl
    python tools/counts_bench.py rows --models noisyor_50_80 --ns 64 >> profiles/counts_bench.jsonl
"""
import argparse
import csv
import glob
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


def rows_mode(name, dname, ns, reps, save_rows):
    m, ev_vars = load(name)
    dt = DT[dname]
    cc, cb = bnpp.Context(0), bnpp.Context(0)                # one cached job each
    rows = draw(cb, m, ev_vars, max(ns))
    if save_rows:
        np.save(save_rows, rows)
    for n in ns:
        st, groups, _, _ = bnpp.plan_counts(m, ev_vars, dtype=dt)
        sb, _, _ = bnpp.plan_batch(m, ev_vars, dtype=dt)
        counts, lz, n_imp = bnpp.expected_counts(cc, m, ev_vars, rows[:n], dtype=dt)          # warm-up
        lzb, _, _ = bnpp.partition_batch(cb, m, ev_vars, rows[:n], dtype=dt)
        tc, tb = [], []
        for _ in range(reps):                                # alternating
            t0 = time.perf_counter()
            bnpp.expected_counts(cc, m, ev_vars, rows[:n], dtype=dt)
            tc.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            bnpp.partition_batch(cb, m, ev_vars, rows[:n], dtype=dt)
            tb.append((time.perf_counter() - t0) * 1e3)
        c, cmm = med(tc)
        b, bmm = med(tb)
        print(json.dumps({"mode": "rows", "case": name + " " + dname, "n_rows": n, "n_evidence_vars": len(ev_vars),
                          "reps": reps, "n_impossible": n_imp, "counts_total": float(counts.sum()),
                          "log10_z_bits_equal_partition_batch": bool(np.array_equal(lz.view(np.int64), lzb.view(np.int64))),
                          "rows_per_launch_planned_at_64GB": st["rows_per_launch"],
                          "batch_rows_per_launch_planned_at_64GB": sb["rows_per_launch"],
                          "count_steps": st["count_steps"], "launch_groups": len(groups),
                          "plan_bytes_moved": st["bytes_moved"], "batch_plan_bytes_moved": sb["bytes_moved"],
                          "expected_counts_ms": c, "expected_counts_ms_min_max": cmm,
                          "partition_batch_ms": b, "partition_batch_ms_min_max": bmm,
                          "ratio_to_partition_batch": c / b, "rows_per_s": n / (c * 1e-3)}), flush=True)
    cc.close()
    cb.close()


def trace_mode(name, dname, n, rows_file):
    m, ev_vars = load(name)
    rows = np.load(rows_file)[:n]
    ctx = bnpp.Context(0)
    for _ in range(2):
        bnpp.expected_counts(ctx, m, ev_vars, rows, dtype=DT[dname])
    ctx.close()


def share_mode(case, directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under " + directory)
    total = acc = gather = 0.0
    calls = 0
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                ns = float(row["TotalDurationNs"])
                total += ns
                if "counts_rows" in row["Name"] or "counts_fold" in row["Name"]:
                    acc += ns
                    calls += int(row["Calls"])
                if "cond_batch_kernel" in row["Name"]:
                    gather += ns
    print(json.dumps({"mode": "share", "case": case, "kernel_ns_total": total, "accumulate_kernel_ns": acc,
                      "accumulate_kernel_calls": calls, "accumulate_share_of_kernel_time": acc / total if total else None,
                      "gather_share_of_kernel_time": gather / total if total else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["rows", "trace", "share"])
    ap.add_argument("--models", nargs="+", default=["alarm", "ising12x12"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    ap.add_argument("--ns", nargs="+", type=int, default=[1 << 10, 1 << 16])
    ap.add_argument("--reps", type=int, default=9)
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
                rows_mode(name, dname, a.ns, a.reps, a.save_rows)
            else:
                trace_mode(name, dname, a.ns[0], a.rows_file)


if __name__ == "__main__":
    main()
