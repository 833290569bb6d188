#!/usr/bin/env python3
"""Batched-sampling measurements (warm calls, the sides alternating in one
process; medians of --reps with min-max; host clock around calls that end in a
device synchronise and the copy of the results to the host):

  rows    per model, dtype and K (--ks), at n_rows = 2^10 and 2^16 (--ns):
          (a) bnpp.sample_batch, automatic rows per launch, row_stride = K: ms
              per call, rows/s, samples/s;
          (b) the same rows through a loop of warm bnpp.sample(n=K) calls over
              256 of them (each row is another evidence assignment, so each
              call plans), scaled per row;
          (c) bnpp.partition_batch over the same rows: the forward pass of the
              same plan shape, without the resident messages or the draws.
          The batched call's time per row at the smallest n with K = 1 is
          compared with the loop's of the same run
          (batch_faster_than_loop_n1024_k1); the tool exits non-zero when it is
          not below it on alarm or ising12x12.
          host_split_ms_n*: the engine's own clocks for one more call (staging
          of the evidence rows, enqueue, wait for the device, copy of the
          results buffer, transposition), read from its BNPP_TIMING line.
  draw    warm bnpp.sample_batch calls only (the largest row count of --ns, one
          K), to be run under `rocprofv3 --kernel-trace --stats` for (d), the
          draw kernel's own time.
  stats   reads the kernel-stats CSV such a run wrote (--csv) and prints
          sample_rows_batch_kernel's calls, average time and share of all
          kernel time as one record.

Rows are drawn from joint samples of the model (bnpp.sample), so every row is
possible.  One JSON line per record; the script ends at the first failure.

    python tools/sample_batch_bench.py rows >> profiles/sample_batch_bench.jsonl
"""
import argparse
import csv
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
# evidence variables (tools/batch_bench.py's); None: those of the model's .evid file
EV_VARS = {"alarm": [3, 10, 20], "ising12x12": [0, 50, 100, 143], "noisyor_50_80": None}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
LOOP_ROWS = 256
DRAW_KERNEL = "sample_rows_batch_kernel"
SEED = 5


def load(name):
    path = os.path.join(MODELS, name + ".uai")
    m = bnpp.Model.load(path)
    ev = EV_VARS[name]
    if ev is None:
        ev = sorted(synth.read_evidence(os.path.join(MODELS, name + ".uai.evid")))
    return m, ev


def draw(ctx, m, ev_vars, n):
    """n possible rows: the evidence columns of 4096 joint samples, repeated."""
    s, _, _ = bnpp.sample(ctx, m, 4096, seed=3)
    rows = np.ascontiguousarray(s[:, ev_vars].astype(np.int64))
    return rows[np.arange(n) % len(rows)]


def med(ts):
    return statistics.median(ts), [min(ts), max(ts)]


def host_split(call):
    """The engine's BNPP_TIMING line of one call -> {phase: ms} (stderr goes through a file for its duration)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.environ["BNPP_TIMING"] = "1"
        os.dup2(f.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["BNPP_TIMING"]
        f.seek(0)
        text = f.read().decode(errors="replace")
    lines = [ln for ln in text.split("\n") if "sample_batch:" in ln]
    if not lines:
        raise SystemExit("no sample_batch timing line")
    return {k: float(v) for k, v in re.findall(r"(\w+) ([0-9.]+) ms", lines[-1])}


def rows_mode(name, dname, ns, ks, reps):
    m, ev_vars = load(name)
    dt = DT[dname]
    ok = True
    for k in ks:
        cb, cl, cp = bnpp.Context(0), bnpp.Context(0), bnpp.Context(0)   # one cached job each
        rows = draw(cl, m, ev_vars, max(ns))
        evs = [dict(zip(ev_vars, (int(x) for x in r))) for r in rows[:LOOP_ROWS]]
        st, _ = bnpp.plan_sample_batch(m, ev_vars, k, dtype=dt)
        x = {n: bnpp.sample_batch(cb, m, ev_vars, rows[:n], k, seed=SEED, dtype=dt)[0] for n in ns}   # warm-up
        x1 = np.array([bnpp.sample(cl, m, k, e, seed=SEED, first_sample=i * k, dtype=dt)[0] for i, e in enumerate(evs)])
        same = bool(np.array_equal(x[ns[0]][:LOOP_ROWS], x1))
        for n in ns:
            bnpp.partition_batch(cp, m, ev_vars, rows[:n], dtype=dt)
        t = {"loop": [], **{("smp", n): [] for n in ns}, **{("pr", n): [] for n in ns}}
        for _ in range(reps):                                    # alternating
            for n in ns:
                t0 = time.perf_counter()
                bnpp.sample_batch(cb, m, ev_vars, rows[:n], k, seed=SEED, dtype=dt)
                t[("smp", n)].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                bnpp.partition_batch(cp, m, ev_vars, rows[:n], dtype=dt)
                t[("pr", n)].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for i, e in enumerate(evs):
                bnpp.sample(cl, m, k, e, seed=SEED, first_sample=i * k, dtype=dt)
            t["loop"].append((time.perf_counter() - t0) * 1e3 / LOOP_ROWS)
        split = {n: host_split(lambda n=n: bnpp.sample_batch(cb, m, ev_vars, rows[:n], k, seed=SEED, dtype=dt)) for n in ns}
        for c in (cb, cl, cp):
            c.close()
        loop, loop_mm = med(t["loop"])
        rec = {"mode": "rows", "case": name + " " + dname, "k": k, "n_evidence_vars": len(ev_vars), "reps": reps,
               "rows_per_launch_planned_at_64GB": st["rows_per_launch"], "state_bytes_per_launch": st["state_bytes"],
               "arena_bytes_per_launch": st["arena_bytes"], "draw_rows": st["draw_rows"], "draw_rows_b": st["draw_rows_b"],
               "batch_samples_equal_single": same,
               "single_loop_ms_per_row": loop, "single_loop_ms_per_row_min_max": loop_mm}
        for n in ns:
            b, mm = med(t[("smp", n)])
            p, pmm = med(t[("pr", n)])
            rec["sample_batch_ms_n%d" % n] = b
            rec["sample_batch_ms_min_max_n%d" % n] = mm
            rec["sample_batch_rows_per_s_n%d" % n] = n / (b * 1e-3)
            rec["sample_batch_samples_per_s_n%d" % n] = n * k / (b * 1e-3)
            rec["sample_batch_ms_per_row_n%d" % n] = b / n
            rec["speedup_vs_loop_n%d" % n] = loop / (b / n)
            rec["partition_batch_ms_n%d" % n] = p
            rec["partition_batch_ms_min_max_n%d" % n] = pmm
            rec["sample_over_partition_batch_n%d" % n] = b / p
            rec["host_split_ms_n%d" % n] = split[n]
        faster = bool(rec["sample_batch_ms_per_row_n%d" % ns[0]] < loop)
        rec["batch_faster_than_loop_n%d_k%d" % (ns[0], k)] = faster
        print(json.dumps(rec), flush=True)
        if k == 1:
            ok = faster
    return ok


def draw_mode(name, dname, n, k, reps):
    m, ev_vars = load(name)
    ctx = bnpp.Context(0)
    rows = draw(ctx, m, ev_vars, n)
    ts = []
    for i in range(reps + 1):                                # the first call plans
        t0 = time.perf_counter()
        bnpp.sample_batch(ctx, m, ev_vars, rows, k, seed=SEED, dtype=DT[dname])
        if i:
            ts.append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    b, mm = med(ts)
    print(json.dumps({"mode": "draw-run", "case": name + " " + dname, "n_rows": n, "k": k, "calls": reps + 1,
                      "ms_under_the_profiler": b, "ms_min_max": mm}), flush=True)


def stats_mode(path, case):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows:
        raise SystemExit("no rows in " + path)
    name_col = next(k for k in rows[0] if "name" in k.lower())

    def num(r, *keys):
        for k in r:
            if k.lower().replace("_", "") in keys:
                return float(r[k])
        raise KeyError(keys)

    total = sum(num(r, "totaldurationns", "totaldurations") for r in rows)
    mine = [r for r in rows if DRAW_KERNEL in r[name_col]]
    if len(mine) != 1:
        raise SystemExit("expected one row of %s, found %d" % (DRAW_KERNEL, len(mine)))
    r = mine[0]
    tot = num(r, "totaldurationns", "totaldurations")
    calls = num(r, "calls")
    print(json.dumps({"mode": "draw-kernel", "case": case, "kernel": DRAW_KERNEL, "calls": int(calls),
                      "average_us": tot / calls / 1e3, "total_us": tot / 1e3, "all_kernels_us": total / 1e3,
                      "share_of_kernel_time": tot / total,
                      "source": "rocprofv3 --kernel-trace --stats, a run of its own"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["rows", "draw", "stats"])
    ap.add_argument("--models", nargs="+", default=list(EV_VARS))
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    ap.add_argument("--ns", nargs="+", type=int, default=[1 << 10, 1 << 16])
    ap.add_argument("--ks", nargs="+", type=int, default=[1, 16])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--csv", help="stats: the kernel-stats CSV of a profiled draw run")
    ap.add_argument("--case", default="", help="stats: the label of the record")
    a = ap.parse_args()
    if a.mode == "stats":
        return stats_mode(a.csv, a.case)
    slower = []
    for name in a.models:
        for dname in a.dtypes:
            ns = sorted(a.ns)
            if a.mode == "rows":
                if not rows_mode(name, dname, ns, sorted(a.ks), a.reps) and name in ("alarm", "ising12x12"):
                    slower.append(name + " " + dname)
            else:
                for k in sorted(a.ks):
                    draw_mode(name, dname, ns[-1], k, a.reps)
    if slower:
        raise SystemExit("the batched call is not below the loop per row at n = %d, K = 1: %s" % (a.ns[0], ", ".join(slower)))


if __name__ == "__main__":
    main()
