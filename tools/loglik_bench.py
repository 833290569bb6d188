#!/usr/bin/env python3
"""Forward plus backward of bnpp.tensor.log_partition beside what a torch caller does without it.  One JSON line
per case.

bench   new: ln_z = bt.log_partition(..., log_soft=(soft, loglik)); ln_z.sum().backward() -- one call of
        bnpp_log_partition_dv with post (the batched-marginals plan on the soft variables), and a torch multiply.
        base: what the caller writes on the parent commit, in the same process and alternating with `new` rep by
        rep: torch max / sub / exp to an fp64 lik (one shift per row), bt.partition_batch for the value,
        bt.marginals_batch(targets=soft_vars) for the gradient, and the shift added back in torch.  Both end with
        ln Z and d ln Z / d loglik on the device; the record holds their largest differences.
trace   reads the kernel trace of a `bench --only new` run made under rocprofv3 (a run of its own) and prints the
        durations of the two new steps, stage_loglik_kernel and emit_logs_kernel.
table   reads the records and prints the comparison.

Cases: alarm and ising12x12, 3-4 evidence and 3-4 soft variables, 2^10 and 2^16 rows, fp64 and fp32; warm, medians
of `reps` repetitions with min-max.

    python tools/loglik_bench.py bench >> profiles/loglik_bench.jsonl
    rocprofv3 --kernel-trace --stats -d trace -o ll --output-format csv -- python tools/loglik_bench.py bench --only new --ns 65536 --reps 3
    python tools/loglik_bench.py trace --csv trace/ll_kernel_trace.csv >> profiles/loglik_bench.jsonl
    python tools/loglik_bench.py table < profiles/loglik_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
MODELS = os.path.join(REPO, "tests", "golden", "models")
EV_VARS = {"alarm": [3, 10, 20], "ising12x12": [0, 50, 100, 143]}
SOFT_VARS = {"alarm": [5, 12, 30], "ising12x12": [7, 60, 90, 130]}
LOG10_E = float.fromhex("0x1.bcb7b1526e50ep-2")


def med(ts):
    return statistics.median(ts), [min(ts), max(ts)]


def run(models, dtypes, ns, reps, only):
    sys.path.insert(0, os.path.join(REPO, "bn-pp_amd", "python"))
    import torch
    import bnpp
    import bnpp.tensor as bt
    from bnpp import synth
    DT = {"f64": bnpp.F64, "f32": bnpp.F32}
    ctx = bnpp.Context(0)
    for name in models:
        path = os.path.join(MODELS, name + ".uai")
        m, d = bnpp.Model.load(path), synth.read_uai(path)
        ev, soft = EV_VARS[name], SOFT_VARS[name]
        ws = sum(d["cards"][v] for v in soft)
        rng = np.random.default_rng(17)
        for n in ns:
            samples, _, _ = bnpp.sample(ctx, m, n, seed=7)
            rows = torch.from_numpy(np.ascontiguousarray(np.asarray(samples)[:, ev].astype(np.int32))).cuda()
            ll = torch.from_numpy(rng.uniform(-14.0, 0.0, (n, ws))).cuda().requires_grad_(True)   # a network's scores
            for dname in dtypes:
                dt = DT[dname]
                res = {}

                def new():
                    ll.grad = None
                    ln_z = bt.log_partition(ctx, m, ev, rows, log_soft=(soft, ll), dtype=dt)
                    ln_z.sum().backward()
                    res["new"] = (ln_z.detach(), ll.grad)
                    torch.cuda.synchronize()

                def base():
                    with torch.no_grad():
                        top = ll.max(dim=1, keepdim=True).values
                        lik = (ll - top).exp()              # the fp64 (n, Ws) copy
                        lz, _, _ = bt.partition_batch(ctx, m, ev, rows, dtype=dt, soft=(soft, lik))
                        post, _ = bt.marginals_batch(ctx, m, ev, rows, targets=soft, dtype=dt, soft=(soft, lik))
                        res["base"] = (lz / LOG10_E + len(soft) * top[:, 0], post)
                    torch.cuda.synchronize()

                fns = [("new", new), ("base", base)] if only is None else [(only, dict(new=new, base=base)[only])]
                ts = {k: [] for k, _ in fns}
                for rep in range(reps + 2):                 # two warm rounds: the plans, the arenas, the allocator's blocks
                    for k, f in fns:
                        t0 = time.perf_counter()
                        f()
                        if rep >= 2:
                            ts[k].append((time.perf_counter() - t0) * 1e3)
                rec = {"mode": "bench", "model": name, "dtype": dname, "n_rows": n, "reps": reps, "ev_vars": ev,
                       "soft_vars": soft, "alternating": only is None}
                for k in ts:
                    rec[k + "_ms"], rec[k + "_ms_min_max"] = med(ts[k])
                if only is None:
                    rec["ratio_base_over_new"] = rec["base_ms"] / rec["new_ms"]
                    fin = torch.isfinite(res["base"][0])
                    rec["max_abs_ln_z_diff"] = float((res["new"][0][fin] - res["base"][0][fin]).abs().max())
                    rec["max_abs_grad_diff"] = float((res["new"][1][fin] - res["base"][1][fin]).abs().max())
                    rec["possible_rows"] = int(fin.sum())
                print(json.dumps(rec), flush=True)
    ctx.close()


def trace(csv_path, models, dtypes, n, calls):
    """The two new steps in a traced `bench --only new` run at one row count, in start order: `calls` calls per
    (model, dtype), one launch of each step per call (one launch holds the rows)."""
    import csv
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    order = [(m, d) for m in models for d in dtypes]
    for kernel in ("stage_loglik_kernel", "emit_logs_kernel"):
        d = [us(r) for r in rows if kernel in r["Kernel_Name"]]
        per = len(d) // len(order)
        assert per * len(order) == len(d) and per >= calls, (kernel, len(d))
        for i, (m, dt) in enumerate(order):
            g = d[i * per:(i + 1) * per]
            print(json.dumps({"mode": "trace", "kernel": kernel, "model": m, "dtype": dt, "n_rows": n, "launches": len(g),
                              "us_median": round(statistics.median(g), 2), "us_min_max": [round(min(g), 2), round(max(g), 2)],
                              "source": "rocprofv3 --kernel-trace --stats, a run of its own"}))


def table():
    recs = [json.loads(line) for line in sys.stdin if line.strip().startswith("{")]
    print("| model | dtype | rows | base ms (min-max) | new ms (min-max) | base / new |")
    print("|---|---|---|---|---|---|")
    for r in recs:
        if r.get("mode") == "bench" and r.get("alternating"):
            print("| %s | %s | %d | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.2fx |"
                  % (r["model"], r["dtype"], r["n_rows"], r["base_ms"], *r["base_ms_min_max"], r["new_ms"], *r["new_ms_min_max"],
                     r["ratio_base_over_new"]))
    for r in recs:
        if r.get("mode") == "trace":
            print("%s %s %s %d rows: %.2f us (%.2f-%.2f), %d launches"
                  % (r["kernel"], r["model"], r["dtype"], r["n_rows"], r["us_median"], *r["us_min_max"], r["launches"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bench", "trace", "table"])
    ap.add_argument("--models", nargs="+", default=["alarm", "ising12x12"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    ap.add_argument("--ns", nargs="+", type=int, default=[1 << 10, 1 << 16])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", choices=["new", "base"], help="bench: one side alone (the traced run)")
    ap.add_argument("--csv", help="trace: the kernel trace (rocprofv3 ..._kernel_trace.csv)")
    ap.add_argument("--calls", type=int, default=5, help="trace: calls per case in the traced run (2 warm + reps)")
    a = ap.parse_args()
    if a.mode == "table":
        table()
    elif a.mode == "trace":
        trace(a.csv, a.models, a.dtypes, a.ns[-1], a.calls)
    else:
        run(a.models, a.dtypes, a.ns, a.reps, a.only)


if __name__ == "__main__":
    main()
