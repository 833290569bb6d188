#!/usr/bin/env python3
"""One EM iteration and one log-likelihood step on device-resident tables beside the loop a caller writes without
them.  One JSON line per case.

bench   this tree.  em_iter: bt.expected_counts(tables=...), bt.m_step, tables.set -- the body of bt.em -- on a
        BAYES model; loglik: bt.log_likelihood forward and backward (every model); with the engine's own split of
        one more counts call (the line BNPP_TIMING prints: stage / enqueue / wait).  switch: a counts job
        alternating with a log_partition job on one context, which caches one job, beside the same two calls
        each repeated on its own: the cost of one job switch.
host    the baseline: learn.em's iteration (Model.from_dict, expected_counts, m_step) with the rows beginning on
        the device, as a torch caller has them.  The baseline is the parent commit, so this mode runs in a
        process of its own on a checkout of it: --tree names that checkout (its Python package and its
        lib/libbnpp.so are the ones loaded).
table   reads the records of both modes and prints the comparison.
trace   reads the kernel statistics of a `bench` run made under rocprofv3 (a run of its own) and prints the rows of
        the three new steps.

Cases: alarm (em_iter, loglik) and ising12x12 (loglik; a MARKOV model has no M step), fp64 and fp32, 2^10 and 2^16
rows.  Method as the other benches: warm, medians of `reps` repetitions with min-max, one process per mode.

    git worktree add ../parent HEAD~1 && make -C ../parent/bn-pp_amd
    python tools/tables_bench.py host --tree ../parent >> profiles/tables_bench.jsonl
    python tools/tables_bench.py bench >> profiles/tables_bench.jsonl
    python tools/tables_bench.py table < profiles/tables_bench.jsonl
    rocprofv3 --kernel-trace --stats -d trace -o tb --output-format csv -- python tools/tables_bench.py bench --models alarm --dtypes f64 --ns 65536 --reps 3
    python tools/tables_bench.py trace --csv trace/tb_kernel_stats.csv >> profiles/tables_bench.jsonl
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


def med(ts):
    return statistics.median(ts), [min(ts), max(ts)]


def clock(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def child_last(d):
    """The golden BAYES files list a CPT's child first; the M step wants it last: every table transposed."""
    return dict(d, scopes=[list(s[1:]) + [s[0]] for s in d["scopes"]],
                values=[np.moveaxis(np.asarray(v).reshape([d["cards"][x] for x in s]), 0, -1).reshape(-1).tolist()
                        for s, v in zip(d["scopes"], d["values"])])


def run(mode, tree, models, dtypes, ns, reps):
    sys.path.insert(0, os.path.join(tree, "bn-pp_amd", "python"))
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import torch
    import bnpp
    from bnpp import learn, synth
    from device_io_bench import engine_split
    bt = None
    if mode == "bench":
        import bnpp.tensor as bt
    DT = {"f64": bnpp.F64, "f32": bnpp.F32}
    ctx = bnpp.Context(0)
    for name in models:
        d = synth.read_uai(os.path.join(MODELS, name + ".uai"))
        bayes = d.get("type") == "BAYES"
        if bayes:
            d = child_last(d)
        m = bnpp.Model.from_dict(d)
        ev = EV_VARS[name]
        for n in ns:
            samples, _, _ = bnpp.sample(ctx, m, n, seed=7)
            t_rows = torch.from_numpy(np.ascontiguousarray(np.asarray(samples)[:, ev].astype(np.int32))).cuda()
            for dname in dtypes:
                dt = DT[dname]
                rec0 = {"mode": mode, "model": name, "dtype": dname, "n_rows": n, "reps": reps,
                        "lib_version": bnpp._lib.bnpp_version()}

                def emit(case, fn, extra=None):
                    def timed():
                        fn()
                        torch.cuda.synchronize()
                    timed()                                     # warm: the plan, the arena, the allocator's blocks
                    timed()
                    rec = dict(rec0, case=case)
                    rec["ms"], rec["ms_min_max"] = med([clock(timed) for _ in range(reps)])
                    if extra:
                        rec.update(extra(timed))
                    print(json.dumps(rec), flush=True)
                    return rec["ms"]

                if mode == "host":
                    if bayes:
                        state = {"cur": d}

                        def host_iter():
                            counts, lz, _ = bnpp.expected_counts(ctx, bnpp.Model.from_dict(state["cur"]), ev,
                                                                 t_rows.cpu().numpy(), dtype=dt)
                            ok = np.isfinite(lz)
                            float(np.sum(lz[ok]))
                            state["cur"] = learn.m_step(state["cur"], counts)
                        emit("em_iter", host_iter)
                    continue
                tables = bt.Tables(ctx, m, dt)
                if bayes:
                    def em_iter():
                        counts, lz, _ = bt.expected_counts(ctx, m, ev, t_rows, tables=tables)
                        torch.sum(lz[torch.isfinite(lz)])
                        tables.set(bt.m_step(ctx, m, counts, tables.values))
                    emit("em_iter", em_iter, lambda timed: {"engine": engine_split(timed, "expected_counts_dv")})
                    tables.set(torch.tensor([x for v in d["values"] for x in v], dtype=torch.float64, device="cuda"))
                with np.errstate(divide="ignore"):
                    logs = np.log(np.concatenate([np.asarray(v, dtype=np.float64) for v in d["values"]]))
                theta = torch.from_numpy(logs).cuda().requires_grad_(True)

                def loglik():
                    theta.grad = None
                    ll, _, _ = bt.log_likelihood(ctx, m, ev, t_rows, theta, tables=tables)
                    ll.backward()
                a = emit("loglik", loglik, lambda timed: {"engine": engine_split(timed, "expected_counts_dv")})
                # one job switch: the counts job and a log_partition job take turns in the context's one cache slot
                soft = SOFT_VARS[name]
                ws = sum(d["cards"][v] for v in soft)
                ll_soft = torch.zeros((n, ws), dtype=torch.float64, device="cuda", requires_grad=True)

                def logpart():
                    ll_soft.grad = None
                    bt.log_partition(ctx, m, ev, t_rows, log_soft=(soft, ll_soft), dtype=dt).sum().backward()
                b = emit("log_partition", logpart)

                def both():
                    loglik()
                    logpart()
                c = emit("loglik_then_log_partition", both)
                print(json.dumps(dict(rec0, case="switch", ms=round((c - a - b) / 2, 4),
                                      what="(alternating pair - the two calls on their own) / 2")), flush=True)
                tables.close()
    ctx.close()


def table():
    recs = [json.loads(line) for line in sys.stdin if line.strip().startswith("{")]
    key = lambda r: (r["case"], r["model"], r["dtype"], r["n_rows"])
    host = {key(r): r for r in recs if r.get("mode") == "host"}
    print("| case | model | dtype | rows | parent ms (min-max) | this tree ms (min-max) | stage / enqueue / wait | ratio |")
    print("|---|---|---|---|---|---|---|---|")
    for r in recs:
        if r.get("mode") != "bench":
            continue
        if r["case"] == "switch":
            print("| switch | %s | %s | %d | - | %.3f per switch | - | - |" % (r["model"], r["dtype"], r["n_rows"], r["ms"]))
            continue
        h = host.get(key(r))
        e = r.get("engine") or {}
        split = "%.2f / %.2f / %.2f" % (e["stage_ms"], e["enqueue_ms"], e["wait_ms"]) if e else "-"
        mine = "%.3f (%.3f-%.3f)" % (r["ms"], *r["ms_min_max"])
        if h is None:
            print("| %s | %s | %s | %d | - | %s | %s | - |" % (*key(r), mine, split))
        else:
            print("| %s | %s | %s | %d | %.3f (%.3f-%.3f) | %s | %s | %.2fx |"
                  % (*key(r), h["ms"], *h["ms_min_max"], mine, split, h["ms"] / r["ms"]))


def trace(csv_path):
    import csv
    for r in csv.DictReader(open(csv_path)):
        if any(k in r["Name"] for k in ("stage_tables", "tables_shift", "stage_weights", "mstep_kernel")):
            print(json.dumps({"mode": "trace", "kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]),
                              "us_average": round(float(r["AverageNs"]) / 1e3, 2), "us_min": round(float(r["MinNs"]) / 1e3, 2),
                              "us_max": round(float(r["MaxNs"]) / 1e3, 2),
                              "source": "rocprofv3 --kernel-trace --stats, a run of its own"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bench", "host", "table", "trace"])
    ap.add_argument("--tree", default=REPO, help="host: the checkout whose package and library are loaded (the parent commit)")
    ap.add_argument("--models", nargs="+", default=["alarm", "ising12x12"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    ap.add_argument("--ns", nargs="+", type=int, default=[1 << 10, 1 << 16])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--csv", help="trace: the kernel statistics (rocprofv3 ..._kernel_stats.csv)")
    a = ap.parse_args()
    if a.mode == "table":
        table()
    elif a.mode == "trace":
        trace(a.csv)
    else:
        run(a.mode, os.path.abspath(a.tree), a.models, a.dtypes, a.ns, a.reps)


if __name__ == "__main__":
    main()
