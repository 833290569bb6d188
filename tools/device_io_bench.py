#!/usr/bin/env python3
"""Device-resident batched calls beside the host-array calls a torch caller makes today.  One JSON line per case.

dv      bnpp.tensor.<call> on tensors that begin and end on the device (this
        tree), with the engine's own split of one more call (the line
        BNPP_TIMING prints: stage / enqueue / wait).
host    the host-array call on the same rows with the tensors beginning and
        ending on the device: the caller does .cpu().numpy() before and
        torch.from_numpy().cuda() after, which is what a torch caller does
        today.  The baseline is the parent commit, so this mode runs in a
        process of its own on a checkout of it: --tree names that checkout (its
        Python package and its lib/libbnpp.so are the ones loaded).
table   reads the records of both modes and prints the comparison: a _dv case
        counts as slower when its median exceeds the baseline's median by more
        than the baseline's own min-max spread.
trace   reads the kernel trace of a `dv` run made under rocprofv3 (a run of its
        own: --ns 65536 --reps 3, so six calls per case) and prints, per case,
        the durations of the four row steps (mode "trace") and the sum and the
        first-start-to-last-end span of all of a call's kernels (mode
        "trace_call"), beside the untraced call's median where --dv names the
        records of the `dv` run.

Cases: partition_batch with 3-4 soft variables, marginals_batch with all
targets, mpe_batch, sample_batch with K = 1 and 16; alarm and ising12x12, fp64
and fp32, 2^10 and 2^16 rows.  Method as the other benches: warm, medians of
`reps` repetitions with min-max, one process per mode.

    git worktree add ../parent HEAD~1 && make -C ../parent/bn-pp_amd
    python tools/device_io_bench.py host --tree ../parent >> profiles/device_io_bench.jsonl
    python tools/device_io_bench.py dv >> profiles/device_io_bench.jsonl
    python tools/device_io_bench.py table < profiles/device_io_bench.jsonl
    rocprofv3 --kernel-trace --stats -d trace -o dv --output-format csv -- python tools/device_io_bench.py dv --ns 65536 --reps 3
    python tools/device_io_bench.py trace --csv trace/dv_kernel_trace.csv --dv profiles/device_io_bench.jsonl >> profiles/device_io_bench.jsonl
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
MODELS = os.path.join(REPO, "tests", "golden", "models")
EV_VARS = {"alarm": [3, 10, 20], "ising12x12": [0, 50, 100, 143]}
SOFT_VARS = {"alarm": [5, 12, 30], "ising12x12": [7, 60, 90, 130]}
CASES = ("partition_soft", "marginals", "mpe", "sample_k1", "sample_k16")


def med(ts):
    return statistics.median(ts), [min(ts), max(ts)]


def clock(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def engine_split(call, name):
    """The engine's own clock of one call under BNPP_TIMING: its stderr line parsed -> dict or None."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        os.environ["BNPP_TIMING"] = "1"
        try:
            call()
        finally:
            del os.environ["BNPP_TIMING"]
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    found = re.findall(name + r": stage ([0-9.]+) ms, enqueue ([0-9.]+) ms, wait ([0-9.]+) ms", text)
    return dict(zip(("stage_ms", "enqueue_ms", "wait_ms"), map(float, found[-1]))) if found else None


def run(mode, tree, models, dtypes, ns, reps, cases):
    sys.path.insert(0, os.path.join(tree, "bn-pp_amd", "python"))
    import torch
    import bnpp
    from bnpp import synth
    bt = None
    if mode == "dv":
        import bnpp.tensor as bt
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
            t_rows = torch.from_numpy(np.ascontiguousarray(np.asarray(samples)[:, ev].astype(np.int32))).cuda()
            t_none = torch.zeros((n, 0), dtype=torch.int32, device="cuda")
            t_lik = torch.from_numpy(np.exp2(rng.uniform(-20, 0, (n, ws)))).cuda()

            def same(case, got, dt):
                """The _dv results beside this tree's host-array call on the same rows: z, marginals, assignments,
                samples and n_degenerate bit for bit (log10_z is compared by the tests, within 4 ulp)."""
                rows, none, lik = t_rows.cpu().numpy(), t_none.cpu().numpy(), t_lik.cpu().numpy()
                eq = lambda a, b: bool(np.array_equal(a.cpu().numpy().view(np.uint8), np.ascontiguousarray(b).view(np.uint8)))
                if case == "partition_soft":
                    return eq(got[1], bnpp.partition_batch(ctx, m, [], none, dtype=dt, soft=(soft, lik))[1])
                if case == "marginals":
                    return eq(got[0], bnpp.marginals_batch(ctx, m, ev, rows, dtype=dt)[0])
                if case == "mpe":
                    return eq(got[1], bnpp.mpe_batch(ctx, m, ev, rows, dtype=dt)[1])
                want = bnpp.sample_batch(ctx, m, ev, rows, 1 if case == "sample_k1" else 16, seed=5, dtype=dt)
                return eq(got[0], want[0]) and eq(got[2], want[2])

            for dname in dtypes:
                dt = DT[dname]
                for case in cases:
                    if mode == "dv":
                        fn, dvname = {
                            "partition_soft": (lambda: bt.partition_batch(ctx, m, [], t_none, dtype=dt, soft=(soft, t_lik)), "partition_batch_dv"),
                            "marginals": (lambda: bt.marginals_batch(ctx, m, ev, t_rows, dtype=dt), "marginals_batch_dv"),
                            "mpe": (lambda: bt.mpe_batch(ctx, m, ev, t_rows, dtype=dt), "mpe_batch_dv"),
                            "sample_k1": (lambda: bt.sample_batch(ctx, m, ev, t_rows, 1, seed=5, dtype=dt), "sample_batch_dv"),
                            "sample_k16": (lambda: bt.sample_batch(ctx, m, ev, t_rows, 16, seed=5, dtype=dt), "sample_batch_dv"),
                        }[case]
                    else:
                        dvname = None

                        def back(res):
                            return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in res if isinstance(a, np.ndarray)]

                        fn = {
                            "partition_soft": lambda: back(bnpp.partition_batch(ctx, m, [], t_none.cpu().numpy(), dtype=dt,
                                                                                soft=(soft, t_lik.cpu().numpy()))),
                            "marginals": lambda: back(bnpp.marginals_batch(ctx, m, ev, t_rows.cpu().numpy(), dtype=dt)),
                            "mpe": lambda: back(bnpp.mpe_batch(ctx, m, ev, t_rows.cpu().numpy(), dtype=dt)),
                            "sample_k1": lambda: back(bnpp.sample_batch(ctx, m, ev, t_rows.cpu().numpy(), 1, seed=5, dtype=dt)),
                            "sample_k16": lambda: back(bnpp.sample_batch(ctx, m, ev, t_rows.cpu().numpy(), 16, seed=5, dtype=dt)),
                        }[case]

                    def timed():
                        fn()
                        torch.cuda.synchronize()

                    timed()                                     # warm: the plan, the arena, the allocator's blocks
                    timed()
                    ts = [clock(timed) for _ in range(reps)]
                    rec = {"mode": mode, "case": case, "model": name, "dtype": dname, "n_rows": n, "reps": reps,
                           "lib_version": bnpp._lib.bnpp_version()}
                    rec["ms"], rec["ms_min_max"] = med(ts)
                    if dvname:
                        rec["engine"] = engine_split(timed, dvname)
                        rec["same_as_host_array"] = same(case, fn(), dt)   # this tree's host-array call, at this size
                    print(json.dumps(rec), flush=True)
    ctx.close()


def table():
    recs = [json.loads(line) for line in sys.stdin if line.strip().startswith("{")]
    key = lambda r: (r["case"], r["model"], r["dtype"], r["n_rows"])
    host = {key(r): r for r in recs if r.get("mode") == "host"}
    print("| case | model | dtype | rows | host-array ms (min-max) | _dv ms (min-max) | stage / enqueue / wait | ratio | |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in recs:
        if r.get("mode") != "dv":
            continue
        h = host.get(key(r))
        e = r.get("engine") or {}
        split = "%.2f / %.2f / %.2f" % (e["stage_ms"], e["enqueue_ms"], e["wait_ms"]) if e else "-"
        if h is None:
            print("| %s | %s | %s | %d | - | %.3f (%.3f-%.3f) | %s | - | no baseline |" % (*key(r), r["ms"], *r["ms_min_max"], split))
            continue
        spread = h["ms_min_max"][1] - h["ms_min_max"][0]
        flag = "SLOWER" if r["ms"] > h["ms"] + spread else ""
        print("| %s | %s | %s | %d | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %s | %.2fx | %s |"
              % (*key(r), h["ms"], *h["ms_min_max"], r["ms"], *r["ms_min_max"], split, h["ms"] / r["ms"], flag))


STEP_CASES = {"stage_rows_kernel": CASES[1:], "stage_lik_kernel": CASES[:1], "emit_scalars_kernel": CASES,
              "emit_states_mpe_kernel": ("mpe",), "emit_states_sample_kernel": ("sample_k1", "sample_k16")}
TRACE_SOURCE = "rocprofv3 --kernel-trace --stats, a run of its own"


def trace(csv_path, dv_path, models, dtypes, calls):
    """The kernels of a traced `dv` run at one row count, in start order: `calls` calls per case, the cases in
    run()'s order.  A call begins with its first staging kernel and ends with its last emit kernel."""
    import csv
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    order = [(m, d) for m in models for d in dtypes]
    for kernel, cases in STEP_CASES.items():
        d = [us(r) for r in rows if kernel in r["Kernel_Name"]]
        assert len(d) == len(order) * len(cases) * calls, (kernel, len(d))
        for i, (m, dt, c) in enumerate((m, dt, c) for m, dt in order for c in cases):
            g = d[i * calls:(i + 1) * calls]
            print(json.dumps({"mode": "trace", "kernel": kernel, "model": m, "dtype": dt, "case": c, "n_rows": 65536,
                              "launches": len(g), "us_median": round(statistics.median(g), 2),
                              "us_min_max": [round(min(g), 2), round(max(g), 2)], "source": TRACE_SOURCE}))
    dv = {}
    for line in open(dv_path) if dv_path else ():
        r = json.loads(line) if line.strip().startswith("{") else {}
        if r.get("mode") == "dv":
            dv[(r["case"], r["model"], r["dtype"], r["n_rows"])] = r["ms"]
    segs, cur = [], None
    for r in rows:
        if "stage_rows_kernel" in r["Kernel_Name"] or "stage_lik_kernel" in r["Kernel_Name"]:
            if cur:
                segs.append(cur)
            cur = [r]
        elif cur is not None:
            cur.append(r)
    segs.append(cur)
    segs = [s[:max(i for i, r in enumerate(s) if "::emit_s" in r["Kernel_Name"]) + 1] for s in segs]
    assert len(segs) == len(order) * len(CASES) * calls, len(segs)
    for i, (m, dt, c) in enumerate((m, dt, c) for m, dt in order for c in CASES):
        g = segs[i * calls:(i + 1) * calls]
        span = statistics.median((int(s[-1]["End_Timestamp"]) - int(s[0]["Start_Timestamp"])) / 1e6 for s in g)
        rec = {"mode": "trace_call", "case": c, "model": m, "dtype": dt, "n_rows": 65536,
               "kernels_per_call": statistics.median(len(s) for s in g),
               "kernel_sum_ms": round(statistics.median(sum(us(r) for r in s) / 1e3 for s in g), 4),
               "first_start_to_last_end_ms": round(span, 4), "source": TRACE_SOURCE}
        if (c, m, dt, 65536) in dv:
            rec["dv_call_ms"] = dv[(c, m, dt, 65536)]
            rec["dv_minus_span_ms"] = round(rec["dv_call_ms"] - span, 4)
        print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["dv", "host", "table", "trace"])
    ap.add_argument("--tree", default=REPO, help="host: the checkout whose package and library are loaded (the parent commit)")
    ap.add_argument("--models", nargs="+", default=["alarm", "ising12x12"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    ap.add_argument("--ns", nargs="+", type=int, default=[1 << 10, 1 << 16])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=CASES)
    ap.add_argument("--csv", help="trace: the kernel trace (rocprofv3 ..._kernel_trace.csv)")
    ap.add_argument("--dv", help="trace: the records of the untraced dv run")
    ap.add_argument("--calls", type=int, default=6, help="trace: calls per case in the traced run (2 warm + reps + 1)")
    a = ap.parse_args()
    if a.mode == "table":
        table()
    elif a.mode == "trace":
        trace(a.csv, a.dv, a.models, a.dtypes, a.calls)
    else:
        run(a.mode, os.path.abspath(a.tree), a.models, a.dtypes, a.ns, a.reps, a.cases)


if __name__ == "__main__":
    main()
