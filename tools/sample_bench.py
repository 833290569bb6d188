#!/usr/bin/env python3
"""Posterior-sampling measurements (warm relaunches of cached jobs, the sides
alternating in one call; medians with min-max):

  (default) bnpp.sample at n = 1, 2^10, 2^16, 2^20 beside a warm
      bnpp.partition of the same model, dtype and order -- the forward pass
      that sampling cannot avoid -- on ising12x12, Munin1 and noisyor_50_80
      (with its evidence); samples/s at n = 2^20.  Host clock around calls
      that end in a device synchronise and the copy of the samples to the host.
  --kernel MODEL: only warm bnpp.sample calls at n = 2^20 in both dtypes, to be
      run under `rocprofv3 --kernel-trace --stats` for sample_rows_kernel's time.
  --from-stats MODEL DIR: that run's *kernel_stats.csv under DIR -> the
      kernel's time per launch and its rate over its algorithmic bytes: per
      sample and row the gathered entries (n_in * k of the dtype) plus one byte
      read per separator variable plus one byte written, plus one byte written
      per evidence variable.

    python tools/sample_bench.py > profiles/sample_bench.jsonl
"""
import csv
import glob
import json
import os
import statistics
import sys
import time

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(REPO, "bn-pp_amd", "python"))
import bnpp  # noqa: E402
from bnpp import synth  # noqa: E402

MODELS = os.path.join(REPO, "tests", "golden", "models")
CASES = {"ising12x12": None, "Munin1": None, "noisyor_50_80": "noisyor_50_80.uai.evid"}
NS = (1, 1 << 10, 1 << 16, 1 << 20)
SEED = 1


def load(name):
    m = bnpp.Model.load(os.path.join(MODELS, name + ".uai"))
    ev = synth.read_evidence(os.path.join(MODELS, CASES[name])) if CASES[name] else {}
    return m, ev


def bytes_per_sample(name, eb):
    """Algorithmic bytes of the sampling step per sample, from the scopes alone
    (the bucket assignment of plan_sample restated)."""
    mm, ev = load(name)
    m = synth.read_uai(os.path.join(MODELS, name + ".uai"))
    order, _ = bnpp.ordering(mm, ev)
    rank = {v: i for i, v in enumerate(order)}
    buckets = [[] for _ in order]
    for scope in m["scopes"]:
        s = [v for v in scope if v not in ev]
        if s:
            buckets[min(rank[v] for v in s)].append(s)
    total = len(ev)
    for i, x in enumerate(order):
        sep = []
        for s in buckets[i]:
            sep += [v for v in s if v != x and v not in sep]
        total += len(buckets[i]) * m["cards"][x] * eb + len(sep) + 1
        if sep:
            buckets[min(rank[v] for v in sep)].append(sep)
    return total


def whole(name, dt, dname, reps=9):
    m, ev = load(name)
    # one context caches one job: each side gets its own, so all relaunch warm
    cp = bnpp.Context(0)
    cs = {n: bnpp.Context(0) for n in NS}
    lz = bnpp.partition(cp, m, ev, dtype=dt)[0]
    for n in NS:
        assert bnpp.sample(cs[n], m, n, ev, seed=SEED, dtype=dt)[2] == 0
    t = {"pr": [], **{n: [] for n in NS}}
    for r in range(reps):                                # alternating
        t0 = time.perf_counter()
        bnpp.partition(cp, m, ev, dtype=dt)
        assert bnpp.last_timing()["plan_ms"] == 0
        t["pr"].append((time.perf_counter() - t0) * 1e3)
        for n in NS:
            t0 = time.perf_counter()
            bnpp.sample(cs[n], m, n, ev, seed=SEED + r, dtype=dt)
            assert bnpp.last_timing()["plan_ms"] == 0
            t[n].append((time.perf_counter() - t0) * 1e3)
    cp.close()
    for c in cs.values():
        c.close()
    pr = statistics.median(t["pr"])
    rec = {"case": name + " " + dname, "n_vars": m.n_vars, "n_evidence": len(ev), "log10_Z": lz, "reps": reps,
           "pr_ms": pr, "pr_ms_min_max": [min(t["pr"]), max(t["pr"])]}
    for n in NS:
        md = statistics.median(t[n])
        rec["sample_ms_n%d" % n] = md
        rec["sample_ms_min_max_n%d" % n] = [min(t[n]), max(t[n])]
        rec["sample_over_pr_n%d" % n] = md / pr
    rec["samples_per_s_n%d" % NS[-1]] = NS[-1] / (rec["sample_ms_n%d" % NS[-1]] * 1e-3)
    print(json.dumps(rec), flush=True)


def kernel_run(name):
    m, ev = load(name)
    for dt in (bnpp.F64, bnpp.F32):
        ctx = bnpp.Context(0)
        for r in range(6):
            deg = bnpp.sample(ctx, m, NS[-1], ev, seed=SEED + r, dtype=dt)[2]
        ctx.close()
    print(json.dumps({"case": name + " kernel run", "n": NS[-1], "n_degenerate": deg}), flush=True)


def from_stats(name, root):
    rows = []
    for path in glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "sample_rows_kernel" in r["Name"]]
    if not rows:
        raise SystemExit("no sample_rows_kernel in a *kernel_stats.csv under " + root)
    for r in rows:
        f32 = "<float>" in r["Name"]
        b = bytes_per_sample(name, 4 if f32 else 8) * NS[-1]
        ns = float(r["AverageNs"])
        print(json.dumps({"case": name + (" f32" if f32 else " f64") + " sample_rows_kernel", "n": NS[-1],
                          "launches": int(r["Calls"]), "kernel_ms": ns * 1e-6,
                          "kernel_ms_min_max": [float(r["MinNs"]) * 1e-6, float(r["MaxNs"]) * 1e-6],
                          "algorithmic_bytes": b, "GBps": b / ns, "kernel_samples_per_s": NS[-1] / (ns * 1e-9)}),
              flush=True)


def main():
    if "--kernel" in sys.argv:
        return kernel_run(sys.argv[sys.argv.index("--kernel") + 1])
    if "--from-stats" in sys.argv:
        i = sys.argv.index("--from-stats")
        return from_stats(sys.argv[i + 1], sys.argv[i + 2])
    for dt, dname in ((bnpp.F64, "f64"), (bnpp.F32, "f32")):
        for name in CASES:
            whole(name, dt, dname)


if __name__ == "__main__":
    main()
