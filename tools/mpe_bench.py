#!/usr/bin/env python3
"""MPE measurements (warm, device events, the two sides alternating in one call):

  (a) bnpp_bucket_max beside bnpp_bucket_eliminate on one k = 4 Potts-shaped
      bucket of 2^26 outputs (a message over 14 card-4 variables times two
      pairwise factors, the first variable maximised / summed); the max
      kernel's achieved bytes/s over its algorithmic bytes
      sizeof(T) * (sum |in| + |out|) + |out| * 1 B.
  (b) bnpp.mpe beside bnpp.partition, warm relaunches of the cached jobs, on
      ising12x12, Munin1 and noisyor_50_80 (with its evidence).
  --buckets: (a) only.
  --decode: only warm bnpp.mpe calls on ising12x32 (a chain: the deepest
      elimination tree, the worst case of the depth-stepped decode), to be run
      under `rocprofv3 --kernel-trace --stats` for mpe_decode_kernel's time.

    python tools/mpe_bench.py > profiles/mpe_bench.jsonl
"""
import json
import os
import statistics
import sys
import time

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(REPO, "bn-pp_amd", "python"))
import torch  # noqa: E402
import bnpp  # noqa: E402
from bnpp import synth  # noqa: E402

MODELS = os.path.join(REPO, "tests", "golden", "models")


def bucket(ctx, dt, name, reps=7):
    td = torch.float32 if dt == bnpp.F32 else torch.float64
    eb = 4 if dt == bnpp.F32 else 8
    nv = 14
    cards = [4] * nv
    scopes = [list(range(nv)), [0, 1], [0, nv - 1]]
    out_vars = list(range(1, nv))
    n_out = 4 ** (nv - 1)
    g = torch.Generator(device="cuda").manual_seed(1)
    tabs = [torch.rand(4 ** len(s), dtype=td, device="cuda", generator=g) + 0.5 for s in scopes]
    out = torch.empty(n_out, dtype=td, device="cuda")
    arg = torch.empty(n_out, dtype=torch.uint8, device="cuda")
    ptrs = [t.data_ptr() for t in tabs]
    # a stream of its own: a null handle would mean the context's stream, not the one the events are on
    ts = torch.cuda.Stream()
    torch.cuda.set_stream(ts)
    stream = ts.cuda_stream
    info_max = bnpp.plan_max_single(dt, cards, scopes, 0, out_vars)
    info_sum = bnpp.plan_single(dt, cards, scopes, 0, out_vars)

    def run_max():
        bnpp.bucket_max(ctx, dt, cards, ptrs, scopes, 0, out.data_ptr(), out_vars, out_arg=arg.data_ptr(), stream=stream)

    def run_sum():
        bnpp.bucket_eliminate(ctx, dt, cards, ptrs, scopes, 0, out.data_ptr(), out_vars, stream=stream)

    t = {"max": [], "sum": []}
    for fn in (run_max, run_sum):
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):                                # alternating
        for key, fn in (("max", run_max), ("sum", run_sum)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t[key].append(a.elapsed_time(b))
    in_entries = sum(4 ** len(s) for s in scopes)
    max_bytes = eb * (in_entries + n_out) + n_out
    sum_bytes = eb * (in_entries + n_out)
    mx, sm = statistics.median(t["max"]), statistics.median(t["sum"])
    print(json.dumps({"case": "potts k=4 bucket, 2^26 outputs, " + name, "max_key": info_max["key"],
                      "sum_family": bnpp.FAMILIES[info_sum["family"]], "sum_key": info_sum["key"],
                      "max_ms": mx, "max_ms_min_max": [min(t["max"]), max(t["max"])], "sum_ms": sm,
                      "sum_ms_min_max": [min(t["sum"]), max(t["sum"])], "max_over_sum": mx / sm,
                      "max_bytes": max_bytes, "max_TBps": max_bytes / mx / 1e9, "sum_TBps": sum_bytes / sm / 1e9,
                      "reps": reps}), flush=True)


def whole(name, evf, dt, dname, reps=9):
    m = bnpp.Model.load(os.path.join(MODELS, name + ".uai"))
    ev = synth.read_evidence(os.path.join(MODELS, evf)) if evf else {}
    t = {"mpe": [], "pr": []}
    # one context caches one job: each side gets its own, so both relaunch warm
    cm, cp = bnpp.Context(0), bnpp.Context(0)
    lv = bnpp.mpe(cm, m, ev, dtype=dt)[0]
    lz = bnpp.partition(cp, m, ev, dtype=dt)[0]
    for _ in range(reps):
        t0 = time.perf_counter()
        bnpp.mpe(cm, m, ev, dtype=dt)
        assert bnpp.last_timing()["plan_ms"] == 0
        t1 = time.perf_counter()
        bnpp.partition(cp, m, ev, dtype=dt)
        assert bnpp.last_timing()["plan_ms"] == 0
        t2 = time.perf_counter()
        t["mpe"].append((t1 - t0) * 1e3)
        t["pr"].append((t2 - t1) * 1e3)
    cm.close()
    cp.close()
    a, b = statistics.median(t["mpe"]), statistics.median(t["pr"])
    print(json.dumps({"case": name + " " + dname, "mpe_ms": a, "mpe_ms_min_max": [min(t["mpe"]), max(t["mpe"])],
                      "pr_ms": b, "pr_ms_min_max": [min(t["pr"]), max(t["pr"])], "mpe_over_pr": a / b,
                      "log10_max": lv, "log10_Z": lz, "reps": reps}), flush=True)


def decode_only():
    ctx = bnpp.Context(0)
    m = bnpp.Model.load(os.path.join(MODELS, "ising12x32.uai"))
    for dt in (bnpp.F32, bnpp.F64):
        for _ in range(6):
            lv = bnpp.mpe(ctx, m, dtype=dt)[0]
    print(json.dumps({"case": "ising12x32 decode run", "log10_max": lv}), flush=True)
    ctx.close()


def main():
    if "--decode" in sys.argv:
        return decode_only()
    ctx = bnpp.Context(0)
    for dt, name in ((bnpp.F32, "f32"), (bnpp.F64, "f64")):
        bucket(ctx, dt, name)
    if "--buckets" in sys.argv:
        return ctx.close()
    for dt, name in ((bnpp.F64, "f64"), (bnpp.F32, "f32")):
        for model, evf in (("ising12x12", None), ("Munin1", None), ("noisyor_50_80", "noisyor_50_80.uai.evid")):
            whole(model, evf, dt, name)
    ctx.close()


if __name__ == "__main__":
    main()
