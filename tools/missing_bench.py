#!/usr/bin/env python3
"""Missing-values measurements (warm calls, medians of --reps with min-max; host
clock around calls that end in a device synchronise and the copy of the results
to the host).

  rows    rows with --frac of the cells of every evidence column missing (seeded),
          drawn from joint samples of the model so that every row is possible:
            mv        the call with partial = all evidence variables, its job cached;
            grouped   (a) what a caller does without it: the rows grouped by missing
                      pattern and one existing batched call per pattern over the
                      pattern's observed variables, in one context -- so every
                      pattern plans, as a caller's loop does; the planning is
                      included, the grouping itself (numpy) is not;
            filled    (b) the existing call over the same rows with the gaps filled
                      in from the sample: the floor, what keeping the variables costs.
          For partition_batch and expected_counts; the worst difference between mv
          and grouped is reported.  One JSON line per model, dtype, n and frac.
  gather  the masked gather step alone against the unmasked gather of the same
          source and R (bnpp.condition_batch, --launches enqueued back to back,
          then one synchronise): a source over (p, free, hard) with p partial and a
          third of its values missing, against the same call with p hard.

    python tools/missing_bench.py rows --models alarm ising12x12 >> profiles/missing_bench.jsonl
    python tools/missing_bench.py rows --models noisyor_50_80 --ns 64 >> profiles/missing_bench.jsonl
    python tools/missing_bench.py gather >> profiles/missing_bench.jsonl
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


def groups_of(rows):
    """The rows grouped by missing pattern -> [(observed columns, row indices)]."""
    pat = rows >= 0
    keys, inv = np.unique(pat, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    return [(np.flatnonzero(k), np.flatnonzero(inv == i)) for i, k in enumerate(keys)]


def rows_mode(name, dname, ns, fracs, reps):
    m, ev = load(name)
    dt = DT[dname]
    cv, cf, cg = bnpp.Context(0), bnpp.Context(0), bnpp.Context(0)
    full = draw(cv, m, ev, max(ns))
    for n in ns:
        for frac in fracs:
            rng = np.random.default_rng(17)
            rows = full[:n].copy()
            rows[rng.random(rows.shape) < frac] = bnpp.MISSING
            groups = groups_of(rows)

            def grouped_z():
                lz = np.zeros(n)
                for cols, idx in groups:
                    lz[idx] = bnpp.partition_batch(cg, m, [ev[j] for j in cols], rows[np.ix_(idx, cols)], dtype=dt)[0]
                return lz

            def grouped_counts():
                total = 0
                for cols, idx in groups:
                    total = total + bnpp.expected_counts(cg, m, [ev[j] for j in cols], rows[np.ix_(idx, cols)], dtype=dt)[0]
                return total

            lz, _, _ = bnpp.partition_batch(cv, m, ev, rows, dtype=dt, partial=ev)       # warm-up, all sides
            lzg = grouped_z()
            bnpp.partition_batch(cf, m, ev, full[:n], dtype=dt)
            ok = np.isfinite(lzg)
            worst_z = float(np.max(np.abs(lz[ok] - lzg[ok]) / np.maximum(1.0, np.abs(lzg[ok])))) if ok.any() else 0.0
            tv, tg, tf = [], [], []
            for _ in range(reps):
                tv.append(clock(lambda: bnpp.partition_batch(cv, m, ev, rows, dtype=dt, partial=ev)))
                tf.append(clock(lambda: bnpp.partition_batch(cf, m, ev, full[:n], dtype=dt)))
                tg.append(clock(grouped_z))
            cnt, _, _ = bnpp.expected_counts(cv, m, ev, rows, dtype=dt, partial=ev)
            cg_ = grouped_counts()
            bnpp.expected_counts(cf, m, ev, full[:n], dtype=dt)
            worst_c = float(np.max(np.abs(cnt - cg_) / np.maximum(1.0, np.abs(cg_))))
            cvt, cgt, cft = [], [], []
            for _ in range(reps):
                cvt.append(clock(lambda: bnpp.expected_counts(cv, m, ev, rows, dtype=dt, partial=ev)))
                cft.append(clock(lambda: bnpp.expected_counts(cf, m, ev, full[:n], dtype=dt)))
                cgt.append(clock(grouped_counts))
            sp = bnpp.plan_batch(m, ev, dtype=dt, partial=ev)
            sh = bnpp.plan_batch(m, ev, dtype=dt)
            rec = {"mode": "rows", "case": name + " " + dname, "n_rows": n, "frac_missing": frac,
                   "cells_missing": int((rows < 0).sum()), "n_evidence_vars": len(ev), "patterns": len(groups), "reps": reps,
                   "width_mv": sp[0]["width"], "width_hard": sh[0]["width"], "gather_steps_mv": sp[0]["gather_steps"],
                   "plan_bytes_moved_mv": sp[0]["bytes_moved"], "plan_bytes_moved_hard": sh[0]["bytes_moved"],
                   "rows_per_launch_mv": sp[0]["rows_per_launch"], "rows_per_launch_hard": sh[0]["rows_per_launch"],
                   "worst_rel_log10_z_mv_vs_grouped": worst_z, "worst_rel_counts_mv_vs_grouped": worst_c}
            for key, ts in (("partition_mv", tv), ("partition_grouped", tg), ("partition_filled", tf),
                            ("counts_mv", cvt), ("counts_grouped", cgt), ("counts_filled", cft)):
                rec[key + "_ms"], rec[key + "_ms_min_max"] = med(ts)
            rec["partition_grouped_over_mv"] = rec["partition_grouped_ms"] / rec["partition_mv_ms"]
            rec["partition_mv_over_filled"] = rec["partition_mv_ms"] / rec["partition_filled_ms"]
            rec["counts_grouped_over_mv"] = rec["counts_grouped_ms"] / rec["counts_mv_ms"]
            rec["counts_mv_over_filled"] = rec["counts_mv_ms"] / rec["counts_filled_ms"]
            print(json.dumps(rec), flush=True)
    for c in (cv, cf, cg):
        c.close()


def gather_mode(dname, Rs, reps, launches):
    import torch
    td = torch.float64 if dname == "f64" else torch.float32
    cards, scope, evv = [8, 64, 4], [0, 1, 2], [0, 2]          # (p, free, hard): 2048 entries, rest 512 masked / 64 unmasked
    ctx = bnpp.Context(0)
    rng = np.random.default_rng(5)
    src = torch.tensor(rng.uniform(0.05, 1.0, 2048), dtype=td, device="cuda")
    for R in Rs:
        ev = np.stack([rng.integers(0, cards[v], R) for v in evv]).astype(np.int32)
        evm = ev.copy()
        evm[0][rng.random(R) < 0.33] = bnpp.MISSING
        t_ev = torch.tensor(ev.reshape(-1), dtype=torch.int32, device="cuda")
        t_evm = torch.tensor(evm.reshape(-1), dtype=torch.int32, device="cuda")
        out = torch.zeros(512 * R, dtype=td, device="cuda")

        def run(masked):
            for _ in range(launches):
                bnpp.condition_batch(ctx, DT[dname], cards, src.data_ptr(), scope, evv, R,
                                     (t_evm if masked else t_ev).data_ptr(), out.data_ptr(), partial=[0] if masked else None)
            torch.cuda.synchronize()

        run(True)
        run(False)
        tm, tu = [], []
        for _ in range(reps):
            tm.append(clock(lambda: run(True)) / launches)
            tu.append(clock(lambda: run(False)) / launches)
        eb = 8 if dname == "f64" else 4
        a, amm = med(tm)
        b, bmm = med(tu)
        print(json.dumps({"mode": "gather", "case": "(p=8, free=64, hard=4) " + dname, "n_rows": R, "reps": reps,
                          "launches_per_rep": launches, "masked_out_bytes": 512 * R * eb, "unmasked_out_bytes": 64 * R * eb,
                          "masked_ms_per_launch": a, "masked_ms_min_max": amm, "unmasked_ms_per_launch": b,
                          "unmasked_ms_min_max": bmm, "masked_GBps_written": 512 * R * eb / (a * 1e-3) / 1e9,
                          "unmasked_GBps_written": 64 * R * eb / (b * 1e-3) / 1e9}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["rows", "gather"])
    ap.add_argument("--models", nargs="+", default=["alarm", "ising12x12"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    ap.add_argument("--ns", nargs="+", type=int, default=[1 << 10, 1 << 16])
    ap.add_argument("--fracs", nargs="+", type=float, default=[0.1, 0.3])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20, help="gather: launches between two synchronises")
    a = ap.parse_args()
    for dname in a.dtypes:
        if a.mode == "gather":
            gather_mode(dname, a.ns, a.reps, a.launches)
        else:
            for name in a.models:
                rows_mode(name, dname, a.ns, a.fracs, a.reps)


if __name__ == "__main__":
    main()
