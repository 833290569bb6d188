#!/usr/bin/env python3
"""Soft evidence in batched calls: what the weights cost.  One JSON line per case.

rows    partition_batch with soft=(the evidence variables of the case, random
        likelihoods) against
        (a) what a caller did before: per row a model with the likelihoods as
            one more unary factor each, uploaded, and the single call, planning
            included -- a loop over 64 of the rows, scaled to the row count;
        (b) the floor: the _mv call over the same rows with the same variables
            declared partial and all missing -- the same plan shape, no
            likelihood traffic -- so soft / (b) is what the weights cost;
        and the host's share: staging, scaling and transposition of lik, from
        the engine's own clock (the line BNPP_TIMING prints, read back from
        stderr of one more call).
gather  the weighted gather step alone beside the masked step on the same
        source, the (p = 8, free = 64, hard = 4) case of tools/missing_bench.py:
        the dim of card 8 soft instead of partial, in bytes written per second.

Method as the other benches: warm, medians of `reps` repetitions, one process.

    python tools/soft_bench.py rows --models alarm ising12x12 >> profiles/soft_bench.jsonl
    python tools/soft_bench.py rows --models noisyor_50_80 --ns 64 >> profiles/soft_bench.jsonl
    python tools/soft_bench.py gather >> profiles/soft_bench.jsonl
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
# the soft variables; None: the variables of the model's .evid file (tools/batch_bench.py's)
SOFT_VARS = {"alarm": [3, 10, 20], "ising12x12": [0, 50, 100, 143], "noisyor_50_80": None}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}


def med(ts):
    return statistics.median(ts), [min(ts), max(ts)]


def clock(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def staging_ms(call):
    """The engine's own clock for the staging of lik: one call under BNPP_TIMING, its stderr line parsed."""
    import re
    import tempfile
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
    found = re.findall(r"soft evidence: staging ([0-9.]+) ms", text)
    return float(found[-1]) if found else None


def with_unary(d, soft, lik_row):
    """The model with the row's likelihoods as one more unary factor per soft variable."""
    scopes, values, at = list(d["scopes"]), list(d["values"]), 0
    for v in soft:
        k = d["cards"][v]
        scopes.append([v])
        values.append([float(x) for x in lik_row[at:at + k]])
        at += k
    return dict(d, scopes=scopes, values=values)


def rows_mode(name, dname, ns, reps):
    path = os.path.join(MODELS, name + ".uai")
    m, d = bnpp.Model.load(path), synth.read_uai(path)
    soft = SOFT_VARS[name]
    if soft is None:
        soft = sorted(synth.read_evidence(os.path.join(MODELS, name + ".uai.evid")))
    dt = DT[dname]
    ws = sum(d["cards"][v] for v in soft)
    cs, cb, ca = bnpp.Context(0), bnpp.Context(0), bnpp.Context(0)
    rng = np.random.default_rng(17)
    for n in ns:
        lik = np.exp2(rng.uniform(-20, 0, (n, ws)))
        none = np.zeros((n, 0), dtype=np.int64)
        missing = np.full((n, len(soft)), bnpp.MISSING)
        n_loop = min(n, 64)

        def before():
            out = []
            for b in range(n_loop):
                out.append(bnpp.partition(ca, bnpp.Model.from_dict(with_unary(d, soft, lik[b])), None, dtype=dt)[0])
            return np.array(out)

        lz, _, _ = bnpp.partition_batch(cs, m, [], none, dtype=dt, soft=(soft, lik))          # warm-up, all sides
        bnpp.partition_batch(cb, m, soft, missing, dtype=dt, partial=soft)
        lza = before()
        worst = float(np.max(np.abs(lz[:n_loop] - lza) / np.maximum(1.0, np.abs(lza))))
        ts, tb, ta = [], [], []
        for _ in range(reps):
            ts.append(clock(lambda: bnpp.partition_batch(cs, m, [], none, dtype=dt, soft=(soft, lik))))
            tb.append(clock(lambda: bnpp.partition_batch(cb, m, soft, missing, dtype=dt, partial=soft)))
        for _ in range(min(reps, 3)):
            ta.append(clock(before) * n / n_loop)
        stage = [staging_ms(lambda: bnpp.partition_batch(cs, m, [], none, dtype=dt, soft=(soft, lik))) for _ in range(3)]
        sp = bnpp.plan_batch(m, [], dtype=dt, soft=soft)
        rec = {"mode": "rows", "case": name + " " + dname, "n_rows": n, "n_soft": len(soft), "Ws": ws, "reps": reps,
               "lik_bytes": n * ws * 8, "width": sp[0]["width"], "gather_steps": sp[0]["gather_steps"],
               "rows_per_launch": sp[0]["rows_per_launch"], "before_rows_timed": n_loop,
               "worst_rel_log10_z_soft_vs_before": worst}
        for key, t in (("soft", ts), ("floor_all_missing", tb), ("before_scaled_to_n", ta)):
            rec[key + "_ms"], rec[key + "_ms_min_max"] = med(t)
        rec["host_staging_ms"] = statistics.median(stage) if None not in stage else None
        rec["host_staging_share_of_soft"] = rec["host_staging_ms"] / rec["soft_ms"] if rec["host_staging_ms"] is not None else None
        rec["before_over_soft"] = rec["before_scaled_to_n_ms"] / rec["soft_ms"]
        rec["soft_over_floor"] = rec["soft_ms"] / rec["floor_all_missing_ms"]
        rec["soft_minus_floor_ms"] = rec["soft_ms"] - rec["floor_all_missing_ms"]
        print(json.dumps(rec), flush=True)
    for c in (cs, cb, ca):
        c.close()


def gather_mode(dname, Rs, reps, launches):
    import torch
    td = torch.float64 if dname == "f64" else torch.float32
    cards, scope = [8, 64, 4], [0, 1, 2]                        # (p or s, free, hard): 2048 entries, rest 512
    ctx = bnpp.Context(0)
    rng = np.random.default_rng(5)
    src = torch.tensor(rng.uniform(0.05, 1.0, 2048), dtype=td, device="cuda")
    for R in Rs:
        ev = np.stack([rng.integers(0, cards[v], R) for v in (0, 2)]).astype(np.int32)
        ev[0][rng.random(R) < 0.33] = bnpp.MISSING
        t_evm = torch.tensor(ev.reshape(-1), dtype=torch.int32, device="cuda")
        t_evh = torch.tensor(ev[1].reshape(-1), dtype=torch.int32, device="cuda")
        lam = torch.tensor(np.exp2(rng.uniform(-20, 0, (8, R))).reshape(-1), dtype=td, device="cuda")
        out = torch.zeros(512 * R, dtype=td, device="cuda")

        def run(weighted):
            for _ in range(launches):
                if weighted:
                    bnpp.condition_batch(ctx, DT[dname], cards, src.data_ptr(), scope, [2], R, t_evh.data_ptr(),
                                         out.data_ptr(), soft=([0], lam.data_ptr()))
                else:
                    bnpp.condition_batch(ctx, DT[dname], cards, src.data_ptr(), scope, [0, 2], R, t_evm.data_ptr(),
                                         out.data_ptr(), partial=[0])
            torch.cuda.synchronize()

        run(True)
        run(False)
        tw, tm = [], []
        for _ in range(reps):
            tw.append(clock(lambda: run(True)) / launches)
            tm.append(clock(lambda: run(False)) / launches)
        eb = 8 if dname == "f64" else 4
        a, amm = med(tw)
        b, bmm = med(tm)
        print(json.dumps({"mode": "gather", "case": "(s=8, free=64, hard=4) " + dname, "n_rows": R, "reps": reps,
                          "launches_per_rep": launches, "out_bytes": 512 * R * eb, "lam_bytes": 8 * R * eb,
                          "weighted_ms_per_launch": a, "weighted_ms_min_max": amm, "masked_ms_per_launch": b,
                          "masked_ms_min_max": bmm, "weighted_GBps_written": 512 * R * eb / (a * 1e-3) / 1e9,
                          "masked_GBps_written": 512 * R * eb / (b * 1e-3) / 1e9, "weighted_over_masked": a / b}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["rows", "gather"])
    ap.add_argument("--models", nargs="+", default=["alarm", "ising12x12"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    ap.add_argument("--ns", nargs="+", type=int, default=[1 << 10, 1 << 16])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20, help="gather: launches between two synchronises")
    a = ap.parse_args()
    for dname in a.dtypes:
        if a.mode == "gather":
            gather_mode(dname, a.ns, a.reps, a.launches)
        else:
            for name in a.models:
                rows_mode(name, dname, a.ns, a.reps)


if __name__ == "__main__":
    main()
