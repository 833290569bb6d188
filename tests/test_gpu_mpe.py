"""GPU tests of MPE: the max kernels one bucket at a time (bnpp_bucket_max,
max_catalogue.py), the tie rule, the tile loop, and whole bnpp.mpe runs against
the numpy reference (mpe_ref.py).

  * single ops: values bit-identical and args identical to the numpy
    restatement of the kernels' loop (max_catalogue.restate) in the dtype of
    the run; the output and the arg table sit inside guard bands that stay
    untouched.  bnpp_bucket_max takes whole tables, so the view at an offset is
    a table address moved past the slices of a conditioned slowest variable;
    conditioned views with a stride run in the whole-model cases with evidence.
  * whole runs on the small models: brute force in fp64 finds one maximiser
    with a log gap > 1e-3 to the runner-up (asserted first), so the assignment
    must equal it in both dtypes.
  * larger models: by score (tie-safe): the fp64 log-score of the returned
    assignment is within 1e-9 (fp64) / 1e-4 (fp32) of the reference's maximum
    and equals the engine's own value.
  * log10 of the value: 1e-12 (fp64) / 1e-6 (fp32) relative to
    max(1, |log10 value|), the form the project's log10 Z checks take
    (test_gpu_parity.py).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import bnpp
import max_catalogue as mc
import mpe_ref
from bnpp import synth
from conftest import GOLDEN, evidence_of, model_path

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"f64": torch.float64, "f32": torch.float32}
ND = {"f64": np.float64, "f32": np.float32}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
LOG10_TOL = {"f64": 1e-12, "f32": 1e-6}
SCORE_TOL = {"f64": 1e-9, "f32": 1e-4}
GUARD = 64
LN10 = math.log(10.0)
SMALL = [("ising4x4", "-"), ("grid3x3", "-"), ("grid3x3", "grid3x3-PR.uai.evid"), ("asia", "-"),
         ("asia", "asia.uai.evid"), ("cancer", "-"), ("cancer", "cancer.uai.evid"), ("earthquake", "-"),
         ("earthquake", "earthquake.uai.evid")]


@pytest.fixture(scope="module")
def entries():
    return mc.load()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "mpe_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def stream():
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    return s.cuda_stream


@pytest.fixture
def grid_cap(ctx):
    yield ctx.set_max_grid
    ctx.set_max_grid(0)


def _run_max(ctx, stream, e, dt, ins, with_arg=True, tabs=None, scopes=None):
    """One bnpp_bucket_max call inside guard bands -> (values, args)."""
    n = mc.size_of(e["cards"], e["out"])
    if tabs is None:
        tabs = [torch.tensor(v, dtype=TD[dt], device=DEV) for v in ins]
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=TD[dt], device=DEV)
    abuf = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    out, arg = buf[GUARD:GUARD + n], abuf[GUARD:GUARD + n]
    bnpp.bucket_max(ctx, DT[dt], e["cards"], [t.data_ptr() for t in tabs], scopes or e["scopes"], e["elim"],
                    out.data_ptr(), e["out"], out_arg=arg.data_ptr() if with_arg else None, stream=stream)
    torch.cuda.synchronize()
    got, agot = buf.cpu().numpy(), abuf.cpu().numpy()
    assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + n:]).all(), ("value guard band written", e)
    assert (agot[:GUARD] == 0xAB).all() and (agot[GUARD + n:] == 0xAB).all(), ("arg guard band written", e)
    assert not np.isnan(got[GUARD:GUARD + n]).any(), ("output entry not written", e)
    return got[GUARD:GUARD + n], agot[GUARD:GUARD + n]


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_single_op_catalogue(ctx, entries, stream, monkeypatch, dt):
    sel = [(i, e) for i, e in enumerate(entries) if e["dtype"] == dt]
    assert sel
    for i, e in sel:
        ins = mc.make_inputs(e, i)
        want, want_arg = mc.restate(e, ins, ND[dt])
        monkeypatch.setenv("BNPP_NO_O32", "1" if e["no_o32"] else "0")
        info = bnpp.plan_max_single(DT[dt], e["cards"], e["scopes"], e["elim"], e["out"])
        assert info["key"] == e["key"], (e, info)
        vals, args = _run_max(ctx, stream, e, dt, ins)
        assert np.array_equal(vals, want), (e["name"], int((vals != want).sum()))
        assert np.array_equal(args, want_arg), (e["name"], int((args != want_arg).sum()))
        if e["name"] == "k1_copy":
            assert not args.any()
        if e["name"] == "card256":
            assert args.max() > 127                      # the byte is unsigned
        if e["name"].endswith("_a"):                     # values only: a null arg table
            vals2, args2 = _run_max(ctx, stream, e, dt, ins, with_arg=False)
            assert np.array_equal(vals2, want) and (args2 == 0xAB).all()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_single_op_view_at_an_offset(ctx, stream, monkeypatch, dt):
    """Variable 4, slowest in two inputs, conditioned on value 2: the tables'
    addresses move past two slices (a view's base offset; the slices are
    multiples of 16 B here, so the 4x1 tile's vector loads stay aligned: the
    planner sees the natural view of the slice, the address is the caller's)."""
    monkeypatch.setenv("BNPP_NO_O32", "0")
    cards = [3, 5, 6, 4, 3]
    full_scopes = [[4, 0, 1, 2, 3], [4, 3, 0], [2, 1]]
    scopes = [[0, 1, 2, 3], [3, 0], [2, 1]]
    e = {"cards": cards, "scopes": scopes, "elim": 0, "out": [1, 2, 3], "name": "offset"}
    full = mc.make_inputs({"cards": cards, "scopes": full_scopes}, 77)
    sl = [mc.size_of(cards, s) for s in scopes]
    ins = [full[0][2 * sl[0]:3 * sl[0]], full[1][2 * sl[1]:3 * sl[1]], full[2]]
    want, want_arg = mc.restate(e, ins, ND[dt])
    big = [torch.tensor(v, dtype=TD[dt], device=DEV) for v in full]
    tabs = [big[0][2 * sl[0]:], big[1][2 * sl[1]:], big[2]]
    vals, args = _run_max(ctx, stream, e, dt, None, tabs=tabs)
    assert np.array_equal(vals, want) and np.array_equal(args, want_arg)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_ties_keep_the_lowest_value(ctx, entries, stream, monkeypatch, dt):
    """Inputs from {0, 0.5, 1}: products are exact and many values of the
    maximised variable tie (all-zero rows included); the arg is the lowest
    maximiser, computed here directly from the products."""
    done = 0
    for i, e in enumerate(entries):
        if e["dtype"] != dt or not e["name"].endswith(("_a", "_b")) or e["no_o32"]:
            continue
        ins = mc.make_inputs(e, i, ties=True)
        monkeypatch.setenv("BNPP_NO_O32", "0")
        vals, args = _run_max(ctx, stream, e, dt, ins)
        # all products per value, then numpy's argmax (the first maximum)
        k = e["k"]
        prods = []
        for v in range(k):
            one = dict(e, scopes=[[x for x in s if x != e["elim"]] for s in e["scopes"]], elim=-1)
            sl = []
            for s, t in zip(e["scopes"], ins):
                a = t.reshape([e["cards"][x] for x in s])
                sl.append(np.take(a, v, axis=s.index(e["elim"])).reshape(-1) if e["elim"] in s else t)
            prods.append(mc.restate(one, sl, np.float64)[0])
        prods = np.stack(prods)
        assert np.array_equal(args, np.argmax(prods, axis=0).astype(np.uint8)), e["name"]
        assert np.array_equal(vals.astype(np.float64), prods.max(axis=0)), e["name"]
        ties = (prods == prods.max(axis=0)).sum(axis=0)
        assert (ties > 1).mean() > 0.2 and (prods.max(axis=0) == 0).any(), e["name"]
        done += 1
    assert done == 24


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_tile_loop_under_a_capped_grid(ctx, entries, stream, monkeypatch, grid_cap, dt):
    """The largest case of each key again with at most 1, 2 and 3 workgroups:
    the persistent loops then walk every virtual block; results identical."""
    by_key = {}
    for i, e in enumerate(entries):
        if e["dtype"] == dt and (e["key"] not in by_key or e["n_tiles"] > by_key[e["key"]][1]["n_tiles"]):
            by_key[e["key"]] = (i, e)
    assert len(by_key) == 24
    for i, e in by_key.values():
        assert e["n_tiles"] > 3 * 256
        ins = mc.make_inputs(e, i)
        want, want_arg = mc.restate(e, ins, ND[dt])
        monkeypatch.setenv("BNPP_NO_O32", "1" if e["no_o32"] else "0")
        for cap in (1, 2, 3):
            grid_cap(cap)
            vals, args = _run_max(ctx, stream, e, dt, ins)
            assert np.array_equal(vals, want) and np.array_equal(args, want_arg), (e["name"], cap)


def _check_value(dt, lv, score):
    assert abs(lv - score / LN10) <= LOG10_TOL[dt] * max(1.0, abs(score / LN10)), (lv, score / LN10)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name,evf", SMALL)
def test_small_models_against_brute_force(ctx, name, evf, dt):
    m = synth.read_uai(model_path(name + ".uai"))
    ev = evidence_of(evf)
    top, want, gap = mpe_ref.brute_force(m, ev)
    assert gap > 1e-3
    lv, x, _ = bnpp.mpe(ctx, bnpp.Model.load(model_path(name + ".uai")), ev, dtype=DT[dt])
    assert x == want
    _check_value(dt, lv, top)
    # a prepared job gives the same
    job = bnpp.Job(ctx, bnpp.Model.load(model_path(name + ".uai")), "mpe", ev, dtype=DT[dt])
    job.launch()
    lv2, x2 = job.results()
    job.close()
    assert (lv2, x2) == (lv, x)


def _check_by_score(dt, m, ev, rec, lv, x):
    assert len(x) == len(m["cards"]) and all(0 <= x[v] < m["cards"][v] for v in range(len(x)))
    assert all(x[v] == val for v, val in ev.items())
    score = mpe_ref.log_score(m, x)
    assert abs(score - rec["log_max"]) <= SCORE_TOL[dt], (score, rec["log_max"])
    _check_value(dt, lv, score)                           # a wrong traceback shows here without any reference


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["alarm", "Munin1", "potts4x5k3", "ising12x12", "noisyor_50_80"])
def test_larger_models_by_score(ctx, golden, name, dt):
    rec = golden[name]
    m = synth.read_uai(model_path(name + ".uai"))
    ev = evidence_of(rec["evidence"]) if rec["evidence"] else {}
    lv, x, _ = bnpp.mpe(ctx, bnpp.Model.load(model_path(name + ".uai")), ev, dtype=DT[dt])
    _check_by_score(dt, m, ev, rec, lv, x)


def test_scaling_keeps_fp32_finite(ctx, golden):
    """ising12x32: the maximum is e^367, far above fp32's range, so the fp32
    run is finite only through the power-of-two rescaling of the messages."""
    rec = golden["ising12x32"]
    assert rec["log_max"] > math.log(float(np.finfo(np.float32).max))
    m = synth.read_uai(model_path("ising12x32.uai"))
    lv, x, _ = bnpp.mpe(ctx, bnpp.Model.load(model_path("ising12x32.uai")), dtype=bnpp.F32)
    assert math.isfinite(lv)
    _check_by_score("f32", m, {}, rec, lv, x)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_relaunch_of_the_cached_job(golden, dt):
    """A second identical call relaunches the cached job (no planning, same
    result); a partition on the same model and context is its own job and
    returns the Z it returned before the MPE calls."""
    c = bnpp.Context(0)
    try:
        mm = bnpp.Model.load(model_path("alarm.uai"))
        ev = evidence_of("alarm.uai.evid")
        lz0 = bnpp.partition(c, mm, ev, dtype=DT[dt])[0]
        first = bnpp.mpe(c, mm, ev, dtype=DT[dt])
        t1 = bnpp.last_timing()
        assert t1["plan_ms"] > 0
        second = bnpp.mpe(c, mm, ev, dtype=DT[dt])
        t2 = bnpp.last_timing()
        assert t2["plan_ms"] == 0 and t2["upload_ms"] == 0 and t2["program_ms"] == 0 and t2["arena_reused"] == 1
        assert second[:2] == first[:2]
        assert bnpp.partition(c, mm, ev, dtype=DT[dt])[0] == lz0
        assert bnpp.last_timing()["plan_ms"] > 0         # never the MPE job
        assert bnpp.mpe(c, mm, ev, dtype=DT[dt])[:2] == first[:2]
        assert all(first[1][v] == val for v, val in ev.items())
    finally:
        c.close()


@pytest.mark.parametrize("flags", [[], ["-f32"]])
def test_cli_writes_the_mpe_file(ctx, tmp_path, flags):
    """bin/bnpp model.uai evid -mpe -uai base (the C++ mirror's Model::mpe):
    base.MPE is "MPE", then "N x_0 .. x_{N-1}", the assignment bnpp.mpe returns;
    stdout carries log10 of the value and the same assignment."""
    import subprocess
    from conftest import REPO
    exe = os.path.join(REPO, "bn-pp_amd", "bin", "bnpp")
    base = str(tmp_path / "asia")
    ev = evidence_of("asia.uai.evid")
    r = subprocess.run([exe, model_path("asia.uai"), model_path("asia.uai.evid"), "-mpe", "-uai", base] + flags,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lv, x, _ = bnpp.mpe(ctx, bnpp.Model.load(model_path("asia.uai")), ev, dtype=bnpp.F32 if flags else bnpp.F64)
    with open(base + ".MPE") as f:
        assert f.read() == "MPE\n%d %s\n" % (len(x), " ".join(str(v) for v in x))
    assert ">> MPE assignment: " + " ".join(str(v) for v in x) + "\n" in r.stdout
    got = float(r.stdout.split(">> MPE log10 value = ")[1].split()[0])
    assert abs(got - lv) <= 1e-5 * max(1.0, abs(lv))     # printed with six significant digits
    assert not os.path.exists(base + ".PR") and not os.path.exists(base + ".MAR")
