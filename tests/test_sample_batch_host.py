"""CPU tests of batched sampling's host side: the plan of one launch
(bnpp_plan_sample_batch: gather steps, the unfused forward pass, draw rows with
and without the row variable, one draw step), the argument checks of
bnpp_sample_batch (made before a device is looked at), the card limits, the
compile check of the draw kernel, and the numpy restatement
(sample_batch_ref.py) under the statistical bound for the very inputs the GPU
distribution test uses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_ref
import bnpp
import sample_batch_ref as sbr
import sample_ref
from bnpp import synth
from conftest import REPO, model_path

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
SAMPLE_BATCH_KEY = (1 << 24) + 24576
# the evidence sets of tests/test_gpu_batch.py; alarm takes the scope of its first CPT with a zero entry
EV_VARS = {"cancer": [0, 3], "ising6x6": [0, 7, 20, 35]}
MODELS = ("alarm", "cancer", "ising6x6")


def _zero_scope(d):
    for s, v in zip(d["scopes"], d["values"]):
        if 2 <= len(s) <= 4 and (np.asarray(v) == 0).any():
            return sorted(s)
    raise AssertionError("no zero entry")


@pytest.fixture(scope="module")
def models():
    out = {}
    for name in MODELS:
        path = model_path(name + ".uai")
        d = synth.read_uai(path)
        out[name] = (bnpp.Model.load(path), d, EV_VARS.get(name) or _zero_scope(d))
    return out


def test_symbols_are_exported():
    for name in ("bnpp_sample_batch", "bnpp_plan_sample_batch"):
        assert name in bnpp.EXPORTED and hasattr(bnpp._lib, name)
    assert bnpp.SAMPLE_BATCH_KEY == SAMPLE_BATCH_KEY
    assert bnpp.ABI_VERSION == 205 and bnpp._lib.bnpp_version() == 205


def _sum_key(k):
    """An ordinary sum-plan key: generic (< 2048), stream (4096 ..) or slab (16384 .. 32767), never a
    chain run (8192 .. 16383), a max bucket (65536 ..) or an executor step (test_sample_host.py)."""
    return k < 8192 or 16384 <= k < 32768


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", MODELS)
def test_plan_of_one_launch(models, name, dt):
    m, _, ev = models[name]
    R, K = 64, 3
    st, groups = bnpp.plan_sample_batch(m, ev, K, dtype=DT[dt], rows_per_launch=R)
    assert st["rows_per_launch"] == R and st["n_per_row"] == K
    # as many gather steps as plan_batch, all at level 0
    bst, _, _ = bnpp.plan_batch(m, ev, dtype=DT[dt], rows_per_launch=R)
    gathers = [g for g in groups if g["key"] == bnpp.COND_BATCH_KEY]
    assert len(gathers) == st["gather_steps"] == bst["gather_steps"] > 0
    assert all(g["level"] == 0 and g["n_desc"] == 1 for g in gathers)
    # as many draw rows as plan_sample for the same evidence variables: one per free variable
    sst, _ = bnpp.plan_sample(m, 1, {v: 0 for v in ev}, dtype=DT[dt])
    assert st["draw_rows"] == sst["sample_rows"] == m.n_vars - len(ev)
    assert st["draw_rows"] == st["draw_rows_b"] + st["draw_rows_no_b"]
    # exactly one draw step, the last group; every other key a sum, product or gather key
    assert [g["key"] for g in groups].count(SAMPLE_BATCH_KEY) == 1 and groups[-1]["key"] == SAMPLE_BATCH_KEY
    assert groups[-1]["level"] == max(g["level"] for g in groups) and groups[-1]["n_desc"] == 1
    assert all(g["level"] < groups[-1]["level"] for g in groups[:-1])
    for g in groups[:-1]:
        assert _sum_key(g["key"]) or g["key"] == bnpp.COND_BATCH_KEY, g
    # the state is a table of the plan: the arena counts it
    assert st["state_bytes"] == m.n_vars * R * K
    assert st["arena_bytes"] >= st["state_bytes"] + 8 * R
    st2, _ = bnpp.plan_sample_batch(m, ev, 1024 + K, dtype=DT[dt], rows_per_launch=R)
    assert st2["state_bytes"] == m.n_vars * R * (1024 + K)
    assert st2["arena_bytes"] >= st2["state_bytes"] + 8 * R and st2["arena_bytes"] > st["arena_bytes"]


def test_alarm_has_draw_rows_with_and_without_the_row_variable(models):
    """Evidence reaches only part of alarm: the draw step reads inputs with a
    stride of B and rows none of whose inputs has one."""
    m, _, ev = models["alarm"]
    st, _ = bnpp.plan_sample_batch(m, ev, 2, rows_per_launch=64)
    assert st["draw_rows_b"] > 0 and st["draw_rows_no_b"] > 0


def test_same_plan_for_heuristic_and_given_order(models):
    m, _, ev = models["alarm"]
    order, _ = bnpp.ordering(m, {v: 0 for v in ev}, "mf")
    assert (bnpp.plan_sample_batch(m, ev, 4, rows_per_launch=16) ==
            bnpp.plan_sample_batch(m, ev, 4, rows_per_launch=16, order=order))
    with pytest.raises(bnpp.BnppError) as e:                # a sampling order covers every free variable
        bnpp.plan_sample_batch(m, ev, 4, rows_per_launch=16, order=order[:-1])
    assert e.value.status == bnpp.ERR_INVALID


def test_automatic_rows_shrink_with_k_and_fit_the_budget(models, monkeypatch):
    m, _, ev = models["alarm"]
    monkeypatch.setenv("BNPP_MEM_BUDGET_GB", "1e-3")
    rs = []
    for K in (1, 16, 256):
        st, _ = bnpp.plan_sample_batch(m, ev, K)
        r = int(st["rows_per_launch"])
        assert 1 <= r < 1 << 16 and r & (r - 1) == 0 and st["arena_bytes"] <= 1e6, (K, r, st["arena_bytes"])
        assert st["state_bytes"] == m.n_vars * r * K
        rs.append(r)
    assert rs[0] > rs[1] > rs[2], rs
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_sample_batch(m, ev, 256, rows_per_launch=2 * rs[2])
    assert e.value.status == bnpp.ERR_OOM
    assert "messages" in str(e.value) and "state" in str(e.value) and "%d rows per launch" % (2 * rs[2]) in str(e.value)
    # even one row is over budget: both sizes are named
    monkeypatch.setenv("BNPP_MEM_BUDGET_GB", "1e-6")
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_sample_batch(m, ev, 256)
    msg = str(e.value)
    assert e.value.status == bnpp.ERR_OOM and "1 row per launch" in msg
    assert re.search(r"messages \d+ bytes", msg) and "state %d bytes" % (m.n_vars * 256) in msg, msg


def test_card_limits_of_sampled_and_evidence_variables():
    for card, ok in ((256, True), (257, False)):
        vals = [1.0 + (i % 7) for i in range(card * 2)] + [0.5, 0.25]
        m = bnpp.Model.from_arrays([card, 2], [[0, 1], [1]], vals)
        for dt in DT.values():
            for ev in ([1], [0]):                           # the wide variable sampled, then observed: `out` is bytes
                if ok:
                    assert bnpp.plan_sample_batch(m, ev, 2, dtype=dt, rows_per_launch=8)[1][-1]["key"] == SAMPLE_BATCH_KEY
                else:
                    with pytest.raises(bnpp.BnppError) as e:
                        bnpp.plan_sample_batch(m, ev, 2, dtype=dt, rows_per_launch=8)
                    assert e.value.status == bnpp.ERR_UNSUPPORTED and "257" in str(e.value), str(e.value)
                    assert ("evidence variable 0" in str(e.value)) == (ev == [0])


def _sample_batch_raw(m, ev_vars, rows, k=2, first=0, stride=2):
    """bnpp_sample_batch with a NULL context: the arguments are checked first."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.intc).reshape(-1, max(len(ev_vars), 1))[:, :len(ev_vars)])
    n = len(rows)
    out = np.zeros(max(n, 1) * max(k, 1) * m.n_vars, dtype=np.uint8)
    IP = C.POINTER(C.c_int)
    vs = (C.c_int * max(len(ev_vars), 1))(*ev_vars)
    rc = bnpp._lib.bnpp_sample_batch(None, m.handle, len(ev_vars), vs, n, rows.ctypes.data_as(IP), bnpp.HEURISTICS["mf"],
                                     None, 0, bnpp.F64, 0, k, first, stride, 0, C.c_void_p(out.ctypes.data), None, None, None)
    return rc, bnpp._lib.bnpp_last_error().decode()


def test_invalid_arguments(models):
    m, d, _ = models["alarm"]
    ev = [3, 10, 20]
    good = batch_ref.draw_rows(d["cards"], ev, 5, 1)
    # a valid call passes the argument checks and fails at the context: without a GPU the entry
    # itself reports that there is no device
    for kw in ({}, {"stride": 0}, {"first": 2 ** 63 - 1 - 4 * 2 - 2}):
        rc, msg = _sample_batch_raw(m, ev, good, **kw)
        if bnpp.device_count() == 0:
            assert rc == bnpp.ERR_NO_DEVICE and "device" in msg, (kw, msg)
        else:
            assert rc == bnpp.ERR_INVALID and "context" in msg, (kw, msg)
    rc, msg = _sample_batch_raw(m, ev, good, k=0)
    assert rc == bnpp.ERR_INVALID and "n_per_row" in msg
    rc, msg = _sample_batch_raw(m, ev, good, stride=-1)
    assert rc == bnpp.ERR_INVALID and "row_stride" in msg
    # first_sample + (n_rows - 1) * row_stride + K past int64: in the sum, and in the product alone
    for kw in ({"first": 2 ** 63 - 1 - 4 * 2 - 1}, {"stride": 2 ** 62}):
        rc, msg = _sample_batch_raw(m, ev, good, **kw)
        assert rc == bnpp.ERR_INVALID and "overflows" in msg, (kw, msg)
    rc, msg = _sample_batch_raw(m, ev, np.zeros((0, 3)))
    assert rc == bnpp.ERR_INVALID and "n_rows" in msg
    rc, msg = _sample_batch_raw(m, [3, 10, 3], np.zeros((2, 3)))
    assert rc == bnpp.ERR_INVALID and "twice" in msg and "3" in msg
    for bad in (-1, m.n_vars):
        rc, msg = _sample_batch_raw(m, [3, bad], np.zeros((2, 2)))
        assert rc == bnpp.ERR_INVALID and "out of range" in msg and str(bad) in msg
    for row, col, val in ((3, 1, 1 << 20), (0, 0, -1), (4, 2, d["cards"][ev[2]])):
        rows = good.copy()
        rows[row, col] = val
        rc, msg = _sample_batch_raw(m, ev, rows)
        assert rc == bnpp.ERR_INVALID, msg
        assert "row %d" % row in msg and "variable %d" % ev[col] in msg and str(val) in msg, msg
    for bad_k in (0, -3):
        with pytest.raises(bnpp.BnppError) as e:
            bnpp.plan_sample_batch(m, ev, bad_k)
        assert e.value.status == bnpp.ERR_INVALID
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_sample_batch(m, [3, 3], 2)
    assert e.value.status == bnpp.ERR_INVALID


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_draw_kernel_uses_no_scratch(tmp_path, dt):
    """The compile check: each unit that instantiates sample_rows_batch_kernel,
    for gfx950 with the flags of the other units: once per dtype, 0 bytes of
    scratch."""
    src = os.path.join(REPO, "bn-pp_amd", "csrc")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + src,
                        "-I" + os.path.join(REPO, "include"), "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(src, "k_sample_%s.hip" % dt), "-o", str(tmp_path / "k.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", p.stderr, flags=re.S)
    mine = [(n, int(s)) for n, s in blocks if "sample_rows_batch_kernel" in n]
    assert len(mine) == 1, [n for n, _ in blocks]           # instantiated once
    assert mine[0][1] == 0, p.stderr


@pytest.mark.parametrize("name", sbr.DIST_MODELS)
def test_reference_meets_the_bound_on_the_distribution_inputs(name):
    """The restatement alone, for the exact rows, K, stride and seed of
    test_gpu_sample_batch.py's distribution test: were a frequency of this
    reference outside sample_ref.bound, that test would fail on the
    reference's own noise."""
    path = model_path(name + ".uai")
    d = synth.read_uai(path)
    ev_vars, rows = sbr.dist_case(d)
    assert len(rows) == 8 and len({tuple(r) for r in rows.tolist()}) == 8
    order, _ = bnpp.ordering(bnpp.Model.load(path), {v: 0 for v in ev_vars}, "mf")
    x, deg = sbr.run(d, ev_vars, rows, order, sbr.DIST_K, sbr.DIST_SEED, sbr.DIST_FIRST, sbr.DIST_K)
    assert not deg.any() and np.array_equal(x[:, :, ev_vars], np.broadcast_to(rows[:, None, :], (8, sbr.DIST_K, 3)))
    bad = sbr.frequency_violations(d, ev_vars, rows, x)
    assert not bad, bad[:3]
    # common random numbers: equal rows give equal samples, and a row's samples are sample_ref.run's at first + s
    x0, _ = sbr.run(d, ev_vars, rows[[2, 5, 2]], order, 64, sbr.DIST_SEED, 7, 0)
    assert np.array_equal(x0[0], x0[2]) and not np.array_equal(x0[0], x0[1])


def test_reference_gives_an_impossible_row_degenerate_zeros():
    """The contract's rule for Z = 0 in the restatement: zeros beside the
    evidence and every draw counted, also where the zero entry's CPT is wholly
    observed and enters no bucket (asia's deterministic CPT); its neighbours
    are sample_ref.run's."""
    path = model_path("asia.uai")
    d = synth.read_uai(path)
    ev_vars = _zero_scope(d)
    scope, vals = next((s, v) for s, v in zip(d["scopes"], d["values"]) if sorted(s) == ev_vars)
    idx = np.unravel_index(int(np.flatnonzero(np.asarray(vals) == 0)[0]), [d["cards"][v] for v in scope])
    bad = [int(idx[scope.index(v)]) for v in ev_vars]
    order, _ = bnpp.ordering(bnpp.Model.load(path), {v: 0 for v in ev_vars}, "mf")
    ok = next(r for r in ([0, 0, 0], [1, 1, 1], [0, 1, 1]) if sbr.partition(d, dict(zip(ev_vars, r)), order) > 0)
    x, deg = sbr.run(d, ev_vars, [ok, bad, ok], order, 4, 9, 2, 4)
    free = [v for v in range(len(d["cards"])) if v not in ev_vars]
    assert sbr.partition(d, dict(zip(ev_vars, bad)), order) == 0
    assert not x[1][:, free].any() and (x[1][:, ev_vars] == bad).all() and deg[1] == 4 * len(free)
    for b in (0, 2):
        want, wdeg = sample_ref.run(d, dict(zip(ev_vars, ok)), order, 4, 9, np.float64, first=2 + b * 4)
        assert np.array_equal(x[b], want) and deg[b] == wdeg == 0
