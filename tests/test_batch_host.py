"""CPU tests of batched evidence: the plan of one launch (bnpp_plan_batch), the
argument checks of bnpp_partition_batch / bnpp_posterior_batch (made before a
device is looked at) and the multi-sample evidence loader."""
import ctypes as C
import re

import numpy as np
import pytest

import batch_ref
import bnpp
from bnpp import synth
from conftest import model_path

EV = [3, 10, 20]


@pytest.fixture(scope="module")
def alarm():
    return bnpp.Model.load(model_path("alarm.uai")), synth.read_uai(model_path("alarm.uai"))


@pytest.fixture
def budget(monkeypatch):
    return lambda gb: monkeypatch.setenv("BNPP_MEM_BUDGET_GB", repr(gb))


@pytest.mark.parametrize("target", [None, 5])
def test_plan_of_alarm(alarm, target):
    m, d = alarm
    touched = [s for s in d["scopes"] if set(s) & set(EV)]
    assert 0 < len(touched) < len(d["scopes"])
    st, groups, scope = bnpp.plan_batch(m, EV, target=target, rows_per_launch=64)
    gathers = [g for g in groups if g["key"] == bnpp.COND_BATCH_KEY]
    # one gather group per factor that mentions an evidence variable, all at level 0;
    # the sources evidence does not touch have none
    assert len(gathers) == len(touched) == st["gather_steps"]
    assert all(g["level"] == 0 and g["n_desc"] == 1 for g in gathers)
    assert all(g["level"] >= 1 for g in groups if g["key"] != bnpp.COND_BATCH_KEY)
    assert all(g["key"] < 8192 or g["key"] >= 16384 for g in groups if g["key"] != bnpp.COND_BATCH_KEY), "a chain key"
    assert st["rows_per_launch"] == 64
    B = m.n_vars
    assert scope == ([B] if target is None else [target, B])


def test_plan_levels_are_the_single_calls(alarm, monkeypatch):
    """The gathered tables take the place of the conditioned views: the plan has
    the levels and, beside the gather steps, the buckets of the single call's
    unfused plan for the same evidence variables."""
    m, _ = alarm
    st, groups, _ = bnpp.plan_batch(m, EV, rows_per_launch=4)
    monkeypatch.setenv("BNPP_NO_CHAIN", "1")
    single = bnpp.plan_stats(m, 0, {v: 0 for v in EV}, "mf", bnpp.F64)
    assert max(g["level"] for g in groups) == st["levels"] == single[2]
    assert st["buckets"] - st["gather_steps"] == single[3]
    assert st["width"] == single[4]


def test_no_evidence_has_no_gather_and_no_row_variable(alarm):
    m, _ = alarm
    st, groups, scope = bnpp.plan_batch(m, [], rows_per_launch=16)
    assert st["gather_steps"] == 0 and not [g for g in groups if g["key"] == bnpp.COND_BATCH_KEY]
    assert scope == []


@pytest.mark.parametrize("gb", [1e-3, 1e-4])
def test_automatic_rows_fit_the_budget(alarm, budget, gb):
    m, _ = alarm
    budget(gb)
    st, _, _ = bnpp.plan_batch(m, EV)
    r = int(st["rows_per_launch"])
    assert 1 <= r <= 1 << 16 and r & (r - 1) == 0
    assert st["arena_bytes"] <= gb * 1e9
    if r < 1 << 16:                       # the next power of two does not fit
        with pytest.raises(bnpp.BnppError) as e:
            bnpp.plan_batch(m, EV, rows_per_launch=2 * r)
        assert e.value.status == bnpp.ERR_OOM


def test_budget_too_small_for_one_row(alarm, budget):
    m, _ = alarm
    budget(1e-6)
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_batch(m, EV)
    assert e.value.status == bnpp.ERR_OOM
    sizes = re.findall(r"([0-9.]+) GB", str(e.value))
    assert len(sizes) == 2 and float(sizes[0]) > float(sizes[1]) > 0, str(e.value)
    assert "1 row per launch" in str(e.value)


def _partition_batch_raw(m, ev_vars, rows, target=None):
    """bnpp_partition_batch / bnpp_posterior_batch with a NULL context: the
    arguments are checked first, so every bad call fails as it would on a GPU."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.intc).reshape(-1, max(len(ev_vars), 1))[:, :len(ev_vars)])
    n = len(rows)
    out = np.zeros(max(n, 1) * 8)
    IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
    vs = (C.c_int * max(len(ev_vars), 1))(*ev_vars)
    if target is None:
        rc = bnpp._lib.bnpp_partition_batch(None, m.handle, len(ev_vars), vs, n, rows.ctypes.data_as(IP), bnpp.HEURISTICS["mf"],
                                            None, 0, bnpp.F64, 0, out.ctypes.data_as(DP), None, None)
    else:
        rc = bnpp._lib.bnpp_posterior_batch(None, m.handle, len(ev_vars), vs, n, rows.ctypes.data_as(IP),
                                            bnpp.HEURISTICS["mf"], target, bnpp.F64, 0, out.ctypes.data_as(DP), None)
    return rc, bnpp._lib.bnpp_last_error().decode()


def test_invalid_arguments(alarm):
    m, d = alarm
    good = batch_ref.draw_rows(d["cards"], EV, 5, 1)
    # a valid call reaches the context check and fails there, not before
    rc, msg = _partition_batch_raw(m, EV, good)
    assert rc == bnpp.ERR_INVALID and "context" in msg
    rc, msg = _partition_batch_raw(m, EV, np.zeros((0, 3)))
    assert rc == bnpp.ERR_INVALID and "n_rows" in msg
    rc, msg = _partition_batch_raw(m, [3, 10, 3], np.zeros((2, 3)))
    assert rc == bnpp.ERR_INVALID and "twice" in msg and "3" in msg
    for bad in (-1, m.n_vars):
        rc, msg = _partition_batch_raw(m, [3, bad], np.zeros((2, 2)))
        assert rc == bnpp.ERR_INVALID and "out of range" in msg and str(bad) in msg
    # an evidence value outside its variable's range, in any row: the row and the variable are named
    for row, col, val in ((0, 0, -1), (4, 2, d["cards"][EV[2]]), (3, 1, 1 << 20)):
        rows = good.copy()
        rows[row, col] = val
        rc, msg = _partition_batch_raw(m, EV, rows)
        assert rc == bnpp.ERR_INVALID, msg
        assert "row %d" % row in msg and "variable %d" % EV[col] in msg and str(val) in msg, msg
        rc, msg = _partition_batch_raw(m, EV, rows, target=5)
        assert rc == bnpp.ERR_INVALID and "row %d" % row in msg and "variable %d" % EV[col] in msg, msg
    # the target must exist and must not be an evidence variable
    rc, msg = _partition_batch_raw(m, EV, good, target=10)
    assert rc == bnpp.ERR_INVALID and "target" in msg and "evidence variable" in msg
    for bad in (-1, m.n_vars):
        rc, msg = _partition_batch_raw(m, EV, good, target=bad)
        assert rc == bnpp.ERR_INVALID and "target" in msg
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_batch(m, EV, target=10)
    assert e.value.status == bnpp.ERR_INVALID
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_batch(m, [3, 3])
    assert e.value.status == bnpp.ERR_INVALID


def test_no_limit_on_cardinalities():
    """Evidence values are int32: a variable of 1000 values plans and passes the value check."""
    vals = np.arange(1, 2001, dtype=float)
    m = bnpp.Model.from_arrays([1000, 2], [[0, 1]], [vals])
    st, groups, scope = bnpp.plan_batch(m, [0], rows_per_launch=8)
    assert st["gather_steps"] == 1 and scope == [2]
    rc, msg = _partition_batch_raw(m, [0], [[999], [300]])
    assert rc == bnpp.ERR_INVALID and "context" in msg
    rc, msg = _partition_batch_raw(m, [0], [[999], [1000]])
    assert rc == bnpp.ERR_INVALID and "row 1" in msg and "variable 0" in msg


def test_evidence_load_batch(tmp_path):
    one = tmp_path / "one.evid"
    one.write_text("1\n2 4 1 2 0\n")
    vs, rows = bnpp.load_evidence_batch(str(one))
    assert vs == [2, 4] and rows.tolist() == [[0, 1]]
    assert bnpp.load_evidence(str(one)) == {4: 1, 2: 0}
    three = tmp_path / "three.evid"
    three.write_text("3\n3 7 1 2 0 5 2\n3 2 1 5 0 7 0\n3 5 1 7 1 2 1\n")      # the variable order permuted per sample
    vs, rows = bnpp.load_evidence_batch(str(three))
    assert vs == [2, 5, 7] and rows.tolist() == [[0, 2, 1], [1, 0, 0], [1, 1, 1]]
    assert bnpp.load_evidence(str(three)) == {}, "the single-sample loader's answer changed"
    other = tmp_path / "other.evid"
    other.write_text("3\n2 1 0 2 0\n2 2 1 1 1\n2 1 0 3 1\n")
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.load_evidence_batch(str(other))
    assert e.value.status == bnpp.ERR_UNSUPPORTED and "sample 2" in str(e.value)
    short = tmp_path / "short.evid"
    short.write_text("2\n1 0 1\n1 0\n")
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.load_evidence_batch(str(short))
    assert e.value.status == bnpp.ERR_IO
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.load_evidence_batch(str(tmp_path / "missing.evid"))
    assert e.value.status == bnpp.ERR_IO
    none = tmp_path / "none.evid"
    none.write_text("2\n0\n0\n")
    vs, rows = bnpp.load_evidence_batch(str(none))
    assert vs == [] and rows.shape == (2, 0)


@pytest.mark.parametrize("unit", ["k_condb_f32.hip", "k_condb_f64.hip"])
def test_gather_kernels_use_no_scratch(unit, tmp_path):
    """The compile check of DESIGN 12: every gather kernel for gfx950 with zero
    bytes of scratch (its odometer and offsets stay in registers)."""
    import os
    import subprocess
    from conftest import REPO
    src = os.path.join(REPO, "bn-pp_amd", "csrc")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + src,
                        "-I" + os.path.join(REPO, "include"), "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(src, unit), "-o", str(tmp_path / "k.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    assert len(names) == 4 and all("cond_batch" in n for n in names), names      # V = 1 and wide, plan and single-op
    assert scratch == [0, 0, 0, 0], p.stderr


def test_gather_reference_on_a_known_table():
    cards = [3, 2, 4]
    src = np.arange(24.0)
    ev = np.array([[1, 0, 1, 1, 0]])
    out = batch_ref.gather(src, cards, [0, 1, 2], [1], ev).reshape(3, 4, 5)
    t = src.reshape(3, 2, 4)
    for b in range(5):
        assert np.array_equal(out[:, :, b], t[:, ev[0, b], :])
    out = batch_ref.gather(src, cards, [0, 1, 2], [2, 0, 1], np.array([[3, 0], [2, 1], [1, 0]]))
    assert out.tolist() == [t[2, 1, 3], t[1, 0, 0]]
    out = batch_ref.gather(src, cards, [0, 1, 2], [7], np.array([[0, 0, 0]])).reshape(24, 3)
    assert all(np.array_equal(out[:, b], src) for b in range(3))
