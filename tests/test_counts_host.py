"""CPU tests of expected counts: the exported symbols, the plan of one launch
(bnpp_plan_counts: a batched bucket tree), the argument checks of
bnpp_expected_counts (made before a device is looked at) and the M step."""
import ctypes as C

import numpy as np
import pytest

import bnpp
from bnpp import learn, synth
from conftest import model_path
from counts_ref import EV_VARS

PLAN_MODELS = ("asia", "alarm", "ising6x6")


def _load(name):
    return bnpp.Model.load(model_path(name + ".uai")), synth.read_uai(model_path(name + ".uai"))


def test_symbols_are_exported_and_bound():
    for name in ("bnpp_expected_counts", "bnpp_plan_counts", "bnpp_bucket_counts", "bnpp_counts_size"):
        assert name in bnpp.EXPORTED and hasattr(bnpp._lib, name)
    assert bnpp.COUNTS_KEY == (1 << 24) + 16384
    assert bnpp._lib.bnpp_version() == bnpp.ABI_VERSION == 205


@pytest.mark.parametrize("name", PLAN_MODELS)
def test_plan_is_a_batched_bucket_tree(name):
    m, d = _load(name)
    ev = EV_VARS[name]
    B = m.n_vars
    st, groups, beliefs, no_b_elim = bnpp.plan_counts(m, ev, rows_per_launch=64)
    counts = [g for g in groups if g["key"] == bnpp.COUNTS_KEY]
    # one accumulate group per factor, after every other group (so after the groups of its inputs)
    assert len(counts) == m.n_factors == st["count_steps"] and all(g["n_desc"] == 1 for g in counts)
    fwd = int(st["forward_levels"])
    assert all(g["level"] > fwd for g in counts)
    # ... and the plan ends on one: nothing runs after the last accumulate step
    assert max(g["level"] for g in groups) == max(g["level"] for g in counts) == st["levels"]
    # B is summed nowhere and sits in no composite variable
    assert no_b_elim
    # every belief covers its factor's non-evidence variables; where evidence reaches its bucket it carries B
    assert len(beliefs) == m.n_factors
    for s, bv in zip(d["scopes"], beliefs):
        assert sorted(v for v in bv if v != B) == sorted(v for v in s if v not in ev), (s, bv)
        assert bv.count(B) <= 1 and (B not in bv or bv[-1] == B)
        if set(s) & set(ev):
            assert B in bv, ("a factor that mentions evidence must see the row variable", s, bv)
    # in a connected model with evidence, every bucket is reached through the backward pass
    assert all(B in bv for bv in beliefs), "alarm, asia and the grid are connected: every belief carries B"
    # the forward groups are plan_batch's for the same arguments, in level and key sequence
    _, bgroups, scope = bnpp.plan_batch(m, ev, rows_per_launch=64)
    assert scope == [B]
    mine = [(g["level"], g["key"], g["n_desc"], g["vblocks"]) for g in groups if g["level"] <= fwd]
    assert mine == [(g["level"], g["key"], g["n_desc"], g["vblocks"]) for g in bgroups]
    assert st["gather_steps"] == sum(1 for g in groups if g["key"] == bnpp.COND_BATCH_KEY)
    assert st["rows_per_launch"] == 64


def test_no_evidence_has_no_row_variable():
    m, d = _load("asia")
    st, groups, beliefs, no_b_elim = bnpp.plan_counts(m, [], rows_per_launch=16)
    assert st["gather_steps"] == 0 and st["count_steps"] == m.n_factors and no_b_elim
    assert all(m.n_vars not in bv for bv in beliefs)
    assert [sorted(bv) for bv in beliefs] == [sorted(s) for s in d["scopes"]]


def test_budget_too_small_for_one_row(monkeypatch):
    m, _ = _load("alarm")
    monkeypatch.setenv("BNPP_MEM_BUDGET_GB", repr(1e-6))
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_counts(m, EV_VARS["alarm"])
    assert e.value.status == bnpp.ERR_OOM and "1 row per launch" in str(e.value) and "budget" in str(e.value)


def test_counts_plan_needs_more_memory_than_the_batch_plan():
    """Every forward message stays resident through the backward pass."""
    m, _ = _load("alarm")
    sc, _, _, _ = bnpp.plan_counts(m, EV_VARS["alarm"], rows_per_launch=256)
    sb, _, _ = bnpp.plan_batch(m, EV_VARS["alarm"], rows_per_launch=256)
    assert sc["arena_bytes"] > sb["arena_bytes"]


def _raw(m, ev_vars, rows, weights=None, counts=True, dtype=bnpp.F64, rpl=0):
    """bnpp_expected_counts with a NULL context: the arguments are checked first."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.intc).reshape(-1, max(len(ev_vars), 1))[:, :len(ev_vars)])
    IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
    vs = (C.c_int * max(len(ev_vars), 1))(*ev_vars)
    out = np.zeros(4096)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    rc = bnpp._lib.bnpp_expected_counts(None, m.handle if m is not None else None, len(ev_vars), vs, len(rows),
                                        rows.ctypes.data_as(IP), w.ctypes.data_as(DP) if w is not None else None,
                                        bnpp.HEURISTICS["mf"], None, 0, dtype, rpl,
                                        out.ctypes.data_as(DP) if counts else None, None, None, None)
    return rc, bnpp._lib.bnpp_last_error().decode()


def test_argument_errors_without_a_device():
    m, _ = _load("asia")
    good = [[0, 1], [1, 0]]
    assert _raw(None, [0, 3], good)[0] == bnpp.ERR_INVALID
    assert _raw(m, [0, 3], np.zeros((0, 2)))[0] == bnpp.ERR_INVALID
    assert _raw(m, [0, 3], good, counts=False)[0] == bnpp.ERR_INVALID
    rc, msg = _raw(m, [0, 0], good)
    assert rc == bnpp.ERR_INVALID and "twice" in msg
    rc, msg = _raw(m, [0, 99], good)
    assert rc == bnpp.ERR_INVALID and "out of range" in msg
    rc, msg = _raw(m, [0, 3], [[0, 1], [1, 2]])
    assert rc == bnpp.ERR_INVALID and "row 1" in msg and "variable 3" in msg
    for bad in (-1.0, np.nan, np.inf):
        rc, msg = _raw(m, [0, 3], good, weights=[1.0, bad])
        assert rc == bnpp.ERR_INVALID and "row 1" in msg and "weight" in msg, (bad, msg)
    assert _raw(m, [0, 3], good, dtype=7)[0] == bnpp.ERR_INVALID
    # every argument good: the call gets as far as the missing context
    rc, msg = _raw(m, [0, 3], good, weights=[0.0, 2.5])
    assert rc == bnpp.ERR_INVALID and "context" in msg


def test_bucket_counts_checks_its_arguments():
    cards = (C.c_int * 2)(2, 3)
    sc = (C.c_int * 2)(0, 1)
    rc = bnpp._lib.bnpp_bucket_counts(None, None, bnpp.F64, 2, cards, None, 2, sc, 0, None, 4, 4, None, None, None, 1, None)
    assert rc == bnpp.ERR_INVALID


BAYES2 = dict(type="BAYES", cards=[2, 3], scopes=[[0], [0, 1]], values=[[0.5, 0.5], [0.2, 0.3, 0.5, 0.1, 0.1, 0.8]])


def test_m_step_normalises_over_the_child():
    counts = np.array([3.0, 1.0, 1.0, 1.0, 2.0, 0.5, 0.25, 0.25])
    out = learn.m_step(BAYES2, counts)
    assert out["values"][0] == [0.75, 0.25]
    assert out["values"][1] == [0.25, 0.25, 0.5, 0.5, 0.25, 0.25]
    assert BAYES2["values"][0] == [0.5, 0.5], "the input model is left alone"
    per = bnpp.split_counts(BAYES2, counts)
    assert [p.shape for p in per] == [(2,), (2, 3)]
    assert learn.m_step(BAYES2, per)["values"] == out["values"]


def test_m_step_keeps_the_row_of_an_unseen_parent_configuration():
    counts = np.array([4.0, 0.0, 1.0, 1.0, 2.0, 0.0, 0.0, 0.0])
    out = learn.m_step(BAYES2, counts)
    assert out["values"][1] == [0.25, 0.25, 0.5, 0.1, 0.1, 0.8]
    assert out["values"][0] == [1.0, 0.0]


def test_m_step_prior():
    counts = np.array([4.0, 0.0, 1.0, 1.0, 2.0, 0.0, 0.0, 0.0])
    out = learn.m_step(BAYES2, counts, prior=1.0)
    assert out["values"][0] == [5.0 / 6.0, 1.0 / 6.0]
    assert out["values"][1] == [2.0 / 7.0, 2.0 / 7.0, 3.0 / 7.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0]


def test_m_step_refuses_markov_models():
    with pytest.raises(ValueError):
        learn.m_step(dict(BAYES2, type="MARKOV"), np.ones(8))
    with pytest.raises(ValueError):
        bnpp.split_counts(BAYES2, np.ones(7))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_level_keys_of_the_counts_plans_are_instantiated(dt):
    dtype = bnpp.F64 if dt == "f64" else bnpp.F32
    have = set()
    for fam in (0, 1, 2):
        have |= set(bnpp.kernel_keys(dtype, fam, level=True))
    for name in sorted(EV_VARS):
        m, _ = _load(name)
        for R in (1, 7, 64, 256):
            _, groups, _, _ = bnpp.plan_counts(m, EV_VARS[name], dtype=dtype, rows_per_launch=R)
            for g in groups:
                if g["key"] not in (bnpp.COUNTS_KEY, bnpp.COND_BATCH_KEY):
                    assert g["key"] in have, (name, R, g)
