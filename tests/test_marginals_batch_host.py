"""CPU tests of batched marginals: the exported symbols, the plan of one launch
(bnpp_plan_marginals_batch: plan_counts's batched bucket tree, then one emit
step), its memory, the argument checks of bnpp_marginals_batch,
bnpp_plan_marginals_batch and bnpp_bucket_marginal_rows (made before a device
is looked at), the numpy restatement, split_marginals and learn's argmax."""
import ctypes as C

import numpy as np
import pytest

import bnpp
import marginals_batch_ref
from bnpp import learn, synth
from conftest import model_path
from counts_ref import EV_VARS

PLAN_MODELS = ("asia", "alarm", "ising6x6", "potts4x5k3")
IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)

# two components, {0, 1} and {2, 3}, and variable 4 in no factor
SPLIT = dict(type="MARKOV", cards=[2, 3, 2, 4, 5], scopes=[[0, 1], [2, 3], [3]],
             values=[[0.5, 1.0, 2.0, 0.25, 0.75, 1.5], [1.0, 0.5, 0.25, 2.0, 0.125, 1.0, 3.0, 0.5], [1.0, 2.0, 0.5, 1.5]])


def _load(name):
    return bnpp.Model.load(model_path(name + ".uai")), synth.read_uai(model_path(name + ".uai"))


def test_symbols_are_exported_and_bound():
    for name in ("bnpp_marginals_batch", "bnpp_plan_marginals_batch", "bnpp_bucket_marginal_rows"):
        assert name in bnpp.EXPORTED and hasattr(bnpp._lib, name)
    assert bnpp.MARG_ROWS_KEY == (1 << 24) + 28672
    assert bnpp._lib.bnpp_version() == bnpp.ABI_VERSION == 205
    for f in (bnpp.plan_marginals_batch, bnpp.marginals_batch, bnpp.split_marginals, bnpp.bucket_marginal_rows,
              learn.classify):
        assert callable(f)


@pytest.mark.parametrize("name", PLAN_MODELS)
def test_plan_is_the_batch_plan_then_a_backward_pass_then_one_emit_step(name):
    m, d = _load(name)
    ev = EV_VARS[name]
    B = m.n_vars
    st, groups, kinds = bnpp.plan_marginals_batch(m, ev, rows_per_launch=64)
    fwd = int(st["forward_levels"])
    # the forward groups are plan_batch's for the same arguments, in level and key sequence
    _, bgroups, scope = bnpp.plan_batch(m, ev, rows_per_launch=64)
    assert scope == [B]
    mine = [(g["level"], g["key"], g["n_desc"], g["vblocks"]) for g in groups if g["level"] <= fwd]
    assert mine == [(g["level"], g["key"], g["n_desc"], g["vblocks"]) for g in bgroups]
    # exactly one emit step: the last group, alone at the last level
    emit = [g for g in groups if g["key"] == bnpp.MARG_ROWS_KEY]
    assert len(emit) == 1 == st["emit_steps"] and emit[0] == groups[-1] and emit[0]["n_desc"] == 1
    assert emit[0]["level"] == st["levels"] and [g for g in groups if g["level"] == st["levels"]] == emit
    assert emit[0]["level"] > fwd + 1, "the backward pass has levels of its own between the forward pass and the emit step"
    # the column kinds add up to the targets; W and the output bytes
    assert len(kinds) == m.n_vars
    assert st["belief_cols"] + st["evidence_cols"] + st["free_cols"] == m.n_vars
    assert st["belief_cols"] == sum(k.startswith("belief") for k in kinds)
    assert st["belief_cols_b"] == kinds.count("belief_b")
    assert st["evidence_cols"] == kinds.count("evidence") == len(ev) and st["free_cols"] == kinds.count("free") == 0
    assert [k == "evidence" for k in kinds] == [v in ev for v in range(m.n_vars)]
    assert st["width"] == sum(d["cards"]) and st["out_bytes"] == 64 * sum(d["cards"]) * 8
    # a connected model: evidence reaches every target
    assert kinds.count("belief") == 0
    assert st["rows_per_launch"] == 64 and st["gather_steps"] == sum(1 for g in groups if g["key"] == bnpp.COND_BATCH_KEY)
    # a subset, permuted, an evidence variable among it
    sub = [ev[0], m.n_vars - 1, 2]
    st2, groups2, kinds2 = bnpp.plan_marginals_batch(m, ev, targets=sub, rows_per_launch=64)
    assert kinds2 == [kinds[t] for t in sub] and st2["width"] == sum(d["cards"][t] for t in sub)
    assert groups2[-1]["key"] == bnpp.MARG_ROWS_KEY and st2["levels"] <= st["levels"]


def test_targets_no_evidence_reaches_carry_no_row_variable():
    m = bnpp.Model.from_dict(SPLIT)
    # evidence in no factor: no gather step, no table carries the row variable, and the emit step still reads its row
    st, groups, kinds = bnpp.plan_marginals_batch(m, [4], rows_per_launch=16)
    assert kinds == ["belief", "belief", "belief", "belief", "evidence"] and st["gather_steps"] == 0
    assert (st["belief_cols"], st["belief_cols_b"], st["evidence_cols"], st["free_cols"]) == (4, 0, 1, 0)
    assert st["width"] == 16 and st["out_bytes"] == 16 * 16 * 8
    # evidence in the other component: its root message depends on the row (it can make a row impossible), so it
    # scales the beliefs of {2, 3} row by row and they carry the row variable too
    st, groups, kinds = bnpp.plan_marginals_batch(m, [1], rows_per_launch=16)
    assert kinds == ["belief_b", "evidence", "belief_b", "belief_b", "free"]
    assert (st["belief_cols"], st["belief_cols_b"], st["evidence_cols"], st["free_cols"]) == (3, 3, 1, 1)


def test_no_evidence_has_no_row_variable():
    m, d = _load("asia")
    st, groups, kinds = bnpp.plan_marginals_batch(m, [], rows_per_launch=16)
    assert st["gather_steps"] == 0 and kinds == ["belief"] * m.n_vars and st["belief_cols_b"] == 0
    assert groups[-1]["key"] == bnpp.MARG_ROWS_KEY and st["out_bytes"] == 16 * sum(d["cards"]) * 8


def test_plan_needs_the_batch_plan_and_the_output():
    m, _ = _load("alarm")
    for R in (1, 64, 256):
        sm, _, _ = bnpp.plan_marginals_batch(m, EV_VARS["alarm"], rows_per_launch=R)
        sb, _, _ = bnpp.plan_batch(m, EV_VARS["alarm"], rows_per_launch=R)
        assert sm["arena_bytes"] >= sb["arena_bytes"] + sm["out_bytes"], (R, sm, sb)


def test_budget_too_small_for_one_row(monkeypatch):
    m, _ = _load("alarm")
    monkeypatch.setenv("BNPP_MEM_BUDGET_GB", repr(1e-6))
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_marginals_batch(m, EV_VARS["alarm"])
    s = str(e.value)
    assert e.value.status == bnpp.ERR_OOM and "1 row per launch" in s and "budget" in s
    assert "messages" in s and "output %d bytes" % (105 * 8) in s, s


def _raw(m, ev_vars, rows, targets=None, n_targets=None, order=None, out=True, dtype=bnpp.F64, rpl=0):
    """bnpp_marginals_batch with a NULL context: the arguments are checked first."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.intc).reshape(-1, max(len(ev_vars), 1))[:, :len(ev_vars)])
    vs = (C.c_int * max(len(ev_vars), 1))(*ev_vars)
    buf = np.zeros(4096)
    ts = None if targets is None else (C.c_int * max(len(targets), 1))(*targets)
    nt = (0 if targets is None else len(targets)) if n_targets is None else n_targets
    oa = None if order is None else (C.c_int * max(len(order), 1))(*order)
    rc = bnpp._lib.bnpp_marginals_batch(None, m.handle if m is not None else None, len(ev_vars), vs, len(rows),
                                        rows.ctypes.data_as(IP), bnpp.ORDER_GIVEN if order is not None else bnpp.MIN_FILL,
                                        oa, 0 if order is None else len(order), nt, ts, dtype, rpl,
                                        buf.ctypes.data_as(DP) if out else None, None, None)
    return rc, bnpp._lib.bnpp_last_error().decode()


def test_argument_errors_without_a_device():
    m, _ = _load("asia")
    good = [[0, 1], [1, 0]]
    assert _raw(None, [0, 3], good)[0] == bnpp.ERR_INVALID
    assert _raw(m, [0, 3], np.zeros((0, 2)))[0] == bnpp.ERR_INVALID
    assert _raw(m, [0, 3], good, out=False)[0] == bnpp.ERR_INVALID
    rc, msg = _raw(m, [0, 0], good)
    assert rc == bnpp.ERR_INVALID and "twice" in msg
    rc, msg = _raw(m, [0, 99], good)
    assert rc == bnpp.ERR_INVALID and "out of range" in msg
    rc, msg = _raw(m, [0, 3], [[0, 1], [1, 2]])
    assert rc == bnpp.ERR_INVALID and "row 1" in msg and "variable 3" in msg
    assert _raw(m, [0, 3], good, dtype=7)[0] == bnpp.ERR_INVALID
    # the targets
    rc, msg = _raw(m, [0, 3], good, targets=[1, 8])
    assert rc == bnpp.ERR_INVALID and "target 8" in msg and "out of range" in msg
    rc, msg = _raw(m, [0, 3], good, targets=[-1])
    assert rc == bnpp.ERR_INVALID and "out of range" in msg
    rc, msg = _raw(m, [0, 3], good, targets=[2, 5, 2])
    assert rc == bnpp.ERR_INVALID and "target 2" in msg and "twice" in msg
    rc, msg = _raw(m, [0, 3], good, targets=[2], n_targets=0)
    assert rc == bnpp.ERR_INVALID and "n_targets" in msg
    # an order that leaves out a non-evidence variable (5), or is no order at all
    rc, msg = _raw(m, [0, 3], good, order=[1, 2, 4, 6, 7])
    assert rc == bnpp.ERR_INVALID and "cover every non-evidence variable" in msg
    assert _raw(m, [0, 3], good, order=[1, 1, 2, 4, 5, 6, 7])[0] == bnpp.ERR_INVALID
    # every argument good (a target that is an evidence variable included): the call gets as far as the missing context
    for kw in (dict(), dict(targets=[3, 1]), dict(order=[7, 6, 5, 4, 2, 1]), dict(order=[7, 6, 5, 4, 3, 2, 1, 0])):
        rc, msg = _raw(m, [0, 3], good, **kw)
        assert rc == bnpp.ERR_INVALID and "context" in msg, (kw, msg)
    with pytest.raises(bnpp.BnppError):
        bnpp.marginals_batch(None, m, [0, 3], good, targets=[])


def test_plan_entry_checks_the_same_targets_and_order():
    m, _ = _load("asia")
    for kw, word in ((dict(targets=[1, 8]), "out of range"), (dict(targets=[2, 2]), "twice"), (dict(targets=[]), "n_targets"),
                     (dict(order=[1, 2, 4, 6, 7]), "cover every non-evidence variable")):
        with pytest.raises(bnpp.BnppError) as e:
            bnpp.plan_marginals_batch(m, [0, 3], **kw)
        assert e.value.status == bnpp.ERR_INVALID and word in str(e.value), (kw, str(e.value))
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_marginals_batch(m, [0, 0])
    assert "twice" in str(e.value)
    st, _, kinds = bnpp.plan_marginals_batch(m, [0, 3], order=[7, 6, 5, 4, 2, 1], rows_per_launch=8)
    assert st["width"] == 16 and kinds.count("evidence") == 2


def _rows_raw(n_targets, cards, tables, has_b, ev_row, n_rows, rows_live, ev, out=1):
    """bnpp_bucket_marginal_rows with a NULL context and made-up addresses: the shape is checked first."""
    cs = (C.c_int * max(len(cards), 1))(*cards)
    tabs = (C.c_void_p * max(len(tables), 1))(*[C.c_void_p(t) if t else None for t in tables])
    hb = (C.c_int * max(len(has_b), 1))(*has_b)
    er = (C.c_int * max(len(ev_row), 1))(*ev_row)
    rc = bnpp._lib.bnpp_bucket_marginal_rows(None, None, bnpp.F64, n_targets, cs, tabs, hb, er, n_rows, rows_live,
                                             C.c_void_p(ev) if ev else None, C.c_void_p(out) if out else None)
    return rc, bnpp._lib.bnpp_last_error().decode()


def test_bucket_marginal_rows_checks_its_arguments():
    ok = dict(n_targets=2, cards=[2, 3], tables=[4096, 0], has_b=[1, 0], ev_row=[-1, 0], n_rows=8, rows_live=8, ev=8192)
    rc, msg = _rows_raw(**ok)
    assert rc == bnpp.ERR_INVALID and "context" in msg, "every argument good: as far as the missing context"
    for kw, word in ((dict(n_targets=0), "n_targets"), (dict(cards=[2, 0]), "card"), (dict(rows_live=9), "rows_live"),
                     (dict(rows_live=-1), "rows_live"), (dict(tables=[0, 0], ev_row=[-1, 0]), "has_b"),
                     (dict(ev=0), "evidence"), (dict(n_rows=0), "n_rows"), (dict(out=0), "null")):
        rc, msg = _rows_raw(**dict(ok, **kw))
        assert rc == bnpp.ERR_INVALID and word in msg and "context" not in msg, (kw, msg)
    many = dict(ok, n_targets=65, cards=[2] * 65, tables=[4096] * 65, has_b=[1] * 65, ev_row=[-1] * 65)
    assert _rows_raw(**many)[0] == bnpp.ERR_UNSUPPORTED


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_level_keys_of_the_marginals_plans_are_instantiated(dt):
    dtype = bnpp.F64 if dt == "f64" else bnpp.F32
    have = set()
    for fam in (0, 1, 2):
        have |= set(bnpp.kernel_keys(dtype, fam, level=True))
    for name in sorted(EV_VARS):
        m, _ = _load(name)
        for R in (1, 7, 64, 256):
            for targets in (None, [m.n_vars - 1, 0]):
                _, groups, _ = bnpp.plan_marginals_batch(m, EV_VARS[name], targets=targets, dtype=dtype, rows_per_launch=R)
                for g in groups:
                    if g["key"] not in (bnpp.MARG_ROWS_KEY, bnpp.COND_BATCH_KEY):
                        assert g["key"] in have, (name, R, g)


def test_restatement_normalises_sequentially():
    out = np.full((4, 6), -7.0)
    T = np.array([1.0, 2.0, 0.0, 5.0, 3.0, 2.0, 0.0, 5.0], dtype=np.float32)       # (x, b), b fastest: 2 x 4
    ev = np.array([[2, 0, 9, -4]])
    marginals_batch_ref.emit_rows(out, [2, 3, 1], [T, None, None], [True, False, False], [-1, 0, -1], 4, 3, ev)
    assert np.array_equal(out[:3, :2], np.array([[0.25, 0.75], [0.5, 0.5], [np.nan, np.nan]]), equal_nan=True)
    assert np.array_equal(out[:3, 2:5], np.array([[0, 0, 1], [1, 0, 0], [0, 0, 1]]))
    assert (out[:3, 5] == 1.0).all() and (out[3] == -7.0).all()
    # the sum is sequential from 0.0 in fp64: 1e-17 is absorbed term by term, never added up first
    t = np.array([1.0] + [1e-17] * 9)
    got = marginals_batch_ref.emit_rows(np.zeros((1, 10)), [10], [t], [False], [-1], 1, 1, None)
    assert got[0, 0] == 1.0 and got[0, 1] == 1e-17


def test_brute_force_marginals_of_a_split_model():
    out, z = marginals_batch_ref.brute_marginals(SPLIT, [1], [[0], [2]], targets=[0, 1, 4, 3])
    assert np.allclose(out[0, :2], [0.5 / 0.75, 0.25 / 0.75]) and np.array_equal(out[:, 2:5], [[1, 0, 0], [0, 0, 1]])
    assert np.allclose(out[:, 5:10], 0.2) and np.allclose(out[0, 10:], out[1, 10:]) and np.allclose(out[:, 10:].sum(axis=1), 1)
    assert (z > 0).all()


def test_split_marginals_and_the_tie_rule():
    cards = [2, 3, 2]
    out = np.array([[0.5, 0.5, 0.2, 0.4, 0.4, 1.0, 0.0],
                    [0.1, 0.9, 0.3, 0.3, 0.3, 0.0, 1.0],
                    [np.nan, np.nan, 0.0, 0.0, 1.0, 0.5, 0.5]])
    per = bnpp.split_marginals(cards, None, out)
    assert [p.shape for p in per] == [(3, 2), (3, 3), (3, 2)]
    per[1][0, 0] = 0.25
    assert out[0, 2] == 0.25, "views, not copies"
    per = bnpp.split_marginals(cards, [2, 0], out[:, [5, 6, 0, 1]])
    assert [p.shape for p in per] == [(3, 2), (3, 2)] and per[0][1, 1] == 1.0
    with pytest.raises(ValueError):
        bnpp.split_marginals(cards, [0, 1], out)
    # the lowest value wins a tie; a block of NaN (an impossible row) reads 0
    lab = learn.argmax_marginals(cards, None, out)
    assert lab.dtype == np.int64 and lab.tolist() == [[0, 1, 0], [1, 0, 1], [0, 2, 0]]
    assert learn.argmax_marginals(cards, [1], out[:, 2:5]).tolist() == [[1], [0], [2]]
