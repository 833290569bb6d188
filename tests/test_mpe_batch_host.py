"""CPU tests of batched MPE's host side: the plan of one launch
(bnpp_plan_mpe_batch: gather steps, max buckets, arg tables with and without
the row variable, one traceback step), the argument checks of bnpp_mpe_batch
(made before a device is looked at), the card limit and the compile check of
the traceback kernel."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_ref
import bnpp
from bnpp import synth
from conftest import REPO, model_path

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
DECODE_BATCH_KEY = (1 << 24) + 20480
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


def _arg_tables(d, ev, order):
    """(entries per row, carries B) of every eliminating bucket's arg table, by a
    symbolic elimination of `order`: a bucket carries the row variable when one
    of its inputs does, a factor does when it mentions an evidence variable."""
    cards = d["cards"]
    rank = {v: i for i, v in enumerate(order)}
    buckets = [[] for _ in order]
    for scope in d["scopes"]:
        s = [v for v in scope if v not in ev]
        if s:
            buckets[min(rank[v] for v in s)].append((s, any(v in ev for v in scope)))
    out = []
    for i, x in enumerate(order):
        if not buckets[i]:
            continue
        sep = sorted({v for s, _ in buckets[i] for v in s} - {x})
        has_b = any(b for _, b in buckets[i])
        out.append((math.prod(cards[v] for v in sep), has_b))
        if sep:
            buckets[min(rank[v] for v in sep)].append((sep, has_b))
    return out


def test_symbols_are_exported():
    for name in ("bnpp_mpe_batch", "bnpp_plan_mpe_batch"):
        assert name in bnpp.EXPORTED and hasattr(bnpp._lib, name)
    assert bnpp.MPE_DECODE_BATCH_KEY == DECODE_BATCH_KEY
    assert bnpp.ABI_VERSION == 205 and bnpp._lib.bnpp_version() == 205


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", MODELS)
def test_plan_of_one_launch(models, name, dt):
    m, d, ev = models[name]
    st, groups = bnpp.plan_mpe_batch(m, ev, dtype=DT[dt], rows_per_launch=64)
    assert st["rows_per_launch"] == 64
    # as many gather steps as plan_batch, all at level 0
    bst, _, _ = bnpp.plan_batch(m, ev, dtype=DT[dt], rows_per_launch=64)
    gathers = [g for g in groups if g["key"] == bnpp.COND_BATCH_KEY]
    assert len(gathers) == st["gather_steps"] == bst["gather_steps"] > 0
    assert all(g["level"] == 0 and g["n_desc"] == 1 for g in gathers)
    # as many max buckets as plan_mpe for any one row
    max_keys = set(bnpp.kernel_keys(DT[dt], 4, level=True))
    product_keys = set(bnpp.kernel_keys(DT[dt], 0, level=True))
    single = bnpp.plan_mpe_groups(m, {v: 0 for v in ev}, dtype=DT[dt])
    n_single = sum(g["n_desc"] for g in single if g["key"] in max_keys)
    n_max = sum(g["n_desc"] for g in groups if g["key"] in max_keys)
    assert n_max == n_single == st["max_buckets"] > 0
    # one traceback step, the last group; every other key a family-4, product or gather key
    assert [g["key"] for g in groups].count(DECODE_BATCH_KEY) == 1 and groups[-1]["key"] == DECODE_BATCH_KEY
    assert groups[-1]["level"] == max(g["level"] for g in groups) and groups[-1]["n_desc"] == 1
    for g in groups[:-1]:
        assert g["key"] in max_keys or g["key"] in product_keys or g["key"] == bnpp.COND_BATCH_KEY, g
    # arg bytes: entries x 64 where the table carries B, entries otherwise
    order, _ = bnpp.ordering(m, {v: 0 for v in ev}, "mf")
    tabs = _arg_tables(d, set(ev), order)
    assert len(tabs) == n_max
    assert st["arg_tables_b"] == sum(1 for _, b in tabs if b) and st["arg_tables_no_b"] == sum(1 for _, b in tabs if not b)
    assert st["arg_bytes"] == sum(e * 64 if b else e for e, b in tabs)
    assert st["arg_bytes"] == st["arg_entries_per_row"] * 64 + st["arg_entries_no_b"]
    # the arena holds every arg table and the assignment state beside the messages
    assert st["arena_bytes"] >= st["arg_bytes"] + m.n_vars * 64
    assert st["arena_bytes"] > bst["arena_bytes"]


def test_alarm_has_arg_tables_with_and_without_the_row_variable(models):
    """Evidence reaches only part of alarm: the traceback reads tables with a B
    stride of 1 and tables with none."""
    m, _, ev = models["alarm"]
    st, _ = bnpp.plan_mpe_batch(m, ev, rows_per_launch=64)
    assert st["arg_tables_b"] > 0 and st["arg_tables_no_b"] > 0
    assert st["arg_tables_b"] + st["arg_tables_no_b"] == st["max_buckets"]


def test_plans_reach_1x1_and_4x1_max_tiles(models):
    """Across R in {1, 3, 64} the max buckets run on 1x1 tiles (odd R, or tables
    without B) and on 4x1 tiles (B the fastest dimension, R a multiple of 4).
    Keys: 65536 + [1024] + n_in * 64 + v1 * 8 + 1 (maxout.cuh)."""
    v1_seen = set()
    for name in MODELS:
        m, _, ev = models[name]
        for dt in DT.values():
            max_keys = set(bnpp.kernel_keys(dt, 4, level=True))
            for R in (1, 3, 64):
                _, groups = bnpp.plan_mpe_batch(m, ev, dtype=dt, rows_per_launch=R)
                keys = {g["key"] for g in groups if g["key"] in max_keys}
                v1 = {((k & 63) - 1) // 8 for k in keys}
                assert v1 <= {1, 2, 4}
                v1_seen |= v1
    assert {1, 4} <= v1_seen, v1_seen


def test_same_plan_for_heuristic_and_given_order(models):
    m, _, ev = models["alarm"]
    order, _ = bnpp.ordering(m, {v: 0 for v in ev}, "mf")
    assert bnpp.plan_mpe_batch(m, ev, rows_per_launch=16) == bnpp.plan_mpe_batch(m, ev, rows_per_launch=16, order=order)
    with pytest.raises(bnpp.BnppError) as e:                # an MPE order covers every free variable
        bnpp.plan_mpe_batch(m, ev, rows_per_launch=16, order=order[:-1])
    assert e.value.status == bnpp.ERR_INVALID


def test_automatic_rows_fit_the_budget(models, monkeypatch):
    m, _, ev = models["alarm"]
    monkeypatch.setenv("BNPP_MEM_BUDGET_GB", "1e-3")
    st, _ = bnpp.plan_mpe_batch(m, ev)
    r = int(st["rows_per_launch"])
    assert 1 <= r < 1 << 16 and r & (r - 1) == 0 and st["arena_bytes"] <= 1e6
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_mpe_batch(m, ev, rows_per_launch=2 * r)
    assert e.value.status == bnpp.ERR_OOM
    assert "messages" in str(e.value) and "arg tables" in str(e.value) and "%d rows per launch" % (2 * r) in str(e.value)
    monkeypatch.setenv("BNPP_MEM_BUDGET_GB", "1e-6")
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_mpe_batch(m, ev)
    assert e.value.status == bnpp.ERR_OOM and "1 row per launch" in str(e.value)


def test_card_limit_of_a_maximised_variable():
    for card, ok in ((256, True), (257, False)):
        vals = [1.0 + (i % 7) for i in range(card * 2)] + [0.5, 0.25]
        m = bnpp.Model.from_arrays([card, 2], [[0, 1], [1]], vals)
        for dt in DT.values():
            if ok:
                assert bnpp.plan_mpe_batch(m, [1], dtype=dt, rows_per_launch=8)[1][-1]["key"] == DECODE_BATCH_KEY
            else:
                with pytest.raises(bnpp.BnppError) as e:
                    bnpp.plan_mpe_batch(m, [1], dtype=dt, rows_per_launch=8)
                assert e.value.status == bnpp.ERR_UNSUPPORTED and "257" in str(e.value)
                # as evidence the variable is not maximised (values are int: no limit)
                assert bnpp.plan_mpe_batch(m, [0], dtype=dt, rows_per_launch=8)[1][-1]["key"] == DECODE_BATCH_KEY


def _mpe_batch_raw(m, ev_vars, rows):
    """bnpp_mpe_batch with a NULL context: the arguments are checked first."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.intc).reshape(-1, max(len(ev_vars), 1))[:, :len(ev_vars)])
    n = len(rows)
    lv = np.zeros(max(n, 1))
    x = np.zeros(max(n, 1) * m.n_vars, dtype=np.intc)
    IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
    vs = (C.c_int * max(len(ev_vars), 1))(*ev_vars)
    rc = bnpp._lib.bnpp_mpe_batch(None, m.handle, len(ev_vars), vs, n, rows.ctypes.data_as(IP), bnpp.HEURISTICS["mf"], None, 0,
                                  bnpp.F64, 0, lv.ctypes.data_as(DP), x.ctypes.data_as(IP), None)
    return rc, bnpp._lib.bnpp_last_error().decode()


def test_invalid_arguments(models):
    m, d, _ = models["alarm"]
    ev = [3, 10, 20]
    good = batch_ref.draw_rows(d["cards"], ev, 5, 1)
    # a valid call passes the argument checks and fails at the context: without a GPU the entry
    # itself reports that there is no device
    rc, msg = _mpe_batch_raw(m, ev, good)
    if bnpp.device_count() == 0:
        assert rc == bnpp.ERR_NO_DEVICE and "device" in msg
    else:
        assert rc == bnpp.ERR_INVALID and "context" in msg
    rc, msg = _mpe_batch_raw(m, ev, np.zeros((0, 3)))
    assert rc == bnpp.ERR_INVALID and "n_rows" in msg
    rc, msg = _mpe_batch_raw(m, [3, 10, 3], np.zeros((2, 3)))
    assert rc == bnpp.ERR_INVALID and "twice" in msg and "3" in msg
    for bad in (-1, m.n_vars):
        rc, msg = _mpe_batch_raw(m, [3, bad], np.zeros((2, 2)))
        assert rc == bnpp.ERR_INVALID and "out of range" in msg and str(bad) in msg
    for row, col, val in ((3, 1, 1 << 20), (0, 0, -1), (4, 2, d["cards"][ev[2]])):
        rows = good.copy()
        rows[row, col] = val
        rc, msg = _mpe_batch_raw(m, ev, rows)
        assert rc == bnpp.ERR_INVALID, msg
        assert "row %d" % row in msg and "variable %d" % ev[col] in msg and str(val) in msg, msg
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_mpe_batch(m, [3, 3])
    assert e.value.status == bnpp.ERR_INVALID


def test_traceback_kernel_uses_no_scratch(tmp_path):
    """The compile check: the unit that instantiates mpe_decode_batch_kernel,
    for gfx950 with the flags of the other units, 0 bytes of scratch."""
    src = os.path.join(REPO, "bn-pp_amd", "csrc")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + src,
                        "-I" + os.path.join(REPO, "include"), "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(src, "k_max_f64.hip"), "-o", str(tmp_path / "k.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", p.stderr, flags=re.S)
    mine = [(n, int(s)) for n, s in blocks if "mpe_decode_batch_kernel" in n]
    assert len(mine) == 1, [n for n, _ in blocks]           # instantiated once
    assert mine[0][1] == 0, p.stderr
