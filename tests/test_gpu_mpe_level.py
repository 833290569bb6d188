"""GPU tests of the max family's level kernels (max_level_kernel) in both
offset widths, through whole bnpp.mpe / bnpp.mpe_batch runs.

test_gpu_mpe.py runs every max key as a single op (max_single_kernel) and
whole models under the default switch only, where every plan holds the twelve
32-bit-offset keys.  Here

  * per entry of mpe_level_catalogue.py (every one of the 24 keys per dtype as
    the first launch group of a model's MPE plan, under one wave and over
    11-21 virtual blocks): the plan reports the key right before the run
    (BNPP_NO_O32 per entry); the assignment equals brute force over the joint
    (at most 2^20 states), whose maximum is strict (asserted first: the log gap
    to the runner-up exceeds the catalogue's MIN_GAP); log10 of the value
    within test_gpu_mpe.LOG10_TOL of the reference.
  * per (input class, tile): the 64-bit entry's model under BNPP_NO_O32=0 and
    =1 gives the same log10 value, bit for bit, and the same assignment in both
    dtypes -- the same arithmetic from other offset registers; each side's plan
    is asserted before its call.
  * whole models (alarm and noisyor_30_40 with their evidence, potts4x5k3):
    bnpp.mpe under =1 has the bits of =0; bnpp.mpe_batch on alarm, cancer and
    ising6x6 (test_gpu_batch.py's evidence variables and 67 rows) at 1, 3 and
    64 rows per launch likewise, the =1 plan holding no 32-bit max key.
  * the entry with the most virtual blocks per dtype and offset width again on
    a context capped at 1, 2 and 3 workgroups: same bits.
  * the job cache: a context's cached job of one width does not answer for the
    other (a plan is made on the switch, none on a repeat).
"""
import numpy as np
import pytest

import bnpp
import max_catalogue as mc
import mpe_level_catalogue as ml
import mpe_ref
from conftest import evidence_of, model_path
from test_gpu_mpe import DT, LN10, LOG10_TOL

pytestmark = pytest.mark.gpu

WHOLE = [("alarm", "alarm.uai.evid"), ("potts4x5k3", "-"), ("noisyor_30_40", "noisyor_30_40.uai.evid")]
BATCHED = ["alarm", "cancer", "ising6x6"]


@pytest.fixture(scope="module")
def entries():
    return ml.load()


@pytest.fixture
def grid_cap(ctx):
    yield ctx.set_max_grid
    ctx.set_max_grid(0)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def _max_keys(dt):
    return set(bnpp.kernel_keys(DT[dt], 4, level=True))


def _mpe(ctx, monkeypatch, e, dt, no_o32, model=None):
    """bnpp.mpe of an entry's model under a switch, its plan's first key asserted first -> (log10 value, x)."""
    monkeypatch.setenv("BNPP_NO_O32", "1" if no_o32 else "0")
    m = model or ml.model_of(bnpp, e)
    g = bnpp.plan_mpe_groups(m, None, dtype=DT[dt], order=ml.order_of(e))[0]
    want = (e["key"] & ~mc.O32) | (0 if no_o32 else mc.O32)
    assert g["key"] == want and g["vblocks"] == e["vblocks"], (e["name"], no_o32, g)
    lv, x, _ = bnpp.mpe(ctx, m, {}, dtype=DT[dt], order=ml.order_of(e))
    return lv, x


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("no_o32", [0, 1])
def test_level_catalogue_against_brute_force(ctx, entries, monkeypatch, dt, no_o32):
    sel = [e for e in entries if e["no_o32"] == no_o32]
    assert len(sel) == 24 and len({e["key"] for e in sel}) == 12
    for e in sel:
        top, want, gap = mpe_ref.brute_force(ml.model_dict(e))
        assert gap > ml.MIN_GAP, (e["name"], gap)        # a strict maximum: the assignments are comparable
        lv, x = _mpe(ctx, monkeypatch, e, dt, no_o32)
        assert x == want, (e["name"], x, want)
        assert abs(lv - top / LN10) <= LOG10_TOL[dt] * max(1.0, abs(top / LN10)), (e["name"], lv, top / LN10)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_offset_widths_give_the_same_bits(ctx, entries, monkeypatch, dt):
    """The 64-bit entries' models under both switches, on one model handle: the
    second call of a pair is also the job cache's case (a cached 32-bit job
    must not answer for the 64-bit run; plan.hpp keys a job on the switch)."""
    sel = [e for e in entries if e["no_o32"]]
    assert len({e["key"] for e in sel}) == 12
    for e in sel:
        m = ml.model_of(bnpp, e)
        a = _mpe(ctx, monkeypatch, e, dt, 0, m)
        b = _mpe(ctx, monkeypatch, e, dt, 1, m)
        assert bnpp.last_timing()["plan_ms"] > 0, (e["name"], "the 32-bit job answered for the 64-bit run")
        again = _mpe(ctx, monkeypatch, e, dt, 1, m)
        assert bnpp.last_timing()["plan_ms"] == 0        # ... while a repeat under one switch is the cached job
        assert _bits(a[0]) == _bits(b[0]) == _bits(again[0]) and a[1] == b[1] == again[1], (e["name"], a, b)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name,evf", WHOLE)
def test_whole_models_under_both_widths(ctx, monkeypatch, name, evf, dt):
    m = bnpp.Model.load(model_path(name + ".uai"))
    ev = evidence_of(evf)
    got = []
    for flag in (0, 1):
        monkeypatch.setenv("BNPP_NO_O32", str(flag))
        keys = {g["key"] for g in bnpp.plan_mpe_groups(m, ev, dtype=DT[dt])} & _max_keys(dt)
        assert keys and all(bool(k & mc.O32) == (not flag) for k in keys), (flag, sorted(keys))
        lv, x, _ = bnpp.mpe(ctx, m, ev, dtype=DT[dt])
        got.append((lv, x))
    assert _bits(got[0][0]) == _bits(got[1][0]) and got[0][1] == got[1][1]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", BATCHED)
def test_batched_mpe_under_both_widths(ctx, monkeypatch, name, dt):
    """The 4x1 tile with the row variable fastest on 64-bit offsets (R = 64),
    and the odd-row forms (R = 1, 3)."""
    from test_gpu_batch import _case
    c = _case(ctx, name)
    for R in (1, 3, 64):
        got = []
        for flag in (0, 1):
            monkeypatch.setenv("BNPP_NO_O32", str(flag))
            _, groups = bnpp.plan_mpe_batch(c["m"], c["ev_vars"], dtype=DT[dt], rows_per_launch=R)
            keys = {g["key"] for g in groups} & _max_keys(dt)
            assert keys and all(bool(k & mc.O32) == (not flag) for k in keys), (R, flag, sorted(keys))
            lv, x, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=DT[dt], rows_per_launch=R)
            got.append((lv, x))
        assert got[0][0].shape == (len(c["rows"]),)
        assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])), (R, np.flatnonzero(_bits(got[0][0]) != _bits(got[1][0])))
        assert np.array_equal(got[0][1], got[1][1]), R


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("no_o32", [0, 1])
def test_level_tile_loop_under_a_capped_grid(ctx, entries, monkeypatch, grid_cap, dt, no_o32):
    sel = [e for e in entries if e["no_o32"] == no_o32]
    e = max(sel, key=lambda x: x["vblocks"])
    assert e["vblocks"] > 3
    m = ml.model_of(bnpp, e)
    ref = _mpe(ctx, monkeypatch, e, dt, no_o32, m)
    assert ref[1] == mpe_ref.brute_force(ml.model_dict(e))[1]
    for cap in (1, 2, 3):
        grid_cap(cap)
        got = _mpe(ctx, monkeypatch, e, dt, no_o32, m)
        grid_cap(0)
        assert _bits(got[0]) == _bits(ref[0]) and got[1] == ref[1], (e["name"], cap)
