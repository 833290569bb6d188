"""GPU tests of batched MPE: whole bnpp.mpe_batch runs against the single call
they batch, row by row, and against the numpy brute force (mpe_ref.py).

  * rows: the 67 rows per model of tests/test_gpu_batch.py (half uniform, half
    from joint samples; the impossible row, where a CPT has a zero entry, in
    the middle), through its _case helper, so the sets are computed once.
  * assignment[b] equals bnpp.mpe's for row b in EVERY entry, in fp64 and in
    fp32 (the comparisons of the max kernels do not see the shared scale);
    log10_value[b] lies within 4 ulp of max(1, |.|) of the single call's in
    fp64 (the three roundings of log10(p) + exp2 * log10(2)); in fp32 within
    1e-6 x max(1, |.|) of the fp64 batch (test_partition_batch_fp32's bound
    for the same rescaled arithmetic).
  * results do not depend on the rows per launch, nor on the grid cap.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import batch_ref
import bnpp
import mpe_ref
from conftest import REPO, model_path
from test_gpu_batch import MODELS, N_ROWS, _bits, _case

pytestmark = pytest.mark.gpu

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
# asia, brute-force test: the seed of batch_ref.draw_rows.  A uniform row over
# the scope of asia's deterministic CPT is impossible half the time (4 of its 8
# value combinations), and an impossible row has no unique maximiser; this seed
# (searched on the CPU) draws 27 possible rows among the 33 uniform ones, which
# with the 33 sampled rows (always possible) makes the 60 the test asserts.
ASIA_BRUTE_SEED = 2240
_SINGLE = {}


def _ev(c, r):
    return dict(zip(c["ev_vars"], (int(x) for x in c["rows"][r])))


def _single(ctx, name, dt):
    """bnpp.mpe per row of a case, computed once per (model, dtype): (log10 values, assignments)."""
    if (name, dt) not in _SINGLE:
        c = _case(ctx, name)
        lv, xs = np.zeros(N_ROWS), np.zeros((N_ROWS, c["m"].n_vars), dtype=np.int64)
        for r in range(N_ROWS):
            lv[r], x, _ = bnpp.mpe(ctx, c["m"], _ev(c, r), "mf", DT[dt])
            xs[r] = x
        _SINGLE[(name, dt)] = (lv, xs)
    return _SINGLE[(name, dt)]


def _check_values_fp64(lv, lv1):
    for r in range(len(lv)):
        if lv1[r] == -np.inf:
            assert lv[r] == -np.inf, (r, lv[r])
        else:
            bound = 4 * np.spacing(max(1.0, abs(lv1[r])))
            print("row", r, "log10_value", lv[r], "single", lv1[r], "bound", bound)
            assert abs(lv[r] - lv1[r]) <= bound, (r, lv[r], lv1[r])


@pytest.mark.parametrize("name", MODELS)
def test_fp64_equals_the_single_call(ctx, name):
    c = _case(ctx, name)
    lv1, x1 = _single(ctx, name, "f64")
    lv, x, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=bnpp.F64)
    assert x.shape == (N_ROWS, c["m"].n_vars) and x.dtype == np.int32 and lv.shape == (N_ROWS,)
    assert np.array_equal(x, x1), np.argwhere(x != x1)[:8]
    assert np.array_equal(x[:, c["ev_vars"]], c["rows"]), "an evidence variable lost its value"
    _check_values_fp64(lv, lv1)
    # an impossible row (Z == 0) has maximum 0; the others' maxima are positive
    assert np.array_equal(lv == -np.inf, c["z1"] == 0)


@pytest.mark.parametrize("name", MODELS)
def test_fp32_equals_the_single_call(ctx, name):
    c = _case(ctx, name)
    lv1, x1 = _single(ctx, name, "f32")
    lv64, _, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=bnpp.F64)
    lv, x, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=bnpp.F32)
    assert np.array_equal(x, x1), np.argwhere(x != x1)[:8]
    for r in range(N_ROWS):
        if c["z1"][r] == 0:
            assert lv[r] == -np.inf and lv1[r] == -np.inf
        else:
            print("row", r, "fp32", lv[r], "fp64", lv64[r])
            assert abs(lv[r] - lv64[r]) <= 1e-6 * max(1.0, abs(lv64[r])), (r, lv[r], lv64[r])


@pytest.mark.parametrize("name", ["asia", "cancer"])
def test_against_brute_force(ctx, name):
    """An independent reference: where the maximiser is unique (at least 60 of
    the 67 rows, asserted) the assignments are equal; elsewhere the returned
    assignment scores the brute-force maximum."""
    c = _case(ctx, name)
    rows = c["rows"]
    if name == "asia":
        samples, _, _ = bnpp.sample(ctx, c["m"], N_ROWS, seed=7)
        rows = batch_ref.draw_rows(c["d"]["cards"], c["ev_vars"], N_ROWS, ASIA_BRUTE_SEED, samples)
        rows[c["bad"]] = c["rows"][c["bad"]]
    lv, x, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], rows, dtype=bnpp.F64)
    n_unique = 0
    for r in range(N_ROWS):
        ev = dict(zip(c["ev_vars"], (int(v) for v in rows[r])))
        top, want, gap = mpe_ref.brute_force(c["d"], ev)
        got = [int(v) for v in x[r]]
        assert all(got[v] == val for v, val in ev.items())
        if top > -math.inf and gap > 1e-9:
            n_unique += 1
            assert got == want, (r, got, want)
        score = mpe_ref.log_score(c["d"], got)
        if top == -math.inf:
            assert score == -math.inf and lv[r] == -np.inf, (r, score, lv[r])
        else:
            assert abs(score - top) <= 1e-12 * max(1.0, abs(top)), (r, score, top)
            assert abs(lv[r] * math.log(10.0) - top) <= 1e-12 * max(1.0, abs(top)), (r, lv[r], top)
    print(name, "rows with a unique maximiser:", n_unique)
    assert n_unique >= 60, n_unique


@pytest.mark.parametrize("name", ["asia", "alarm"])
def test_impossible_row(ctx, name):
    """Its log10_value is -inf, its assignment the single call's (all-zero
    entries take arg 0), and its neighbours are what they are without it."""
    c = _case(ctx, name)
    b = c["bad"]
    assert b == N_ROWS // 2 and c["z1"][b] == 0
    lv1, x1 = _single(ctx, name, "f64")
    lv, x, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=bnpp.F64, rows_per_launch=N_ROWS)
    assert lv[b] == -np.inf and lv1[b] == -np.inf and np.array_equal(x[b], x1[b])
    # the same launch without the row: a possible row in its place
    ok = np.flatnonzero(c["z1"] > 0)
    rows = c["rows"].copy()
    rows[b] = rows[ok[-1]]
    lv2, x2, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], rows, dtype=bnpp.F64, rows_per_launch=N_ROWS)
    keep = np.arange(N_ROWS) != b
    assert np.array_equal(x2[keep], x[keep]) and np.array_equal(_bits(lv2[keep]), _bits(lv[keep]))
    assert np.array_equal(x2[b], x[ok[-1]]) and lv2[b] == lv[ok[-1]]


@pytest.mark.parametrize("name", ["alarm", "ising6x6"])
def test_rows_per_launch(ctx, name):
    """67 rows: R = 3 and 16 end on a padded launch, R = 1 makes 67 launches."""
    c = _case(ctx, name)
    lv1, x1 = _single(ctx, name, "f64")
    ref = None
    for R in (1, 3, 16, 64, 0):
        lv, x, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=bnpp.F64, rows_per_launch=R)
        if ref is None:
            ref = (lv, x)
            assert np.array_equal(x, x1)
            _check_values_fp64(lv, lv1)
        assert np.array_equal(x, ref[1]), (R, np.argwhere(x != ref[1])[:8])
        assert np.array_equal(_bits(lv), _bits(ref[0])), (R, np.flatnonzero(_bits(lv) != _bits(ref[0])))


def test_grid_loop(ctx):
    """257 rows are one row past a workgroup: with the grid capped at 1 the
    traceback's one workgroup walks two virtual blocks."""
    c = _case(ctx, "alarm")
    rows = c["rows"][np.arange(257) % N_ROWS]
    out = []
    try:
        for cap in (1, 2, 0):
            ctx.set_max_grid(cap)
            out.append(bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], rows, dtype=bnpp.F64, rows_per_launch=257))
    finally:
        ctx.set_max_grid(0)
    for lv, x, _ in out[1:]:
        assert np.array_equal(x, out[0][1]) and np.array_equal(_bits(lv), _bits(out[0][0]))
    lv1, x1 = _single(ctx, "alarm", "f64")
    lv, x, _ = out[0]
    for r in (0, 255, 256):
        assert np.array_equal(x[r], x1[r % N_ROWS]), r
    _check_values_fp64(lv[[0, 255, 256]], lv1[[0, 255 % N_ROWS, 256 % N_ROWS]])
    assert np.array_equal(x, x1[np.arange(257) % N_ROWS])


def test_one_row(ctx):
    c = _case(ctx, "alarm")
    lv1, x1 = _single(ctx, "alarm", "f64")
    lv, x, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], c["rows"][5:6], dtype=bnpp.F64)
    assert x.shape == (1, c["m"].n_vars) and np.array_equal(x[0], x1[5])
    _check_values_fp64(lv, lv1[5:6])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_no_evidence_variables(ctx, dt):
    """n_ev = 0: no gather step, no row variable; every row gets the plain answer."""
    c = _case(ctx, "alarm")
    lv1, x1, _ = bnpp.mpe(ctx, c["m"], {}, "mf", DT[dt])
    lv, x, _ = bnpp.mpe_batch(ctx, c["m"], [], np.zeros((5, 0), dtype=np.int64), dtype=DT[dt])
    assert x.shape == (5, c["m"].n_vars) and all(np.array_equal(x[r], x1) for r in range(5))
    _check_values_fp64(lv, np.full(5, lv1))


def test_every_variable_is_evidence(ctx):
    """cancer, all five variables observed: the assignment is the row itself and
    the maximum is the row's probability, bnpp.partition's Z."""
    c = _case(ctx, "cancer")
    cards = c["d"]["cards"]
    ev_vars = list(range(len(cards)))
    rows = batch_ref.draw_rows(cards, ev_vars, 9, 3)
    lv, x, _ = bnpp.mpe_batch(ctx, c["m"], ev_vars, rows, dtype=bnpp.F64)
    assert np.array_equal(x, rows)
    lz = np.array([bnpp.partition(ctx, c["m"], dict(zip(ev_vars, (int(v) for v in r))), "mf", bnpp.F64)[0] for r in rows])
    _check_values_fp64(lv, lz)


def test_cached_job_relaunches_with_other_values(ctx):
    c = _case(ctx, "alarm")
    lv1, x1 = _single(ctx, "alarm", "f64")
    a, b = c["rows"][:32], c["rows"][32:64]
    bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], a, rows_per_launch=32)
    lvb, xb, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], b, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] == 0, "the second call planned again"
    assert np.array_equal(xb, x1[32:64])
    _check_values_fp64(lvb, lv1[32:64])
    # a partition batch on the same variables is another job kind: it plans, and so does the MPE call after it
    bnpp.partition_batch(ctx, c["m"], c["ev_vars"], a, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] > 0
    _, xa, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], a, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] > 0 and np.array_equal(xa, x1[:32])


def test_cli_mpe_batch(ctx, tmp_path):
    c = _case(ctx, "asia")
    rows = c["rows"][[0, c["bad"], 40]]
    evid = tmp_path / "three.evid"
    evid.write_text("3\n" + "".join(
        "%d %s\n" % (len(c["ev_vars"]), " ".join("%d %d" % (v, x) for v, x in zip(c["ev_vars"], r))) for r in rows))
    base = str(tmp_path / "out")
    exe = os.path.join(REPO, "bn-pp_amd", "bin", "bnpp")
    p = subprocess.run([exe, model_path("asia.uai"), str(evid), "-mpe-batch", "-uai", base], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.count(">> MPE row ") == 3
    words = open(base + ".MPE").read().split()
    n = c["m"].n_vars
    assert words[0] == "MPE" and words[1] == "3" and len(words) == 2 + 3 * (n + 1)
    got = np.array([int(w) for w in words[2:]]).reshape(3, n + 1)
    _, x, _ = bnpp.mpe_batch(ctx, c["m"], c["ev_vars"], rows)
    assert (got[:, 0] == n).all() and np.array_equal(got[:, 1:], x)
