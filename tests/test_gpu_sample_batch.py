"""GPU tests of batched posterior sampling: whole bnpp.sample_batch runs against
the single call they batch, byte for byte, against the numpy restatement
(sample_ref.py through sample_batch_ref.py), and against brute-force posteriors.

  * rows: the 67 rows per model of tests/test_gpu_batch.py (half uniform, half
    from joint samples; the impossible row, where a CPT has a zero entry, in
    the middle), through its _case helper, so the sets are computed once.
  * samples[b, s] equals bnpp.sample's draw for evidence row b at the global
    index first + b * row_stride + s in EVERY byte, in fp64 and in fp32 (the
    draw does not see the scale the rows of a launch share); n_degenerate[b]
    is equal; log10_z has partition_batch's bits.
  * results do not depend on the rows per launch, the grid cap or the split of
    the rows over calls.
Nothing here fixes a tolerance of its own: equalities are exact, the one
statistical bound is sample_ref.bound.
"""
import os
import subprocess

import numpy as np
import pytest

import batch_ref
import bnpp
import sample_batch_ref as sbr
from bnpp import learn, synth
from conftest import REPO, model_path
from test_gpu_batch import MODELS, N_ROWS, _bits, _case

pytestmark = pytest.mark.gpu

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
SEED = 20261020
FIRST = 3
K = 5
STRIDES = (0, 5, 1000)
_SINGLE = {}


def _ev(c, r):
    return dict(zip(c["ev_vars"], (int(x) for x in c["rows"][r])))


def _single(ctx, name, dt, k=K, strides=STRIDES):
    """bnpp.sample per row of a case at first + b * stride, computed once per
    (model, dtype, k): {stride: (samples [67][k][n_vars], n_degenerate [67])}.
    The calls of one row follow each other: the first plans, the others relaunch."""
    key = (name, dt, k, strides)
    if key not in _SINGLE:
        c = _case(ctx, name)
        out = {s: (np.zeros((N_ROWS, k, c["m"].n_vars), dtype=np.uint8), np.zeros(N_ROWS, dtype=np.int64)) for s in strides}
        for r in range(N_ROWS):
            for s in strides:
                x, _, deg = bnpp.sample(ctx, c["m"], k, _ev(c, r), seed=SEED, first_sample=FIRST + r * s, dtype=DT[dt])
                out[s][0][r] = x
                out[s][1][r] = deg
        _SINGLE[key] = out
    return _SINGLE[key]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", MODELS)
def test_equals_the_single_call(ctx, name, dt):
    c = _case(ctx, name)
    one = _single(ctx, name, dt)
    lzb, _, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=DT[dt])
    for stride in STRIDES:
        x, lz, deg = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"], K, seed=SEED, first_sample=FIRST,
                                       row_stride=stride, dtype=DT[dt])
        assert x.shape == (N_ROWS, K, c["m"].n_vars) and x.dtype == np.uint8
        assert lz.shape == (N_ROWS,) and deg.shape == (N_ROWS,) and deg.dtype == np.int64
        x1, deg1 = one[stride]
        assert np.array_equal(x, x1), (stride, np.argwhere(x != x1)[:8])
        assert np.array_equal(deg, deg1), (stride, deg, deg1)
        assert np.array_equal(_bits(lz), _bits(lzb)), (stride, np.flatnonzero(_bits(lz) != _bits(lzb)))
        assert np.array_equal(x[:, :, c["ev_vars"]], np.broadcast_to(c["rows"][:, None, :], (N_ROWS, K, len(c["ev_vars"])))), \
            "an evidence variable lost its value"
    assert np.array_equal(lzb == -np.inf, c["z1"] == 0)


@pytest.mark.parametrize("name", ["asia", "cancer"])
def test_bit_for_bit_against_the_restatement(ctx, name):
    """fp64, the engine's order: sample_ref.run per row at first + b * stride
    (the impossible row: the contract's zeros, sample_batch_ref.run)."""
    c = _case(ctx, name)
    order, _ = bnpp.ordering(c["m"], {v: 0 for v in c["ev_vars"]}, "mf")
    for stride in (0, 7):
        want, wdeg = sbr.run(c["d"], c["ev_vars"], c["rows"], order, K, SEED, FIRST, stride)
        x, _, deg = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"], K, seed=SEED, first_sample=FIRST,
                                      row_stride=stride, dtype=bnpp.F64)
        assert np.array_equal(x, want), (stride, np.argwhere(x != want)[:8])
        assert np.array_equal(deg, wdeg)


@pytest.mark.parametrize("name", ["alarm", "ising6x6"])
@pytest.mark.parametrize("k", [1, 3])
def test_rows_per_launch(ctx, name, k):
    """67 rows: R * K = 64 * 1 (one wave), 3 * 3, 67 * 3 and 16 * 3 lanes; R = 1
    makes 67 launches, R = 3, 16 and 64 end on a padded launch."""
    c = _case(ctx, name)
    args = dict(seed=SEED, first_sample=FIRST, row_stride=k, dtype=bnpp.F64)
    ref = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"], k, rows_per_launch=0, **args)
    for r in (0, c["bad"] if c["bad"] is not None else 1, N_ROWS - 1):
        x1, _, deg1 = bnpp.sample(ctx, c["m"], k, _ev(c, r), seed=SEED, first_sample=FIRST + r * k, dtype=bnpp.F64)
        assert np.array_equal(ref[0][r], x1) and ref[2][r] == deg1, r
    for R in (1, 3, 16, 64, N_ROWS):
        x, lz, deg = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"], k, rows_per_launch=R, **args)
        assert np.array_equal(x, ref[0]), (R, np.argwhere(x != ref[0])[:8])
        assert np.array_equal(_bits(lz), _bits(ref[1])) and np.array_equal(deg, ref[2]), R


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_row_of_257_draws_and_257_rows_of_one_draw(ctx, dt):
    """R = 1 with K = 257: s alone spans two blocks.  R = 257 (rows repeated)
    with K = 1: b alone does."""
    c = _case(ctx, "alarm")
    r = 5
    x, _, deg = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"][r:r + 1], 257, seed=SEED, first_sample=FIRST,
                                  dtype=DT[dt], rows_per_launch=1)
    x1, _, deg1 = bnpp.sample(ctx, c["m"], 257, _ev(c, r), seed=SEED, first_sample=FIRST, dtype=DT[dt])
    assert np.array_equal(x[0], x1) and deg[0] == deg1
    rows = c["rows"][np.arange(257) % N_ROWS]
    one = _single(ctx, "alarm", dt)[0]                   # stride 0: every row draws at first + s
    x, _, deg = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], rows, 1, seed=SEED, first_sample=FIRST, row_stride=0,
                                  dtype=DT[dt], rows_per_launch=257)
    assert np.array_equal(x[:, 0], one[0][np.arange(257) % N_ROWS, 0])
    assert (deg <= one[1][np.arange(257) % N_ROWS]).all()    # the first of the five draws the single call counted over


def test_grid_loop(ctx):
    """67 rows of 5 draws are 335 lanes, more than a workgroup: with the grid
    capped at 1 and 2 the persistent loop iterates."""
    c = _case(ctx, "alarm")
    out = []
    try:
        for cap in (1, 2, 0):
            ctx.set_max_grid(cap)
            out.append(bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"], K, seed=SEED, first_sample=FIRST,
                                         row_stride=5, rows_per_launch=N_ROWS))
    finally:
        ctx.set_max_grid(0)
    x1, deg1 = _single(ctx, "alarm", "f64")[5]
    for x, lz, deg in out:
        assert np.array_equal(x, x1) and np.array_equal(deg, deg1)
        assert np.array_equal(_bits(lz), _bits(out[0][1]))


@pytest.mark.parametrize("stride", [0, 5, 1000])
def test_rows_split_over_two_calls(ctx, stride):
    c = _case(ctx, "alarm")
    b0 = 30
    args = dict(seed=SEED, row_stride=stride, dtype=bnpp.F64)
    x, lz, deg = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"], K, first_sample=FIRST, **args)
    xa, lza, dega = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"][:b0], K, first_sample=FIRST, **args)
    xb, lzb, degb = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"][b0:], K, first_sample=FIRST + b0 * stride, **args)
    assert np.array_equal(np.concatenate([xa, xb]), x)
    assert np.array_equal(np.concatenate([dega, degb]), deg)
    assert np.array_equal(_bits(np.concatenate([lza, lzb])), _bits(lz))


def _impossible(ctx, name):
    c = _case(ctx, name)
    b = c["bad"]
    assert b == N_ROWS // 2 and c["z1"][b] == 0
    got = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"], K, seed=SEED, first_sample=FIRST, row_stride=5,
                            dtype=bnpp.F64, rows_per_launch=N_ROWS)
    return c, b, got


@pytest.mark.parametrize("name", ["asia", "alarm"])
def test_impossible_row_is_the_single_calls_and_leaves_its_neighbours_alone(ctx, name):
    """Its log10_z is -inf, its bytes and its count of degenerate draws are the
    single call's, and its neighbours are what they are with a possible row in
    its place."""
    c, b, (x, lz, deg) = _impossible(ctx, name)
    x1, deg1 = _single(ctx, name, "f64")[5]
    assert lz[b] == -np.inf and np.array_equal(x[b], x1[b]) and deg[b] == deg1[b]
    ok = np.flatnonzero(c["z1"] > 0)
    rows = c["rows"].copy()
    rows[b] = rows[ok[-1]]
    x2, lz2, deg2 = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], rows, K, seed=SEED, first_sample=FIRST, row_stride=5,
                                      dtype=bnpp.F64, rows_per_launch=N_ROWS)
    keep = np.arange(N_ROWS) != b
    assert np.array_equal(x2[keep], x[keep]) and np.array_equal(deg2[keep], deg[keep])
    assert np.array_equal(_bits(lz2[keep]), _bits(lz[keep]))
    assert lz2[b] == lz[ok[-1]] and deg2[b] == 0


@pytest.mark.parametrize("name", ["asia", "alarm"])
def test_impossible_row_draws_only_degenerate_zeros(ctx, name):
    """All sampled bytes of the impossible row are 0, its n_degenerate is
    positive -- every draw of every sampled variable -- and equals the single
    call's, and its log10_z is -inf.  The impossible rows of these cases
    observe the whole scope of the CPT with the zero entry, so the zero reaches
    the result and the bucket of no draw: the rule is the call's (Z = 0: there
    is no posterior to draw from), not a property of the weights."""
    c, b, (x, lz, deg) = _impossible(ctx, name)
    free = [v for v in range(c["m"].n_vars) if v not in c["ev_vars"]]
    print(name, "impossible row", b, "n_degenerate", deg[b], "non-zero sampled bytes", int((x[b][:, free] != 0).sum()))
    assert lz[b] == -np.inf
    assert not x[b][:, free].any()
    assert deg[b] > 0 and deg[b] == K * len(free)
    x1, _, deg1 = bnpp.sample(ctx, c["m"], K, _ev(c, b), seed=SEED, first_sample=FIRST + b * 5, dtype=bnpp.F64)
    assert deg1 == deg[b] and np.array_equal(x1, x[b])


def test_one_row(ctx):
    c = _case(ctx, "alarm")
    x1, deg1 = _single(ctx, "alarm", "f64")[0]
    x, lz, deg = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"][9:10], K, seed=SEED, first_sample=FIRST)
    assert x.shape == (1, K, c["m"].n_vars) and np.array_equal(x[0], x1[9]) and deg[0] == deg1[9]
    assert _bits(lz)[0] == _bits(bnpp.partition_batch(ctx, c["m"], c["ev_vars"], c["rows"][9:10])[0])[0]


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_no_evidence_variables(ctx, dt):
    """n_ev = 0: no gather step, no row variable; row b is bnpp.sample at first + b * stride."""
    c = _case(ctx, "alarm")
    x1, lz1, deg1 = bnpp.sample(ctx, c["m"], 4 * 6, {}, seed=SEED, first_sample=FIRST, dtype=DT[dt])
    x, lz, deg = bnpp.sample_batch(ctx, c["m"], [], np.zeros((4, 0), dtype=np.int64), 6, seed=SEED, first_sample=FIRST,
                                   dtype=DT[dt])
    assert x.shape == (4, 6, c["m"].n_vars) and np.array_equal(x.reshape(24, -1), x1)
    assert deg.sum() == deg1 == 0
    lzb, _, _ = bnpp.partition_batch(ctx, c["m"], [], np.zeros((4, 0), dtype=np.int64), dtype=DT[dt])
    assert np.array_equal(_bits(lz), _bits(lzb))


def test_every_variable_is_evidence(ctx):
    """cancer, all five variables observed: every sample is the row itself."""
    c = _case(ctx, "cancer")
    cards = c["d"]["cards"]
    ev_vars = list(range(len(cards)))
    rows = batch_ref.draw_rows(cards, ev_vars, 9, 3)
    x, lz, deg = bnpp.sample_batch(ctx, c["m"], ev_vars, rows, 3, seed=SEED)
    assert np.array_equal(x, np.broadcast_to(rows[:, None, :], (9, 3, len(cards)))) and not deg.any()
    lzb, _, _ = bnpp.partition_batch(ctx, c["m"], ev_vars, rows)
    assert np.array_equal(_bits(lz), _bits(lzb))


@pytest.mark.parametrize("name", sbr.DIST_MODELS)
def test_distribution(ctx, name):
    """Independent of the single call: 8 distinct possible rows, 4096 draws each
    from disjoint streams; every single-variable frequency of every row within
    sample_ref.bound of the brute-force posterior.  (test_sample_batch_host.py
    puts the same bound on the restatement alone for these inputs.)"""
    path = model_path(name + ".uai")
    m, d = bnpp.Model.load(path), synth.read_uai(path)
    ev_vars, rows = sbr.dist_case(d)
    x, lz, deg = bnpp.sample_batch(ctx, m, ev_vars, rows, sbr.DIST_K, seed=sbr.DIST_SEED, first_sample=sbr.DIST_FIRST,
                                   row_stride=sbr.DIST_K, dtype=bnpp.F64)
    assert not deg.any() and np.isfinite(lz).all()
    bad = sbr.frequency_violations(d, ev_vars, rows, x)
    assert not bad, bad[:3]
    # common random numbers: with row_stride 0 two equal rows give equal samples
    twice = rows[[2, 5, 2]]
    x0, _, _ = bnpp.sample_batch(ctx, m, ev_vars, twice, 64, seed=sbr.DIST_SEED, row_stride=0)
    assert np.array_equal(x0[0], x0[2]) and not np.array_equal(x0[0], x0[1])


def test_impute_completes_the_rows(ctx):
    c = _case(ctx, "cancer")
    x = learn.impute(ctx, c["m"], c["ev_vars"], c["rows"], k=2, seed=SEED)
    want, _, _ = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], c["rows"], 2, seed=SEED)
    assert x.shape == (N_ROWS, 2, c["m"].n_vars) and np.array_equal(x, want)
    assert np.array_equal(x[:, 0, c["ev_vars"]], c["rows"])


def test_cached_job_relaunches_with_other_values_and_seed(ctx):
    c = _case(ctx, "alarm")
    x1, _ = _single(ctx, "alarm", "f64")[5]
    a, b = c["rows"][:32], c["rows"][32:64]
    bnpp.sample_batch(ctx, c["m"], c["ev_vars"], a, K, seed=1, rows_per_launch=32)
    xb, _, _ = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], b, K, seed=SEED, first_sample=FIRST + 32 * 5, row_stride=5,
                                 rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] == 0, "the second call planned again"
    assert np.array_equal(xb, x1[32:64])
    # another K is another plan
    bnpp.sample_batch(ctx, c["m"], c["ev_vars"], a, K + 1, seed=SEED, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] > 0
    # a partition batch on the same variables is another job kind: it plans, and so does the sampling call after it
    bnpp.partition_batch(ctx, c["m"], c["ev_vars"], a, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] > 0
    xa, _, _ = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], a, K, seed=SEED, first_sample=FIRST, row_stride=5, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] > 0 and np.array_equal(xa, x1[:32])


def test_cli_sample_batch(ctx, tmp_path):
    c = _case(ctx, "asia")
    rows = c["rows"][[0, c["bad"], 40]]
    evid = tmp_path / "three.evid"
    evid.write_text("3\n" + "".join(
        "%d %s\n" % (len(c["ev_vars"]), " ".join("%d %d" % (v, x) for v, x in zip(c["ev_vars"], r))) for r in rows))
    base = str(tmp_path / "out")
    exe = os.path.join(REPO, "bn-pp_amd", "bin", "bnpp")
    p = subprocess.run([exe, model_path("asia.uai"), str(evid), "-sample-batch", "4", "-seed", "7", "-uai", base],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    x, _, _ = bnpp.sample_batch(ctx, c["m"], c["ev_vars"], rows, 4, seed=7)
    with open(base + ".SAMPLES") as f:
        lines = f.read().split("\n")
    n = c["m"].n_vars
    assert lines[0] == "SAMPLES" and lines[1] == "3 4 %d" % n and lines[-1] == ""
    assert lines[2:-1] == [" ".join(str(int(v)) for v in s) for s in x.reshape(12, n)]
    assert ">> First sample: " + lines[2] + "\n" in p.stdout
    assert not any(os.path.exists(base + e) for e in (".PR", ".MAR", ".MPE"))
