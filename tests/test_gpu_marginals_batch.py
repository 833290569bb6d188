"""GPU tests of whole bnpp.marginals_batch runs: against brute force, against
the single calls (bnpp.marginals per row, bnpp.posterior_batch per target),
across rows per launch, splits over calls and grid caps (bit for bit in fp64),
target subsets, an impossible row, no evidence, expected_counts, a cached job,
learn.classify, the CLI and the C++ mirror.

Tolerances: the bucket-tree MAR tolerances the project states
(tests/test_gpu_bucket_tree.py, tests/test_gpu_counts.py) -- 1e-12 absolute in
fp64, 1e-5 in fp32.
"""
import os
import subprocess

import numpy as np
import pytest

import batch_ref
import bnpp
import marginals_batch_ref
from bnpp import learn, synth
from conftest import REPO, model_path
from counts_ref import EV_VARS

pytestmark = pytest.mark.gpu

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
TOL = {"f64": 1e-12, "f32": 1e-5}
LIB = os.path.join(REPO, "bn-pp_amd", "lib")

# two components, {0, 1} and {2, 3}, and variable 4 in no factor
SPLIT = dict(type="MARKOV", cards=[2, 3, 2, 4, 5], scopes=[[0, 1], [2, 3], [3]],
             values=[[0.5, 1.0, 2.0, 0.25, 0.75, 1.5], [1.0, 0.5, 0.25, 2.0, 0.125, 1.0, 3.0, 0.5], [1.0, 2.0, 0.5, 1.5]])


@pytest.fixture
def grid_cap(ctx):
    yield ctx.set_max_grid
    ctx.set_max_grid(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_CASES = {}


def _case(ctx, name, n):
    key = (name, n)
    if key not in _CASES:
        path = model_path(name + ".uai")
        m, d = bnpp.Model.load(path), synth.read_uai(path)
        samples, _, _ = bnpp.sample(ctx, m, max(n, 2), seed=7)
        rows = batch_ref.draw_rows(d["cards"], EV_VARS[name], n, 11, samples)
        _CASES[key] = dict(m=m, d=d, ev=EV_VARS[name], rows=rows)
    return _CASES[key]


_BRUTE = {}


def _brute(c, name, n):
    if (name, n) not in _BRUTE:
        _BRUTE[(name, n)] = marginals_batch_ref.brute_marginals(c["d"], c["ev"], c["rows"])
    return _BRUTE[(name, n)]


def _belief_cols(cards, ev, targets=None):
    """The columns of an (n, W) array that belong to targets that are no evidence variables."""
    ts = list(range(len(cards))) if targets is None else targets
    return np.concatenate([np.full(cards[t], t not in ev) for t in ts])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 5, 130])
@pytest.mark.parametrize("name", ["asia", "cancer", "earthquake", "ising4x4"])
def test_whole_run_against_brute_force(ctx, name, n, dt):
    c = _case(ctx, name, n)
    want, z = _brute(c, name, n)
    out, lz = bnpp.marginals_batch(ctx, c["m"], c["ev"], c["rows"], dtype=DT[dt])
    ok = z > 0
    assert out.shape == want.shape and np.array_equal(np.isfinite(lz), ok) and ok.any()
    worst = float(np.abs(out[ok] - want[ok]).max())
    sums = [b[ok].sum(axis=1) for b in bnpp.split_marginals(c["d"]["cards"], None, out)]
    worst_sum = max(float(np.abs(s - 1).max()) for s in sums)
    print(name, n, dt, "worst |marginal - brute|", worst, "worst |block sum - 1|", worst_sum, "bound", TOL[dt])
    assert worst <= TOL[dt] and worst_sum <= TOL[dt]
    # an impossible row: NaN in its belief columns, its evidence columns one-hot
    bel = _belief_cols(c["d"]["cards"], c["ev"])
    assert np.isnan(out[~ok][:, bel]).all() and np.array_equal(out[~ok][:, ~bel], want[~ok][:, ~bel])
    assert np.allclose(lz[ok], np.log10(z[ok]), rtol=0, atol=1e-5 if dt == "f32" else 1e-11)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["alarm", "ising6x6", "potts4x5k3", "noisyor_30_40"])
def test_against_the_single_calls(ctx, name, dt):
    c = _case(ctx, name, 12)
    m, d, ev = c["m"], c["d"], c["ev"]
    rows = c["rows"][6:]                                    # drawn from joint samples: possible rows
    out, lz = bnpp.marginals_batch(ctx, m, ev, rows, dtype=DT[dt])
    assert np.isfinite(lz).all()
    per = bnpp.split_marginals(d["cards"], None, out)
    worst_single = worst_post = 0.0
    for b, row in enumerate(rows):
        marg, _ = bnpp.marginals(ctx, m, dict(zip(ev, (int(x) for x in row))), dtype=DT[dt])
        for t in range(m.n_vars):
            worst_single = max(worst_single, float(np.abs(per[t][b] - np.asarray(marg[t])).max()))
    for t in range(m.n_vars):
        if t in ev:
            assert np.array_equal(per[t], np.eye(d["cards"][t])[rows[:, ev.index(t)]])
        else:
            post, _ = bnpp.posterior_batch(ctx, m, ev, rows, t, dtype=DT[dt])
            worst_post = max(worst_post, float(np.abs(per[t] - post).max()))
    print(name, dt, "worst vs marginals", worst_single, "worst vs posterior_batch", worst_post, "bound", TOL[dt])
    assert worst_single <= TOL[dt] and worst_post <= TOL[dt]


def test_log10_z_has_the_bits_of_partition_batch(ctx):
    c = _case(ctx, "alarm", 130)
    lzb, _, _ = bnpp.partition_batch(ctx, c["m"], c["ev"], c["rows"], dtype=bnpp.F64)
    _, lz = bnpp.marginals_batch(ctx, c["m"], c["ev"], c["rows"], dtype=bnpp.F64)
    assert np.array_equal(_bits(lz), _bits(lzb)) and np.isfinite(lz).any()
    lzb, _, _ = bnpp.partition_batch(ctx, c["m"], c["ev"], c["rows"], dtype=bnpp.F32, rows_per_launch=64)
    _, lz = bnpp.marginals_batch(ctx, c["m"], c["ev"], c["rows"], dtype=bnpp.F32, rows_per_launch=64)
    assert np.array_equal(_bits(lz), _bits(lzb))


def test_rows_per_launch_splits_and_grid_caps_fp64_bit_identical(ctx, grid_cap):
    """130 rows: R = 3 and 64 end on a padded launch, R = 1 makes 130 launches."""
    c = _case(ctx, "alarm", 130)
    m, ev, rows = c["m"], c["ev"], c["rows"]
    ref, ref_lz = bnpp.marginals_batch(ctx, m, ev, rows, rows_per_launch=1)
    assert np.isfinite(ref).any() and ref.shape == (130, sum(c["d"]["cards"]))
    for R in (3, 64, 0):
        out, lz = bnpp.marginals_batch(ctx, m, ev, rows, rows_per_launch=R)
        assert np.array_equal(_bits(out), _bits(ref)), (R, np.argwhere(_bits(out) != _bits(ref))[:8])
        assert np.array_equal(_bits(lz), _bits(ref_lz))
    a, _ = bnpp.marginals_batch(ctx, m, ev, rows[:47])
    b, _ = bnpp.marginals_batch(ctx, m, ev, rows[47:])
    assert np.array_equal(_bits(np.concatenate([a, b])), _bits(ref)), "rows split over two calls"
    for cap in (1, 2, 3):
        grid_cap(cap)
        out, _ = bnpp.marginals_batch(ctx, m, ev, rows, rows_per_launch=64)
        assert np.array_equal(_bits(out), _bits(ref)), ("grid cap", cap)


def test_target_subsets(ctx):
    c = _case(ctx, "alarm", 130)
    m, d, ev, rows = c["m"], c["d"], c["ev"], c["rows"][65:98]
    full, _ = bnpp.marginals_batch(ctx, m, ev, rows)
    every = bnpp.split_marginals(d["cards"], None, full)
    none, _ = bnpp.marginals_batch(ctx, m, ev, rows, targets=None)
    assert np.array_equal(_bits(none), _bits(full))
    targets = [30, ev[1], 2, 17, 0]                         # a subset, permuted, an evidence variable among it
    sub, lz = bnpp.marginals_batch(ctx, m, ev, rows, targets=targets)
    assert sub.shape == (len(rows), sum(d["cards"][t] for t in targets)) and np.isfinite(lz).all()
    for t, blk in zip(targets, bnpp.split_marginals(d["cards"], targets, sub)):
        if t in ev:
            assert np.array_equal(blk, np.eye(d["cards"][t])[rows[:, ev.index(t)]]), "one-hot of each row's value"
        assert np.abs(blk - every[t]).max() <= 1e-12, t
    one, _ = bnpp.marginals_batch(ctx, m, ev, rows, targets=[ev[0]])
    assert np.array_equal(one, np.eye(d["cards"][ev[0]])[rows[:, 0]])


def test_a_given_result_array_is_written_in_place(ctx):
    c = _case(ctx, "alarm", 130)
    m, ev, rows = c["m"], c["ev"], c["rows"]
    ref, _ = bnpp.marginals_batch(ctx, m, ev, rows, rows_per_launch=64)
    mine = np.full(ref.shape, -7.0)
    got, _ = bnpp.marginals_batch(ctx, m, ev, rows, rows_per_launch=64, out=mine)
    assert np.shares_memory(got, mine) and np.array_equal(_bits(mine), _bits(ref))
    with pytest.raises(ValueError):
        bnpp.marginals_batch(ctx, m, ev, rows, out=np.zeros((130, 7)))
    with pytest.raises(ValueError):
        bnpp.marginals_batch(ctx, m, ev, rows, out=np.zeros(ref.shape, dtype=np.float32))


def test_every_column_kind_in_one_run(ctx):
    """A belief with the row variable, an evidence block, beliefs no evidence reaches and a free block."""
    m = bnpp.Model.from_dict(SPLIT)
    rows = np.array([[0], [2], [1], [2], [0]])
    for dt in ("f64", "f32"):
        out, lz = bnpp.marginals_batch(ctx, m, [1], rows, dtype=DT[dt])
        want, z = marginals_batch_ref.brute_marginals(SPLIT, [1], rows)
        assert np.abs(out - want).max() <= TOL[dt] and np.allclose(lz, np.log10(z), rtol=0, atol=1e-5)
        assert np.array_equal(out[:, 11:], np.full((5, 5), 0.2))
    # the evidence variable sits in no factor: no gather step, and its block is still the rows' one-hot
    rows = np.array([[4], [0], [3]])
    out, lz = bnpp.marginals_batch(ctx, m, [4], rows)
    want, z = marginals_batch_ref.brute_marginals(SPLIT, [4], rows)
    assert np.abs(out - want).max() <= 1e-12 and np.array_equal(out[:, 11:], np.eye(5)[rows[:, 0]])
    assert _bits(lz).tolist() == [_bits(lz)[0]] * 3


def test_an_impossible_row(ctx):
    c = _case(ctx, "asia", 65)
    d = c["d"]
    # the evidence variables: the scope of asia's first CPT with an entry that is exactly 0; that entry is the row
    zero = next((list(s), np.asarray(v).reshape([d["cards"][x] for x in s])) for s, v in zip(d["scopes"], d["values"])
                if len(s) >= 2 and (np.asarray(v) == 0).any())
    ev = sorted(zero[0])
    at = np.argwhere(zero[1] == 0)[0]
    bad_row = np.array([[int(at[zero[0].index(v)]) for v in ev]])
    samples, _, _ = bnpp.sample(ctx, c["m"], 40, seed=9)
    good = np.asarray(samples)[:, ev].astype(np.int64)
    _, z = marginals_batch_ref.brute_marginals(d, ev, np.concatenate([bad_row, good]))
    assert z[0] == 0 and (z[1:] > 0).all()
    with_bad = np.concatenate([good[:7], bad_row, good[7:]])
    a, lza = bnpp.marginals_batch(ctx, c["m"], ev, with_bad, rows_per_launch=8)
    b, lzb = bnpp.marginals_batch(ctx, c["m"], ev, good, rows_per_launch=8)
    bel = _belief_cols(d["cards"], ev)
    assert lza[7] == -np.inf and np.isnan(a[7][bel]).all()
    assert np.array_equal(a[7][~bel], np.concatenate([np.eye(d["cards"][v])[x] for v, x in zip(ev, bad_row[0])]))
    assert np.array_equal(_bits(np.delete(a, 7, axis=0)), _bits(b)) and not np.isnan(b).any()
    assert np.array_equal(_bits(np.delete(lza, 7)), _bits(lzb))


def test_no_evidence_variables(ctx):
    c = _case(ctx, "asia", 65)
    out, lz = bnpp.marginals_batch(ctx, c["m"], [], np.zeros((5, 0), dtype=np.int64))
    marg, _ = bnpp.marginals_tree(ctx, c["m"], {}, dtype=bnpp.F64)
    want = np.concatenate([np.asarray(marg[t]) for t in range(c["m"].n_vars)])
    assert out.shape == (5, len(want)) and len(lz) == 5
    assert np.abs(out - want).max() <= 1e-12
    assert all(np.array_equal(_bits(out[b]), _bits(out[0])) for b in range(5))


@pytest.mark.parametrize("name", ["alarm", "ising6x6"])
def test_consistency_with_expected_counts(ctx, name):
    n = 33
    c = _case(ctx, name, n)
    d, ev, rows = c["d"], c["ev"], c["rows"]
    counts, lz, n_imp = bnpp.expected_counts(ctx, c["m"], ev, rows, dtype=bnpp.F64)
    out, lzm = bnpp.marginals_batch(ctx, c["m"], ev, rows, dtype=bnpp.F64)
    ok = np.isfinite(lz)
    assert np.array_equal(_bits(lz), _bits(lzm)) and n_imp == int((~ok).sum()) <= n / 2
    mine = [blk[ok].sum(axis=0) for blk in bnpp.split_marginals(d["cards"], None, out)]
    for s, N in zip(d["scopes"], bnpp.split_counts(d, counts)):
        for ax, v in enumerate(s):
            marg = N.sum(axis=tuple(a for a in range(len(s)) if a != ax))
            assert np.abs(marg - mine[v]).max() <= n * 1e-12, (s, v, marg, mine[v])


def test_cached_job_relaunches_with_other_values(ctx):
    c = _case(ctx, "alarm", 130)
    m, ev = c["m"], c["ev"]
    a, b = c["rows"][:32], c["rows"][32:64]
    fresh_b, _ = bnpp.marginals_batch(ctx, m, ev, b, rows_per_launch=32)
    bnpp.marginals_batch(ctx, m, ev, a, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] == 0, "other values planned again"
    again_b, _ = bnpp.marginals_batch(ctx, m, ev, b, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] == 0, "the second call planned again"
    assert np.array_equal(_bits(again_b), _bits(fresh_b))
    bnpp.marginals_batch(ctx, m, ev, b, targets=[5, 6], rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] > 0, "another target list must plan afresh"
    bnpp.marginals_batch(ctx, m, ev, b, targets=[6, 5], rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] > 0, "the targets' order is part of the plan"
    bnpp.expected_counts(ctx, m, ev, b, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] > 0, "a counts job is another kind"


def test_classify_on_asia(ctx):
    c = _case(ctx, "asia", 130)
    want, z = _brute(c, "asia", 130)
    ok = z > 0
    targets = [t for t in range(c["m"].n_vars) if t not in c["ev"]][::-1]
    labels, out = learn.classify(ctx, c["m"], c["ev"], c["rows"][ok], targets)
    per = bnpp.split_marginals(c["d"]["cards"], None, want[ok])
    # brute force decides wherever its own margin is above both tolerances
    for j, t in enumerate(targets):
        top = np.sort(per[t], axis=1)
        clear = top[:, -1] - top[:, -2] > 1e-9
        assert clear.sum() > ok.sum() / 2
        assert np.array_equal(labels[clear, j], np.argmax(per[t], axis=1)[clear]), t
    assert labels.shape == (ok.sum(), len(targets)) and out.shape[1] == sum(c["d"]["cards"][t] for t in targets)
    assert np.array_equal(labels, learn.argmax_marginals(c["d"]["cards"], targets, out))


def _write_evid(path, ev, rows):
    path.write_text("%d\n" % len(rows) + "".join(
        "%d %s\n" % (len(ev), " ".join("%d %d" % (v, x) for v, x in zip(ev, r))) for r in rows))


def test_cli_mar_batch(ctx, tmp_path):
    c = _case(ctx, "asia", 65)
    rows = c["rows"][33:42]
    evid = tmp_path / "nine.evid"
    _write_evid(evid, c["ev"], rows)
    base = str(tmp_path / "out")
    exe = os.path.join(REPO, "bn-pp_amd", "bin", "bnpp")
    p = subprocess.run([exe, model_path("asia.uai"), str(evid), "-mar-batch", "-uai", base], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    lines = open(base + ".MAR").read().split("\n")
    assert lines[0] == "MAR" and int(lines[1]) == len(rows)
    out, lz = bnpp.marginals_batch(ctx, c["m"], c["ev"], rows)
    cards = c["d"]["cards"]
    for r in range(len(rows)):
        tok = lines[2 + r].split()
        assert int(tok[0]) == len(cards)
        got, at = [], 1
        for k in cards:
            assert int(tok[at]) == k
            got += [float(x) for x in tok[at + 1:at + 1 + k]]
            at += 1 + k
        assert at == len(tok) and np.array_equal(_bits(got), _bits(out[r])), r
    assert p.stdout.count(">> MAR row ") == len(rows)


def test_cpp_mirror(ctx, tmp_path):
    exe = str(tmp_path / "marginals_batch_check")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests", "cpp", "marginals_batch_check.cpp"),
                    "-I" + os.path.join(REPO, "include"), "-L" + LIB, "-lbnpp", "-Wl,-rpath," + LIB, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    c = _case(ctx, "asia", 65)
    rows = c["rows"][33:40]
    evid = tmp_path / "seven.evid"
    _write_evid(evid, c["ev"], rows)
    for targets in (None, [5, c["ev"][0], 1]):
        p = subprocess.run([exe, model_path("asia.uai"), str(evid)] + [str(t) for t in targets or []], capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        out, lz = bnpp.marginals_batch(ctx, c["m"], c["ev"], rows, targets=targets)
        got = [line.split("|") for line in p.stdout.strip().split("\n")]
        assert len(got) == len(rows)
        assert np.array_equal(_bits([float(g[0]) for g in got]), _bits(lz))
        assert np.array_equal(_bits([[float(x) for x in g[1].split()] for g in got]), _bits(out))
