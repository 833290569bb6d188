"""GPU tests of posterior sampling: bnpp_bucket_sample one draw at a time and
whole bnpp.sample runs against the numpy restatement (sample_ref.py).

  * single ops: the written row is identical to sample_ref.draw in the dtype
    of the run, x sits between guard bands that stay untouched, as do the rows
    of the other variables; inputs from {0, 0.5, 1} with all-zero rows: a value
    of zero weight is never drawn, all-zero rows give 0 and are counted.
  * a sample depends on (seed, global index) only: capped grids and split
    ranges give identical rows.
  * whole fp64 runs are bit for bit sample_ref.run with the engine's order.
  * distribution at n = 65536, fixed seed: every compared frequency within
    sample_ref.bound (five binomial standard deviations + 4 / n) of the exact
    probability: brute force on the small models, bnpp.marginals_tree (fp64) on
    the larger ones.
"""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import bnpp
import mpe_ref
import sample_ref as sr
from bnpp import synth
from conftest import REPO, evidence_of, model_path

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"f64": torch.float64, "f32": torch.float32}
ND = {"f64": np.float64, "f32": np.float32}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
GUARD = 64
SEED = 20261019
N_DIST = 65536
SMALL = [("asia", "-"), ("asia", "asia.uai.evid"), ("cancer", "-"), ("cancer", "cancer.uai.evid"),
         ("earthquake", "-"), ("earthquake", "earthquake.uai.evid"), ("grid3x3", "-"),
         ("grid3x3", "grid3x3-PR.uai.evid"), ("ising4x4", "-")]
LARGER = [("alarm", "alarm.uai.evid"), ("noisyor_50_80", "noisyor_50_80.uai.evid"), ("potts4x5k3", "-"),
          ("Munin1", "-")]

# the smallest shapes that reach each branch: n_in 0, 1, 2 (the two-slot row
# form) and 4, 5, 8 (the eight-slot form); var in every input, in some (stride
# 0), in none; var slowest, in the middle, fastest; cards 2, 3, 7, 256;
# n_samples around the wave (63, 64, 65), a partial last block (257, 1000)
CASES = [
    dict(name="n0_uniform", cards=[7], scopes=[], var=0, n=65),
    dict(name="n1_alone", cards=[3], scopes=[[0]], var=0, n=1),
    dict(name="n1_slowest", cards=[3, 5, 2], scopes=[[0, 1, 2]], var=0, n=63),
    dict(name="n1_middle", cards=[3, 5, 2], scopes=[[0, 1, 2]], var=1, n=64),
    dict(name="n1_fastest", cards=[3, 5, 2], scopes=[[0, 1, 2]], var=2, n=65),
    dict(name="n1_absent", cards=[7, 3, 2], scopes=[[1, 2]], var=0, n=64),
    dict(name="n2_both", cards=[7, 3, 2], scopes=[[0, 1], [2, 0]], var=0, n=257),
    dict(name="n2_some", cards=[3, 7, 2], scopes=[[0, 1], [1, 2]], var=0, n=257),
    dict(name="n2_card256", cards=[256, 3], scopes=[[1, 0], [0]], var=0, n=1000),
    dict(name="n4", cards=[2, 3, 7, 2, 3], scopes=[[0, 1], [2, 0], [3, 4], [1, 0, 4]], var=0, n=1000),
    dict(name="n5", cards=[7, 2, 3, 2, 3], scopes=[[1, 0], [0, 2], [3], [4, 1, 0], [2, 3]], var=0, n=65),
    dict(name="n8", cards=[3, 2, 7, 2, 3, 2], scopes=[[0, 1], [2, 0], [0], [3, 0, 4], [5], [1, 2], [4, 5, 0], [0, 3]],
         var=0, n=1000),
    dict(name="n8_card256", cards=[256, 2, 3], scopes=[[0, 1], [2, 0], [0], [1], [2], [1, 0, 2], [2, 1], [0]], var=0, n=257),
]


@pytest.fixture(scope="module")
def stream():
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    return s.cuda_stream


@pytest.fixture
def grid_cap(ctx):
    yield ctx.set_max_grid
    ctx.set_max_grid(0)


def _size(cards, scope):
    n = 1
    for v in scope:
        n *= cards[v]
    return n


def _inputs(case, seed, ties):
    """Tables of the case: positive values, or {0, 0.5, 1} with every entry of
    input 0 zeroed where its first other variable is 0 (all-zero rows)."""
    rng = np.random.default_rng(seed)
    ins = []
    for i, s in enumerate(case["scopes"]):
        n = _size(case["cards"], s)
        if not ties:
            ins.append(rng.uniform(0.05, 1.0, n))
            continue
        t = rng.choice([0.0, 0.5, 1.0], size=n, p=[0.4, 0.3, 0.3]).reshape([case["cards"][v] for v in s])
        others = [j for j, v in enumerate(s) if v != case["var"]]
        if i == 0 and others:
            t[tuple(0 if j == others[0] else slice(None) for j in range(len(s)))] = 0.0
        ins.append(t.reshape(-1))
    return ins


def _state(case, seed):
    rng = np.random.default_rng(seed + 1)
    return np.stack([rng.integers(0, min(c, 256), case["n"]).astype(np.uint8) for c in case["cards"]])


def _run_draw(ctx, stream, case, dt, ins, x0, seed=SEED, first=0, n=None, tabs=None, scopes=None, col0=0):
    """One bnpp_bucket_sample call on samples [col0, col0 + n) of the state x0,
    inside guard bands -> (x after the call, n_degenerate)."""
    n = case["n"] if n is None else n
    nc = len(case["cards"])
    xs = np.ascontiguousarray(x0[:, col0:col0 + n])
    if tabs is None:
        tabs = [torch.tensor(v, dtype=TD[dt], device=DEV) for v in ins]
    buf = torch.full((nc * n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    buf[GUARD:GUARD + nc * n] = torch.tensor(xs.reshape(-1), dtype=torch.uint8, device=DEV)
    cnt = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    bnpp.bucket_sample(ctx, DT[dt], case["cards"], [t.data_ptr() for t in tabs], scopes or case["scopes"], case["var"],
                       n, buf[GUARD:].data_ptr(), seed=seed, first_sample=first, n_degenerate=cnt[1:].data_ptr(),
                       stream=stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    c = cnt.cpu().numpy()
    assert (got[:GUARD] == 0xAB).all() and (got[GUARD + nc * n:] == 0xAB).all(), ("guard band written", case["name"])
    assert c[0] == -1 and c[2] == -1
    x = got[GUARD:GUARD + nc * n].reshape(nc, n)
    keep = [v for v in range(nc) if v != case["var"]]
    assert np.array_equal(x[keep], xs[keep]), ("another variable's row written", case["name"])
    return x, int(c[1])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ties", [False, True])
def test_single_op_bit_for_bit(ctx, stream, dt, ties):
    big = 0
    for i, case in enumerate(CASES):
        ins = [np.asarray(t, dtype=ND[dt]) for t in _inputs(case, 100 + i, ties)]
        x0 = _state(case, 100 + i)
        want, wdeg = sr.draw(ins, case["scopes"], case["cards"], case["var"], x0, SEED, 0, ND[dt])
        x, deg = _run_draw(ctx, stream, case, dt, ins, x0)
        row = x[case["var"]]
        assert np.array_equal(row, want), (case["name"], int((row != want).sum()))
        assert deg == wdeg, (case["name"], deg, wdeg)
        assert (row < case["cards"][case["var"]]).all()
        big = max(big, int(row.max()))
        if ties:
            p = sr.weights(ins, case["scopes"], case["cards"], case["var"], x0, ND[dt])
            cols = np.arange(case["n"])
            zero_row = ~(p > 0).any(axis=0)
            assert (p[row, cols] > 0)[~zero_row].all(), case["name"]     # never a value of zero weight
            assert not row[zero_row].any() and deg == int(zero_row.sum())  # all-zero rows: 0, counted
            if any(len([v for v in s if v != case["var"]]) for s in case["scopes"][:1]):
                assert deg > 0, case["name"]
        else:
            assert deg == 0
    assert big > 127                                                     # the byte is unsigned


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_single_op_view_at_an_offset(ctx, stream, dt):
    """Variable 4, slowest in two inputs, conditioned on value 2: the tables'
    addresses move past two slices (a view's base offset)."""
    cards = [3, 5, 6, 4, 3]
    full_scopes = [[4, 0, 1, 2, 3], [4, 3, 0], [2, 1]]
    scopes = [[0, 1, 2, 3], [3, 0], [2, 1]]
    case = dict(name="offset", cards=cards, scopes=scopes, var=0, n=257)
    rng = np.random.default_rng(77)
    full = [rng.uniform(0.05, 1.0, _size(cards, s)).astype(ND[dt]) for s in full_scopes]
    sl = [_size(cards, s) for s in scopes]
    ins = [full[0][2 * sl[0]:3 * sl[0]], full[1][2 * sl[1]:3 * sl[1]], full[2]]
    x0 = _state(case, 77)
    want, _ = sr.draw(ins, scopes, cards, 0, x0, SEED, 0, ND[dt])
    bigt = [torch.tensor(v, dtype=TD[dt], device=DEV) for v in full]
    tabs = [bigt[0][2 * sl[0]:], bigt[1][2 * sl[1]:], bigt[2]]
    x, deg = _run_draw(ctx, stream, case, dt, None, x0, tabs=tabs)
    assert np.array_equal(x[0], want) and deg == 0


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_grid_and_split_independence_single_op(ctx, stream, grid_cap, dt):
    for name in ("n4", "n8"):
        case = next(c for c in CASES if c["name"] == name)
        assert case["n"] == 1000
        ins = [np.asarray(t, dtype=ND[dt]) for t in _inputs(case, 5, False)]
        x0 = _state(case, 5)
        want, _ = sr.draw(ins, case["scopes"], case["cards"], case["var"], x0, SEED, 0, ND[dt])
        for cap in (1, 2, 3):
            grid_cap(cap)
            x, _ = _run_draw(ctx, stream, case, dt, ins, x0)
            assert np.array_equal(x[case["var"]], want), (name, cap)
        grid_cap(0)
        a, _ = _run_draw(ctx, stream, case, dt, ins, x0, n=300)
        b, _ = _run_draw(ctx, stream, case, dt, ins, x0, n=700, first=300, col0=300)
        assert np.array_equal(np.concatenate([a[case["var"]], b[case["var"]]]), want), name


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_grid_and_split_independence_whole_model(grid_cap, dt):
    c = bnpp.Context(0)
    try:
        mm = bnpp.Model.load(model_path("alarm.uai"))
        ev = evidence_of("alarm.uai.evid")
        whole = bnpp.sample(c, mm, 1000, ev, seed=SEED, dtype=DT[dt])[0].copy()
        a = bnpp.sample(c, mm, 300, ev, seed=SEED, dtype=DT[dt])[0].copy()
        b = bnpp.sample(c, mm, 700, ev, seed=SEED, first_sample=300, dtype=DT[dt])[0].copy()
        assert np.array_equal(np.concatenate([a, b]), whole)
        for cap in (1, 2, 3):
            c.set_max_grid(cap)
            assert np.array_equal(bnpp.sample(c, mm, 1000, ev, seed=SEED, dtype=DT[dt])[0], whole), cap
    finally:
        c.close()


@pytest.mark.parametrize("name,evf", SMALL)
def test_whole_runs_fp64_bit_for_bit(ctx, name, evf):
    m = synth.read_uai(model_path(name + ".uai"))
    mm = bnpp.Model.load(model_path(name + ".uai"))
    ev = evidence_of(evf)
    order, _ = bnpp.ordering(mm, ev)
    want, wdeg = sr.run(m, ev, order, 4096, SEED, np.float64)
    got, lz, deg = bnpp.sample(ctx, mm, 4096, ev, seed=SEED)
    assert got.shape == (4096, mm.n_vars) and got.dtype == np.uint8
    assert np.array_equal(got, want), int((got != want).sum())
    assert deg == wdeg == 0
    lz0 = bnpp.partition(ctx, mm, ev)[0]
    assert abs(lz - lz0) <= 1e-12 * max(1.0, abs(lz0)), (lz, lz0)


def _check_samples(m, ev, x, deg):
    cards = m["cards"]
    assert deg == 0
    assert all((x[:, v] == val).all() for v, val in ev.items())          # every sample keeps the evidence
    assert all((x[:, v] < cards[v]).all() for v in range(len(cards)))    # every value in range
    # no zero-probability configuration: a sample's log-score is finite exactly
    # when every factor entry it selects is positive (all samples, vectorised),
    # and mpe_ref.log_score says so of the first 64
    xi = x.astype(np.int64)
    for scope, vals in zip(m["scopes"], m["values"]):
        off = np.zeros(x.shape[0], dtype=np.int64)
        for v in scope:
            off = off * cards[v] + xi[:, v]
        assert (np.asarray(vals)[off] > 0).all(), scope
    for row in x[:64]:
        assert math.isfinite(mpe_ref.log_score(m, [int(v) for v in row])), row.tolist()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name,evf", SMALL)
def test_distribution_small_models(ctx, name, evf, dt):
    m = synth.read_uai(model_path(name + ".uai"))
    ev = evidence_of(evf)
    x, _, deg = bnpp.sample(ctx, bnpp.Model.load(model_path(name + ".uai")), N_DIST, ev, seed=SEED, dtype=DT[dt])
    _check_samples(m, ev, x, deg)
    bad = sr.check_frequencies(x, m["cards"], joint_of=sr.joint(m, ev), scopes=m["scopes"])
    assert not bad, bad[:3]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name,evf", LARGER)
def test_distribution_larger_models(ctx, name, evf, dt):
    m = synth.read_uai(model_path(name + ".uai"))
    mm = bnpp.Model.load(model_path(name + ".uai"))
    ev = evidence_of(evf)
    marg, _ = bnpp.marginals_tree(ctx, mm, ev, "mf", bnpp.F64)
    x, _, deg = bnpp.sample(ctx, mm, N_DIST, ev, seed=SEED, dtype=DT[dt])
    _check_samples(m, ev, x, deg)
    bad = sr.check_frequencies(x, m["cards"], marginals={v: marg[v] for v in range(mm.n_vars) if v not in ev})
    assert not bad, bad[:3]


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_relaunch_of_the_cached_job(dt):
    """Another seed relaunches the cached job (no planning) and gives other
    samples; the first seed again reproduces the first result; a partition in
    between plans its own job and returns the same Z."""
    c = bnpp.Context(0)
    try:
        mm = bnpp.Model.load(model_path("alarm.uai"))
        ev = evidence_of("alarm.uai.evid")
        lz0 = bnpp.partition(c, mm, ev, dtype=DT[dt])[0]
        first = bnpp.sample(c, mm, 4096, ev, seed=1, dtype=DT[dt])
        x1 = first[0].copy()
        assert bnpp.last_timing()["plan_ms"] > 0
        second = bnpp.sample(c, mm, 4096, ev, seed=2, dtype=DT[dt])
        t2 = bnpp.last_timing()
        assert t2["plan_ms"] == 0 and t2["upload_ms"] == 0 and t2["program_ms"] == 0 and t2["arena_reused"] == 1
        assert not np.array_equal(second[0], x1) and second[1] == first[1]
        assert bnpp.partition(c, mm, ev, dtype=DT[dt])[0] == lz0
        assert bnpp.last_timing()["plan_ms"] > 0         # never the sampling job
        again = bnpp.sample(c, mm, 4096, ev, seed=1, dtype=DT[dt])
        assert np.array_equal(again[0], x1) and again[1] == first[1]
    finally:
        c.close()


def test_fp32_beyond_its_range(ctx):
    """ising12x32: Z is far above FLT_MAX, so the fp32 run is finite and free of
    degenerate draws only through the power-of-two rescaling of the messages."""
    mm = bnpp.Model.load(model_path("ising12x32.uai"))
    x, lz, deg = bnpp.sample(ctx, mm, 1024, seed=SEED, dtype=bnpp.F32)
    assert math.isfinite(lz) and lz > math.log10(float(np.finfo(np.float32).max))
    assert deg == 0 and x.shape == (1024, mm.n_vars) and (x < 2).all()


def test_cli_writes_the_samples_file(ctx, tmp_path):
    exe = os.path.join(REPO, "bn-pp_amd", "bin", "bnpp")
    base = str(tmp_path / "asia")
    ev = evidence_of("asia.uai.evid")
    r = subprocess.run([exe, model_path("asia.uai"), model_path("asia.uai.evid"), "-sample", "16", "-seed", "7",
                        "-uai", base], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    x, lz, _ = bnpp.sample(ctx, bnpp.Model.load(model_path("asia.uai")), 16, ev, seed=7)
    with open(base + ".SAMPLES") as f:
        lines = f.read().split("\n")
    assert lines[0] == "SAMPLES" and lines[1] == "16 %d" % x.shape[1] and lines[-1] == ""
    assert lines[2:-1] == [" ".join(str(int(v)) for v in row) for row in x]
    assert ">> First of 16 samples: " + lines[2] + "\n" in r.stdout
    got = float(r.stdout.split(">> log10 Z = ")[1].split()[0])
    assert abs(got - lz) <= 1e-5 * max(1.0, abs(lz))     # printed with six significant digits
    assert not any(os.path.exists(base + e) for e in (".PR", ".MAR", ".MPE"))
