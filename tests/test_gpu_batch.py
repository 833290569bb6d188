"""GPU tests of batched evidence: bnpp_condition_batch one gather at a time
against the numpy restatement (batch_ref.py), and whole bnpp.partition_batch /
bnpp.posterior_batch runs against the single calls they batch.

  * single ops: the output equals batch_ref.gather bit for bit in the dtype of
    the run (values are moved, never computed on), between guard bands that
    stay untouched; capped grids give the same output.
  * whole fp64 runs: z[b] has the bits of bnpp.partition's z for row b (and of
    the CPU oracle's), log10_z[b] lies within 4 ulp of max(1, |log10_z|) of the
    single call's (the three roundings of log10(p) + exp2 * log10(2), the scale
    differing between the two).  Every row is compared.
  * an impossible row (Z == 0 exactly, found from a zero entry of a CPT on the
    CPU) gives -inf / 0 and leaves its neighbours' bits alone.  asia and alarm
    have such an entry; cancer's and noisyor_30_40's tables are strictly
    positive (asserted), so no evidence is impossible there.
  * results do not depend on the rows per launch; fp32 too, on a row set whose
    single-call fp32 Z values span less than 2^40 (asserted).
  * fp32: log10_z within 1e-6 relative of the fp64 batch, posteriors within
    1e-5 absolute (the project's fp32 tolerances).
"""
import os
import subprocess

import numpy as np
import pytest
import torch

import batch_ref
import bnpp
import refcpu
from bnpp import synth
from conftest import REPO, model_path

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"f64": torch.float64, "f32": torch.float32}
ND = {"f64": np.float64, "f32": np.float32}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
GUARD = 64
N_ROWS = 67
# evidence variables of the models without a zero entry (2-4 each); asia and
# alarm take the scope of their first CPT with a zero entry
EV_VARS = {"cancer": [0, 3], "ising6x6": [0, 7, 20, 35], "potts4x5k3": [1, 8, 19], "noisyor_30_40": [2, 35, 50, 65]}
BAYES = ("asia", "cancer", "alarm", "noisyor_30_40")
MODELS = ("asia", "cancer", "alarm", "ising6x6", "potts4x5k3", "noisyor_30_40")
TARGET = {"alarm": 5, "asia": 7, "noisyor_30_40": 40}

# cards, scope, evidence variables (in the order of the evidence table's rows)
OPS = [
    dict(name="middle", cards=[3, 2, 4], scope=[0, 1, 2], ev=[1]),
    dict(name="all_three", cards=[3, 2, 4], scope=[0, 1, 2], ev=[2, 0, 1]),
    dict(name="outside", cards=[3, 2, 4, 5], scope=[0, 1, 2], ev=[3, 1]),
    dict(name="only_outside", cards=[3, 2, 4, 5], scope=[0, 1, 2], ev=[3]),
    dict(name="card21_two_runs", cards=[21, 3, 21], scope=[0, 1, 2], ev=[1]),
    dict(name="card21_ends", cards=[21, 5, 21], scope=[2, 1, 0], ev=[0, 2]),
    dict(name="four_runs", cards=[2, 3, 2, 5, 3, 2, 4], scope=[0, 1, 2, 3, 4, 5, 6], ev=[5, 1, 3]),
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


def _run_op(ctx, stream, op, dt, n_rows, seed):
    cards, scope = op["cards"], op["scope"]
    rng = np.random.default_rng(seed)
    size = int(np.prod([cards[v] for v in scope]))
    src = rng.uniform(0.05, 1.0, size).astype(ND[dt])
    ev = np.stack([rng.integers(0, cards[v], n_rows) for v in op["ev"]]).astype(np.int32)
    want = batch_ref.gather(src, cards, scope, op["ev"], ev)
    t_src = torch.tensor(src, dtype=TD[dt], device=DEV)
    t_ev = torch.tensor(ev.reshape(-1), dtype=torch.int32, device=DEV)
    buf = torch.full((want.size + 2 * GUARD,), -7.0, dtype=TD[dt], device=DEV)
    bnpp.condition_batch(ctx, DT[dt], cards, t_src.data_ptr(), scope, op["ev"], n_rows, t_ev.data_ptr(),
                         buf[GUARD:].data_ptr(), stream=stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == -7.0).all() and (got[GUARD + want.size:] == -7.0).all(), ("guard band written", op["name"])
    return got[GUARD:GUARD + want.size], want


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n_rows", [1, 5, 64, 257])
def test_single_op_bit_for_bit(ctx, stream, dt, n_rows):
    for i, op in enumerate(OPS):
        got, want = _run_op(ctx, stream, op, dt, n_rows, 100 + i)
        assert got.dtype == want.dtype and np.array_equal(got, want), (op["name"], dt, n_rows)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_single_op_capped_grid(ctx, stream, grid_cap, dt, cap):
    grid_cap(cap)
    for i, op in enumerate(OPS):
        got, want = _run_op(ctx, stream, op, dt, 257, 200 + i)
        assert np.array_equal(got, want), (op["name"], dt, cap)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _zero_entry(d):
    """(scope, assignment) of the first CPT entry that is exactly 0 in a factor of 2-4 variables, or None."""
    for s, v in zip(d["scopes"], d["values"]):
        v = np.asarray(v)
        if 2 <= len(s) <= 4 and (v == 0).any():
            idx = np.unravel_index(int(np.flatnonzero(v == 0)[0]), [d["cards"][x] for x in s])
            return list(s), [int(i) for i in idx]
    return None


_CASES = {}


def _case(ctx, name):
    """Per model, computed once and shared: the evidence variables, 67 rows (half
    uniform, half from joint samples; the impossible row, where one exists, in
    the middle) and per row the single call's fp64 (log10 Z, Z) and the oracle's Z."""
    if name in _CASES:
        return _CASES[name]
    path = model_path(name + ".uai")
    m, d = bnpp.Model.load(path), synth.read_uai(path)
    zero = _zero_entry(d) if name in BAYES else None
    if name in EV_VARS:
        assert zero is None and all((np.asarray(v) > 0).all() for v in d["values"]), "a zero entry: use it"
        ev_vars = EV_VARS[name]
    else:
        assert zero is not None, "no zero entry in " + name
        ev_vars = sorted(zero[0])
    assert 2 <= len(ev_vars) <= 4
    samples, _, _ = bnpp.sample(ctx, m, N_ROWS, seed=7)
    rows = batch_ref.draw_rows(d["cards"], ev_vars, N_ROWS, 11, samples)
    bad = None
    if zero is not None:
        bad = N_ROWS // 2
        rows[bad] = [zero[1][zero[0].index(v)] for v in ev_vars]
    oracle = refcpu.Model.load(path)
    lz1, z1, rz = np.zeros(N_ROWS), np.zeros(N_ROWS), np.zeros(N_ROWS)
    for r in range(N_ROWS):
        ev = dict(zip(ev_vars, (int(x) for x in rows[r])))
        lz1[r], z1[r], _ = bnpp.partition(ctx, m, ev, "mf", bnpp.F64)
        rz[r] = oracle.partition(ev, "mf")[0]
    if bad is not None:
        assert rz[bad] == 0.0, "the chosen row is not impossible"
    _CASES[name] = dict(m=m, d=d, ev_vars=ev_vars, rows=rows, bad=bad, lz1=lz1, z1=z1, rz=rz)
    return _CASES[name]


def _check_fp64(c, lz, z):
    assert np.array_equal(_bits(z), _bits(c["z1"])), np.flatnonzero(_bits(z) != _bits(c["z1"]))
    assert np.array_equal(z, c["rz"]), "the CPU oracle disagrees"
    for r in range(len(z)):
        if c["z1"][r] == 0:
            assert lz[r] == -np.inf and c["lz1"][r] == -np.inf and z[r] == 0.0
        else:
            bound = 4 * np.spacing(max(1.0, abs(c["lz1"][r])))
            print("row", r, "log10_z", lz[r], "single", c["lz1"][r], "bound", bound)
            assert abs(lz[r] - c["lz1"][r]) <= bound, (r, lz[r], c["lz1"][r])


@pytest.mark.parametrize("name", MODELS)
def test_partition_batch_fp64_bit_identical(ctx, name):
    c = _case(ctx, name)
    lz, z, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=bnpp.F64)
    assert len(z) == N_ROWS
    _check_fp64(c, lz, z)
    if c["bad"] is not None:
        b = c["bad"]
        assert lz[b] == -np.inf and z[b] == 0.0             # its neighbours' bits are compared above, with every row
    else:
        assert (z > 0).all()


@pytest.mark.parametrize("name", MODELS)
def test_partition_batch_fp32(ctx, name):
    c = _case(ctx, name)
    lz64, _, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=bnpp.F64)
    lz32, z32, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=bnpp.F32)
    for r in range(N_ROWS):
        if c["z1"][r] == 0:
            assert lz32[r] == -np.inf and z32[r] == 0.0
        else:
            assert abs(lz32[r] - lz64[r]) <= 1e-6 * max(1.0, abs(lz64[r])), (r, lz32[r], lz64[r])


@pytest.mark.parametrize("R", [1, 16, 64, 0])
def test_rows_per_launch_fp64(ctx, R):
    """67 rows: R = 16 and 64 end on a padded launch, R = 1 makes 67 launches."""
    c = _case(ctx, "alarm")
    lz, z, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=bnpp.F64, rows_per_launch=R)
    _check_fp64(c, lz, z)


def _possible_rows(ctx, c):
    """The possible rows of a case's set (alarm's uniform rows hit other zero entries too), repeated to 67
    rows; their single-call fp32 Z values span less than 2^40 (asserted).  Computed once per case."""
    if "rows32" not in c:
        good = c["rows"][c["z1"] > 0]
        assert len(good) >= N_ROWS // 2
        rows = good[np.arange(N_ROWS) % len(good)]
        z1 = np.array([bnpp.partition(ctx, c["m"], dict(zip(c["ev_vars"], (int(x) for x in r))), "mf", bnpp.F32)[1] for r in rows])
        assert (z1 > 0).all() and z1.max() / z1.min() < 2.0 ** 40, (z1.min(), z1.max())
        c["rows32"] = rows
    return c["rows32"]


def test_rows_per_launch_fp32(ctx):
    c = _case(ctx, "alarm")
    rows = _possible_rows(ctx, c)
    ref = None
    for R in (1, 16, 64, 0):
        lz, z, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], rows, dtype=bnpp.F32, rows_per_launch=R)
        if ref is None:
            ref = (lz, z)
        assert np.array_equal(_bits(z), _bits(ref[1])) and np.array_equal(_bits(lz), _bits(ref[0])), R


@pytest.mark.parametrize("name", sorted(TARGET))
def test_posterior_batch(ctx, name):
    c = _case(ctx, name)
    t = TARGET[name]
    assert t not in c["ev_vars"]
    single = np.array([bnpp.marginals(ctx, c["m"], dict(zip(c["ev_vars"], (int(x) for x in r))), "mf", bnpp.F64,
                                      targets=[t])[0][t] for r in c["rows"]])
    post, _ = bnpp.posterior_batch(ctx, c["m"], c["ev_vars"], c["rows"], t, dtype=bnpp.F64)
    assert post.shape == single.shape == (N_ROWS, c["d"]["cards"][t])
    assert np.array_equal(post, single, equal_nan=True)
    ok = c["z1"] > 0                                         # uniform rows may hit zero entries too
    if c["bad"] is not None:
        # pinned: an impossible row normalises 0 / 0, as bnpp_marginals does for that evidence
        assert not ok[c["bad"]] and ok[c["bad"] + 1:].all()
        assert np.isnan(single[~ok]).all() and np.isnan(post[~ok]).all()
    else:
        assert ok.all()
    assert np.array_equal(_bits(post[ok]), _bits(single[ok]))
    assert np.allclose(post[ok].sum(axis=1), 1.0, atol=1e-12)
    post32, _ = bnpp.posterior_batch(ctx, c["m"], c["ev_vars"], c["rows"], t, dtype=bnpp.F32)
    assert np.abs(post32[ok] - post[ok]).max() <= 1e-5
    for R in (16, 1):
        p2, _ = bnpp.posterior_batch(ctx, c["m"], c["ev_vars"], c["rows"], t, dtype=bnpp.F64, rows_per_launch=R)
        assert np.array_equal(_bits(p2[ok]), _bits(post[ok])), R


def test_cached_job_relaunches_with_other_values(ctx):
    c = _case(ctx, "alarm")
    a, b = c["rows"][:32], c["rows"][32:64]
    bnpp.partition_batch(ctx, c["m"], c["ev_vars"], a, rows_per_launch=32)
    _, zb, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], b, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] == 0, "the second call planned again"
    assert np.array_equal(_bits(zb), _bits(c["z1"][32:64]))
    _, za, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], a, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] == 0 and np.array_equal(_bits(za), _bits(c["z1"][:32]))
    other = [3, 10, 20]
    assert other != c["ev_vars"]
    rows = batch_ref.draw_rows(c["d"]["cards"], other, 32, 5)
    bnpp.partition_batch(ctx, c["m"], other, rows, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] > 0, "another evidence variable set must plan afresh"


def test_no_evidence_variables(ctx):
    c = _case(ctx, "alarm")
    _, z1, _ = bnpp.partition(ctx, c["m"], {}, "mf", bnpp.F64)
    lz, z, _ = bnpp.partition_batch(ctx, c["m"], [], np.zeros((5, 0), dtype=np.int64))
    assert len(z) == 5 and (_bits(z) == _bits([z1])[0]).all()


def test_cli_pr_batch(ctx, tmp_path):
    c = _case(ctx, "asia")
    rows = c["rows"][[0, c["bad"], 40]]
    evid = tmp_path / "three.evid"
    evid.write_text("3\n" + "".join(
        "%d %s\n" % (len(c["ev_vars"]), " ".join("%d %d" % (v, x) for v, x in zip(c["ev_vars"], r))) for r in rows))
    base = str(tmp_path / "out")
    exe = os.path.join(REPO, "bn-pp_amd", "bin", "bnpp")
    p = subprocess.run([exe, model_path("asia.uai"), str(evid), "-pr-batch", "-uai", base], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    lines = open(base + ".PR").read().split()
    assert lines[0] == "PR" and lines[1] == "3" and len(lines) == 5
    got = np.array([float(x) for x in lines[2:]])
    lz, _, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], rows)
    assert np.array_equal(got, lz) and got[1] == -np.inf
