"""GPU tests of expected counts: bnpp_bucket_counts one accumulate step at a
time against the numpy restatement (counts_ref.accumulate, bit for bit), and
whole bnpp.expected_counts runs against brute force, against the batched
posteriors, across rows per launch, weights, impossible rows, a cached job, the
EM driver and the CLI.

Tolerances of the whole runs: n x the bucket-tree MAR tolerances the project
states (tests/test_gpu_config4.py) -- 1e-12 per row in fp64, 1e-5 in
fp32 -- since a count is a sum of n posteriors.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

import batch_ref
import bnpp
import counts_ref
from bnpp import learn, synth
from conftest import REPO, model_path
from counts_ref import EV_VARS

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"f64": torch.float64, "f32": torch.float32}
ND = {"f64": np.float64, "f32": np.float32}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
TOL = {"f64": 1e-12, "f32": 1e-5}
GUARD = 16

# cards, factor scope, evidence variables (rows of the evidence table); rest entries 1, 3, 33; key spaces 1, 2, 6, 81
OPS = [
    dict(name="rest1_key2", cards=[2], scope=[0], ev=[0]),
    dict(name="rest3_key1", cards=[3, 4], scope=[0], ev=[1]),
    dict(name="rest3_key2", cards=[3, 2], scope=[0, 1], ev=[1]),
    dict(name="rest3_key6", cards=[2, 3, 3], scope=[0, 1, 2], ev=[2, 0]),
    dict(name="rest33_key1", cards=[3, 11], scope=[1, 0], ev=[]),
    dict(name="rest33_key2", cards=[3, 2, 11], scope=[0, 1, 2], ev=[1]),
    dict(name="rest33_key6", cards=[2, 11, 3, 3], scope=[0, 1, 2, 3], ev=[2, 0]),
    dict(name="rest1_key6", cards=[2, 3], scope=[1, 0], ev=[0, 1]),
    dict(name="rest3_key81", cards=[3, 3, 3, 3, 3], scope=[0, 1, 2, 3, 4], ev=[4, 3, 1, 0]),
]
ROWS = [1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def stream():
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    return s.cuda_stream


@pytest.fixture
def grid_cap(ctx):
    yield ctx.set_max_grid
    ctx.set_max_grid(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _run_op(ctx, stream, op, dt, R, seed, live=None, has_b=True, same_key=False, zero_col=False, valid0=False,
            weights=True, twice=False):
    cards, scope, evv = op["cards"], op["scope"], op["ev"]
    rng = np.random.default_rng(seed)
    live = R if live is None else live
    rest = [v for v in scope if v not in evv]
    n_rest = int(np.prod([cards[v] for v in rest])) if rest else 1
    size = int(np.prod([cards[v] for v in scope]))
    T = rng.uniform(0.05, 1.0, n_rest * (R if has_b else 1)).astype(ND[dt])
    if zero_col and has_b:
        T.reshape(n_rest, R)[:, R // 2] = 0
    ev = np.stack([rng.integers(0, cards[v], R) for v in evv]).astype(np.int32) if evv else np.zeros((0, R), np.int32)
    if same_key and evv:
        ev[:] = ev[:, :1]
    w = None
    if weights:
        w = rng.uniform(0.0, 3.0, R)
        if R >= 5:
            w[rng.integers(0, R, R // 5)] = 0.0
    valid = None
    if valid0:
        valid = rng.uniform(0.5, 1.0, R).astype(ND[dt])
        valid[R // 3] = 0
    start = rng.uniform(0.0, 2.0, size) if twice else np.zeros(size)
    want = counts_ref.accumulate(start.copy(), T, cards, scope, evv, ev, w, live, valid, has_b, R)
    if twice:
        want = counts_ref.accumulate(want, T, cards, scope, evv, ev, w, live, valid, has_b, R)
    t_T = torch.tensor(T, dtype=TD[dt], device=DEV)
    t_ev = torch.tensor(ev.reshape(-1), dtype=torch.int32, device=DEV) if evv else None
    t_w = torch.tensor(w, dtype=torch.float64, device=DEV) if w is not None else None
    t_v = torch.tensor(valid, dtype=TD[dt], device=DEV) if valid is not None else None
    buf = torch.full((size + 2 * GUARD,), -7.0, dtype=torch.float64, device=DEV)
    buf[GUARD:GUARD + size] = torch.tensor(start, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    for _ in range(2 if twice else 1):
        bnpp.bucket_counts(ctx, DT[dt], cards, t_T.data_ptr(), scope, evv, R, live, t_ev.data_ptr() if evv else 0,
                           buf[GUARD:].data_ptr(), weights=t_w.data_ptr() if t_w is not None else 0,
                           valid=t_v.data_ptr() if t_v is not None else 0, has_b=has_b, stream=stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == -7.0).all() and (got[GUARD + size:] == -7.0).all(), ("guard band written", op["name"])
    return got[GUARD:GUARD + size], want


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), (what, np.flatnonzero(_bits(got) != _bits(want))[:8], got, want)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("R", ROWS)
def test_single_op_bit_for_bit(ctx, stream, dt, R):
    for i, op in enumerate(OPS):
        got, want = _run_op(ctx, stream, op, dt, R, 100 + i)
        _same(got, want, (op["name"], dt, R))
        assert want.sum() > 0


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_single_op_edge_cases(ctx, stream, dt):
    for i, op in enumerate(OPS):
        for kw in (dict(same_key=True), dict(live=65), dict(has_b=False), dict(zero_col=True), dict(valid0=True),
                   dict(weights=False), dict(twice=True), dict(live=65, zero_col=True, valid0=True, twice=True)):
            got, want = _run_op(ctx, stream, op, dt, 128, 300 + i, **kw)
            _same(got, want, (op["name"], dt, kw))


def test_padded_rows_and_skipped_rows_count_nothing(ctx, stream):
    """The reference itself: live = 65 of 128 differs from all 128, so the bit-for-bit cases above can tell."""
    op = OPS[3]
    a, _ = _run_op(ctx, stream, op, "f64", 128, 7, live=65)
    b, _ = _run_op(ctx, stream, op, "f64", 128, 7)
    assert a.sum() < b.sum()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_single_op_capped_grid(ctx, stream, grid_cap, dt, cap):
    grid_cap(cap)
    for i in (5, 6, 8):
        got, want = _run_op(ctx, stream, OPS[i], dt, 257, 200 + i, twice=True)
        _same(got, want, (OPS[i]["name"], dt, cap))


# ---- whole runs ----
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
        _BRUTE[(name, n)] = counts_ref.brute_counts(c["d"], c["ev"], c["rows"])
    return _BRUTE[(name, n)]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("name", ["asia", "cancer", "earthquake", "ising4x4"])
def test_whole_run_against_brute_force(ctx, name, n, dt):
    c = _case(ctx, name, n)
    want, z = _brute(c, name, n)
    counts, lz, n_imp = bnpp.expected_counts(ctx, c["m"], c["ev"], c["rows"], dtype=DT[dt])
    got = bnpp.split_counts(c["d"], counts)
    assert n_imp == int((z == 0).sum()) and n_imp <= n / 2
    assert np.array_equal(np.isfinite(lz), z > 0)
    worst = max(float(np.abs(g - w).max()) for g, w in zip(got, want))
    print(name, n, dt, "worst |count - brute|", worst, "bound", n * TOL[dt], "impossible", n_imp)
    assert worst <= n * TOL[dt]
    assert np.allclose(lz[z > 0], np.log10(z[z > 0]), rtol=0, atol=1e-5 if dt == "f32" else 1e-11)


@pytest.mark.parametrize("name", ["alarm", "ising6x6", "potts4x5k3", "noisyor_30_40"])
def test_consistency_with_the_batched_posteriors(ctx, name):
    n = 33
    c = _case(ctx, name, n)
    d, ev, rows = c["d"], c["ev"], c["rows"]
    counts, lz, n_imp = bnpp.expected_counts(ctx, c["m"], ev, rows, dtype=bnpp.F64)
    ok = np.isfinite(lz)
    assert n_imp == int((~ok).sum()) and n_imp <= n / 2
    per = bnpp.split_counts(d, counts)
    tol = n * 1e-12
    post = {}
    for s, N in zip(d["scopes"], per):
        assert abs(N.sum() - ok.sum()) <= tol, (s, N.sum(), ok.sum())
        for ax, v in enumerate(s):
            marg = N.sum(axis=tuple(a for a in range(len(s)) if a != ax))
            if v in ev:
                want = np.bincount(rows[ok][:, ev.index(v)], minlength=d["cards"][v]).astype(np.float64)
            else:
                if v not in post:
                    post[v] = bnpp.posterior_batch(ctx, c["m"], ev, rows, v, dtype=bnpp.F64)[0][ok].sum(axis=0)
                want = post[v]
            assert np.abs(marg - want).max() <= tol, (s, v, marg, want)


def test_log10_z_has_the_bits_of_partition_batch(ctx):
    c = _case(ctx, "alarm", 130)
    lzb, _, _ = bnpp.partition_batch(ctx, c["m"], c["ev"], c["rows"], dtype=bnpp.F64)
    _, lz, n_imp = bnpp.expected_counts(ctx, c["m"], c["ev"], c["rows"], dtype=bnpp.F64)
    assert np.array_equal(_bits(lz), _bits(lzb))
    assert n_imp == int(np.isinf(lzb).sum())


def test_rows_per_launch_fp64_bit_identical(ctx):
    """130 rows: R = 7 and 64 end on a padded launch, R = 1 makes 130 launches."""
    c = _case(ctx, "alarm", 130)
    ref = None
    for R in (1, 7, 64, 0):
        counts, lz, n_imp = bnpp.expected_counts(ctx, c["m"], c["ev"], c["rows"], dtype=bnpp.F64, rows_per_launch=R)
        if ref is None:
            ref = (counts, lz, n_imp)
            assert counts.sum() > 0 and n_imp <= 65
        assert np.array_equal(_bits(counts), _bits(ref[0])), (R, np.flatnonzero(_bits(counts) != _bits(ref[0]))[:8])
        assert np.array_equal(_bits(lz), _bits(ref[1])) and n_imp == ref[2]


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_whole_run_capped_grid(ctx, grid_cap, cap):
    """All accumulate steps run in one launch (blockIdx.y picks the step): on 1-3 workgroups per
    step its loops iterate, and the counts keep their bits."""
    c = _case(ctx, "alarm", 130)
    ref, _, _ = bnpp.expected_counts(ctx, c["m"], c["ev"], c["rows"], rows_per_launch=64)
    grid_cap(cap)
    got, _, _ = bnpp.expected_counts(ctx, c["m"], c["ev"], c["rows"], rows_per_launch=64)
    assert np.array_equal(_bits(got), _bits(ref))


def test_weights(ctx):
    n = 65
    c = _case(ctx, "alarm", n)
    rows = c["rows"]
    rng = np.random.default_rng(3)
    w = rng.uniform(0.25, 2.0, n)
    off = rng.random(n) < 0.3
    w[off] = 0.0
    a, _, _ = bnpp.expected_counts(ctx, c["m"], c["ev"], rows, weights=w, rows_per_launch=16)
    b, _, _ = bnpp.expected_counts(ctx, c["m"], c["ev"], rows[~off], weights=w[~off], rows_per_launch=16)
    assert off.any() and np.array_equal(_bits(a), _bits(b)), "a zero-weight row must leave no trace"
    w2 = np.ones(n)
    w2[5] = w2[40] = 2.0
    twice, _, _ = bnpp.expected_counts(ctx, c["m"], c["ev"], rows, weights=w2)
    dup, _, _ = bnpp.expected_counts(ctx, c["m"], c["ev"], np.concatenate([rows, rows[[5, 40]]]))
    assert np.abs(twice - dup).max() <= (n + 2) * 1e-12


def test_an_impossible_row_counts_nowhere(ctx):
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
    _, z = counts_ref.brute_counts(d, ev, np.concatenate([bad_row, good]))
    assert z[0] == 0 and (z[1:] > 0).all()
    with_bad = np.concatenate([good[:7], bad_row, good[7:]])
    a, lza, na = bnpp.expected_counts(ctx, c["m"], ev, with_bad, rows_per_launch=8)
    b, _, nb = bnpp.expected_counts(ctx, c["m"], ev, good, rows_per_launch=8)
    assert na == 1 and nb == 0 and lza[7] == -np.inf
    assert np.array_equal(_bits(a), _bits(b))
    assert all(abs(N.sum() - len(good)) <= len(good) * 1e-12 for N in bnpp.split_counts(d, a))


def test_cached_job_relaunches_with_other_values(ctx):
    c = _case(ctx, "alarm", 130)
    a, b = c["rows"][:32], c["rows"][32:64]
    fresh_b, _, _ = bnpp.expected_counts(ctx, c["m"], c["ev"], b, rows_per_launch=32)
    bnpp.expected_counts(ctx, c["m"], c["ev"], a, rows_per_launch=32)
    again_b, _, _ = bnpp.expected_counts(ctx, c["m"], c["ev"], b, rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] == 0, "the second call planned again"
    assert np.array_equal(_bits(again_b), _bits(fresh_b))
    wa, _, _ = bnpp.expected_counts(ctx, c["m"], c["ev"], a, weights=np.full(32, 0.5), rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] == 0, "weights are launch data"
    assert not np.array_equal(wa, again_b)
    other = [3, 10, 21]
    bnpp.expected_counts(ctx, c["m"], other, batch_ref.draw_rows(c["d"]["cards"], other, 32, 5), rows_per_launch=32)
    assert bnpp.last_timing()["plan_ms"] > 0, "another evidence variable set must plan afresh"


def test_no_evidence_variables(ctx):
    c = _case(ctx, "asia", 65)
    counts, lz, n_imp = bnpp.expected_counts(ctx, c["m"], [], np.zeros((5, 0), dtype=np.int64))
    want, _ = counts_ref.brute_counts(c["d"], [], np.zeros((5, 0), dtype=np.int64))
    assert n_imp == 0 and len(lz) == 5
    for g, w in zip(bnpp.split_counts(c["d"], counts), want):
        assert np.abs(g - w).max() <= 5e-12


def test_em_on_asia(ctx):
    path = model_path("asia.uai")
    d = synth.read_uai(path)
    # the golden file lists a CPT's child first; m_step wants it last (the UAI convention): transpose every table
    d = dict(d, scopes=[list(s[1:]) + [s[0]] for s in d["scopes"]],
             values=[np.moveaxis(np.asarray(v).reshape([d["cards"][x] for x in s]), 0, -1).reshape(-1).tolist()
                     for s, v in zip(d["scopes"], d["values"])])
    for s, v in zip(d["scopes"], d["values"]):
        assert np.allclose(np.asarray(v).reshape(-1, d["cards"][s[-1]]).sum(axis=1), 1.0), "not a CPT over the last variable"
    truth = bnpp.Model.from_dict(d)
    samples, _, _ = bnpp.sample(ctx, truth, 512, seed=21)
    ev = [1, 3, 5, 7]
    rows = np.asarray(samples)[:, ev]
    rng = np.random.default_rng(4)
    start = dict(d)
    start["values"] = []
    for s, v in zip(d["scopes"], d["values"]):
        k = d["cards"][s[-1]]
        t = np.asarray(v).reshape(-1, k) * rng.uniform(0.5, 1.5, (len(v) // k, k)) + 0.05
        start["values"].append((t / t.sum(axis=1, keepdims=True)).reshape(-1).tolist())
    fitted, lls = learn.em(ctx, start, ev, rows, iters=6)
    print("EM log10-likelihoods", lls)
    assert len(lls) == 6 and all(np.isfinite(lls)) and max(lls) < 0, "the likelihood of a Bayesian network is below 1"
    for a, b in zip(lls, lls[1:]):
        assert b >= a - 1e-9 * abs(a), lls
    assert lls[-1] > lls[0]
    for s, v in zip(fitted["scopes"], fitted["values"]):
        assert np.allclose(np.asarray(v).reshape(-1, d["cards"][s[-1]]).sum(axis=1), 1.0, atol=1e-12)
    first, _, n_imp = bnpp.expected_counts(ctx, bnpp.Model.from_dict(start), ev, rows)
    want, _ = counts_ref.brute_counts(start, ev, rows)
    assert n_imp == 0
    for g, w in zip(bnpp.split_counts(start, first), want):
        assert np.abs(g - w).max() <= 512 * 1e-12


def test_cli_counts(ctx, tmp_path):
    c = _case(ctx, "asia", 65)
    rows = c["rows"][:9]
    evid = tmp_path / "nine.evid"
    evid.write_text("%d\n" % len(rows) + "".join(
        "%d %s\n" % (len(c["ev"]), " ".join("%d %d" % (v, x) for v, x in zip(c["ev"], r))) for r in rows))
    base = str(tmp_path / "out")
    exe = os.path.join(REPO, "bn-pp_amd", "bin", "bnpp")
    p = subprocess.run([exe, model_path("asia.uai"), str(evid), "-counts", "-uai", base], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    lines = open(base + ".COUNTS").read().split("\n")
    assert lines[0] == "COUNTS" and int(lines[1]) == c["m"].n_factors
    got = []
    for f in range(c["m"].n_factors):
        tok = lines[2 + f].split()
        assert int(tok[0]) == len(tok) - 1
        got += [float(x) for x in tok[1:]]
    counts, lz, n_imp = bnpp.expected_counts(ctx, c["m"], c["ev"], rows)
    assert np.array_equal(_bits(got), _bits(counts))
    assert "n_impossible %d" % n_imp in p.stdout
