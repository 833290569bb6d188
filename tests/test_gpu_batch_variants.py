"""GPU parity of the level kernels only a batched plan reaches: the catalogue
of batch_catalogue.py (per key outside test_variant_census.LEVEL_KEYS the
smallest batched plan that holds it, with its evidence rows) run through
bnpp.partition_batch / bnpp.posterior_batch, and alarm at the rows per launch
no other test takes.

Per catalogue entry (n_rows = R + 3 or R + 1: two launches, the second padded):

  * instrument: right before the call bnpp.plan_batch of the same arguments
    reports the entry's key (BNPP_NO_O32 set per entry).
  * fp64 partitions: z[b] has the bits of bnpp.partition's z for row b's
    assignment and equals the CPU oracle's; log10_z[b] within 4 ulp of
    max(1, |log10_z|) of the single call's; an impossible row gives -inf / 0 and
    its neighbours are compared like every row.
  * fp64 posteriors: bit-identical to bnpp.marginals(targets=[t]), NaN rows
    equal as NaN; possible rows sum to 1 within 1e-12.
  * fp32: the same rows at rows_per_launch = 1 (a plan of kernels the suite
    already compares bit for bit: test_batch_census.py) give the same bits of
    z and log10_z (of the posterior); the R = 1 Z values span less than 2^40
    (asserted first; the catalogue's rows span less than 2^30 by the oracle).
    log10_z within 1e-6 relative of the fp64 batch, posteriors within 1e-5
    absolute: the project's fp32 tolerances.
  * entries of the other batched calls ("call": counts, marginals; plain
    evidence), with their own plan function as the instrument: every
    output has the bits of the same call at rows_per_launch = 1 (fp32 after the
    span assertion), a plan of kernels already held to bits
    (test_batch_census.py).  counts, fp64: log10_z with partition_batch's
    bits, counts within n x 1e-12 of counts_ref's brute force where the joint
    has at most 2^16 states, else every factor's counts sum to the possible
    rows within n x 1e-12.  marginals, fp64: log10_z with partition_batch's
    bits, every distinct row within 1e-12 of bnpp.marginals, evidence
    variables one-hot, impossible rows NaN.  fp32: marginals within 1e-5,
    counts within n x 1e-5, log10_z within 1e-6 relative of the fp64 call.
  * entries with partial evidence variables (plan_batch; the stored rows hold MISSING in about a quarter of the partial cells): the
    bits of rows_per_launch = 1 as above, and against the single calls on the
    per-row masked model of missing_ref.py with the row's hard entries as
    evidence -- fp64 partitions: z with bnpp.partition's bits, log10_z within
    4 ulp; fp64 posteriors within 1e-12 of bnpp.marginals; fp32
    within 1e-6 relative (log10_z) / 1e-5 (posteriors) of the fp64 call.
  * the entry of each (dtype, family) whose key has the most virtual blocks
    runs again on a context capped at 1, 2 and 3 workgroups with the same bits
    (generic and stream; the slab grid is flat and is not capped).
"""
import numpy as np
import pytest

import batch_catalogue as bc
import bnpp
import refcpu
from conftest import model_path
from test_gpu_batch import _bits, _case, _possible_rows

pytestmark = pytest.mark.gpu

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
ALARM_R = (2, 3, 5, 6, 7, 8, 12, 63, 65, 100)


@pytest.fixture(scope="module")
def cat():
    return bc.load()


@pytest.fixture
def grid_cap(ctx):
    """ctx.set_max_grid for one test: the default grids are restored after it."""
    yield ctx.set_max_grid
    ctx.set_max_grid(0)


_MODELS, _SINGLE = {}, {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = (bnpp.Model.load(model_path(name + ".uai")), refcpu.Model.load(model_path(name + ".uai")))
    return _MODELS[name]


def _single(ctx, e):
    """Per distinct assignment of an entry, computed once per (model, evidence
    set, target, offset width): the single call's fp64 (log10 Z, Z), the
    oracle's Z and, with a target, bnpp.marginals' posterior."""
    k = (e["model"], tuple(e["ev_vars"]), e["target"], e["no_o32"], tuple(map(tuple, e["rows"])))
    if k not in _SINGLE:
        m, oracle = _model(e["model"])
        lz, z, rz, post = [], [], [], []
        for a in e["rows"]:
            ev = dict(zip(e["ev_vars"], a))
            l1, z1, _ = bnpp.partition(ctx, m, ev, "mf", bnpp.F64)
            lz.append(l1)
            z.append(z1)
            rz.append(oracle.partition(ev, "mf")[0])
            if e["target"] is not None:
                post.append(bnpp.marginals(ctx, m, ev, "mf", bnpp.F64, targets=[e["target"]])[0][e["target"]])
        _SINGLE[k] = dict(lz=np.array(lz), z=np.array(z), rz=np.array(rz), post=np.array(post))
    return _SINGLE[k]


def _run(ctx, e, rows, dtype, R):
    """(log10_z, z) of a partition entry, (posterior,) of a posterior entry."""
    m, _ = _model(e["model"])
    if e["target"] is None:
        lz, z, _ = bnpp.partition_batch(ctx, m, e["ev_vars"], rows, dtype=dtype, rows_per_launch=R)
        return lz, z
    return (bnpp.posterior_batch(ctx, m, e["ev_vars"], rows, e["target"], dtype=dtype, rows_per_launch=R)[0],)


def _same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _same(a, b):
    """Two calls' outputs: same shapes, NaN in the same places, the same bits elsewhere (floats) or equal (integers)."""
    for x, y in zip(a, b):
        if x.shape != y.shape:
            return False
        if x.dtype.kind != "f":
            if not np.array_equal(x, y):
                return False
            continue
        nan = np.isnan(x)
        if not np.array_equal(nan, np.isnan(y)) or not np.array_equal(_bits(x)[~nan], _bits(y)[~nan]):
            return False
    return True


def _run_call(ctx, e, rows, dtype, R):
    """Every output of an entry's batched call, as a tuple of arrays."""
    m, _ = _model(e["model"])
    call, ev = bc.call_of(e), e["ev_vars"]
    if call == "batch":
        if e["target"] is None:
            lz, z, _ = bnpp.partition_batch(ctx, m, ev, rows, dtype=dtype, rows_per_launch=R, partial=e.get("partial"))
            return lz, z
        return (bnpp.posterior_batch(ctx, m, ev, rows, e["target"], dtype=dtype, rows_per_launch=R,
                                     partial=e.get("partial"))[0],)
    assert e.get("partial") is None, "counts and marginals are swept with plain evidence"
    if call == "counts":
        counts, lz, n_imp = bnpp.expected_counts(ctx, m, ev, rows, dtype=dtype, rows_per_launch=R)
        return counts, lz, np.array([n_imp])
    assert call == "marginals", call                     # no sample or mpe plan supplies an entry: their keys, where
    return bnpp.marginals_batch(ctx, m, ev, rows, dtype=dtype, rows_per_launch=R)   # any, have a plan_batch entry


def _check_call_entry(ctx, e, capped, grid_cap):
    """An entry of plan_counts / plan_marginals_batch (module docstring)."""
    from bnpp import synth
    import counts_ref
    m, _ = _model(e["model"])
    call, ev, R, n = bc.call_of(e), e["ev_vars"], e["R"], e["n_rows"]
    assert call in ("counts", "marginals") and e["partial"] is None and e["soft"] is None
    rows = np.array(bc.rows_of(e), dtype=np.int64)
    idx = np.arange(n) % len(e["rows"])
    tag = (e["dtype"], e["key"], call, e["model"], ev, R)
    dtype = DT[e["dtype"]]
    _, groups = bc.plan(bnpp, e, model=m)
    assert e["key"] in {g["key"] for g in groups}, (tag, bc.sum_keys(groups))
    got = _run_call(ctx, e, rows, dtype, R)
    assert len(got[1]) == n
    distinct = np.array(e["rows"], dtype=np.int64)
    if e["dtype"] == "f32":
        _, zc, _ = bnpp.partition_batch(ctx, m, ev, distinct, dtype=bnpp.F32, rows_per_launch=1)
        assert (zc > 0).all() and zc.max() / zc.min() < 2.0 ** 40, (tag, zc.min(), zc.max())
    one = _run_call(ctx, e, rows, dtype, 1)
    assert _same(got, one), (tag, "differs from rows_per_launch = 1")
    b64 = got if e["dtype"] == "f64" else _run_call(ctx, e, rows, bnpp.F64, R)
    free = [v for v in range(m.n_vars) if v not in ev]
    if call in ("counts", "marginals"):
        lz = got[1]
        if e["dtype"] == "f64":
            lzb, zb, _ = bnpp.partition_batch(ctx, m, ev, rows, dtype=bnpp.F64, rows_per_launch=R)
            assert np.array_equal(_bits(lz), _bits(lzb)), (tag, "log10_z is not partition_batch's")
            ok = zb > 0
        else:
            fin = np.isfinite(b64[1])
            assert np.array_equal(np.isfinite(lz), fin) and fin.all(), tag
            assert (np.abs(lz - b64[1]) <= 1e-6 * np.maximum(1.0, np.abs(b64[1]))).all(), (tag, lz, b64[1])
            ok = fin
    if call == "counts":
        d = synth.read_uai(model_path(e["model"] + ".uai"))
        per = bnpp.split_counts(d, got[0])
        assert int(got[2][0]) == int((~ok).sum()), tag
        if e["dtype"] == "f64":
            if np.prod([float(c) for c in d["cards"]]) <= 2 ** 16:
                want, z = counts_ref.brute_counts(d, ev, rows)
                assert np.array_equal(z > 0, ok), tag
                worst = max(float(np.abs(g - w).max()) for g, w in zip(per, want))
                print(tag, "worst |count - brute|", worst, "bound", n * 1e-12)
                assert worst <= n * 1e-12, (tag, worst)
            else:
                for sc, N in zip(d["scopes"], per):
                    assert abs(N.sum() - ok.sum()) <= n * 1e-12, (tag, sc, N.sum(), int(ok.sum()))
        else:
            worst = float(np.abs(got[0] - b64[0]).max())
            print(tag, "worst |fp32 count - fp64 count|", worst, "bound", n * 1e-5)
            assert worst <= n * 1e-5, (tag, worst)
    elif call == "marginals":
        blocks = bnpp.split_marginals(m.cards, None, got[0])
        if e["dtype"] == "f64":
            for j, a in enumerate(e["rows"]):
                sel = np.flatnonzero(idx == j)
                for v, x in zip(ev, a):                  # an evidence variable reads one-hot
                    assert np.array_equal(blocks[v][sel], np.tile(np.eye(m.cards[v])[x], (len(sel), 1))), (tag, j, v)
                if not ok[sel[0]]:                       # an impossible row reads NaN elsewhere
                    assert all(np.isnan(blocks[v][sel]).all() for v in free), (tag, j)
                    continue
                single = bnpp.marginals(ctx, m, dict(zip(ev, a)), "mf", bnpp.F64, targets=free)[0]
                for v in free:
                    err = np.abs(blocks[v][sel] - np.array(single[v])).max()
                    assert err <= 1e-12, (tag, j, v, err)
        else:
            err = np.abs(got[0] - b64[0]).max()
            assert err <= 1e-5, (tag, err)
    if capped and e["family"] != "slab":
        for cap in (1, 2, 3):
            grid_cap(cap)
            again = _run_call(ctx, e, rows, dtype, R)
            grid_cap(0)
            assert _same(got, again), (tag, cap)


def _check_partial_entry(ctx, e, capped, grid_cap):
    """An entry of plan_batch with partial evidence variables: against the single calls on
    the per-row masked model (missing_ref.masked_model: the mask-carrying factors times the row's indicator of
    its observed partial entries), with the row's hard entries as evidence (module docstring)."""
    from bnpp import synth
    import missing_ref
    m, _ = _model(e["model"])
    d = synth.read_uai(model_path(e["model"] + ".uai"))
    call, ev, part, R, n = bc.call_of(e), e["ev_vars"], e["partial"], e["R"], e["n_rows"]
    assert call == "batch" and part and e["soft"] is None
    hard = [v for v in ev if v not in part]
    rows = np.array(bc.rows_of(e), dtype=np.int64)
    idx = np.arange(n) % len(e["rows"])
    cols = [ev.index(v) for v in part]
    assert (rows[:, cols] == bnpp.MISSING).any() and (rows[:, cols] != bnpp.MISSING).any()
    tag = (e["dtype"], e["key"], call, e["model"], ev, part, e["target"], R)
    dtype = DT[e["dtype"]]
    _, groups = bc.plan(bnpp, e, model=m)
    assert e["key"] in {g["key"] for g in groups}, (tag, bc.sum_keys(groups))
    mf = bnpp.plan_batch(m, ev, partial=part)[-1]
    assert mf == missing_ref.mask_factors(d, ev, part), tag
    masked = [(bnpp.Model.from_dict(missing_ref.masked_model(d, ev, mf, a)), {v: int(a[ev.index(v)]) for v in hard})
              for a in e["rows"]]
    got = _run_call(ctx, e, rows, dtype, R)
    assert len(got[0]) == n
    distinct = np.array(e["rows"], dtype=np.int64)
    if e["dtype"] == "f32":
        _, zc, _ = bnpp.partition_batch(ctx, m, ev, distinct, dtype=bnpp.F32, rows_per_launch=1, partial=part)
        assert (zc > 0).all() and zc.max() / zc.min() < 2.0 ** 40, (tag, zc.min(), zc.max())
    one = _run_call(ctx, e, rows, dtype, 1)
    assert _same(got, one), (tag, "differs from rows_per_launch = 1")
    if e["dtype"] == "f64":
        for j, (mm, hev) in enumerate(masked):
            sel = np.flatnonzero(idx == j)
            if not len(sel):                             # n_rows = R + 3 may not reach every distinct row
                continue
            if e["target"] is None:
                lz1, z1, _ = bnpp.partition(ctx, mm, hev, "mf", bnpp.F64)
                assert (_bits(got[1][sel]) == _bits(np.array([z1]))[0]).all(), (tag, j, got[1][sel], z1)
                if z1 == 0:
                    assert (got[0][sel] == -np.inf).all() and lz1 == -np.inf, (tag, j)
                else:
                    bound = 4 * np.spacing(max(1.0, abs(lz1)))
                    assert (np.abs(got[0][sel] - lz1) <= bound).all(), (tag, j, got[0][sel], lz1, bound)
            else:
                z1 = bnpp.partition(ctx, mm, hev, "mf", bnpp.F64)[1]
                if z1 == 0:
                    assert np.isnan(got[0][sel]).all(), (tag, j)
                    continue
                want = np.array(bnpp.marginals(ctx, mm, hev, "mf", bnpp.F64, targets=[e["target"]])[0][e["target"]])
                err = np.abs(got[0][sel] - want).max()
                assert err <= 1e-12, (tag, j, err)
    else:
        b64 = _run_call(ctx, e, rows, bnpp.F64, R)
        if e["target"] is None:
            assert (np.abs(got[0] - b64[0]) <= 1e-6 * np.maximum(1.0, np.abs(b64[0]))).all(), (tag, got[0], b64[0])
        else:
            assert np.abs(got[0] - b64[0]).max() <= 1e-5, (tag, np.abs(got[0] - b64[0]).max())
    if capped and e["family"] != "slab":
        for cap in (1, 2, 3):
            grid_cap(cap)
            again = _run_call(ctx, e, rows, dtype, R)
            grid_cap(0)
            assert _same(got, again), (tag, cap)


def _check_entry(ctx, e, capped, grid_cap):
    if e.get("partial"):
        return _check_partial_entry(ctx, e, capped, grid_cap)
    if bc.call_of(e) != "batch":
        return _check_call_entry(ctx, e, capped, grid_cap)
    m, _ = _model(e["model"])
    rows = np.array(bc.rows_of(e), dtype=np.int64)
    idx = np.arange(e["n_rows"]) % len(e["rows"])
    tag = (e["dtype"], e["key"], e["model"], e["ev_vars"], e["target"], e["R"])
    _, groups = bc.plan(bnpp, e, model=m)
    assert e["key"] in {g["key"] for g in groups}, (tag, bc.sum_keys(groups))
    got = _run(ctx, e, rows, DT[e["dtype"]], e["R"])
    assert len(got[0]) == e["n_rows"]
    if e["dtype"] == "f64":
        s = _single(ctx, e)
        if e["mixed_launch"]:
            assert (s["rz"] == 0).any() and (s["rz"] > 0).any(), tag
        if e["target"] is None:
            lz, z = got
            assert np.array_equal(_bits(z), _bits(s["z"][idx])), (tag, np.flatnonzero(_bits(z) != _bits(s["z"][idx])))
            assert np.array_equal(z, s["rz"][idx]), (tag, "the CPU oracle disagrees")
            for r in range(e["n_rows"]):
                want = s["lz"][idx[r]]
                if s["rz"][idx[r]] == 0:
                    assert lz[r] == -np.inf and want == -np.inf and z[r] == 0.0, (tag, r)
                else:
                    bound = 4 * np.spacing(max(1.0, abs(want)))
                    assert abs(lz[r] - want) <= bound, (tag, r, lz[r], want, bound)
        else:
            post, want = got[0], s["post"][idx]
            assert post.shape == want.shape == (e["n_rows"], m.cards[e["target"]])
            assert np.array_equal(post, want, equal_nan=True), tag
            ok = s["rz"][idx] > 0
            assert np.isnan(post[~ok]).all() and not np.isnan(post[ok]).any(), tag
            assert np.array_equal(_bits(post[ok]), _bits(want[ok])), tag
            assert np.allclose(post[ok].sum(axis=1), 1.0, atol=1e-12), tag
    else:
        distinct = np.array(e["rows"], dtype=np.int64)
        _, zc, _ = bnpp.partition_batch(ctx, m, e["ev_vars"], distinct, dtype=bnpp.F32, rows_per_launch=1)
        assert (zc > 0).all() and zc.max() / zc.min() < 2.0 ** 40, (tag, zc.min(), zc.max())
        one = _run(ctx, e, rows, bnpp.F32, 1)
        assert _same_bits(got, one), (tag, [np.flatnonzero((_bits(x) != _bits(y)).reshape(len(x), -1).any(axis=1))
                                            for x, y in zip(got, one)])
        b64 = _run(ctx, e, rows, bnpp.F64, e["R"])
        if e["target"] is None:
            assert (np.abs(got[0] - b64[0]) <= 1e-6 * np.maximum(1.0, np.abs(b64[0]))).all(), (tag, got[0], b64[0])
        else:
            assert np.abs(got[0] - b64[0]).max() <= 1e-5, (tag, np.abs(got[0] - b64[0]).max())
    if capped and e["family"] != "slab":
        for cap in (1, 2, 3):
            grid_cap(cap)
            again = _run(ctx, e, rows, DT[e["dtype"]], e["R"])
            grid_cap(0)
            assert _same_bits(got, again), (tag, cap)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("family", ["generic", "stream", "slab"])
def test_batch_only_level_kernels(ctx, cat, monkeypatch, grid_cap, family, dt):
    sel = [(i, e) for i, e in enumerate(cat["entries"]) if e["family"] == family and e["dtype"] == dt]
    assert sel
    capped = cat["capped"][dt + " " + family]
    assert capped in [i for i, _ in sel]
    for i, e in sel:
        monkeypatch.setenv("BNPP_NO_O32", "1" if e["no_o32"] else "0")
        _check_entry(ctx, e, i == capped, grid_cap)


def test_alarm_rows_per_launch_off_the_powers_of_two(ctx):
    """alarm's 67 rows of test_gpu_batch.py at R = 2, 3, 5, 6, 7, 8, 12, 63, 65 and
    100: odd R, a multiple of 2 but not of 4, one under and one over a wave, an
    R that does not divide 67.  fp64: z with the bits of the single calls (and
    the oracle's, log10_z within 4 ulp: test_gpu_batch._check_fp64) and the
    posterior of variable 5 with the bits of bnpp.marginals; fp32: the bits of
    R = 1 on the possible-row set of test_rows_per_launch_fp32."""
    from test_gpu_batch import _check_fp64
    c = _case(ctx, "alarm")
    t = 5
    assert t not in c["ev_vars"]
    single = np.array([bnpp.marginals(ctx, c["m"], dict(zip(c["ev_vars"], (int(x) for x in r))), "mf", bnpp.F64,
                                      targets=[t])[0][t] for r in c["rows"]])
    rows32 = _possible_rows(ctx, c)
    lz1, z1, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], rows32, dtype=bnpp.F32, rows_per_launch=1)
    for R in ALARM_R:
        lz, z, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], c["rows"], dtype=bnpp.F64, rows_per_launch=R)
        _check_fp64(c, lz, z)
        post, _ = bnpp.posterior_batch(ctx, c["m"], c["ev_vars"], c["rows"], t, dtype=bnpp.F64, rows_per_launch=R)
        assert np.array_equal(post, single, equal_nan=True), R
        ok = c["z1"] > 0
        assert np.array_equal(_bits(post[ok]), _bits(single[ok])) and np.isnan(post[~ok]).all(), R
        lz32, z32, _ = bnpp.partition_batch(ctx, c["m"], c["ev_vars"], rows32, dtype=bnpp.F32, rows_per_launch=R)
        assert np.array_equal(_bits(z32), _bits(z1)) and np.array_equal(_bits(lz32), _bits(lz1)), R
