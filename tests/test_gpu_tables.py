"""GPU tests of the device-resident model tables.

Steps alone: bnpp_stage_tables and bnpp_mstep_dv on caller-owned buffers
against the numpy restatements (tables_ref).  Whole calls: bnpp.tensor's
expected_counts against the host-array call, with a Tables against
tables=None on a model made of the same values, log-form tables against brute
force; accumulate; the errors; bt.em against its three steps written out;
bt.log_likelihood's gradient, torch's gradcheck and five SGD steps.

Bounds.  The linear form of stage_tables, the M step, and every comparison of
two calls that do the same arithmetic: bit for bit.  The log form: 4 ulp of the
restatement for a double table, 1 float ulp for a float table (exp's 3-ulp
bound plus numpy's own; one rounding of values that may differ in their last
fp64 bits) -- the bounds of stage_loglik, for the same reason; tops, exp2,
maxbits and the shift exact.  Counts against brute force: n x 1e-12 (fp64),
n x 1e-5 (fp32).  log10_z / ln_z of two routes: 4 ulp of max(|value|, |shift|,
1).  The M step against learn.m_step: 2k ulp (two summation orders of k
non-negative terms, one rounding of the quotient on each side).  Every case that
computes a result runs with the grid capped at 1, 2 and 3 workgroups and
uncapped, with identical bits (a loop over CAPS inside the test, or the test
parametrised over them and compared with its uncapped run); the two tests that
check only argument errors or the job cache (test_mstep_errors,
test_expected_counts_shares_the_siblings_job) run uncapped.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_ref
import bnpp
import bnpp.tensor as bt
import counts_ref
import loglik_ref
import tables_ref as ref
from bnpp import learn, synth
from conftest import model_path
from counts_ref import EV_VARS
from device_io_ref import NONE

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
ND = {"f64": np.float64, "f32": np.float32}
TOL = {"f64": 1e-12, "f32": 1e-5}
CAPS = (0, 1, 2, 3)
P = C.c_void_p
L = bnpp._lib
GUARD = 256


@pytest.fixture
def grid_cap(ctx):
    yield ctx.set_max_grid
    ctx.set_max_grid(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_UNCAPPED = {}


def _same_at_every_cap(key, cap, *tensors):
    """The results of the uncapped run of a case parametrised over CAPS (it runs first), kept for the capped ones."""
    got = [t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64) for t in tensors]
    if cap == 0:
        _UNCAPPED[key] = got
    assert key in _UNCAPPED, "the uncapped case runs first"
    for a, b in zip(got, _UNCAPPED[key]):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (key, cap, "results depend on the grid")


def _ulp_ok(got, want, what, scale=0.0, bound=4):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (what, "non-finite entries differ")
    ulp = np.spacing(np.maximum(np.maximum(np.abs(want), np.abs(scale)), 1.0)[fin])
    err = np.abs(got[fin] - want[fin])
    worst = float((err / ulp).max()) if fin.any() else 0.0
    print(what, "worst error", worst, "ulp of max(|want|, |shift|, 1); bound", bound)
    assert (err <= bound * ulp).all(), (what, worst)


# ---- stage_tables alone ------------------------------------------------------------------------------------------

def _stage(ctx, values, sizes, dt, log):
    """bnpp_stage_tables between guard bands -> (tables, maxbits, exp2, tops, shift, status)."""
    n = len(sizes)
    off, total = ref.layout(sizes, ND[dt])
    buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    out = buf[GUARD:GUARD + total]
    meta = torch.full((n * 4 + 8,), -7, dtype=torch.int64, device=DEV)
    shift = torch.full((1 + n + 4,), -7.0, dtype=torch.float64, device=DEV)
    st = torch.full((1,), NONE, dtype=torch.int64, device=DEV)
    t_vals = _t(values)
    torch.cuda.synchronize()
    vd = (bnpp.F32 if values.dtype == np.float32 else bnpp.F64) | (bnpp.LIK_LOG if log else 0)
    bnpp._check(L.bnpp_stage_tables(ctx.handle, None, DT[dt], vd, n, (C.c_int64 * n)(*sizes), P(t_vals.data_ptr()),
                                    P(out.data_ptr()), P(meta.data_ptr()), P(shift.data_ptr()), P(st.data_ptr())), "stage_tables")
    ctx.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + total:] == 0xA5).all(), "guard band written"
    eb = np.dtype(ND[dt]).itemsize
    tables = [raw[GUARD + o:GUARD + o + s * eb].view(ND[dt]).copy() for o, s in zip(off, sizes)]
    used = np.zeros(total, dtype=bool)
    for o, s in zip(off, sizes):
        used[o:o + s * eb] = True
    assert (raw[GUARD:GUARD + total][~used] == 0xA5).all(), "the padding between the factors is not written"
    mt = meta.cpu().numpy()
    assert (mt[n * 4:] == -7).all() and (shift.cpu().numpy()[1 + n:] == -7.0).all()
    mt = mt[:n * 4].reshape(n, 4)
    assert np.array_equal(mt[:, 0] - out.data_ptr(), off) and np.array_equal(mt[:, 3], sizes), "the layout of upload_sources"
    sh = shift.cpu().numpy()
    return tables, [int(x) for x in mt[:, 1].view(np.uint64)], [int(x) for x in mt[:, 2]], sh[1:1 + n], sh[0], int(st.cpu()[0])


def _table_ulps(got, want):
    ulp = np.spacing(np.abs(want))                          # spacing(0) is the smallest subnormal
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp.astype(np.float64)).max())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("in_dt", ["f64", "f32"])
def test_stage_tables_linear_bit_for_bit(ctx, grid_cap, in_dt, dt):
    values = ref.linear_case(np.random.default_rng(5), ND[in_dt])
    want = ref.stage_tables(values, ref.SIZES, ND[dt])
    assert want[5] == NONE
    for cap in CAPS:
        grid_cap(cap)
        tables, maxbits, exp2, tops, shift, status = _stage(ctx, values, ref.SIZES, dt, False)
        assert status == NONE and shift == 0.0 and not np.signbit(shift)
        assert maxbits == want[1] and exp2 == want[2], (in_dt, dt, cap)
        assert np.array_equal(_bits(tops), _bits(want[3])), "a factor's top is its own largest entry"
        for f, (g, w) in enumerate(zip(tables, want[0])):
            assert _same_bits(g, w), (in_dt, dt, cap, f, np.flatnonzero(g != w)[:4])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_stage_tables_names_the_first_invalid_entry(ctx, grid_cap, dt):
    at = 1 + 63 + 64 + 65 + 105                             # factor 5 begins here
    for log, xs in ((False, (np.nan, -1.0, np.inf)), (True, (np.nan, np.inf))):
        for x in xs:
            values = (ref.log_case if log else ref.linear_case)(np.random.default_rng(8), np.float64)
            values[at + 300] = x                            # the first: factor 5, entry 300
            values[at + 301] = values[at + 4000] = x
            want = ref.stage_tables(values, ref.SIZES, ND[dt], log)
            assert want[5] == at + 300
            for cap in CAPS:
                grid_cap(cap)
                tables, maxbits, exp2, tops, shift, status = _stage(ctx, values, ref.SIZES, dt, log)
                assert status == at + 300, (log, x, cap, status)
                assert all(np.isfinite(t).all() for t in tables) and tables[5][300] == 0, "the rest of the buffer stays finite"
                assert exp2 == want[2] and maxbits == want[1] and np.array_equal(_bits(tops), _bits(want[3]))
                if not log:
                    assert all(_same_bits(g, w) for g, w in zip(tables, want[0]))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("in_dt", ["f64", "f32"])
def test_stage_tables_log_form(ctx, grid_cap, in_dt, dt):
    values = ref.log_case(np.random.default_rng(7), ND[in_dt])
    want = ref.stage_tables(values, ref.SIZES, ND[dt], log=True)
    assert want[5] == NONE and want[3][-1] == -np.inf and np.isfinite(want[4])
    bound = 4 if dt == "f64" else 1
    first = None
    for cap in CAPS:
        grid_cap(cap)
        tables, maxbits, exp2, tops, shift, status = _stage(ctx, values, ref.SIZES, dt, True)
        assert status == NONE and maxbits == want[1] and exp2 == want[2], (in_dt, dt, cap)
        assert np.array_equal(_bits(tops), _bits(want[3])), "the tops are the input's own entries"
        assert np.array_equal(_bits([shift]), _bits([want[4]])), "the sequential fp64 sum of the tops"
        worst = max(_table_ulps(g, w) for g, w in zip(tables, want[0]))
        print("stage_tables log", in_dt, dt, "cap", cap, "worst", worst, "ulp; bound", bound)
        assert worst <= bound
        assert (tables[-1] == 0).all() and exp2[-1] == 0 and maxbits[-1] == 0, "a factor of nothing but -inf"
        if first is None:
            first = tables
        assert all(_same_bits(g, w) for g, w in zip(tables, first)), "results do not depend on the grid"


# ---- bnpp_mstep_dv alone -----------------------------------------------------------------------------------------

def _cpts(rng, cards, scopes):
    vals = []
    for s in scopes:
        k = cards[s[-1]]
        t = rng.uniform(0.05, 1.0, (int(np.prod([cards[v] for v in s[:-1]], dtype=np.int64)), k))
        vals.append((t / t.sum(axis=1, keepdims=True)).reshape(-1).tolist())
    return {"type": "BAYES", "cards": list(cards), "scopes": [list(s) for s in scopes], "values": vals}


# a root CPT (one parent configuration); 65 parent configurations of a child of 7; children of 2 and of 1 value.
# And 400 configurations: more than a workgroup's lanes
MSTEP_MODELS = {"small": ([5, 13, 7, 2, 1], [[0], [0, 1, 2], [2, 3], [3, 4], [1]]), "wide": ([20, 20, 3], [[0], [0, 1, 2], [1]])}


@pytest.mark.parametrize("prior", [0.0, 0.5])
@pytest.mark.parametrize("name", sorted(MSTEP_MODELS))
def test_mstep_bit_for_bit(ctx, grid_cap, name, prior):
    rng = np.random.default_rng(19)
    d = _cpts(rng, *MSTEP_MODELS[name])
    m = bnpp.Model.from_dict(d)
    sizes, ks = [len(v) for v in d["values"]], ref.child_cards(d)
    old = ref.flat_values(d)
    counts = rng.uniform(0.0, 1.0, old.shape[0]) * 10.0 ** rng.integers(-3, 4, old.shape[0])
    zero = sizes[0] + 9 * ks[1]                             # the tenth parent configuration of the second CPT: unseen
    counts[zero:zero + ks[1]] = 0.0
    want = ref.mstep(counts, old, sizes, ks, prior)
    if prior == 0:
        assert np.array_equal(want[zero:zero + ks[1]], old[zero:zero + ks[1]])
    t_counts, t_old = _t(counts), _t(old)
    for cap in CAPS:
        grid_cap(cap)
        new = bt.m_step(ctx, m, t_counts, t_old, prior)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(new.cpu().numpy()), _bits(want)), (name, prior, cap)
        inplace = t_old.clone()
        assert bt.m_step(ctx, m, t_counts, inplace, prior, out=inplace) is inplace
        assert torch.equal(inplace, new), "in place and out of place: the same bits"
        assert torch.equal(t_old, _t(old)), "old_values are read only"
    host = ref.flat_values(learn.m_step(d, counts, prior))
    at = 0
    for s, k in zip(sizes, ks):
        ulps = np.abs(want[at:at + s] - host[at:at + s]) / np.spacing(np.maximum(want[at:at + s], host[at:at + s]))
        assert (ulps <= 2 * k).all(), (name, k, float(ulps.max()))
        at += s


def test_mstep_errors(ctx):
    d = _cpts(np.random.default_rng(1), *MSTEP_MODELS["small"])
    m = bnpp.Model.from_dict(d)
    n = sum(len(v) for v in d["values"])
    c = torch.ones(n, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        bt.m_step(ctx, m, c.cpu(), c)
    with pytest.raises(ValueError):
        bt.m_step(ctx, m, c[:-1], c)
    with pytest.raises(ValueError):
        bt.m_step(ctx, m, c.float(), c)
    with pytest.raises(bnpp.BnppError) as e:
        bt.m_step(ctx, m, c, c, prior=-1.0)
    assert e.value.status == bnpp.ERR_INVALID
    markov = bnpp.Model.load(model_path("ising4x4.uai"))
    k = bt._counts_size(markov)
    with pytest.raises(bnpp.BnppError) as e:
        bt.m_step(ctx, markov, torch.ones(k, dtype=torch.float64, device=DEV), torch.ones(k, dtype=torch.float64, device=DEV))
    assert e.value.status == bnpp.ERR_UNSUPPORTED


# ---- expected_counts, tables=None, against the host-array call ---------------------------------------------------

SOFT = {"asia": [2, 5], "alarm": [5, 12, 30]}
_CASES = {}


def _zero_scope(d):
    """The sorted scope of asia's first CPT with an entry that is exactly 0, and the row that hits it."""
    s, v = next((list(s), np.asarray(v).reshape([d["cards"][x] for x in s])) for s, v in zip(d["scopes"], d["values"])
                if len(s) >= 2 and (np.asarray(v) == 0).any())
    ev = sorted(s)
    at = np.argwhere(v == 0)[0]
    return ev, np.array([int(at[s.index(x)]) for x in ev])


def _case(ctx, name):
    if name not in _CASES:
        path = model_path(name + ".uai")
        m, d = bnpp.Model.load(path), synth.read_uai(path)
        n = 130
        samples, _, _ = bnpp.sample(ctx, m, n, seed=7)
        if name == "asia":                                  # possible rows, and exactly one impossible row, at 40
            ev, bad = _zero_scope(d)
            rows = np.asarray(samples)[:, ev].astype(np.int64)
            rows[40] = bad
            _, z = counts_ref.brute_counts(d, ev, rows)
            assert z[40] == 0 and (np.delete(z, 40) > 0).all()
        else:
            ev = EV_VARS[name]
            rows = np.asarray(samples)[:, ev].astype(np.int64)
        soft = []                                           # SOFT's variables, others for those that are evidence here
        for v in SOFT[name] + list(range(len(d["cards"]))):
            if v not in ev and v not in soft and len(soft) < len(SOFT[name]):
                soft.append(v)
        rng = np.random.default_rng(13)
        holes = rows.copy()
        holes[rng.random(rows.shape) < 0.3] = -1
        holes[40] = rows[40]
        cards = [d["cards"][v] for v in soft]
        lik = rng.uniform(0.05, 1.0, (n, sum(cards)))
        lik[rng.random(lik.shape) < 0.1] = 0.0
        lik[:, 0] = np.maximum(lik[:, 0], 0.1)
        ll = rng.uniform(-30.0, 30.0, (n, sum(cards)))
        ll[rng.random(ll.shape) < 0.15] = -np.inf
        ll[:, 0] = np.where(np.isfinite(ll[:, 0]), ll[:, 0], -2.0)
        w = rng.uniform(0.25, 2.0, n)
        w[rng.random(n) < 0.3] = 0.0
        w[40] = 1.5
        _CASES[name] = dict(m=m, d=d, ev=ev, rows=rows, holes=holes, soft=soft, cards=cards, lik=lik, ll=ll, w=w)
    return _CASES[name]


# the variants: (partial, soft, log_soft dtype, weights)
VARIANTS = {"plain": (False, False, None, False), "partial": (True, False, None, False), "soft": (False, True, None, False),
            "log64": (False, False, np.float64, False), "log32": (True, False, np.float32, False),
            "weights": (False, False, None, True), "all": (True, True, None, True)}


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", ["asia", "alarm"])
def test_expected_counts_against_the_host_array_call(ctx, grid_cap, name, variant, dt):
    c = _case(ctx, name)
    partial, soft, log_dt, weights = VARIANTS[variant]
    m, ev = c["m"], c["ev"]
    for n, rpl in ((1, 64), (63, 64), (65, 64), (130, 64), (130, 0)):
        rows = (c["holes"] if partial else c["rows"])[:n]
        kw_h, kw_d = dict(dtype=DT[dt], rows_per_launch=rpl), dict(dtype=DT[dt], rows_per_launch=rpl)
        if partial:
            kw_h["partial"] = kw_d["partial"] = ev
        if soft:
            kw_h["soft"], kw_d["soft"] = (c["soft"], c["lik"][:n]), (c["soft"], _t(c["lik"][:n]))
        shift = 0.0
        if log_dt is not None:                              # the host call takes E = exp(l - top); the shifts go back
            a = c["ll"][:n].astype(log_dt)
            kw_h["soft"] = (c["soft"], loglik_ref.linear(a, c["cards"]))
            kw_d["log_soft"] = (c["soft"], _t(a))
            shift = loglik_ref.shift_of(loglik_ref.tops(a, c["cards"], 0, n)) * loglik_ref.LOG10_E
        if weights:
            kw_h["weights"], kw_d["weights"] = c["w"][:n], _t(c["w"][:n])
        want, lz, n_imp = bnpp.expected_counts(ctx, m, ev, rows, **kw_h)
        what = (name, variant, dt, n, rpl)
        first = None
        for cap in (CAPS if (n, rpl) == (130, 64) else (0,)):
            grid_cap(cap)
            got, g_lz, g_ni = bt.expected_counts(ctx, m, ev, _t(rows), **kw_d)
            assert got.dtype == torch.float64 and g_lz.shape == (n,) and g_ni.dtype == torch.int64 and g_ni.dim() == 0
            g = got.cpu().numpy()
            if log_dt is None:
                assert np.array_equal(_bits(g), _bits(want)), (what, cap, np.flatnonzero(_bits(g) != _bits(want))[:8])
            else:                                           # exp on the device against numpy's: the counts' own figure
                assert np.abs(g - want).max() <= n * TOL[dt], (what, cap, float(np.abs(g - want).max()))
            _ulp_ok(g_lz.cpu().numpy(), lz + shift, what + (cap,), shift)
            assert int(g_ni) == n_imp, what
            if name == "asia":
                assert n_imp >= (1 if n > 40 else 0) and (variant not in ("plain", "weights", "partial") or n_imp == (n > 40))
            if first is None:
                first = g
            assert np.array_equal(_bits(g), _bits(first)), "results do not depend on the grid"
        grid_cap(0)


def test_expected_counts_shares_the_siblings_job(ctx):
    c = _case(ctx, "alarm")
    rows = c["rows"]
    bnpp.posterior_batch(ctx, c["m"], c["ev"], rows, 1)                  # another job takes the cache
    bt.expected_counts(ctx, c["m"], c["ev"], _t(rows), rows_per_launch=64)
    assert bnpp.last_timing()["plan_ms"] > 0, "expected_counts planned the job"
    bnpp.expected_counts(ctx, c["m"], c["ev"], rows, rows_per_launch=64)
    assert bnpp.last_timing()["plan_ms"] == 0, "the host-array call found it cached"
    bt.expected_counts(ctx, c["m"], c["ev"], _t(rows), rows_per_launch=64, weights=_t(c["w"]))
    assert bnpp.last_timing()["plan_ms"] == 0, "weights are launch data"


# ---- tables equal the model --------------------------------------------------------------------------------------

def _perturbed(d, rng):
    v = ref.flat_values(d)
    return v * rng.uniform(0.5, 1.5, v.shape[0]) + np.where(v > 0, 0.01, 0.0)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["asia", "alarm"])
def test_tables_equal_the_model(ctx, grid_cap, name, dt):
    c = _case(ctx, name)
    m, d, ev = c["m"], c["d"], c["ev"]
    t_rows = _t(c["rows"])
    kw = dict(dtype=DT[dt], rows_per_launch=64)
    host_before, _, _ = bnpp.expected_counts(ctx, m, ev, c["rows"], **kw)
    base, base_lz, base_ni = bt.expected_counts(ctx, m, ev, t_rows, **kw)
    tables = bt.Tables(ctx, m, DT[dt])
    assert not tables.log and np.array_equal(tables.values.cpu().numpy(), ref.flat_values(d))

    def same(res, want, what):
        assert torch.equal(res[0], want[0]) and torch.equal(res[2], want[2]), what
        assert np.array_equal(_bits(res[1].cpu().numpy()), _bits(want[1].cpu().numpy())), what

    same(bt.expected_counts(ctx, m, ev, t_rows, tables=tables, **kw), (base, base_lz, base_ni), "fresh from create")
    tables.set(_t(ref.flat_values(d)))
    same(bt.expected_counts(ctx, m, ev, t_rows, tables=tables, **kw), (base, base_lz, base_ni), "set to the model's own values")
    assert bnpp.last_timing()["plan_ms"] == 0, "the call after a set does not plan"
    for in_dt in (np.float64, np.float32):
        v = _perturbed(d, np.random.default_rng(23)).astype(in_dt)
        other = bnpp.Model.from_dict(ref.with_values(d, v.astype(np.float64)))
        want = bt.expected_counts(ctx, other, ev, t_rows, **kw)
        assert not torch.equal(want[0], base)
        for cap in CAPS:
            grid_cap(cap)
            values = _t(v)
            assert tables.set(values) is tables and tables.values is values and not tables.log
            same(bt.expected_counts(ctx, m, ev, t_rows, tables=tables, **kw), want, (name, dt, in_dt, cap))
        grid_cap(0)
        bt.expected_counts(ctx, m, ev, t_rows, tables=tables, **kw)
        assert bnpp.last_timing()["plan_ms"] == 0, "the second call after a set does not plan"
        back = bnpp.Model.from_dict(tables.to_model_dict(d))
        same(bt.expected_counts(ctx, back, ev, t_rows, **kw), want, "to_model_dict")
    host_after, _, _ = bnpp.expected_counts(ctx, m, ev, c["rows"], **kw)
    assert np.array_equal(_bits(host_after), _bits(host_before)), "the model's own job and values are untouched"
    same(bt.expected_counts(ctx, m, ev, t_rows, **kw), (base, base_lz, base_ni), "tables=None after the sets")
    # counts == NULL: the batch plan under the tables, against partition_batch on the model of the same values
    _, lz, _, ni = bt._counts_call(ctx, m, ev, t_rows, None, tables, None, None, None, False, None, "mf", None, 64, None,
                                   False, False)
    assert torch.equal(ni, want[2])
    lzb, _, _ = bt.partition_batch(ctx, other, ev, t_rows, **kw)
    assert np.array_equal(_bits(lz.cpu().numpy()), _bits(lzb.cpu().numpy())), "the batch plan under the tables"
    tables.close()


# ---- log tables --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_log_tables_against_brute_force(ctx, grid_cap, dt):
    c = _case(ctx, "asia")
    m, d, ev, rows = c["m"], c["d"], c["ev"], c["rows"]
    n = rows.shape[0]
    t_rows = _t(rows)
    v = _perturbed(d, np.random.default_rng(29))
    sizes = [len(x) for x in d["values"]]
    # per factor an offset: the tables' shift is about their sum, 300, and exp(l) still fits a double
    offs = np.concatenate([np.full(k, o) for k, o in zip(sizes, [90.0, -20.0, 60.0, 0.0, 45.0, 30.0, 80.0, 15.0])])
    with np.errstate(divide="ignore"):
        logs = np.log(v) + offs                             # -inf where asia's CPTs are 0
    assert np.isneginf(logs).any()
    want, z = ref.brute_counts_flat(d, np.exp(logs), ev, rows)
    assert (z > 0).sum() == n - 1
    tables = bt.Tables(ctx, m, DT[dt])
    kw = dict(tables=tables, rows_per_launch=64)
    args = (None, None, None, False, None, "mf", None, 64, None, True, True)
    # The linear call on exp(l).  As for log_soft (test_gpu_loglik), exp(l) is E = exp(l - top) times exp(top), and E is
    # read back from the staging entry: the linear form of E = 2 T is T again, so the two calls read the same tables
    # and differ by the shift alone, which one rounded add restores
    T, _, exp2, tops, shift, st = _stage(ctx, logs, sizes, dt, True)
    assert st == NONE and exp2 == [1] * len(sizes) and abs(shift - 300.0) < 10.0
    tables.set(_t(np.concatenate([2.0 * t.astype(np.float64) for t in T])))
    lin_counts, lin_lz, lin_ln, lin_ni = bt._counts_call(ctx, m, ev, t_rows, None, tables, *args)
    first = None
    for cap in CAPS:
        grid_cap(cap)
        tables.set(_t(logs), log=True)
        assert tables.log
        counts, lz, ni = bt.expected_counts(ctx, m, ev, t_rows, **kw)
        g = counts.cpu().numpy()
        worst = float(np.abs(g - want).max())
        print("log tables", dt, "cap", cap, "worst |count - brute|", worst, "bound", n * TOL[dt])
        assert worst <= n * TOL[dt]
        assert int(ni) == 1 == int(lin_ni) and lz[40] == -np.inf
        assert torch.equal(counts, lin_counts), "the same tables: the counts do not see the shift"
        _, lz2, ln, _ = bt._counts_call(ctx, m, ev, t_rows, None, tables, *args)
        _ulp_ok(ln.cpu().numpy(), lin_ln.cpu().numpy() + shift, ("ln_z of log tables", dt, cap), shift)
        _ulp_ok(lz.cpu().numpy(), lin_lz.cpu().numpy() + shift * loglik_ref.LOG10_E, ("log10_z of log tables", dt, cap), shift)
        assert torch.equal(lz, lz2)
        fin = z > 0
        err = np.abs(ln.cpu().numpy()[fin] - np.log(z[fin]))
        print("log tables", dt, "worst |ln_z - brute|", float(err.max()))
        assert (err <= (1e-12 if dt == "f64" else 1e-5) * np.maximum(1.0, np.abs(np.log(z[fin])))).all()
        if first is None:
            first = (g, ln.cpu().numpy())
        assert np.array_equal(_bits(g), _bits(first[0])) and np.array_equal(_bits(ln.cpu().numpy()), _bits(first[1]))
    # a factor of nothing but -inf: every row is impossible
    dead = logs.copy()
    dead[sizes[0]:sizes[0] + sizes[1]] = -np.inf
    for cap in CAPS:
        grid_cap(cap)
        tables.set(_t(dead), log=True)
        counts, lz, ni = bt.expected_counts(ctx, m, ev, t_rows, **kw)
        assert int(ni) == n and (counts == 0).all() and torch.isneginf(lz).all(), cap
    grid_cap(0)
    tables.close()


# ---- accumulate --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", CAPS)
def test_accumulate_continues_the_fold(ctx, grid_cap, cap):
    c = _case(ctx, "alarm")
    m, ev = c["m"], c["ev"]
    t_rows, w = _t(c["rows"]), _t(c["w"])
    grid_cap(cap)
    whole, _, ni = bt.expected_counts(ctx, m, ev, t_rows, weights=w, rows_per_launch=64)
    _same_at_every_cap("accumulate", cap, whole, ni)
    out = torch.full_like(whole, 7.0)                       # overwritten by the first call
    a, _, na = bt.expected_counts(ctx, m, ev, t_rows[:65], weights=w[:65], rows_per_launch=64, out=out)
    assert a.data_ptr() == out.data_ptr() and not torch.equal(a, whole)
    b, _, nb = bt.expected_counts(ctx, m, ev, t_rows[65:], weights=w[65:], rows_per_launch=64, out=out, accumulate=True)
    assert b.data_ptr() == out.data_ptr()
    assert np.array_equal(_bits(b.cpu().numpy()), _bits(whole.cpu().numpy())), "two halves, one fold"
    assert int(na) + int(nb) == int(ni)
    with pytest.raises(ValueError):
        bt.expected_counts(ctx, m, ev, t_rows, accumulate=True)


# ---- errors ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", CAPS)
def test_errors(ctx, grid_cap, cap):
    grid_cap(cap)
    c = _case(ctx, "alarm")
    m, ev, soft = c["m"], c["ev"], c["soft"]
    n = 130
    rows, lik, ll, w = _t(c["rows"]), _t(c["lik"]), _t(c["ll"]), _t(c["w"])
    call = lambda **k: bt.expected_counts(ctx, m, ev, rows, rows_per_launch=64, **k)

    def raises(msgs, **k):
        with pytest.raises(bnpp.BnppError) as e:
            call(**k)
        assert e.value.status == bnpp.ERR_INVALID and all(s in str(e.value) for s in msgs), str(e.value)

    bad_w = w.clone()
    bad_w[100], bad_w[101] = -0.5, float("nan")
    raises(("evidence row 100", "the weight must be finite and not negative"), weights=bad_w)
    bad_w[100] = float("inf")
    raises(("evidence row 100", "the weight must be finite and not negative"), weights=bad_w)
    bad_rows = rows.clone()
    bad_rows[70, 1], bad_rows[71, 0] = m.cards[ev[1]], -3
    with pytest.raises(bnpp.BnppError) as e:
        bt.expected_counts(ctx, m, ev, bad_rows, rows_per_launch=64)
    assert "evidence row 70: value %d of variable %d is outside" % (m.cards[ev[1]], ev[1]) in str(e.value)
    k0 = m.cards[soft[0]]
    bad_lik = lik.clone()
    bad_lik[100, k0 + 1], bad_lik[101, 0] = -1.0, float("nan")
    raises(("row 100", "value 1 of soft variable %d " % soft[1], "must be finite and not negative"), soft=(soft, bad_lik))
    bad_ll = ll.clone()
    bad_ll[100, k0 + 1] = float("nan")
    raises(("row 100", "value 1 of soft variable %d " % soft[1], "must not be NaN or +inf"), log_soft=(soft, bad_ll))
    # the first bad cell of each kind is also what the host-array call names
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.expected_counts(ctx, m, ev, c["rows"], weights=bad_w.cpu().numpy())
    assert "evidence row 100: the weight must be finite and not negative" in str(e.value)
    with pytest.raises(ValueError):
        call(soft=(soft, lik), log_soft=(soft, ll))
    for k in (dict(weights=w.cpu()), dict(weights=w[:-1]), dict(weights=w.float()), dict(soft=(soft, lik.cpu())),
              dict(out=torch.zeros(3, dtype=torch.float64, device=DEV)), dict(tables=object())):
        with pytest.raises(ValueError):
            call(**k)
    with pytest.raises(ValueError):
        bt.expected_counts(ctx, m, ev, rows.cpu())
    # tables of another model, of another dtype than the call's
    other = _case(ctx, "asia")["m"]
    t_other, t32 = bt.Tables(ctx, other, bnpp.F64), bt.Tables(ctx, m, bnpp.F32)
    raises(("another model",), tables=t_other)
    raises(("another dtype",), tables=t32, dtype=bnpp.F64)
    call(tables=t32)                                        # dtype defaults to the tables'
    # Tables.set: CPU tensors, another size, another dtype; the first invalid entry is named by factor and index
    size = t32.size
    for bad in (torch.ones(size), torch.ones(size - 1, device=DEV), torch.ones(size, device=DEV, dtype=torch.float16)):
        with pytest.raises(ValueError):
            t32.set(bad)
    sizes = [len(v) for v in c["d"]["values"]]
    v = torch.ones(size, dtype=torch.float64, device=DEV)
    v[sum(sizes[:3]) + 1] = -2.0
    v[sum(sizes[:5])] = float("nan")
    with pytest.raises(bnpp.BnppError) as e:
        t32.set(v)
    assert e.value.status == bnpp.ERR_INVALID and "factor 3: entry 1 must be finite and not negative" in str(e.value)
    v[sum(sizes[:3]) + 1] = float("-inf")                   # valid as a log
    with pytest.raises(bnpp.BnppError) as e:
        t32.set(v, log=True)
    assert "factor 5: entry 0 must not be NaN or +inf" in str(e.value)
    for t in (t_other, t32):
        t.close()


# ---- bt.em -------------------------------------------------------------------------------------------------------

def _em_case(ctx):
    d = ref.child_last(synth.read_uai(model_path("asia.uai")))
    truth = bnpp.Model.from_dict(d)
    n = 96
    samples, _, _ = bnpp.sample(ctx, truth, n, seed=21)
    ev = [1, 3, 5, 7]                                       # the other four variables are hidden
    rows = np.asarray(samples)[:, ev].astype(np.int64)
    rng = np.random.default_rng(4)
    start = dict(d)
    start["values"] = []
    for s, v in zip(d["scopes"], d["values"]):
        k = d["cards"][s[-1]]
        t = np.asarray(v).reshape(-1, k) * rng.uniform(0.5, 1.5, (len(v) // k, k)) + 0.05
        start["values"].append((t / t.sum(axis=1, keepdims=True)).reshape(-1).tolist())
    return start, ev, rows, rng.uniform(0.25, 1.0, n)      # weights of at most 1: a row's error is not scaled up


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("weighted", [False, True])
def test_em_is_its_three_steps(ctx, grid_cap, weighted, cap):
    grid_cap(cap)
    start, ev, rows, w = _em_case(ctx)
    n = rows.shape[0]
    m = bnpp.Model.from_dict(start)
    t_rows, t_w = _t(rows), (_t(w) if weighted else None)
    tables, lls = bt.em(ctx, m, ev, t_rows, 3, weights=t_w)
    assert isinstance(tables, bt.Tables) and len(lls) == 3 and not tables.log
    # the same three steps written out
    mine = bt.Tables(ctx, m)
    cur = _t(ref.flat_values(start))
    mine_lls = []
    for it in range(3):
        counts, lz, ni = bt.expected_counts(ctx, m, ev, t_rows, weights=t_w, tables=mine)
        assert int(ni) == 0
        want, z = ref.brute_counts_flat(start, cur.cpu().numpy(), ev, rows, w if weighted else None)
        worst = float(np.abs(counts.cpu().numpy() - want).max())
        print("em iteration", it, "worst |count - brute|", worst, "bound", n * 1e-12)
        assert worst <= n * 1e-12
        mine_lls.append(float(torch.sum(lz if t_w is None else t_w * lz)))
        cur = bt.m_step(ctx, m, counts, cur)
        mine.set(cur)
    assert np.array_equal(_bits(lls), _bits(mine_lls)), (lls, mine_lls)
    assert torch.equal(tables.values, cur), "bit for bit the three steps"
    _same_at_every_cap(("em", weighted), cap, cur, lls)
    for a, b in zip(lls, lls[1:]):
        assert b >= a - 1e-9 * abs(a), lls
    _, host_lls = learn.em(ctx, start, ev, rows, iters=1, weights=w if weighted else None)
    assert abs(lls[0] - host_lls[0]) <= 4 * n * np.spacing(abs(host_lls[0])), (lls[0], host_lls[0])
    fitted = tables.to_model_dict(start)
    for s, v in zip(fitted["scopes"], fitted["values"]):
        assert np.allclose(np.asarray(v).reshape(-1, start["cards"][s[-1]]).sum(axis=1), 1.0, atol=1e-12)
    # a given table set is refitted in place; one in log form is refused
    again, lls2 = bt.em(ctx, m, ev, t_rows, 1, weights=t_w, tables=bt.Tables(ctx, m))
    assert lls2 == lls[:1]
    with pytest.raises(ValueError):
        bt.em(ctx, m, ev, t_rows, 1, tables=bt.Tables(ctx, m).set(torch.zeros(mine.size, dtype=torch.float64, device=DEV), log=True))


# ---- bt.log_likelihood -------------------------------------------------------------------------------------------

CHAIN = {"type": "BAYES", "cards": [2, 3, 2], "scopes": [[0], [0, 1], [1, 2]]}


def _chain(rng):
    d = dict(CHAIN, values=_cpts(rng, CHAIN["cards"], CHAIN["scopes"])["values"])
    return d, bnpp.Model.from_dict(d)


@pytest.mark.parametrize("cap", CAPS)
def test_log_likelihood_gradcheck(ctx, grid_cap, cap):
    grid_cap(cap)
    d, m = _chain(np.random.default_rng(37))
    rows = _t(np.array([[0], [1], [1]], dtype=np.int64))    # the last variable is observed; two are hidden
    x = _t(np.log(ref.flat_values(d)) + np.random.default_rng(2).uniform(-0.5, 0.5, 14)).requires_grad_(True)
    fn = lambda t: bt.log_likelihood(ctx, m, [2], rows, t)[0]
    assert torch.isfinite(fn(x)) and fn(x).dim() == 0
    assert torch.autograd.gradcheck(fn, (x,))               # torch's default eps and tolerances
    w = _t(np.array([0.5, 2.0, 1.25]))
    assert torch.autograd.gradcheck(lambda t: bt.log_likelihood(ctx, m, [2], rows, t, weights=w)[0], (x,))


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_log_likelihood_gradient_is_grad_times_counts(ctx, grid_cap, dt, cap):
    grid_cap(cap)
    c = _case(ctx, "asia")
    m, d, ev = c["m"], c["d"], c["ev"]
    t_rows, w = _t(c["rows"]), _t(c["w"])
    with np.errstate(divide="ignore"):
        logs = np.log(_perturbed(d, np.random.default_rng(41)))
    tables = bt.Tables(ctx, m, DT[dt])
    for in_dt in (torch.float64, torch.float32):
        x = _t(logs).to(in_dt).requires_grad_(True)
        ll, ln_z, ni = bt.log_likelihood(ctx, m, ev, t_rows, x, weights=w, tables=tables, rows_per_launch=64)
        assert ll.requires_grad and not ln_z.requires_grad and not ni.requires_grad and int(ni) == 1
        fin = torch.isfinite(ln_z)
        assert torch.equal(ll.detach(), torch.sum(torch.where(fin, w * ln_z, torch.zeros_like(ln_z))))
        (ll * 1.75).backward()
        counts, lz, _ = bt.expected_counts(ctx, m, ev, t_rows, weights=w, tables=tables, rows_per_launch=64)
        assert bnpp.last_timing()["plan_ms"] == 0, "the counts job of the tables, shared"
        assert x.grad.dtype == in_dt and torch.equal(x.grad, (1.75 * counts).to(in_dt))
        assert (x.grad[torch.isneginf(x.detach())] == 0).all(), "-inf: gradient 0"
        _same_at_every_cap(("loglik", dt, str(in_dt)), cap, ll, ln_z, x.grad)
    # grad mode off, or nothing to differentiate: the batch plan, another job than the counts one
    _, ln_ref, _ = bt.log_likelihood(ctx, m, ev, t_rows, _t(logs).requires_grad_(True), weights=w, tables=tables, rows_per_launch=64)
    ln_ref = ln_ref.cpu().numpy()
    for x in (_t(logs).requires_grad_(True), _t(logs)):
        with torch.no_grad():
            ll0, ln0, ni0 = bt.log_likelihood(ctx, m, ev, t_rows, x, weights=w, tables=tables, rows_per_launch=64)
        assert not ll0.requires_grad and int(ni0) == 1
        ln0 = ln0.cpu().numpy()
        fin = np.isfinite(ln_ref)                           # two plans of one Z: the figures of a Z, not bits
        assert np.array_equal(np.isfinite(ln0), fin) and (np.abs(ln0[fin] - ln_ref[fin]) <= TOL[dt] * np.maximum(1.0, np.abs(ln_ref[fin]))).all()
        bt.log_likelihood(ctx, m, ev, t_rows, x.detach(), weights=w, tables=tables, rows_per_launch=64)
        assert bnpp.last_timing()["plan_ms"] == 0, "the batch job of the tables, cached"
        bt.expected_counts(ctx, m, ev, t_rows, weights=w, tables=tables, rows_per_launch=64)
        assert bnpp.last_timing()["plan_ms"] > 0, "the counts job is another one: the context caches one job"
    # log_soft that requires grad: log_partition's business
    soft = c["soft"]
    ls = _t(c["ll"]).requires_grad_(True)
    with pytest.raises(ValueError, match="log_partition"):
        bt.log_likelihood(ctx, m, ev, t_rows, _t(logs), log_soft=(soft, ls))
    # weights are not differentiated, and a dtype other than the tables' is refused
    with pytest.raises(ValueError, match="weights"):
        bt.log_likelihood(ctx, m, ev, t_rows, _t(logs).requires_grad_(True), weights=w.clone().requires_grad_(True), tables=tables)
    with pytest.raises(ValueError, match="dtype"):
        bt.log_likelihood(ctx, m, ev, t_rows, _t(logs), tables=tables, dtype=bnpp.F32 if dt == "f64" else bnpp.F64)
    ll1, _, _ = bt.log_likelihood(ctx, m, ev, t_rows, _t(logs).requires_grad_(True), log_soft=(soft, ls.detach()), tables=tables)
    assert torch.isfinite(ll1)
    tables.close()


@pytest.mark.parametrize("cap", CAPS)
def test_log_likelihood_keeps_one_table_set_per_model(ctx, grid_cap, cap):
    grid_cap(cap)
    d, m = _chain(np.random.default_rng(43))
    rows = _t(np.array([[0], [1]], dtype=np.int64))
    x = _t(np.log(ref.flat_values(d)))
    a = bt.log_likelihood(ctx, m, [2], rows, x)[0]
    t = bt._LogLikelihood.tables_for(ctx, m, bnpp.F64)
    assert t.log and t.values.data_ptr() == x.data_ptr()
    b = bt.log_likelihood(ctx, m, [2], rows, x)[0]
    assert bt._LogLikelihood.tables_for(ctx, m, bnpp.F64) is t and torch.equal(a, b)
    assert bnpp.last_timing()["plan_ms"] == 0
    # normalised CPTs and every variable observed or summed out: ll is the log of the rows' probability
    want, z = ref.brute_counts_flat(d, ref.flat_values(d), [2], np.array([[0], [1]]))
    assert abs(float(a) - np.log(z).sum()) <= 1e-12
    _same_at_every_cap("one table set", cap, a)


@pytest.mark.parametrize("cap", CAPS)
def test_five_sgd_steps_on_log_tables_do_not_increase_the_loss(ctx, grid_cap, cap):
    grid_cap(cap)
    start, ev, rows, w = _em_case(ctx)
    m = bnpp.Model.from_dict(start)
    t_rows = _t(rows)
    ks = ref.child_cards(start)
    sizes = [len(v) for v in start["values"]]
    theta = _t(np.log(ref.flat_values(start))).requires_grad_(True)
    opt = torch.optim.SGD([theta], lr=0.2)
    losses = []
    for step in range(6):
        opt.zero_grad()
        parts, at = [], 0
        for s, k in zip(sizes, ks):                         # CPTs: log_softmax over the child
            parts.append(torch.log_softmax(theta[at:at + s].reshape(-1, k), dim=1).reshape(-1))
            at += s
        ll, _, ni = bt.log_likelihood(ctx, m, ev, t_rows, torch.cat(parts))
        loss = -ll / rows.shape[0]
        losses.append(float(loss.detach()))
        loss.backward()
        assert int(ni) == 0 and torch.isfinite(theta.grad).all() and (theta.grad != 0).any()
        opt.step()
    print("losses", losses)
    _, host_lls = learn.em(ctx, start, ev, rows, iters=1)
    assert abs(losses[0] + host_lls[0] / loglik_ref.LOG10_E / rows.shape[0]) <= 1e-12 * max(1.0, abs(losses[0]))
    assert np.isfinite(losses).all() and losses[-1] <= losses[0], losses
    _same_at_every_cap("sgd", cap, losses, theta)


def test_a_table_set_outlives_its_context(ctx):
    """A context closed before its table sets takes their buffers with it: they can still be freed, and nothing else."""
    d, m = _chain(np.random.default_rng(47))
    other = bnpp.Context(0)
    t = bt.Tables(other, m)
    t.set(_t(ref.flat_values(d)))
    keep = bt.Tables(other, m)
    other.close()
    with pytest.raises(bnpp.BnppError) as e:
        L_set = bnpp._lib.bnpp_tables_set_dv(t.handle, P(t.values.data_ptr()), bnpp.F64)
        bnpp._check(L_set, "bnpp_tables_set_dv")
    assert e.value.status == bnpp.ERR_INVALID and "context" in str(e.value)
    with pytest.raises(bnpp.BnppError) as e:
        bt.expected_counts(ctx, m, [2], _t(np.array([[0]], dtype=np.int64)), tables=t)
    assert e.value.status == bnpp.ERR_INVALID and "another context" in str(e.value)
    t.close()
    keep.close()
    keep.close()                                            # closing twice is fine
