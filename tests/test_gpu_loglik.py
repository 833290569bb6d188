"""GPU tests of log-space soft evidence and the differentiable log-likelihood.

Steps alone: bnpp_stage_loglikelihoods and bnpp_emit_row_logs on caller-owned
buffers between guard bands, against the numpy restatements (loglik_ref).
Whole calls: bnpp.tensor's four batched calls with log_soft=(vars, loglik)
against the same calls with soft=(vars, E), E read back from the staging entry.
bnpp.tensor.log_partition against brute force, its gradient, torch's gradcheck
and five steps of a training loop.

Bounds.  T of a double table: 4 ulp of the restatement -- OpenCL's 3-ulp bound
for exp plus numpy's own 1 ulp (a subnormal's ulp is 2^-1074).  T of a float
table: 1 float ulp -- one rounding of values that may differ in their last fp64
bits.  e_row, top and the status word are exact.  The log emit alone: ln_z and
log10_z within 4 ulp of max(|value|, 1), the project's figure for log10_z (only
ln / log10 of the mantissa in [0.5, 1) is not numpy's own operation; its
magnitude is below 0.7, so a 3-ulp error of it is under 2^-51 whatever the shift
cancels).  Whole calls: log10_z within 4 ulp of max(|value|, |shift|, 1), the
wider scale the issue sets for them alone.  Measured worst cases are printed by
the tests and recorded in DESIGN.md section 20.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_ref
import bnpp
import bnpp.tensor as bt
import device_io_ref as dref
import loglik_ref as ref
from bnpp import synth
from conftest import model_path
from counts_ref import EV_VARS

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
ND = {"f64": np.float64, "f32": np.float32}
GUARD = 32
ROWS = [1, 63, 64, 65, 257]
P = C.c_void_p
L = bnpp._lib
LOG = bnpp.LIK_LOG


@pytest.fixture
def grid_cap(ctx):
    yield ctx.set_max_grid
    ctx.set_max_grid(0)


def _window(R):
    """(n_rows, row0, rows_live) of a last launch of R rows: row0 > 0, and rows_live < R where R allows."""
    live = max(1, R - 3)
    return 5 + live, 5, live


def _guarded(a, fill):
    a = np.ascontiguousarray(a)
    buf = np.full(a.size + 2 * GUARD, fill, dtype=a.dtype)
    buf[GUARD:GUARD + a.size] = a.reshape(-1)
    t = torch.from_numpy(buf).to(DEV)
    return t, t[GUARD:GUARD + a.size]


def _check_guards(t, n, fill, what):
    got = t.cpu().numpy()
    assert (got[:GUARD] == fill).all() and (got[GUARD + n:] == fill).all(), ("guard band written", what)
    return got[GUARD:GUARD + n]


def _status():
    return torch.full((2,), dref.NONE, dtype=torch.int64, device=DEV)


def _ints(xs):
    return (C.c_int * max(len(xs), 1))(*[int(x) for x in xs])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _ulp_ok(got, want, what, scale=None):
    """Within 4 ulp of max(|want|, 1) -- with `scale` (the whole calls only) of max(|want|, |scale|, 1); non-finite
    entries equal."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (what, "non-finite entries differ")
    ref_mag = np.maximum(np.abs(want), 1.0) if scale is None else np.maximum(np.maximum(np.abs(want), np.abs(scale)), 1.0)
    ulp = np.spacing(ref_mag[fin])
    err = np.abs(got[fin] - want[fin])
    worst = float((err / ulp).max()) if fin.any() else 0.0
    print(what, "worst log error", worst, "ulp of max(|want|, 1)" if scale is None else "ulp of max(|want|, |shift|, 1)", "; bound 4")
    assert (err <= 4 * ulp).all(), (what, worst)


# ---- stage_loglik ------------------------------------------------------------------------------------------------

def _stage_loglik(ctx, ll, cards, row0, R, dt):
    n_rows, ws = ll.shape
    t_ll = torch.from_numpy(np.ascontiguousarray(ll)).to(DEV)
    buf, out = _guarded(np.full(ws * R, -7.0, dtype=ND[dt]), -7.0)
    ebuf, e_row = _guarded(np.full(R, -7, dtype=np.int64), -7)
    tbuf, top = _guarded(np.full(len(cards) * R, -7.0), -7.0)
    st = _status()
    torch.cuda.synchronize()
    bnpp._check(L.bnpp_stage_loglikelihoods(ctx.handle, None, DT[dt], (bnpp.F32 if ll.dtype == np.float32 else bnpp.F64) | LOG,
                                            len(cards), _ints(cards), n_rows, row0, R, P(t_ll.data_ptr()),
                                            P(out.data_ptr()), P(e_row.data_ptr()), P(top.data_ptr()), P(st.data_ptr())),
                "stage_loglik")
    ctx.synchronize()
    got = _check_guards(buf, ws * R, -7.0, ("stage_loglik", cards, R, dt)).reshape(ws, R)
    return (got, _check_guards(ebuf, R, -7, ("stage_loglik e_row", cards, R)),
            _check_guards(tbuf, len(cards) * R, -7.0, ("stage_loglik top", cards, R)).reshape(len(cards), R), st.cpu().numpy())


def _stage_lik(ctx, lik, cards, row0, R, dt):
    n_rows, ws = lik.shape
    t_lik = torch.from_numpy(np.ascontiguousarray(lik)).to(DEV)
    out = torch.full((ws * R,), -7.0, dtype=torch.float32 if dt == "f32" else torch.float64, device=DEV)
    e_row = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    st = _status()
    torch.cuda.synchronize()
    bnpp._check(L.bnpp_stage_likelihoods(ctx.handle, None, DT[dt], bnpp.F32 if lik.dtype == np.float32 else bnpp.F64,
                                         len(cards), _ints(cards), n_rows, row0, R, P(t_lik.data_ptr()),
                                         P(out.data_ptr()), P(e_row.data_ptr()), P(st.data_ptr())), "stage_lik")
    ctx.synchronize()
    return out.cpu().numpy().reshape(ws, R), e_row.cpu().numpy(), st.cpu().numpy()


def _table_ulps(got, want):
    """The worst distance of a staged table from the restatement, in ulp of the table's dtype at the restatement."""
    ulp = np.spacing(np.abs(want))                          # spacing(0) is the smallest subnormal
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp.astype(np.float64)).max())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("in_dt", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(ref.CARDS))
@pytest.mark.parametrize("R", ROWS)
def test_stage_loglik_against_the_restatement(ctx, grid_cap, R, name, in_dt, dt):
    cards = ref.CARDS[name]
    n_rows, row0, _ = _window(R)
    ll = ref.loglik_case(np.random.default_rng(R * 7 + len(cards)), n_rows, cards, ND[in_dt])
    want, e_want, top_want, st = ref.stage_loglik(ll, cards, row0, R, ND[dt])
    assert st == dref.NONE
    first = None
    for cap in ((0, 1, 2, 3) if R == 257 else (0,)):
        grid_cap(cap)
        got, e_got, top_got, status = _stage_loglik(ctx, ll, cards, row0, R, dt)
        assert np.array_equal(e_got, e_want) and (status == dref.NONE).all(), (name, R, in_dt, dt, cap)
        assert _same_bits(top_got, top_want), "the tops are the input's own entries"
        worst = _table_ulps(got, want)
        print("stage_loglik", name, R, in_dt, dt, "cap", cap, "worst", worst, "ulp; bound", 4 if dt == "f64" else 1)
        assert worst <= (4 if dt == "f64" else 1), (name, R, in_dt, dt, cap, worst)
        dead = np.repeat(top_want == -np.inf, cards, axis=0)
        assert (got[dead] == 0).all(), "an all -inf block is stored as zeros"
        if first is None:
            first = got
        assert _same_bits(got, first), "results do not depend on the grid"
    # the contract: what the linear step makes of E = 2 T is T again, and e_row counts the finite blocks
    E = np.ascontiguousarray((2 * first.astype(np.float64)).T.astype(ND[dt]))   # (R, Ws): the launch as a call of R rows
    back, e_back, status = _stage_lik(ctx, E, cards, 0, R, dt)
    assert _same_bits(back, first) and np.array_equal(e_back, e_want) and (status == dref.NONE).all()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("in_dt", ["f64", "f32"])
def test_stage_loglik_names_the_first_invalid_cell(ctx, in_dt, dt):
    cards, R = [40, 2], 65
    n_rows, row0, _ = _window(R)
    rng = np.random.default_rng(9)
    for x in (np.nan, np.inf):
        ll = rng.uniform(-3.0, 0.0, (n_rows, 42)).astype(ND[in_dt])
        first = row0 + 40
        ll[first, 39] = x
        ll[first, 41] = ll[first + 1, 5] = x                # later invalid cells: not the first
        ll[first + 2, :40] = -np.inf
        ll[first + 2, 7] = x                                # an invalid entry counts as -inf: the block is dead
        ll[2, 7] = x                                        # a row of an earlier launch
        ll[first + 3, 3] = -np.inf                          # -inf is valid
        want, e_want, top_want, st = ref.stage_loglik(ll, cards, row0, R, ND[dt])
        assert st == first * 42 + 39
        got, e_got, top_got, status = _stage_loglik(ctx, ll, cards, row0, R, dt)
        assert status[1] == st and status[0] == dref.NONE, (x, status)
        assert np.array_equal(e_got, e_want) and _same_bits(top_got, top_want) and top_got[0, 42] == -np.inf
        assert _table_ulps(got, want) <= (4 if dt == "f64" else 1) and np.isfinite(got).all()
        assert got[39, 40] == 0 and (got[:40, 42] == 0).all() and e_got[42] == 1


# ---- emit_row_logs -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("R", ROWS)
def test_emit_row_logs(ctx, grid_cap, R, dt):
    n_rows, row0, live = _window(R)
    rng = np.random.default_rng(R)
    lo, hi = (-1070, 1000) if dt == "f64" else (-148, 120)
    with np.errstate(under="ignore"):
        table = np.ldexp(rng.uniform(0.5, 1.0, R), rng.integers(lo, hi, R).astype(np.int32)).astype(ND[dt])
    table[:-1:5] = 0                                        # impossible rows (row 0 among them): -inf, and z = 0
    e_row = rng.integers(0, 4, R).astype(np.int64)
    n_soft = 3
    top = rng.uniform(-900.0, 900.0, (n_soft, R))
    top[:, R // 2] = [-2500.0, -2499.5, -0.5]               # a shift of -5000
    top[1, R - 1] = -np.inf                                 # a dead block: the shift is -inf (its row reads p = 0 in a call)
    t_top, t_e = torch.from_numpy(top).to(DEV), torch.from_numpy(e_row).to(DEV)
    cases = ((True, -37, True, n_soft, (1, 1, 1)), (True, 0, False, n_soft, (1, 0, 0)), (False, 2 ** 21, True, n_soft, (0, 1, 0)),
             (True, 5, True, 0, (1, 1, 1)), (None, 3, True, n_soft, (0, 0, 1)), (True, -(2 ** 21), True, 1, (1, 1, 0)))
    for has_b, exp2, use_e, ns, use in cases:
        tab = None if has_b is None else table if has_b else table[-1:]
        want = [np.full(n_rows, -7.0) if u else None for u in use]
        ref.emit_row_logs(*want, tab, bool(has_b), exp2, e_row if use_e else None, top[:ns] if ns else None, row0, live)
        t_tab = torch.from_numpy(np.ascontiguousarray(tab)).to(DEV) if tab is not None else None
        meta = torch.tensor([0, 0, exp2, R], dtype=torch.int64, device=DEV)
        first = None
        for cap in ((0, 1, 2, 3) if R == 257 and has_b and exp2 == -37 else (0,)):
            grid_cap(cap)
            bufs = [_guarded(np.full(n_rows, -7.0), -9.0) if u else (None, None) for u in use]
            torch.cuda.synchronize()
            bnpp._check(L.bnpp_emit_row_logs(ctx.handle, None, DT[dt], P(t_tab.data_ptr()) if tab is not None else None,
                                             1 if has_b else 0, P(meta.data_ptr()), P(t_e.data_ptr()) if use_e else None,
                                             ns, P(t_top.data_ptr()) if ns else None, R, row0, live,
                                             *[P(b[1].data_ptr()) if b[1] is not None else None for b in bufs]),
                        "emit_row_logs")
            ctx.synchronize()
            got = [_check_guards(b[0], n_rows, -9.0, "emit_row_logs") if b[0] is not None else None for b in bufs]
            for i, nm in ((0, "ln_z"), (1, "log10_z")):
                if use[i]:
                    g = got[i]
                    assert (g[:row0] == -7.0).all() and (g[row0 + live:] == -7.0).all(), "rows outside the launch"
                    _ulp_ok(g[row0:row0 + live], want[i][row0:row0 + live], ("emit_row_logs", nm, R, dt, has_b, exp2))
            if use[2]:
                g = got[2][row0:row0 + live]
                if use[0]:                                  # z = exp(ln_z): of the device's own ln_z, to exp's 3 + 1 ulp
                    with np.errstate(over="ignore", under="ignore"):
                        w = np.exp(got[0][row0:row0 + live])
                    fin = np.isfinite(w) & (w > np.ldexp(1.0, -1000))
                    assert np.array_equal(g[~fin] == 0, w[~fin] == 0) and np.array_equal(np.isinf(g[~fin]), np.isinf(w[~fin]))
                    assert (np.abs(g[fin] - w[fin]) <= 4 * np.spacing(w[fin])).all()
                else:
                    w = want[2][row0:row0 + live]
                    fin = np.isfinite(w) & (w > np.ldexp(1.0, -1000))
                    assert np.allclose(g[fin], w[fin], rtol=1e-10, atol=0) and np.array_equal(np.isinf(g), np.isinf(w))
                if tab is not None and has_b:
                    assert (g[tab[:live] == 0] == 0).all(), "an impossible row: z = 0"
            if first is None:
                first = got
            for a, b in zip(got, first):
                assert a is None or np.array_equal(_bits(a), _bits(b)), "results do not depend on the grid"
        if use[0] and has_b and ns == n_soft and R > 1:
            assert want[0][row0] == -np.inf and np.isfinite(want[0][row0 + 1]), "an impossible row among possible ones"


# ---- whole calls -------------------------------------------------------------------------------------------------

SOFT = {"alarm": [5, 12, 30], "ising6x6": [3, 14, 22, 30]}
# every variant carries log_soft: full rows; rows with missing values; missing values and a float32 loglik; no
# evidence but the soft
VARIANTS = ("plain", "partial", "both", "soft_only")
_CASES = {}


def _case(ctx, name):
    if name not in _CASES:
        path = model_path(name + ".uai")
        m, d = bnpp.Model.load(path), synth.read_uai(path)
        n = 300
        samples, _, _ = bnpp.sample(ctx, m, n, seed=7)
        rows = batch_ref.draw_rows(d["cards"], EV_VARS[name], n, 11, samples)
        rng = np.random.default_rng(13)
        holes = rows.copy()
        holes[rng.random(rows.shape) < 0.3] = -1
        cards = [d["cards"][v] for v in SOFT[name]]
        ws = sum(cards)
        ll = rng.uniform(-40.0, 40.0, (n, ws))
        ll[rng.random((n, ws)) < 0.2] = -np.inf
        w = 0
        for i, k in enumerate(cards):                       # every block keeps a finite entry; tops of +-800 among them
            ll[:, w] = np.where(np.isfinite(ll[:, w]), ll[:, w], -3.0) + np.array([0.0, 800.0, -800.0])[(np.arange(n) + i) % 3]
            w += k
        c = dict(m=m, d=d, ev=EV_VARS[name], rows=rows, holes=holes, soft=SOFT[name], cards=cards, E={}, shift={})
        for key, a in (("f64", ll), ("f32", ll.astype(np.float32))):
            t, e_row, top, st = _stage_loglik(ctx, a, cards, 0, n, "f64")     # E, read back from the staging entry
            assert (st == dref.NONE).all() and (e_row == len(cards)).all()
            c["E"][key], c["shift"][key] = np.ascontiguousarray(2 * t.T), ref.shift_of(top)
            c["ll_" + key] = a
        _CASES[name] = c
    return _CASES[name]


def _args(c, variant, n):
    """(ev_vars, rows tensor, keyword arguments of the log call, of the linear call, the rows' shifts)."""
    ev = [] if variant == "soft_only" else c["ev"]
    rows = c["holes"][:n] if variant in ("partial", "both") else c["rows"][:n]
    rows = rows[:, :len(ev)] if len(ev) else np.zeros((n, 0), dtype=np.int64)
    key = "f32" if variant == "both" else "f64"
    kw = {"partial": c["ev"]} if variant in ("partial", "both") else {}
    k_log = dict(kw, log_soft=(c["soft"], torch.from_numpy(c["ll_" + key][:n]).to(DEV)))
    k_lin = dict(kw, soft=(c["soft"], torch.from_numpy(c["E"][key][:n]).to(DEV)))
    return ev, torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), k_log, k_lin, c["shift"][key][:n]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["alarm", "ising6x6"])
@pytest.mark.parametrize("call", ["partition", "marginals", "mpe", "sample"])
def test_whole_calls_against_the_linear_calls_on_E(ctx, call, name, variant, R, dt):
    c = _case(ctx, name)
    m = c["m"]
    for n in (1, 65, 300):                                  # n < R; a padded last launch; several launches
        ev, t_rows, k_log, k_lin, shift = _args(c, variant, n)
        common = dict(dtype=DT[dt], rows_per_launch=R)
        what = (call, name, variant, R, dt, n)
        if call == "partition":
            lz, z, _ = bt.partition_batch(ctx, m, ev, t_rows, **common, **k_lin)
            g_lz, g_z, _ = bt.partition_batch(ctx, m, ev, t_rows, **common, **k_log)
            with np.errstate(over="ignore", under="ignore"):
                w = np.exp(g_lz.cpu().numpy() / ref.LOG10_E)
            fin = np.isfinite(w) & (w > 1e-290)
            assert np.allclose(g_z.cpu().numpy()[fin], w[fin], rtol=1e-9, atol=0), (what, "z = exp(ln Z)")
        elif call == "marginals":
            out, lz = bt.marginals_batch(ctx, m, ev, t_rows, **common, **k_lin)
            g_out, g_lz = bt.marginals_batch(ctx, m, ev, t_rows, **common, **k_log)
            assert np.array_equal(_bits(g_out.cpu().numpy()), _bits(out.cpu().numpy())), what
        elif call == "mpe":
            lz, x, _ = bt.mpe_batch(ctx, m, ev, t_rows, **common, **k_lin)
            g_lz, g_x, _ = bt.mpe_batch(ctx, m, ev, t_rows, **common, **k_log)
            assert torch.equal(g_x, x), what
        else:
            s, lz, deg = bt.sample_batch(ctx, m, ev, t_rows, 3, seed=5, **common, **k_lin)
            g_s, g_lz, g_deg = bt.sample_batch(ctx, m, ev, t_rows, 3, seed=5, **common, **k_log)
            assert torch.equal(g_s, s) and torch.equal(g_deg, deg), what
        lz = lz.cpu().numpy()
        assert n < 300 or np.isfinite(lz).any()
        _ulp_ok(g_lz.cpu().numpy(), lz + shift * ref.LOG10_E, what, shift)


# ---- log_partition -----------------------------------------------------------------------------------------------

LP = {"cancer": ([0], [1, 3]), "asia": ([0, 3], [2, 5, 7])}
_LP_CASES = {}


def _lp_case(name, n=70):
    if name not in _LP_CASES:
        path = model_path(name + ".uai")
        m, d = bnpp.Model.load(path), synth.read_uai(path)
        ev, soft = LP[name]
        rng = np.random.default_rng(17)
        rows = np.stack([rng.integers(0, d["cards"][v], n) for v in ev], axis=1)
        cards = [d["cards"][v] for v in soft]
        ll = rng.uniform(-6.0, 2.0, (n, sum(cards)))
        ll[rng.random(ll.shape) < 0.15] = -np.inf
        w = 0
        for i, k in enumerate(cards):                       # every block keeps a finite entry; tops of +-800 among them
            ll[:, w] = np.where(np.isfinite(ll[:, w]), ll[:, w], -1.0)
            ll[:, w:w + k] += np.array([0.0, 800.0, -800.0])[(np.arange(n) + i) % 3][:, None]
            w += k
        ln_z, post = ref.brute_log(d, ev, rows, soft, ll)   # the reference, once
        for a in (rows, ll, ln_z, post):
            a.setflags(write=False)
        _LP_CASES[name] = dict(m=m, d=d, ev=ev, soft=soft, cards=cards, rows=rows, ll=ll, ln_z=ln_z, post=post)
    return _LP_CASES[name]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(LP))
def test_log_partition_against_brute_force(ctx, name, dt):
    c = _lp_case(name)
    n = 70
    t_rows = torch.from_numpy(c["rows"].copy()).to(DEV)
    common = dict(dtype=DT[dt], rows_per_launch=64)          # the last launch is padded
    fin = np.isfinite(c["ln_z"])
    assert fin.sum() > n // 2
    tol = 1e-12 if dt == "f64" else 1e-5
    for lik_dt in (torch.float64, torch.float32):
        if lik_dt == torch.float32 and dt == "f64":
            continue                                        # a float32 loglik: with the float tables, below
        ll = torch.from_numpy(c["ll"].copy()).to(DEV).to(lik_dt).requires_grad_(True)
        want_ln, want_post = (c["ln_z"], c["post"]) if lik_dt == torch.float64 else \
            ref.brute_log(c["d"], c["ev"], c["rows"], c["soft"], c["ll"].astype(np.float32))
        ln_z = bt.log_partition(ctx, c["m"], c["ev"], t_rows, log_soft=(c["soft"], ll), **common)
        assert ln_z.dtype == torch.float64 and ln_z.shape == (n,) and ln_z.requires_grad
        g = ln_z.detach().cpu().numpy()
        assert np.array_equal(np.isfinite(g), fin) and (g[~fin] == -np.inf).all()
        bound = tol * np.maximum(1.0, np.abs(want_ln[fin])) if dt == "f64" else tol
        print("log_partition", name, dt, lik_dt, "worst ln_z error", float(np.abs(g[fin] - want_ln[fin]).max()))
        assert (np.abs(g[fin] - want_ln[fin]) <= bound).all()
        # post: brute force, and the bits of marginals_batch on the soft variables
        w = torch.from_numpy(np.random.default_rng(5).uniform(-2.0, 2.0, n)).to(DEV)   # signed weights
        (w * torch.where(torch.isfinite(ln_z), ln_z, torch.zeros_like(ln_z))).sum().backward()
        post, _ = bt.marginals_batch(ctx, c["m"], c["ev"], t_rows, targets=c["soft"], log_soft=(c["soft"], ll.detach()), **common)
        assert np.array_equal(np.isnan(post.cpu().numpy()).any(axis=1), ~fin)
        err = np.abs(post.cpu().numpy()[fin] - want_post[fin])
        print("log_partition", name, dt, lik_dt, "worst posterior error", float(err.max()))
        assert (err <= tol).all()
        # the gradient is w * post exactly (cast to a float32 loglik's dtype); rows left out of the loss: zeros
        w_used = torch.where(torch.isfinite(ln_z.detach()), w, torch.zeros_like(w))
        want_grad = (w_used[:, None] * post).to(lik_dt)
        assert ll.grad.dtype == lik_dt
        assert torch.equal(ll.grad[torch.from_numpy(fin).to(DEV)], want_grad[torch.from_numpy(fin).to(DEV)])
        assert (ll.grad[torch.isneginf(ll.detach()) & torch.from_numpy(fin).to(DEV)[:, None]] == 0).all(), "-inf: gradient 0"
        assert torch.isneginf(ll.detach()).any()


def test_log_partition_gradient_of_every_row_is_w_times_post(ctx):
    """All rows in the loss, signed weights: loglik.grad == w[:, None] * post bit for bit, NaN rows included."""
    c = _lp_case("cancer")
    t_rows = torch.from_numpy(c["rows"].copy()).to(DEV)
    ll = torch.from_numpy(c["ll"].copy()).to(DEV).requires_grad_(True)
    ln_z = bt.log_partition(ctx, c["m"], c["ev"], t_rows, log_soft=(c["soft"], ll), rows_per_launch=64)
    w = torch.from_numpy(np.random.default_rng(6).uniform(-2.0, 2.0, 70)).to(DEV)
    ln_z.backward(w)
    post, _ = bt.marginals_batch(ctx, c["m"], c["ev"], t_rows, targets=c["soft"], log_soft=(c["soft"], ll.detach()), rows_per_launch=64)
    assert np.array_equal(_bits(ll.grad.cpu().numpy()), _bits((w[:, None] * post).cpu().numpy()))
    assert (w < 0).any() and (w > 0).any()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(LP))
def test_post_has_the_bits_of_marginals_batch_on_the_soft_variables(ctx, name, dt):
    """A gradient of ones is post itself (1.0 * x is x): loglik.grad against marginals_batch's out with no rounding
    in between; an impossible row is NaN in both."""
    c = _lp_case(name)
    t_rows = torch.from_numpy(c["rows"].copy()).to(DEV)
    ll = torch.from_numpy(c["ll"].copy()).to(DEV).requires_grad_(True)
    common = dict(dtype=DT[dt], rows_per_launch=64)
    ln_z = bt.log_partition(ctx, c["m"], c["ev"], t_rows, log_soft=(c["soft"], ll), **common)
    ln_z.backward(torch.ones_like(ln_z))
    post, _ = bt.marginals_batch(ctx, c["m"], c["ev"], t_rows, targets=c["soft"], log_soft=(c["soft"], ll.detach()), **common)
    got, want = ll.grad.cpu().numpy(), post.cpu().numpy()
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(got[fin]), _bits(want[fin]))
    assert fin.any() and np.array_equal(np.isfinite(ln_z.detach().cpu().numpy()), fin.all(axis=1))


def test_log_partition_with_no_soft_variable_has_an_empty_gradient(ctx):
    c = _lp_case("asia")
    t_rows = torch.from_numpy(c["rows"].copy()).to(DEV)
    ll = torch.zeros((70, 0), dtype=torch.float64, device=DEV, requires_grad=True)
    ln_z = bt.log_partition(ctx, c["m"], c["ev"], t_rows, log_soft=([], ll), rows_per_launch=64)
    want = bt.log_partition(ctx, c["m"], c["ev"], t_rows, rows_per_launch=64)
    assert torch.equal(ln_z.detach(), want)
    fin = torch.isfinite(ln_z.detach())
    ln_z[fin].sum().backward()
    assert ll.grad is not None and ll.grad.shape == (70, 0) and ll.grad.dtype == torch.float64


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_an_impossible_row_reads_minus_inf_and_nan_and_leaves_its_neighbours_alone(ctx, dt):
    c = _lp_case("cancer")
    fin = np.isfinite(c["ln_z"])
    bad = next(i for i in range(65, 69) if fin[i - 1:i + 2].all())      # in the second launch, between possible rows
    t_rows = torch.from_numpy(c["rows"].copy()).to(DEV)
    res = {}
    for key in ("live", "dead"):
        a = c["ll"].copy()
        if key == "dead":
            a[bad, :c["cards"][0]] = -np.inf                # an all -inf block
        ll = torch.from_numpy(a).to(DEV).requires_grad_(True)
        ln_z = bt.log_partition(ctx, c["m"], c["ev"], t_rows, log_soft=(c["soft"], ll), dtype=DT[dt], rows_per_launch=64)
        ln_z.backward(torch.ones_like(ln_z))
        res[key] = (ln_z.detach().cpu().numpy(), ll.grad.cpu().numpy())
    assert res["dead"][0][bad] == -np.inf and np.isnan(res["dead"][1][bad]).all()
    assert np.isfinite(res["live"][0][bad]) and np.isfinite(res["live"][1][bad]).all()
    others = np.arange(70) != bad
    for i in (0, 1):
        assert np.array_equal(res["dead"][i][others], res["live"][i][others], equal_nan=True), "the neighbours keep their bits"


def test_log_partition_gradcheck(ctx):
    c = _lp_case("cancer")
    rows = torch.from_numpy(c["rows"][:3].copy()).to(DEV)
    rng = np.random.default_rng(23)
    ll = torch.from_numpy(rng.uniform(-2.0, 1.0, (3, sum(c["cards"])))).to(DEV).requires_grad_(True)   # finite, possible
    fn = lambda x: bt.log_partition(ctx, c["m"], c["ev"], rows, log_soft=(c["soft"], x))
    assert torch.isfinite(fn(ll)).all()
    assert torch.autograd.gradcheck(fn, (ll,))              # torch's default eps and tolerances


def test_log_partition_shares_the_siblings_jobs(ctx):
    c = _lp_case("asia")
    t_rows = torch.from_numpy(c["rows"].copy()).to(DEV)
    E = ref.linear(c["ll"], c["cards"])
    for grad, host, kw in ((False, bnpp.partition_batch, {}), (True, bnpp.marginals_batch, dict(targets=c["soft"]))):
        ll = torch.from_numpy(c["ll"].copy()).to(DEV).requires_grad_(grad)
        bnpp.posterior_batch(ctx, c["m"], c["ev"], c["rows"], 1)          # another job takes the cache
        bt.log_partition(ctx, c["m"], c["ev"], t_rows, log_soft=(c["soft"], ll), rows_per_launch=64)
        assert bnpp.last_timing()["plan_ms"] > 0, "log_partition planned the job"
        host(ctx, c["m"], c["ev"], c["rows"], rows_per_launch=64, soft=(c["soft"], E), **kw)
        assert bnpp.last_timing()["plan_ms"] == 0, "the host-array call found it cached"
        bt.log_partition(ctx, c["m"], c["ev"], t_rows, log_soft=(c["soft"], ll), rows_per_launch=64)
        assert bnpp.last_timing()["plan_ms"] == 0
    # grad mode off: the batch plan, whatever loglik requires
    ll = torch.from_numpy(c["ll"].copy()).to(DEV).requires_grad_(True)
    bnpp.partition_batch(ctx, c["m"], c["ev"], c["rows"], rows_per_launch=64, soft=(c["soft"], E))
    with torch.no_grad():
        ln_z = bt.log_partition(ctx, c["m"], c["ev"], t_rows, log_soft=(c["soft"], ll), rows_per_launch=64)
    assert bnpp.last_timing()["plan_ms"] == 0 and not ln_z.requires_grad


def test_log_partition_without_soft_evidence_is_ln_z_of_the_rows(ctx):
    c = _lp_case("asia")
    t_rows = torch.from_numpy(c["rows"].copy()).to(DEV)
    ln_z = bt.log_partition(ctx, c["m"], c["ev"], t_rows, rows_per_launch=64)
    _, z, _ = bt.partition_batch(ctx, c["m"], c["ev"], t_rows, rows_per_launch=64)
    with np.errstate(divide="ignore"):
        _ulp_ok(ln_z.cpu().numpy(), np.log(z.cpu().numpy()), "ln_z of hard evidence")
    assert not ln_z.requires_grad and np.isfinite(ln_z.cpu().numpy()).any()


# ---- errors ------------------------------------------------------------------------------------------------------

def test_errors(ctx):
    c = _case(ctx, "alarm")
    m, ev, soft = c["m"], c["ev"], c["soft"]
    rows = torch.from_numpy(c["rows"][:130]).to(DEV)
    ll = torch.from_numpy(c["ll_f64"][:130]).to(DEV)
    E = torch.from_numpy(c["E"]["f64"][:130]).to(DEV)
    calls = [lambda **k: bt.partition_batch(ctx, m, ev, rows, **k), lambda **k: bt.marginals_batch(ctx, m, ev, rows, **k),
             lambda **k: bt.mpe_batch(ctx, m, ev, rows, **k), lambda **k: bt.sample_batch(ctx, m, ev, rows, 2, **k),
             lambda **k: bt.log_partition(ctx, m, ev, rows, **k)]
    for f in calls:
        with pytest.raises(ValueError):
            f(log_soft=(soft, ll.cpu()))                    # a CPU tensor
        with pytest.raises(ValueError):
            f(log_soft=(soft, ll.to(torch.int64)))          # an integer loglik
        with pytest.raises(ValueError):
            f(log_soft=(soft, ll.to(torch.float16)))        # no half input
        with pytest.raises(ValueError):
            f(log_soft=(soft, ll[:, :-1]))                  # another width
    for f in calls[:4]:
        with pytest.raises(ValueError):
            f(soft=(soft, E), log_soft=(soft, ll))          # both forms at once
    w = m.cards[soft[0]]
    for x in (np.nan, np.inf):
        bad = ll.clone()
        bad[100, w + 1] = x                                 # row 100, value 1 of the second soft variable
        bad[101, 0] = x
        for f in calls:
            for grad in (False, True):
                with pytest.raises(bnpp.BnppError) as e:
                    f(log_soft=(soft, bad.clone().requires_grad_(grad)), rows_per_launch=64)
                msg = str(e.value)
                assert e.value.status == bnpp.ERR_INVALID and "row 100" in msg and "value 1 of soft variable %d " % soft[1] in msg
                assert "must not be NaN or +inf" in msg, msg


# ---- a training loop ---------------------------------------------------------------------------------------------

def test_five_sgd_steps_do_not_increase_the_loss(ctx):
    """A 6-step HMM of 3 states whose emission scores are the logits of a 2-layer net: -ln_z.mean() after five SGD
    steps is not above where it began."""
    T, S, n = 6, 3, 40
    rng = np.random.default_rng(31)
    prior = rng.dirichlet(np.ones(S))
    trans = rng.dirichlet(np.ones(S), size=S)
    model = {"type": "BAYES", "cards": [S] * T, "scopes": [[0]] + [[t - 1, t] for t in range(1, T)],
             "values": [prior.tolist()] + [trans.reshape(-1).tolist() for _ in range(1, T)]}
    m = bnpp.Model.from_dict(model)
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Tanh(), torch.nn.Linear(8, S)).to(DEV).double()
    feats = torch.from_numpy(rng.normal(size=(n, T, 4))).to(DEV)
    rows = torch.zeros((n, 0), dtype=torch.int32, device=DEV)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    losses = []
    for step in range(6):
        opt.zero_grad()
        logits = net(feats).reshape(n, T * S)
        if step == 0:                                       # the first loss against brute force over the 3^6 paths
            want, _ = ref.brute_log(model, [], np.zeros((n, 0), dtype=np.int64), list(range(T)), logits.detach().cpu().numpy())
        loss = -bt.log_partition(ctx, m, [], rows, log_soft=(list(range(T)), logits)).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any() for p in net.parameters())
        opt.step()
    print("losses", losses)
    assert abs(losses[0] + want.mean()) <= 1e-12 * max(1.0, abs(want.mean()))
    assert len(losses) == 6 and np.isfinite(losses).all() and losses[-1] <= losses[0], losses
