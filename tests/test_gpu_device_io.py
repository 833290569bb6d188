"""GPU tests of the device-resident batched calls.

Steps alone: bnpp_stage_evidence_rows, bnpp_stage_likelihoods,
bnpp_emit_row_scalars and bnpp_emit_row_states on caller-owned buffers between
guard bands, bit for bit against the numpy restatements (device_io_ref).
Whole calls: the four _dv calls (through bnpp.tensor) against their host-array
siblings with the same arguments.

log10_z / log10_value: within 4 ulp of max(|want|, 1).  The only operation that
can differ from the host's is log10 of a mantissa in [0.5, 1), whose magnitude
is below 0.302; a 3-ulp bound on it (OpenCL's) is under 2^-52, one rounding of
the sum comes on top, and 4 ulp is the figure the project already uses for
log10_z.  Everything else is bit-identical.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_ref
import bnpp
import bnpp.tensor as bt
import device_io_ref as ref
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


@pytest.fixture
def grid_cap(ctx):
    yield ctx.set_max_grid
    ctx.set_max_grid(0)


def _window(R):
    """(n_rows, row0, rows_live) of a last launch of R rows: row0 > 0, and rows_live < R where R allows."""
    live = max(1, R - 3)
    return 5 + live, 5, live


def _guarded(a, fill):
    """A device tensor holding `a` between two guard bands of `fill`, and the view of its payload."""
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
    return torch.full((2,), ref.NONE, dtype=torch.int64, device=DEV)


def _ints(xs):
    return (C.c_int * max(len(xs), 1))(*[int(x) for x in xs])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ulp_ok(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (what, "non-finite entries differ")
    bound = 4 * np.spacing(np.maximum(np.abs(want[fin]), 1.0))
    err = np.abs(got[fin] - want[fin])
    worst = float((err / np.spacing(np.maximum(np.abs(want[fin]), 1.0))).max()) if fin.any() else 0.0
    print(what, "worst log10 error", worst, "ulp of max(|want|, 1); bound 4")
    assert (err <= bound).all(), (what, worst)


# ---- stage_rows --------------------------------------------------------------------------------------------------

EV_CARDS = [2, 300, 3, 2, 5, 2, 2, 7, 2, 2, 2, 4, 2, 2, 2, 2, 3]
EV_PARTIAL = [0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]


def _ev_rows(rng, n_rows, n_ev):
    ev = np.stack([rng.integers(0, EV_CARDS[j], n_rows) for j in range(n_ev)], axis=1).astype(np.int32) if n_ev \
        else np.zeros((n_rows, 0), dtype=np.int32)
    for j in range(n_ev):
        if EV_PARTIAL[j]:
            ev[rng.random(n_rows) < 0.3, j] = -1
    return ev


def _stage_rows(ctx, ev, n_ev, row0, R, partial=True):
    n_rows = ev.shape[0]
    t_ev = torch.from_numpy(np.ascontiguousarray(ev)).to(DEV)
    buf, out = _guarded(np.full(max(n_ev, 1) * R, -7, dtype=np.int32), -7)
    st = _status()
    torch.cuda.synchronize()
    pf = (C.c_ubyte * max(n_ev, 1))(*EV_PARTIAL[:n_ev]) if partial else None
    bnpp._check(L.bnpp_stage_evidence_rows(ctx.handle, None, n_ev, _ints(EV_CARDS[:n_ev]), pf, n_rows, row0, R,
                                           P(t_ev.data_ptr() or None), P(out.data_ptr()), P(st.data_ptr())), "stage_rows")
    ctx.synchronize()
    got = _check_guards(buf, max(n_ev, 1) * R, -7, ("stage_rows", n_ev, R))
    return got[:n_ev * R].reshape(n_ev, R), st.cpu().numpy()


@pytest.mark.parametrize("n_ev", [0, 1, 3, 17])
@pytest.mark.parametrize("R", ROWS)
def test_stage_rows_bit_for_bit(ctx, grid_cap, R, n_ev):
    n_rows, row0, _ = _window(R)
    ev = _ev_rows(np.random.default_rng(R * 31 + n_ev), n_rows, n_ev)
    want, st = ref.stage_rows(ev, EV_CARDS[:n_ev], EV_PARTIAL[:n_ev], row0, R)
    assert st == ref.NONE
    for cap in ((0, 1, 2, 3) if R == 257 else (0,)):
        grid_cap(cap)
        got, status = _stage_rows(ctx, ev, n_ev, row0, R)
        assert np.array_equal(got, want), (R, n_ev, cap)
        assert (status == ref.NONE).all(), "only an invalid cell touches the status block"


@pytest.mark.parametrize("R", [65, 257])
def test_stage_rows_names_the_first_invalid_cell(ctx, R):
    n_rows, row0, _ = _window(R)
    rng = np.random.default_rng(R)
    for (j, x) in ((0, -1), (2, -2), (1, 300), (4, 5), (16, 3)):   # -1 where not partial, -2, a value equal to the card
        ev = _ev_rows(rng, n_rows, 17)
        first = row0 + R // 2
        ev[first, j] = x
        ev[first + 1:, 3] = 2                               # later invalid cells: not the first
        ev[:row0, 0] = 9                                    # rows of earlier launches are not this launch's
        want, st = ref.stage_rows(ev, EV_CARDS, EV_PARTIAL, row0, R)
        assert st == first * 17 + j
        got, status = _stage_rows(ctx, ev, 17, row0, R)
        assert np.array_equal(got, want) and status[0] == st and status[1] == ref.NONE, (j, x, status)
    ev = _ev_rows(rng, n_rows, 17)                          # without partial flags every -1 is invalid
    ev[:, 2] = 0
    ev[row0 + 1, 2] = -1
    ev[:, 4] = ev[:, 16] = 0
    got, status = _stage_rows(ctx, ev, 17, row0, R, partial=False)
    assert status[0] == (row0 + 1) * 17 + 2 and got[2, 1] == 0


# ---- stage_lik ---------------------------------------------------------------------------------------------------

SOFT_CARDS = {"three": [3], "one": [1], "wide": [300, 2], "binaries": [2] * 17}


def _lik(mode, rng, n, cards):
    ws = sum(cards)
    if mode == "wide":                                      # magnitudes over 2^+-1000
        return np.ldexp(rng.uniform(0.5, 1.0, (n, ws)), rng.integers(-1000, 1001, (n, ws)).astype(np.int32))
    if mode == "ones":
        return np.ones((n, ws))
    if mode == "subnormal":                                 # fp64 subnormal inputs among tiny normal ones
        return np.ldexp(rng.uniform(0.5, 1.0, (n, ws)), rng.integers(-1074, -1000, (n, ws)).astype(np.int32))
    a = np.zeros((n, ws))                                   # one-hot; zero_block: the first block all zero
    w = 0
    for i, k in enumerate(cards):
        if not (mode == "zero_block" and i == 0):
            a[np.arange(n), w + rng.integers(0, k, n)] = np.ldexp(1.0, rng.integers(-40, 40, n).astype(np.int32))
        w += k
    return a


def _stage_lik(ctx, lik, cards, row0, R, dt):
    n_rows, ws = lik.shape
    t_lik = torch.from_numpy(np.ascontiguousarray(lik)).to(DEV)
    buf, out = _guarded(np.full(ws * R, -7.0, dtype=ND[dt]), -7.0)
    ebuf, e_row = _guarded(np.full(R, -7, dtype=np.int64), -7)
    st = _status()
    torch.cuda.synchronize()
    bnpp._check(L.bnpp_stage_likelihoods(ctx.handle, None, DT[dt], bnpp.F32 if lik.dtype == np.float32 else bnpp.F64,
                                         len(cards), _ints(cards), n_rows, row0, R, P(t_lik.data_ptr()),
                                         P(out.data_ptr()), P(e_row.data_ptr()), P(st.data_ptr())), "stage_lik")
    ctx.synchronize()
    got = _check_guards(buf, ws * R, -7.0, ("stage_lik", cards, R, dt)).reshape(ws, R)
    return got, _check_guards(ebuf, R, -7, ("stage_lik e_row", cards, R)), st.cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SOFT_CARDS))
@pytest.mark.parametrize("R", ROWS)
def test_stage_lik_bit_for_bit(ctx, grid_cap, R, name, dt):
    cards = SOFT_CARDS[name]
    n_rows, row0, _ = _window(R)
    rng = np.random.default_rng(R * 7 + len(cards))
    for mode in ("wide", "ones", "one_hot", "zero_block", "subnormal", "f32_input"):
        lik = _lik("wide" if mode == "f32_input" else mode, rng, n_rows, cards)
        if mode == "f32_input":
            with np.errstate(under="ignore"):
                lik = np.minimum(lik, 1e38).astype(np.float32)   # fp32 subnormals and zeros among them
        want, e_want, st = ref.stage_lik(lik, cards, row0, R, ND[dt])
        assert st == ref.NONE
        for cap in ((0, 1, 2, 3) if R == 257 and mode == "wide" else (0,)):
            grid_cap(cap)
            got, e_got, status = _stage_lik(ctx, lik, cards, row0, R, dt)
            assert _same_bits(got, want), (name, mode, R, dt, cap, np.argwhere(got != want)[:4])
            assert np.array_equal(e_got, e_want) and (status == ref.NONE).all(), (name, mode, R, dt, cap)


@pytest.mark.parametrize("R", [64, 65])
def test_stage_lik_fp32_subnormal_results_round_as_the_host_conversion(ctx, R):
    """Entries 2^-130 and 2^-160 below their block's top: the scaled value is below 2^-126, and the float stored
    must be the correctly rounded subnormal (float)v (2^-160 below: zero)."""
    cards = [4, 2]
    n_rows, row0, _ = _window(R)
    rng = np.random.default_rng(5)
    lik = np.empty((n_rows, 6))
    top = np.ldexp(rng.uniform(0.5, 1.0, n_rows), rng.integers(-50, 50, n_rows).astype(np.int32))
    lik[:, 0] = top
    lik[:, 1] = top * np.ldexp(rng.uniform(0.5, 1.0, n_rows), -130)
    lik[:, 2] = top * np.ldexp(rng.uniform(0.5, 1.0, n_rows), -160)
    tie = np.where(np.arange(n_rows) % 2 == 0, 1.5, 2.5)    # ties between two subnormals: to the even one, 2 * 2^-149
    lik[:, 3] = np.ldexp(tie, (-149 + np.frexp(top)[1]).astype(np.int32))
    lik[:, 4] = top
    lik[:, 5] = top * np.ldexp(rng.uniform(0.5, 1.0, n_rows), -140)
    want, e_want, _ = ref.stage_lik(lik, cards, row0, R, np.float32)
    assert (want[1] > 0).all() and (want[1] < np.ldexp(1.0, -126)).all() and (want[2] == 0).all(), "subnormal, and zero"
    assert (want[3].view(np.uint32) == 2).all()
    got, e_got, status = _stage_lik(ctx, lik, cards, row0, R, "f32")
    assert _same_bits(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(e_got, e_want) and (status == ref.NONE).all()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_stage_lik_names_the_first_invalid_cell(ctx, dt):
    cards, R = [300, 2], 65
    n_rows, row0, _ = _window(R)
    rng = np.random.default_rng(9)
    for x in (np.nan, np.inf, -np.inf, -1e-300):
        lik = _lik("ones", rng, n_rows, cards) * 0.75
        first = row0 + 40
        lik[first, 299] = x
        lik[first, 301] = lik[first + 1, 5] = x             # later invalid cells: not the first
        lik[2, 7] = x                                       # a row of an earlier launch
        want, e_want, st = ref.stage_lik(lik, cards, row0, R, ND[dt])
        assert st == first * 302 + 299
        got, e_got, status = _stage_lik(ctx, lik, cards, row0, R, dt)
        assert status[1] == st and status[0] == ref.NONE, (x, status)
        assert _same_bits(got, want) and np.array_equal(e_got, e_want), "an invalid entry counts as 0"


# ---- emit_row_scalars --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("R", ROWS)
def test_emit_row_scalars(ctx, grid_cap, R, dt):
    n_rows, row0, live = _window(R)
    rng = np.random.default_rng(R)
    lo, hi = (-1070, 1000) if dt == "f64" else (-148, 120)
    with np.errstate(under="ignore"):
        table = np.ldexp(rng.uniform(0.5, 1.0, R), rng.integers(lo, hi, R).astype(np.int32)).astype(ND[dt])
    table[:-1:5] = 0                                        # impossible rows: -inf, and z = 0
    e_row = rng.integers(-3000, 3000, R).astype(np.int64)
    for has_b, exp2, use_e, use_z in ((True, -37, True, True), (True, 0, False, True), (False, 2 ** 21, True, True),
                                      (True, -(2 ** 21), True, True), (True, 5, True, False), (None, 3, True, True)):
        tab = None if has_b is None else table if has_b else table[-1:]
        lz = np.full(n_rows, -7.0)
        z = np.full(n_rows, -7.0)
        ref.emit_row_scalars(lz, z if use_z else None, tab, bool(has_b), exp2, e_row if use_e else None, row0, live)
        t_tab = torch.from_numpy(np.ascontiguousarray(tab)).to(DEV) if tab is not None else None
        meta = torch.tensor([0, 0, exp2, R], dtype=torch.int64, device=DEV)
        t_e = torch.from_numpy(e_row).to(DEV)
        for cap in ((0, 1, 2, 3) if R == 257 and has_b and use_z and exp2 == -37 else (0,)):
            grid_cap(cap)
            b1, d_lz = _guarded(np.full(n_rows, -7.0), -9.0)
            b2, d_z = _guarded(np.full(n_rows, -7.0), -9.0)
            torch.cuda.synchronize()
            bnpp._check(L.bnpp_emit_row_scalars(ctx.handle, None, DT[dt], P(t_tab.data_ptr()) if tab is not None else None,
                                                1 if has_b else 0, P(meta.data_ptr()),
                                                P(t_e.data_ptr()) if use_e else None, row0, live, P(d_lz.data_ptr()),
                                                P(d_z.data_ptr()) if use_z else None), "emit_row_scalars")
            ctx.synchronize()
            g_lz = _check_guards(b1, n_rows, -9.0, "log10_z")
            g_z = _check_guards(b2, n_rows, -9.0, "z")
            assert np.array_equal(_bits(g_z), _bits(z)), ("z is bit-identical", R, dt, has_b, exp2)
            assert (g_lz[:row0] == -7.0).all() and (g_lz[row0 + live:] == -7.0).all(), "rows outside the launch"
            _ulp_ok(g_lz[row0:row0 + live], lz[row0:row0 + live], ("emit_row_scalars", R, dt, has_b, exp2))
    # no metadata: the scale is 0
    lz = np.full(n_rows, -7.0)
    ref.emit_row_scalars(lz, None, table, True, 0, None, row0, live)
    t_tab = torch.from_numpy(table).to(DEV)
    b1, d_lz = _guarded(np.full(n_rows, -7.0), -9.0)
    torch.cuda.synchronize()
    bnpp._check(L.bnpp_emit_row_scalars(ctx.handle, None, DT[dt], P(t_tab.data_ptr()), 1, None, None, row0, live,
                                        P(d_lz.data_ptr()), None), "emit_row_scalars")
    ctx.synchronize()
    _ulp_ok(_check_guards(b1, n_rows, -9.0, "log10_z")[row0:row0 + live], lz[row0:row0 + live], "no metadata")


# ---- emit_row_states ---------------------------------------------------------------------------------------------

def _states_case(rng, n_vars, K, R):
    """Evidence columns on every third variable (one of 300 values, one partial), unwritten variables among the rest."""
    ev_col = [-1] * n_vars
    cols = list(range(0, n_vars, 3))
    for j, v in enumerate(cols):
        ev_col[v] = j
    n_ev = len(cols)
    ev = np.stack([rng.integers(0, 300 if j == 0 else 4, R) for j in range(n_ev)]).astype(np.int32)
    partial = [j for j in range(n_ev) if j % 2 == 1] or [0]
    for j in partial:
        ev[j, rng.random(R) < 0.4] = -1
    written = [1 if (ev_col[v] < 0 and v % 5 != 1) or (ev_col[v] >= 0 and ev_col[v] in partial) else 0 for v in range(n_vars)]
    x = rng.integers(0, 256, (n_vars, K, R)).astype(np.uint8)
    return ev_col, written, ev, x


@pytest.mark.parametrize("n_vars", [1, 37, 140])
@pytest.mark.parametrize("R", ROWS)
def test_emit_row_states_mpe(ctx, grid_cap, R, n_vars):
    n_rows, row0, live = _window(R)
    ev_col, written, ev, x = _states_case(np.random.default_rng(R + n_vars), n_vars, 1, R)
    want = np.full((n_rows, n_vars), -7, dtype=np.int32)
    ref.emit_row_states(want, None, x, ev, ev_col, written, 1, R, row0, live, False)
    assert want.max() > 255 or n_vars == 1 or R == 1, "an evidence value above a byte"
    t_x, t_ev = torch.from_numpy(x).to(DEV), torch.from_numpy(ev).to(DEV)
    for cap in ((0, 1, 2, 3) if R == 257 else (0,)):
        grid_cap(cap)
        buf, out = _guarded(np.full(n_rows * n_vars, -7, dtype=np.int32), -9)
        torch.cuda.synchronize()
        bnpp._check(L.bnpp_emit_row_states(ctx.handle, None, 0, n_vars, _ints(ev_col), (C.c_ubyte * n_vars)(*written), 1, R,
                                           row0, live, P(t_x.data_ptr()), P(t_ev.data_ptr()), bnpp.F64, None, 0, None, 0,
                                           P(out.data_ptr()), None), "emit_row_states")
        ctx.synchronize()
        got = _check_guards(buf, n_rows * n_vars, -9, ("emit_row_states", R, n_vars)).reshape(n_rows, n_vars)
        assert np.array_equal(got, want), (R, n_vars, cap, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n_vars", [1, 37, 140])
@pytest.mark.parametrize("R", ROWS)
def test_emit_row_states_sampling(ctx, grid_cap, R, n_vars, K, dt):
    n_rows, row0, live = _window(R)
    rng = np.random.default_rng(R + n_vars + K)
    ev_col, written, ev, x = _states_case(rng, n_vars, K, R)
    ev = np.minimum(ev, 255)                                # a sample holds a byte per variable
    table = rng.uniform(0.1, 1.0, R).astype(ND[dt])
    table[::4] = 0                                          # impossible rows
    deg = rng.integers(0, 1000, R).astype(np.int64)
    n_drawn = sum(written)
    t_x, t_ev = torch.from_numpy(x).to(DEV), torch.from_numpy(ev).to(DEV)
    t_deg = torch.from_numpy(deg).to(DEV)
    for has_b in (True, False, None):                       # None: no result table, the constant 1
        tab = None if has_b is None else table if has_b else table[0:1]
        want = np.full((n_rows, K, n_vars), 0xF9, dtype=np.uint8)
        want_deg = np.full(n_rows, -7, dtype=np.int64)
        ref.emit_row_states(want, want_deg, x, ev, ev_col, written, K, R, row0, live, True, tab, bool(has_b), deg, n_drawn)
        t_tab = torch.from_numpy(np.ascontiguousarray(tab)).to(DEV) if tab is not None else None
        for cap in ((0, 1, 2, 3) if R == 257 and has_b else (0,)):
            grid_cap(cap)
            buf, out = _guarded(np.full(n_rows * K * n_vars, 0xF9, dtype=np.uint8), 0xF7)
            dbuf, d_deg = _guarded(np.full(n_rows, -7, dtype=np.int64), -9)
            torch.cuda.synchronize()
            bnpp._check(L.bnpp_emit_row_states(ctx.handle, None, 1, n_vars, _ints(ev_col), (C.c_ubyte * n_vars)(*written), K,
                                               R, row0, live, P(t_x.data_ptr()), P(t_ev.data_ptr()), DT[dt],
                                               P(t_tab.data_ptr()) if tab is not None else None, 1 if has_b else 0,
                                               P(t_deg.data_ptr()), n_drawn, P(out.data_ptr()), P(d_deg.data_ptr())),
                        "emit_row_states")
            ctx.synchronize()
            got = _check_guards(buf, n_rows * K * n_vars, 0xF7, ("emit_row_states", R, n_vars, K)).reshape(n_rows, K, n_vars)
            assert np.array_equal(got, want), (R, n_vars, K, has_b, cap, np.argwhere(got != want)[:4])
            assert np.array_equal(_check_guards(dbuf, n_rows, -9, "n_degenerate"), want_deg)


# ---- whole calls -------------------------------------------------------------------------------------------------

SOFT = {"alarm": [5, 12, 30], "ising6x6": [3, 14, 22, 30]}
VARIANTS = ("plain", "partial", "soft", "both", "soft_only")
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
        ws = sum(d["cards"][v] for v in SOFT[name])
        lik = np.ldexp(rng.uniform(0.5, 1.0, (n, ws)), rng.integers(-30, 30, (n, ws)).astype(np.int32))
        lik[rng.random((n, ws)) < 0.2] = 0
        lik[:, 0] = np.maximum(lik[:, 0], 0.25)             # every block keeps a non-zero entry ...
        w = 0
        for v in SOFT[name]:
            lik[:, w] = np.maximum(lik[:, w], 0.25)
            w += d["cards"][v]
        _CASES[name] = dict(m=m, d=d, ev=EV_VARS[name], rows=rows, holes=holes, soft=SOFT[name], lik=lik)
    return _CASES[name]


def _args(c, variant, n):
    """(ev_vars, rows, keyword arguments) of a variant for the host-array call; the rows the call's first n."""
    ev = [] if variant == "soft_only" else c["ev"]
    rows = c["holes"][:n] if variant in ("partial", "both") else c["rows"][:n]
    rows = rows[:, :len(ev)] if len(ev) else np.zeros((n, 0), dtype=np.int64)
    kw = {}
    if variant in ("partial", "both"):
        kw["partial"] = c["ev"]
    if variant in ("soft", "both", "soft_only"):
        kw["soft"] = (c["soft"], c["lik"][:n])
    return ev, rows, kw


def _dev(rows, kw, lik_dtype=torch.float64):
    t_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
    kd = dict(kw)
    if "soft" in kw:
        kd["soft"] = (kw["soft"][0], torch.from_numpy(np.ascontiguousarray(kw["soft"][1])).to(DEV).to(lik_dtype))
    return t_rows, kd


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["alarm", "ising6x6"])
@pytest.mark.parametrize("call", ["partition", "marginals", "mpe", "sample"])
def test_whole_calls_against_the_host_array_siblings(ctx, call, name, variant, R, dt):
    c = _case(ctx, name)
    m = c["m"]
    for n in (1, 65, 300):                                  # n < R; a padded last launch; several launches
        ev, rows, kw = _args(c, variant, n)
        t_rows, kd = _dev(rows, kw)
        common = dict(dtype=DT[dt], rows_per_launch=R)
        what = (call, name, variant, R, dt, n)
        if call == "partition":
            lz, z, _ = bnpp.partition_batch(ctx, m, ev, rows, **common, **kw)
            g_lz, g_z, _ = bt.partition_batch(ctx, m, ev, t_rows, **common, **kd)
            assert np.array_equal(_bits(g_z.cpu().numpy()), _bits(z)), what
        elif call == "marginals":
            out, lz = bnpp.marginals_batch(ctx, m, ev, rows, **common, **kw)
            g_out, g_lz = bt.marginals_batch(ctx, m, ev, t_rows, **common, **kd)
            assert np.array_equal(_bits(g_out.cpu().numpy()), _bits(out)), what
        elif call == "mpe":
            lz, x, _ = bnpp.mpe_batch(ctx, m, ev, rows, **common, **kw)
            g_lz, g_x, _ = bt.mpe_batch(ctx, m, ev, t_rows, **common, **kd)
            assert g_x.dtype == torch.int32 and np.array_equal(g_x.cpu().numpy(), x), what
        else:
            s, lz, deg = bnpp.sample_batch(ctx, m, ev, rows, 3, seed=5, **common, **kw)
            g_s, g_lz, g_deg = bt.sample_batch(ctx, m, ev, t_rows, 3, seed=5, **common, **kd)
            assert np.array_equal(g_s.cpu().numpy(), s) and np.array_equal(g_deg.cpu().numpy(), deg), what
        assert n < 300 or np.isfinite(lz).any()
        _ulp_ok(g_lz.cpu().numpy(), lz, what)


@pytest.mark.parametrize("call", ["partition", "marginals", "mpe", "sample"])
def test_fp32_likelihoods_are_widened_exactly(ctx, call):
    c = _case(ctx, "alarm")
    ev, rows, kw = _args(c, "soft", 65)
    lik32 = kw["soft"][1].astype(np.float32)
    kw["soft"] = (kw["soft"][0], lik32.astype(np.float64))
    t_rows, kd = _dev(rows, kw, torch.float32)
    assert kd["soft"][1].dtype == torch.float32
    fn = dict(partition=(bnpp.partition_batch, bt.partition_batch, 1), marginals=(bnpp.marginals_batch, bt.marginals_batch, 0),
              mpe=(bnpp.mpe_batch, bt.mpe_batch, 1), sample=(bnpp.sample_batch, bt.sample_batch, 0))[call]
    extra = (2,) if call == "sample" else ()
    want = fn[0](ctx, c["m"], ev, rows, *extra, rows_per_launch=64, **kw)
    got = fn[1](ctx, c["m"], ev, t_rows, *extra, rows_per_launch=64, **kd)
    assert np.array_equal(got[fn[2]].cpu().numpy(), want[fn[2]], equal_nan=True)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_an_impossible_row_leaves_its_neighbours_alone(ctx, dt):
    c = _case(ctx, "alarm")
    m, n = c["m"], 130
    ev = c["ev"]
    rows, lik = c["rows"][150:150 + n], c["lik"][150:150 + n].copy()   # rows drawn from joint samples: possible
    ok_rows = np.isfinite(bnpp.partition_batch(ctx, m, ev, rows, dtype=DT[dt], rows_per_launch=64, soft=(c["soft"], lik))[0])
    bad = next(i for i in range(65, n - 1) if ok_rows[i - 1:i + 2].all())   # in the second launch, between possible rows
    dead = lik.copy()
    dead[bad, :m.cards[c["soft"][0]]] = 0                   # an all-zero likelihood block
    common = dict(dtype=DT[dt], rows_per_launch=64)
    t_rows = torch.from_numpy(rows).to(DEV)
    res = {}
    for key, a in (("live", lik), ("dead", dead)):
        t_lik = torch.from_numpy(a).to(DEV)
        res[key] = dict(
            pr=bt.partition_batch(ctx, m, ev, t_rows, soft=(c["soft"], t_lik), **common),
            mar=bt.marginals_batch(ctx, m, ev, t_rows, soft=(c["soft"], t_lik), **common),
            mpe=bt.mpe_batch(ctx, m, ev, t_rows, soft=(c["soft"], t_lik), **common),
            smp=bt.sample_batch(ctx, m, ev, t_rows, 3, seed=5, soft=(c["soft"], t_lik), **common))
    host = dict(pr=bnpp.partition_batch(ctx, m, ev, rows, soft=(c["soft"], dead), **common),
                mar=bnpp.marginals_batch(ctx, m, ev, rows, soft=(c["soft"], dead), **common),
                mpe=bnpp.mpe_batch(ctx, m, ev, rows, soft=(c["soft"], dead), **common),
                smp=bnpp.sample_batch(ctx, m, ev, rows, 3, seed=5, soft=(c["soft"], dead), **common))
    d = {k: [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in v] for k, v in res["dead"].items()}
    lv = {k: [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in v] for k, v in res["live"].items()}
    # the sibling's -inf / 0 / NaN / zeros in the impossible row
    assert d["pr"][0][bad] == -np.inf == host["pr"][0][bad] and d["pr"][1][bad] == 0 == host["pr"][1][bad]
    assert np.array_equal(_bits(d["mar"][0]), _bits(host["mar"][0])) and np.isnan(d["mar"][0][bad]).any()
    assert d["mpe"][0][bad] == -np.inf and np.array_equal(d["mpe"][1], host["mpe"][1])
    assert np.array_equal(d["smp"][0], host["smp"][0]) and np.array_equal(d["smp"][2], host["smp"][2])
    assert d["smp"][1][bad] == -np.inf and d["smp"][2][bad] == host["smp"][2][bad] > 0
    free = [v for v in range(m.n_vars) if v not in ev]
    assert (d["smp"][0][bad][:, free] == 0).all()
    # every other row keeps its bits
    others = np.arange(n) != bad
    for k, idxs in (("pr", (0, 1)), ("mar", (0, 1)), ("mpe", (0, 1)), ("smp", (0, 1, 2))):
        for i in idxs:
            a, b = d[k][i][others], lv[k][i][others]
            assert np.array_equal(a, b, equal_nan=True), (k, i)


@pytest.mark.parametrize("call", ["partition", "marginals", "mpe", "sample"])
def test_bad_cells_raise_the_siblings_message(ctx, call):
    c = _case(ctx, "alarm")
    m = c["m"]
    fn = dict(partition=(bnpp.partition_batch, bt.partition_batch), marginals=(bnpp.marginals_batch, bt.marginals_batch),
              mpe=(bnpp.mpe_batch, bt.mpe_batch), sample=(bnpp.sample_batch, bt.sample_batch))[call]
    extra = (2,) if call == "sample" else ()
    ev, rows, kw = _args(c, "both", 130)
    lik = kw["soft"][1]

    def both(rows, lik):
        msgs = []
        for f, r, a in ((fn[0], rows, lik), (fn[1], torch.from_numpy(rows).to(DEV), torch.from_numpy(lik).to(DEV))):
            with pytest.raises(bnpp.BnppError) as e:
                f(ctx, m, ev, r, *extra, rows_per_launch=64, partial=c["ev"][:2], soft=(c["soft"], a))
            assert e.value.status == bnpp.ERR_INVALID
            msgs.append(str(e.value).replace("_dv", "_sv"))
        return msgs

    clean = np.where(rows < 0, 0, rows)
    clean[:, :2] = rows[:, :2]
    for (r, j, x) in ((77, 2, -1), (3, 0, -2), (129, 1, m.cards[ev[1]])):   # a -1 where not partial, a -2, the card
        bad = clean.copy()
        bad[r, j] = x
        bad[min(r + 1, 129), 2] = 99                        # a later bad cell
        blik = lik.copy()
        blik[0, 0] = np.nan                                 # a bad likelihood too: the evidence is named first
        host, dev = both(bad, blik)
        assert host == dev and "row %d" % r in dev and "variable %d " % ev[j] in dev, (host, dev)
    for x in (np.nan, np.inf, -1.0):
        blik = lik.copy()
        w = m.cards[c["soft"][0]]
        blik[100, w + 1] = x                                # row 100, value 1 of the second soft variable
        blik[101, 0] = x
        host, dev = both(clean, blik)
        assert host == dev and "row 100" in dev and "soft variable %d" % c["soft"][1] in dev, (host, dev)


def test_a_dv_call_and_its_sibling_share_the_job(ctx):
    c = _case(ctx, "alarm")
    ev, rows, kw = _args(c, "both", 65)
    t_rows, kd = _dev(rows, kw)
    bnpp.posterior_batch(ctx, c["m"], ev, c["rows"][:65], 1)   # another job takes the cache
    for host, dev in ((bnpp.partition_batch, bt.partition_batch), (bnpp.marginals_batch, bt.marginals_batch),
                      (bnpp.mpe_batch, bt.mpe_batch)):
        dev(ctx, c["m"], ev, t_rows, rows_per_launch=64, **kd)
        assert bnpp.last_timing()["plan_ms"] > 0, "the _dv call planned the job"
        host(ctx, c["m"], ev, rows, rows_per_launch=64, **kw)
        assert bnpp.last_timing()["plan_ms"] == 0, "the host-array call found it cached"
        dev(ctx, c["m"], ev, t_rows, rows_per_launch=64, **kd)
        assert bnpp.last_timing()["plan_ms"] == 0


def test_marginals_of_one_model_feed_another_without_leaving_the_device(ctx):
    a, b = _case(ctx, "alarm"), _case(ctx, "ising6x6")
    n = 130
    a_rows = a["rows"][150:150 + n]                         # drawn from joint samples: possible, so no NaN marginal
    t_rows = torch.from_numpy(a_rows).to(DEV)
    # alarm's binary variables that are no evidence feed as many of ising's (binary) variables
    ok = [t for t in range(a["m"].n_vars) if a["m"].cards[t] == 2 and t not in a["ev"]][:4]
    assert ok, "a binary alarm variable to feed the binary ising variables"
    soft_vars = [v for v in range(36) if v not in b["ev"]][:len(ok)]
    marg, _ = bt.marginals_batch(ctx, a["m"], a["ev"], t_rows, targets=ok)
    assert marg.is_cuda and marg.shape == (n, 2 * len(ok))
    rows_b = torch.from_numpy(b["rows"][:n]).to(DEV)
    lz, z, _ = bt.partition_batch(ctx, b["m"], b["ev"], rows_b, soft=(soft_vars, marg))
    post, lz2 = bt.marginals_batch(ctx, b["m"], b["ev"], rows_b, soft=(soft_vars, marg))
    # the same chain through numpy
    h_marg, _ = bnpp.marginals_batch(ctx, a["m"], a["ev"], a_rows, targets=ok)
    assert np.array_equal(_bits(marg.cpu().numpy()), _bits(h_marg)) and np.isfinite(h_marg).all()
    h_lz, h_z, _ = bnpp.partition_batch(ctx, b["m"], b["ev"], b["rows"][:n], soft=(soft_vars, h_marg))
    h_post, _ = bnpp.marginals_batch(ctx, b["m"], b["ev"], b["rows"][:n], soft=(soft_vars, h_marg))
    assert np.array_equal(_bits(z.cpu().numpy()), _bits(h_z)) and np.array_equal(_bits(post.cpu().numpy()), _bits(h_post))
    _ulp_ok(lz.cpu().numpy(), h_lz, "chained log10_z")


def test_tensor_arguments_must_be_on_the_device(ctx):
    c = _case(ctx, "alarm")
    ev, rows, kw = _args(c, "soft", 5)
    t_rows, kd = _dev(rows, kw)
    with pytest.raises(ValueError):
        bt.partition_batch(ctx, c["m"], ev, torch.from_numpy(rows))             # a CPU tensor
    with pytest.raises(ValueError):
        bt.partition_batch(ctx, c["m"], ev, rows)                               # no tensor at all
    with pytest.raises(ValueError):
        bt.partition_batch(ctx, c["m"], ev, t_rows, soft=(kw["soft"][0], torch.from_numpy(kw["soft"][1])))
    with pytest.raises(ValueError):
        bt.marginals_batch(ctx, c["m"], ev, t_rows, out=torch.empty((5, sum(c["d"]["cards"])), dtype=torch.float64))
    with pytest.raises(ValueError):
        bt.mpe_batch(ctx, c["m"], ev, t_rows.to(torch.float32))
    # partial="auto" is evaluated on the device
    ev, rows, kw = _args(c, "partial", 65)
    want = bnpp.partition_batch(ctx, c["m"], ev, rows, partial="auto")
    got = bt.partition_batch(ctx, c["m"], ev, torch.from_numpy(rows).to(DEV), partial="auto")
    assert np.array_equal(_bits(got[1].cpu().numpy()), _bits(want[1]))
    # out= is written in place
    out = torch.empty((65, sum(c["d"]["cards"])), dtype=torch.float64, device=DEV)
    res, _ = bt.marginals_batch(ctx, c["m"], ev, torch.from_numpy(rows).to(DEV), partial="auto", out=out)
    assert res.data_ptr() == out.data_ptr()
