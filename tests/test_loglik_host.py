"""Host tests of log-space soft evidence: the three symbols, the lik_dtype
values the _dv calls accept, the argument checks bnpp_log_partition_dv makes
before a device is needed (the _sv siblings' statuses and messages), and the
properties of the numpy restatements (tests/loglik_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import bnpp
import device_io_ref as dref
import loglik_ref as ref
import soft_ref
from bnpp import synth
from conftest import model_path

DV = ("partition_batch", "marginals_batch", "mpe_batch", "sample_batch")
NEW = ("bnpp_stage_loglikelihoods", "bnpp_emit_row_logs", "bnpp_log_partition_dv")
P = C.c_void_p
FAKE = 0x1000                           # a "device pointer": the host checks never read through it
LOG64, LOG32 = bnpp.F64 | 2, bnpp.F32 | 2


def _load(name):
    path = model_path(name + ".uai")
    return bnpp.Model.load(path), synth.read_uai(path)


def _ints(xs):
    return (C.c_int * max(len(xs), 1))(*xs)


def test_symbols_and_version():
    for name in NEW:
        assert name in bnpp.EXPORTED and hasattr(bnpp._lib, name)
    assert bnpp._lib.bnpp_version() == 205 == bnpp.ABI_VERSION, "symbols are added, the version stays"
    assert bnpp.LIK_LOG == 2 and (LOG64, LOG32) == (2, 3)
    import bnpp.tensor as bt
    assert callable(bt.log_partition)


def _dv(fn, m, ev_vars, n_rows, soft_vars, lik_dtype):
    """A _dv entry with a NULL context and pointers that are never read."""
    L = bnpp._lib
    head = (None, m.handle, len(ev_vars), _ints(ev_vars), n_rows, P(FAKE), None, len(soft_vars), _ints(soft_vars), P(FAKE),
            lik_dtype, bnpp.MIN_FILL, None, 0)
    o = P(FAKE)
    if fn == "partition_batch":
        rc = L.bnpp_partition_batch_dv(*head, bnpp.F64, 0, o, None, None)
    elif fn == "marginals_batch":
        rc = L.bnpp_marginals_batch_dv(*head, 0, None, bnpp.F64, 0, o, None, None)
    elif fn == "mpe_batch":
        rc = L.bnpp_mpe_batch_dv(*head, bnpp.F64, 0, o, None, None)
    else:
        rc = L.bnpp_sample_batch_dv(*head, bnpp.F64, 0, 1, 0, 1, 7, o, None, None, None)
    return rc, L.bnpp_last_error().decode()


@pytest.mark.parametrize("fn", DV)
def test_the_dv_calls_accept_the_log_lik_dtypes(fn):
    m, _ = _load("asia")
    want = _dv(fn, m, [0, 3], 3, [2, 5], bnpp.F64)
    assert (want[0] == bnpp.ERR_INVALID and "context" in want[1]) or want[0] == bnpp.ERR_NO_DEVICE
    for lik_dtype in (LOG64, LOG32):
        assert _dv(fn, m, [0, 3], 3, [2, 5], lik_dtype) == want, "past the argument checks, and no further"
    for lik_dtype in (4, 5, -1):
        rc, msg = _dv(fn, m, [0, 3], 3, [2, 5], lik_dtype)
        assert rc == bnpp.ERR_INVALID and msg == "bad lik_dtype", (lik_dtype, msg)


def test_the_linear_staging_entry_keeps_its_lik_dtypes():
    L = bnpp._lib
    f, cards = P(FAKE), _ints([2, 3])
    assert L.bnpp_stage_likelihoods(None, None, 0, 3, 2, cards, 4, 0, 4, f, f, f, f) == bnpp.ERR_INVALID
    assert "dtype" in L.bnpp_last_error().decode()
    assert L.bnpp_stage_likelihoods(None, None, 0, 2, 2, cards, 4, 0, 4, f, f, f, f) == bnpp.ERR_INVALID
    assert "dtype" in L.bnpp_last_error().decode()


def test_single_step_argument_checks_without_a_device():
    L = bnpp._lib
    f, cards = P(FAKE), _ints([2, 3])
    err = lambda: L.bnpp_last_error().decode()
    st = lambda *a: L.bnpp_stage_loglikelihoods(None, None, *a)
    assert st(0, 2, 2, cards, 4, 0, 4, f, f, f, None, f) == bnpp.ERR_INVALID and "null" in err()      # no top
    assert st(0, 2, 2, cards, 4, 0, 4, f, f, f, f, None) == bnpp.ERR_INVALID and "null" in err()      # no status
    for lik_dtype in (0, 1, 4, -1):
        assert st(0, lik_dtype, 2, cards, 4, 0, 4, f, f, f, f, f) == bnpp.ERR_INVALID and "lik_dtype" in err()
    assert st(3, 2, 2, cards, 4, 0, 4, f, f, f, f, f) == bnpp.ERR_INVALID and "dtype" in err()
    assert st(0, 2, 2, cards, 0, 0, 4, f, f, f, f, f) == bnpp.ERR_INVALID and "n_rows" in err()
    assert st(0, 2, 2, cards, 4, 4, 4, f, f, f, f, f) == bnpp.ERR_INVALID and "row0" in err()
    assert st(0, 2, 2, _ints([2, 0]), 4, 0, 4, f, f, f, f, f) == bnpp.ERR_INVALID and "card" in err()
    assert st(0, 2, 321, _ints([2] * 321), 4, 0, 4, f, f, f, f, f) == bnpp.ERR_UNSUPPORTED
    for lik_dtype in (2, 3):
        assert st(1, lik_dtype, 2, cards, 4, 0, 4, f, f, f, f, f) == bnpp.ERR_INVALID and "context" in err()
    em = lambda *a: L.bnpp_emit_row_logs(None, None, *a)
    assert em(0, f, 1, None, None, 0, None, 4, 0, 4, None, None, None) == bnpp.ERR_INVALID and "output" in err()
    assert em(5, f, 1, None, None, 0, None, 4, 0, 4, f, None, None) == bnpp.ERR_INVALID and "dtype" in err()
    assert em(0, f, 1, None, None, 2, None, 4, 0, 4, f, None, None) == bnpp.ERR_INVALID and "null" in err()
    assert em(0, f, 1, None, None, 2, f, 0, 0, 0, f, None, None) == bnpp.ERR_INVALID and "R must" in err()
    assert em(0, f, 1, None, None, 2, f, 4, 0, 5, f, None, None) == bnpp.ERR_INVALID and "rows_live" in err()
    for outs in ((f, None, None), (None, f, None), (None, None, f)):
        assert em(0, f, 1, None, None, 2, f, 4, 0, 4, *outs) == bnpp.ERR_INVALID and "context" in err()


def _lp(m, ev_vars, n_rows, soft_vars, lik_dtype=LOG64, ln_z=FAKE, post=None, lik=FAKE, ev=FAKE, dtype=bnpp.F64, order=None,
        rpl=0):
    L = bnpp._lib
    h, oa, no = (bnpp.MIN_FILL, None, 0) if order is None else (bnpp.ORDER_GIVEN, _ints(order), len(order))
    rc = L.bnpp_log_partition_dv(None, m.handle if m is not None else None, len(ev_vars), _ints(ev_vars), n_rows, P(ev), None,
                                 len(soft_vars), _ints(soft_vars), P(lik), lik_dtype, h, oa, no, dtype, rpl,
                                 P(ln_z) if ln_z else None, P(post) if post else None, None)
    return rc, L.bnpp_last_error().decode()


def _sv(fn, m, ev_vars, n_rows, soft_vars, dtype=bnpp.F64, order=None, rpl=0, null_out=False):
    """The _sv sibling (partition_batch or marginals_batch on targets = soft_vars) with a NULL context."""
    L = bnpp._lib
    IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
    rows = np.zeros((max(n_rows, 1), max(len(ev_vars), 1)), dtype=np.intc)
    lik = np.full((max(n_rows, 1), 64), 0.25)
    h, oa, no = (bnpp.MIN_FILL, None, 0) if order is None else (bnpp.ORDER_GIVEN, _ints(order), len(order))
    head = (None, m.handle if m is not None else None, len(ev_vars), _ints(ev_vars), n_rows, rows.ctypes.data_as(IP), None,
            len(soft_vars), _ints(soft_vars), lik.ctypes.data_as(DP), h, oa, no)
    buf = np.zeros(4096)
    o = None if null_out else buf.ctypes.data_as(DP)
    if fn == "partition_batch":
        rc = L.bnpp_partition_batch_sv(*head, dtype, rpl, o, None, None)
    else:
        rc = L.bnpp_marginals_batch_sv(*head, len(soft_vars), _ints(soft_vars), dtype, rpl, o, None, None)
    return rc, L.bnpp_last_error().decode()


@pytest.mark.parametrize("with_post", [False, True])
def test_log_partition_argument_checks_are_the_siblings(with_post):
    m, _ = _load("asia")
    ev, soft = [0, 3], [2, 5]
    post = FAKE if with_post else None
    fn = "marginals_batch" if with_post else "partition_batch"
    for lik_dtype in (bnpp.F64, bnpp.F32, 4, 5, -1):        # a linear dtype, and what no call takes
        rc, msg = _lp(m, ev, 3, soft, lik_dtype=lik_dtype, post=post)
        assert rc == bnpp.ERR_INVALID and "lik_dtype" in msg, (lik_dtype, msg)
    rc, msg = _lp(m, ev, 3, soft, ln_z=None, post=post)
    assert rc == bnpp.ERR_INVALID and msg == "null output"
    assert _lp(m, ev, 0, soft, post=post) == _sv(fn, m, ev, 0, soft) == (bnpp.ERR_INVALID, "n_rows must be at least 1")
    assert _lp(None, ev, 3, soft, post=post) == _sv(fn, None, ev, 3, soft)
    cases = [dict(soft_vars=[2, 3]),                        # a soft variable that is also evidence
             dict(soft_vars=[2, 2]), dict(soft_vars=[2, 8]), dict(soft_vars=[-1]), dict(ev_vars=[0, 0]), dict(ev_vars=[0, 99]),
             dict(dtype=7), dict(rpl=-1), dict(order=[1, 1]), dict(order=[99])]
    for kw in cases:
        a = dict(ev_vars=ev, soft_vars=soft)
        a.update(kw)
        ev_vars, soft_vars = a.pop("ev_vars"), a.pop("soft_vars")
        got = _lp(m, ev_vars, 3, soft_vars, post=post, **a)
        # a bad soft variable is named as one (partition_batch's message), also where it would become a target
        want = _sv("partition_batch" if "soft_vars" in kw else fn, m, ev_vars, 3, soft_vars, **a)
        if want[0] == bnpp.ERR_NO_DEVICE or "context" in want[1]:
            assert got[0] == want[0] and ("context" in got[1] or got[0] == bnpp.ERR_NO_DEVICE), (kw, got, want)
            assert set(kw) <= {"dtype", "rpl", "order"}, kw  # only a device can tell (the plan)
        else:
            assert got == want and got[0] != bnpp.OK, (kw, got, want)
    rc, msg = _lp(m, ev, 3, soft, ev=None, post=post)
    assert rc == bnpp.ERR_INVALID and msg == "bad evidence arrays"
    rc, msg = _lp(m, ev, 3, soft, lik=None, post=post)
    assert rc == bnpp.ERR_INVALID and msg == "bad soft evidence arrays"
    # a valid call, n_soft == 0 included, gets as far as the missing context (or the missing device)
    for e_, s_ in ((ev, soft), ([], soft), (ev, [])):
        for lik_dtype in (LOG64, LOG32):
            rc, msg = _lp(m, e_, 3, s_, lik_dtype=lik_dtype, post=post)
            assert (rc == bnpp.ERR_INVALID and "context" in msg) or rc == bnpp.ERR_NO_DEVICE, (e_, s_, rc, msg)


# ---- the restatements --------------------------------------------------------------------------------------------

CARDS, loglik_case = ref.CARDS, ref.loglik_case


@pytest.mark.parametrize("out_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("in_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", sorted(CARDS))
def test_stage_loglik_restatement_is_stage_lik_of_E(name, in_dtype, out_dtype):
    cards = CARDS[name]
    n, R, row0 = 27, 16, 16                                 # the second launch: 11 live rows, 5 padding
    ll = loglik_case(np.random.default_rng(len(cards)), n, cards, in_dtype)
    out, e_row, top, status = ref.stage_loglik(ll, cards, row0, R, out_dtype)
    out2, e2, top2, st2 = ref.stage_loglik_via_linear(ll, cards, row0, R, out_dtype)
    assert out.dtype == out_dtype and np.array_equal(out.view(np.uint8), out2.view(np.uint8)), "bit for bit"
    assert np.array_equal(e_row, e2) and np.array_equal(top, top2) and status == st2 == dref.NONE
    rows = dref.launch_rows(n, row0, R)
    v = ll[rows].astype(np.float64)
    w, finite = 0, np.zeros(R, dtype=np.int64)
    for i, k in enumerate(cards):
        blk_top = v[:, w:w + k].max(axis=1)
        assert np.array_equal(top[i], blk_top)
        live = blk_top > -np.inf
        finite += live
        assert (out[w:w + k][:, ~live] == 0).all(), "an all -inf block gives zeros"
        assert (out[w:w + k][:, live].max(axis=0) == 0.5).all(), "the top of every other block is 0.5 = 1.0 * 2^-1"
        w += k
    assert np.array_equal(e_row, finite) and (~(finite == len(cards))).any(), "e_row counts the finite blocks"
    assert np.array_equal(out[:, 10], out[:, 15]) and e_row[10] == e_row[15], "padding rows copy the last row"
    if out_dtype == np.float64 and in_dtype == np.float64 and len(cards) > 1:
        assert ((out > 0) & (out < np.ldexp(1.0, -1022))).any(), "fp64 subnormal results are among the cases"
        assert ((out == 0) & np.isfinite(v.T)).any(), "and entries that underflow to zero"
    if out_dtype == np.float32 and len(cards) > 1:
        assert ((out > 0) & (out < np.ldexp(1.0, -126))).any(), "float subnormal results are among the cases"


def test_stage_loglik_restatement_names_the_first_invalid_cell():
    cards = [2, 3]
    ll = np.log(np.full((5, 5), 0.5))
    for x in (np.nan, np.inf):
        bad = ll.copy()
        bad[3, 4] = bad[4, 1] = x
        bad[3, 0] = -np.inf                                 # -inf is valid
        out, e_row, top, status = ref.stage_loglik(bad, cards, 0, 5, np.float64)
        assert status == 3 * 5 + 4 and out[4, 3] == 0 and out[1, 4] == 0 and np.isfinite(out).all()
        assert out[0, 3] == 0 and np.isfinite(top).all() and (e_row == 2).all()
        assert ref.stage_loglik(bad, cards, 4, 4, np.float64)[3] == 4 * 5 + 1, "a launch names the cells of its own rows"
        only = ll.copy()
        only[2, :2] = [x, -np.inf]                          # an invalid entry counts as -inf: the block is dead
        out, e_row, top, status = ref.stage_loglik(only, cards, 0, 5, np.float64)
        assert status == 2 * 5 and top[0, 2] == -np.inf and e_row[2] == 1 and (out[:2, 2] == 0).all()


def test_emit_row_logs_restatement():
    table = np.array([0.75, 0.0, 0.5, 0.625])
    e_row = np.array([2, 2, 1, 2], dtype=np.int64)
    top = np.array([[1.5, -2.0, -np.inf, -2500.0], [0.25, 3.0, 1.0, -2500.0]])
    ln_z, lz, z = np.full(6, -7.0), np.full(6, -7.0), np.full(6, -7.0)
    ref.emit_row_logs(ln_z, lz, z, table, True, -3, e_row, top, 2, 4)
    assert (ln_z[:2] == -7.0).all() and (lz[:2] == -7.0).all(), "rows before row0 are untouched"
    want0 = np.log(0.75 * 2.0 ** (-3 + 2)) + 1.75
    assert abs(ln_z[2] - want0) < 1e-15 and abs(lz[2] - want0 / np.log(10)) < 1e-15 and abs(z[2] - np.exp(want0)) < 1e-15
    assert ln_z[3] == -np.inf == lz[3] and z[3] == 0, "p = 0: an impossible row"
    assert abs(ln_z[5] - (np.log(0.625 * 0.5) - 5000.0)) < 1e-12 and z[5] == 0, "a shift of -5000: z underflows"
    assert np.array_equal(ref.shift_of(top), [1.75, 1.0, -np.inf, -5000.0])


def test_brute_log_stays_finite_where_the_linear_route_overflows():
    m, d = _load("cancer")
    ev, soft = [0], [1, 3]
    cards = [d["cards"][v] for v in soft]
    rng = np.random.default_rng(3)
    n = 6
    rows = rng.integers(0, d["cards"][0], (n, 1))
    small = rng.uniform(-2.0, 0.0, (n, sum(cards)))
    ll = small.copy()
    ll[:, :cards[0]] += 800.0                               # tops of +800 and -800
    ll[:, cards[0]:] -= 800.0
    ln_z, post = ref.brute_log(d, ev, rows, soft, ll)
    assert np.isfinite(ln_z).all() and np.isfinite(post).all()
    # the shifts cancel here, so ln Z is that of the small scores, and the posteriors do not see a shift at all.
    # Adding 800 rounds a score to a multiple of 2^-43 (1.2e-13), which is what the two sides may differ by
    z0, marg0, _ = soft_ref.brute(d, ev, rows, soft, np.exp(small))
    assert np.allclose(ln_z, np.log(z0), rtol=0, atol=1e-12)
    assert np.allclose(post, np.concatenate([marg0[v] for v in soft], axis=1), rtol=0, atol=1e-12)
    assert np.allclose(post[:, :cards[0]].sum(axis=1), 1.0) and np.allclose(post[:, cards[0]:].sum(axis=1), 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        z_naive, _, _ = soft_ref.brute(d, ev, rows, soft, np.exp(ll))
        assert not np.isfinite(np.log(z_naive)).any() or (z_naive == 0).all(), "exp(800) overflows, exp(-800) is 0"
    # an impossible row: -inf and NaN, its neighbours untouched
    dead = ll.copy()
    dead[2, :cards[0]] = -np.inf
    ln_d, post_d = ref.brute_log(d, ev, rows, soft, dead)
    assert ln_d[2] == -np.inf and np.isnan(post_d[2]).all()
    keep = np.arange(n) != 2
    assert np.array_equal(ln_d[keep], ln_z[keep]) and np.array_equal(post_d[keep], post[keep])
