"""Host tests of the device-resident model tables: the new symbols, the
argument checks made before a device is needed, and the numpy restatements
(tests/tables_ref.py) against the rule the engine uploads a model by and
against learn.m_step.

A table set cannot exist without a device, so the checks that need one (tables
of another model or dtype) are in tests/test_gpu_tables.py."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import bnpp
import tables_ref as ref
from bnpp import learn, synth
from conftest import model_path
from device_io_ref import NONE

NEW = ("bnpp_tables_create", "bnpp_tables_free", "bnpp_tables_set_dv", "bnpp_stage_tables", "bnpp_expected_counts_dv",
       "bnpp_mstep_dv", "bnpp_model_values")
P = C.c_void_p
FAKE = 0x1000                           # a "device pointer": the host checks never read through it
L = bnpp._lib


def _err():
    return L.bnpp_last_error().decode()


def _ints(xs):
    return (C.c_int * max(len(xs), 1))(*xs)


def _load(name):
    path = model_path(name + ".uai")
    return bnpp.Model.load(path), synth.read_uai(path)


def _no_device(rc):
    return (rc == bnpp.ERR_INVALID and "context" in _err()) or rc == bnpp.ERR_NO_DEVICE


def test_symbols_and_version():
    for name in NEW:
        assert name in bnpp.EXPORTED and hasattr(L, name)
    assert L.bnpp_version() == 205 == bnpp.ABI_VERSION, "symbols are added, the version stays"
    import bnpp.tensor as bt
    for name in ("Tables", "expected_counts", "m_step", "em", "log_likelihood"):
        assert callable(getattr(bt, name))


def test_model_values_are_the_flat_tables():
    m, d = _load("asia")
    n = C.c_int64()
    assert L.bnpp_counts_size(m.handle, C.byref(n)) == bnpp.OK
    out = (C.c_double * n.value)()
    assert L.bnpp_model_values(m.handle, out) == bnpp.OK
    assert np.array_equal(np.asarray(out[:]), ref.flat_values(d))
    assert L.bnpp_model_values(m.handle, None) == bnpp.ERR_INVALID and L.bnpp_model_values(None, out) == bnpp.ERR_INVALID


def test_tables_argument_checks_without_a_device():
    m, _ = _load("asia")
    h = P()
    assert L.bnpp_tables_create(None, m.handle, bnpp.F64, None) == bnpp.ERR_INVALID and "null" in _err()
    assert L.bnpp_tables_create(None, None, bnpp.F64, C.byref(h)) == bnpp.ERR_INVALID and "model" in _err()
    assert L.bnpp_tables_create(None, m.handle, 2, C.byref(h)) == bnpp.ERR_INVALID and "dtype" in _err()
    assert _no_device(L.bnpp_tables_create(None, m.handle, bnpp.F32, C.byref(h))) and not h.value
    assert L.bnpp_tables_set_dv(None, P(FAKE), 0) == bnpp.ERR_INVALID and "tables" in _err()
    assert L.bnpp_tables_free(None) == bnpp.OK


def test_stage_tables_argument_checks_without_a_device():
    f = P(FAKE)
    sizes = (C.c_int64 * 2)(3, 4)
    st = lambda *a: L.bnpp_stage_tables(None, None, *a)
    assert st(0, 0, 2, sizes, f, f, f, None, f) == bnpp.ERR_INVALID and "null" in _err()       # no shift
    assert st(0, 0, 2, sizes, f, f, f, f, None) == bnpp.ERR_INVALID and "null" in _err()       # no status
    assert st(0, 0, 2, sizes, f, f, None, f, f) == bnpp.ERR_INVALID and "null" in _err()       # no metadata
    assert st(0, 0, 2, None, f, f, f, f, f) == bnpp.ERR_INVALID and "null" in _err()
    for dtype in (2, -1):
        assert st(dtype, 0, 2, sizes, f, f, f, f, f) == bnpp.ERR_INVALID and "dtype" in _err()
    for values_dtype in (4, -1):
        assert st(0, values_dtype, 2, sizes, f, f, f, f, f) == bnpp.ERR_INVALID and "values_dtype" in _err()
    assert st(0, 0, 2, (C.c_int64 * 2)(3, 0), f, f, f, f, f) == bnpp.ERR_INVALID and "size" in _err()
    assert st(0, 0, 97, (C.c_int64 * 97)(*([2] * 97)), f, f, f, f, f) == bnpp.ERR_UNSUPPORTED
    for values_dtype in (0, 1, 2, 3):
        assert _no_device(st(1, values_dtype, 2, sizes, f, f, f, f, f))


def _counts_dv(m, ev_vars, n_rows, counts=FAKE, log10_z=FAKE, dtype=bnpp.F64, flags=0, lik_dtype=0, soft=()):
    rc = L.bnpp_expected_counts_dv(None, m.handle if m is not None else None, None, len(ev_vars), _ints(ev_vars), n_rows,
                                   P(FAKE), None, len(soft), _ints(list(soft)), P(FAKE) if soft else None, lik_dtype, None,
                                   flags, bnpp.MIN_FILL, None, 0, dtype, 0, P(counts) if counts else None,
                                   P(log10_z) if log10_z else None, None, None, None)
    return rc, _err()


def test_expected_counts_dv_argument_checks_without_a_device():
    m, _ = _load("asia")
    ev = [0, 3]
    assert _counts_dv(None, ev, 3)[0] == bnpp.ERR_INVALID
    assert _counts_dv(m, ev, 0) == (bnpp.ERR_INVALID, "n_rows must be at least 1")
    assert _counts_dv(m, ev, 3, flags=2) == (bnpp.ERR_INVALID, "bad flags")
    assert _counts_dv(m, ev, 3, counts=None, log10_z=None) == (bnpp.ERR_INVALID, "null output")
    assert _counts_dv(m, ev, 3, dtype=7) == (bnpp.ERR_INVALID, "bad dtype")
    assert _counts_dv(m, [0, 0], 3)[0] == bnpp.ERR_INVALID and _counts_dv(m, [0, 99], 3)[0] == bnpp.ERR_INVALID
    assert _counts_dv(m, ev, 3, soft=[2, 5], lik_dtype=4) == (bnpp.ERR_INVALID, "bad lik_dtype")
    for kw in (dict(), dict(counts=None), dict(flags=1), dict(soft=[2, 5], lik_dtype=3), dict(log10_z=None)):
        rc, msg = _counts_dv(m, ev, 3, **kw)
        assert (rc == bnpp.ERR_INVALID and "context" in msg) or rc == bnpp.ERR_NO_DEVICE, (kw, rc, msg)


def test_mstep_dv_argument_checks_without_a_device():
    bayes, _ = _load("asia")
    markov, _ = _load("ising4x4")
    f = P(FAKE)
    ms = lambda m, prior=0.0, c=f, o=f, n=f: L.bnpp_mstep_dv(None, None, m.handle if m else None, c, C.c_double(prior), o, n)
    assert ms(None) == bnpp.ERR_INVALID and "model" in _err()
    for kw in (dict(c=None), dict(o=None), dict(n=None)):
        assert ms(bayes, **kw) == bnpp.ERR_INVALID and "null" in _err()
    for prior in (-0.5, float("nan"), float("inf")):
        assert ms(bayes, prior) == bnpp.ERR_INVALID and "prior" in _err()
    assert ms(markov) == bnpp.ERR_UNSUPPORTED and "BAYES" in _err()
    assert _no_device(ms(bayes)) and _no_device(ms(bayes, 0.5))


# ---- the restatements --------------------------------------------------------------------------------------------

def _upload_rule(values, sizes, f32):
    """runtime.cpp upload_sources, entry by entry: mx, frexp's exponent, ldexp, one conversion, the largest stored."""
    out, at = [], 0
    for s in sizes:
        vals = [float(x) for x in values[at:at + s]]
        mx = 0.0
        for v in vals:
            mx = v if v > mx else mx
        e = math.frexp(mx)[1] if mx > 0 else 0
        stored, smax = [], 0.0
        for v in vals:
            x = math.ldexp(v, -e)
            if f32:
                x = struct.unpack("f", struct.pack("f", x))[0]
            stored.append(x)
            smax = x if x > smax else smax
        bits = struct.unpack("I", struct.pack("f", smax))[0] if f32 else struct.unpack("Q", struct.pack("d", smax))[0]
        out.append((stored, bits, e))
        at += s
    return out


@pytest.mark.parametrize("out_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("in_dtype", [np.float64, np.float32])
def test_linear_restatement_is_the_upload_rule(in_dtype, out_dtype):
    values = ref.linear_case(np.random.default_rng(5), in_dtype)
    tables, maxbits, exp2, tops, shift, status = ref.stage_tables(values, ref.SIZES, out_dtype)
    assert status == NONE and shift == 0.0
    for (stored, bits, e), t, mb, e2 in zip(_upload_rule(values, ref.SIZES, out_dtype == np.float32), tables, maxbits, exp2):
        assert t.dtype == out_dtype and np.array_equal(np.asarray(stored, dtype=out_dtype).view(np.uint8), t.view(np.uint8))
        assert (bits, e) == (mb, e2)
    live = [t for t in tables[:-1]]
    assert all(0.5 <= float(t.max()) < 1.0 for t in live), "the largest entry lies in [0.5, 1)"
    assert (tables[-1] == 0).all() and exp2[-1] == 0 and maxbits[-1] == 0, "an all-zero factor"
    assert exp2[1] < -1000 if in_dtype == np.float64 else exp2[1] < -130, "a subnormal maximum"
    assert exp2[3] > 990 if in_dtype == np.float64 else exp2[3] > 120


def test_linear_restatement_names_the_first_invalid_entry():
    for x in (np.nan, -1.0, np.inf):
        values = ref.linear_case(np.random.default_rng(6), np.float64)
        values[1 + 63 + 10] = x                             # factor 2, entry 10
        values[1 + 63 + 64 + 3] = x
        tables, _, exp2, _, _, status = ref.stage_tables(values, ref.SIZES, np.float64)
        assert status == 1 + 63 + 10 and tables[2][10] == 0 and all(np.isfinite(t).all() for t in tables)


@pytest.mark.parametrize("out_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("in_dtype", [np.float64, np.float32])
def test_log_restatement(in_dtype, out_dtype):
    values = ref.log_case(np.random.default_rng(7), in_dtype)
    tables, maxbits, exp2, tops, shift, status = ref.stage_tables(values, ref.SIZES, out_dtype, log=True)
    assert status == NONE
    half = ref._bits(0.5, out_dtype)
    want_shift, at = 0.0, 0
    for s, t, mb, e, top in zip(ref.SIZES, tables, maxbits, exp2, tops):
        v = values[at:at + s].astype(np.float64)
        assert top == v.max()
        if top == -np.inf:
            assert (t == 0).all() and e == 0 and mb == 0
        else:
            assert float(t.max()) == 0.5 and e == 1 and mb == half
            want_shift = want_shift + top
            # the contract: the linear form of E = exp(l - top) is the same table with exp2 = 1
            with np.errstate(under="ignore"):
                lin = ref.stage_tables(np.exp(v - top), [s], out_dtype)
            assert np.array_equal(lin[0][0].view(np.uint8), t.view(np.uint8)) and lin[2] == [1]
        at += s
    assert shift == want_shift and tops[-1] == -np.inf
    for x in (np.nan, np.inf):
        bad = values.copy()
        bad[1 + 63 + 64 + 65 + 4] = x                       # factor 4, entry 4
        assert ref.stage_tables(bad, ref.SIZES, out_dtype, log=True)[5] == 1 + 63 + 64 + 65 + 4


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("prior", [0.0, 0.5])
def test_mstep_restatement_against_learn_m_step(prior):
    """Two summation orders of k non-negative terms differ by at most 2 (k - 1) ulp of the sum, and each side
    rounds its quotient once: 2 k ulp."""
    _, d = _load("asia")
    d = ref.child_last(d)
    sizes, ks = [len(v) for v in d["values"]], ref.child_cards(d)
    rng = np.random.default_rng(11)
    counts = rng.uniform(0.0, 40.0, sum(sizes))
    k0 = ks[-1]
    counts[sum(sizes) - k0:] = 0.0                          # an unseen parent configuration
    old = ref.flat_values(d)
    new = ref.mstep(counts, old, sizes, ks, prior)
    want = ref.flat_values(learn.m_step(d, counts, prior))
    at = 0
    for s, k in zip(sizes, ks):
        assert (_ulps(new[at:at + s], want[at:at + s]) <= 2 * k).all()
        assert np.allclose(new[at:at + s].reshape(-1, k).sum(axis=1), 1.0, atol=1e-15 * 4 * k)
        at += s
    if prior == 0:
        assert np.array_equal(new[-k0:], old[-k0:]), "a configuration whose total is 0 keeps its old row"
    else:
        assert np.array_equal(new[-k0:], np.full(k0, 1.0 / k0))
    # a child of many values, a root, a child of one value: the sum's order shows and stays inside the bound
    m = {"type": "BAYES", "cards": [7, 1, 3], "scopes": [[2], [2, 0], [0, 1]], "values": [[0.2, 0.3, 0.5], [1 / 7] * 21, [1.0] * 7]}
    sizes, ks = [3, 21, 7], ref.child_cards(m)
    assert ks == [3, 7, 1]
    counts = rng.uniform(0.0, 1.0, 31) * 10.0 ** rng.integers(-6, 6, 31)
    new = ref.mstep(counts, ref.flat_values(m), sizes, ks, prior)
    want = ref.flat_values(learn.m_step(m, counts, prior))
    assert (_ulps(new[:3], want[:3]) <= 6).all() and (_ulps(new[3:24], want[3:24]) <= 14).all()
    assert np.array_equal(new[24:], np.ones(7))
