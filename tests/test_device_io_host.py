"""Host tests of the device-resident batched calls: the eight symbols, the
argument checks the _dv calls make before a device is needed (the _sv siblings'
statuses and messages), and the properties of the numpy restatements of the
staging steps (tests/device_io_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import bnpp
import device_io_ref as ref
from bnpp import synth
from conftest import model_path

DV = ("partition_batch", "marginals_batch", "mpe_batch", "sample_batch")
STEPS = ("bnpp_stage_evidence_rows", "bnpp_stage_likelihoods", "bnpp_emit_row_scalars", "bnpp_emit_row_states")
P = C.c_void_p
FAKE = 0x1000                           # a "device pointer": the host checks never read through it


def _load(name):
    path = model_path(name + ".uai")
    return bnpp.Model.load(path), synth.read_uai(path)


def test_symbols_and_version():
    for name in DV:
        assert "bnpp_%s_dv" % name in bnpp.EXPORTED and hasattr(bnpp._lib, "bnpp_%s_dv" % name)
    for name in STEPS:
        assert name in bnpp.EXPORTED and hasattr(bnpp._lib, name)
    assert bnpp._lib.bnpp_version() == 205 == bnpp.ABI_VERSION, "symbols are added, the version stays"
    import bnpp.tensor as bt
    for name in DV:
        assert callable(getattr(bt, name))


def _ints(xs):
    return (C.c_int * max(len(xs), 1))(*xs)


def _dv(fn, m, ev_vars, n_rows, soft_vars=(), partial=None, dtype=bnpp.F64, lik_dtype=bnpp.F64, ev=FAKE, lik=FAKE,
        out=FAKE, order=None, targets=None, rpl=0, K=1, first=0, stride=1):
    """A _dv entry with a NULL context and pointers that are never read: the arguments are checked first."""
    L = bnpp._lib
    pf = None if partial is None else (C.c_ubyte * max(len(ev_vars), 1))(*[1 if v in partial else 0 for v in ev_vars])
    h, oa, no = (bnpp.MIN_FILL, None, 0) if order is None else (bnpp.ORDER_GIVEN, _ints(order), len(order))
    head = (None, m.handle if m is not None else None, len(ev_vars), _ints(ev_vars), n_rows, P(ev), pf, len(soft_vars),
            _ints(soft_vars), P(lik), lik_dtype, h, oa, no)
    o = P(out)
    if fn == "partition_batch":
        rc = L.bnpp_partition_batch_dv(*head, dtype, rpl, o, None, None)
    elif fn == "marginals_batch":
        nt, ta = (0, None) if targets is None else (len(targets), _ints(targets))
        rc = L.bnpp_marginals_batch_dv(*head, nt, ta, dtype, rpl, o, None, None)
    elif fn == "mpe_batch":
        rc = L.bnpp_mpe_batch_dv(*head, dtype, rpl, o, None, None)
    else:
        rc = L.bnpp_sample_batch_dv(*head, dtype, rpl, K, first, stride, 7, o, None, None, None)
    return rc, L.bnpp_last_error().decode()


def _sv(fn, m, ev_vars, rows, soft_vars=(), lik=None, partial=None, dtype=bnpp.F64, order=None, targets=None, rpl=0,
        K=1, first=0, stride=1, null_out=False):
    """The _sv sibling with a NULL context and the same arguments (valid values in the host arrays)."""
    L = bnpp._lib
    IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.intc).reshape(len(rows), len(ev_vars)))
    lik = np.ascontiguousarray(lik if lik is not None else np.zeros((len(rows), 1)), dtype=np.float64)
    pf = None if partial is None else (C.c_ubyte * max(len(ev_vars), 1))(*[1 if v in partial else 0 for v in ev_vars])
    h, oa, no = (bnpp.MIN_FILL, None, 0) if order is None else (bnpp.ORDER_GIVEN, _ints(order), len(order))
    head = (None, m.handle if m is not None else None, len(ev_vars), _ints(ev_vars), len(rows), rows.ctypes.data_as(IP), pf,
            len(soft_vars), _ints(soft_vars), lik.ctypes.data_as(DP), h, oa, no)
    buf = np.zeros(4096)
    xs = np.zeros(4096, dtype=np.intc)
    o = None if null_out else buf.ctypes.data_as(DP)
    if fn == "partition_batch":
        rc = L.bnpp_partition_batch_sv(*head, dtype, rpl, o, None, None)
    elif fn == "marginals_batch":
        nt, ta = (0, None) if targets is None else (len(targets), _ints(targets))
        rc = L.bnpp_marginals_batch_sv(*head, nt, ta, dtype, rpl, o, None, None)
    elif fn == "mpe_batch":
        rc = L.bnpp_mpe_batch_sv(*head, dtype, rpl, o, None, None)
    else:
        rc = L.bnpp_sample_batch_sv(*head, dtype, rpl, K, first, stride, 7, None if null_out else P(xs.ctypes.data), None,
                                    None, None)
    return rc, L.bnpp_last_error().decode()


@pytest.mark.parametrize("fn", DV)
def test_argument_errors_are_the_siblings_without_a_device(fn):
    m, d = _load("asia")
    ev, soft = [0, 3], [2, 5]
    rows = [[0, 1], [1, 0], [1, 1]]
    good = np.full((3, d["cards"][2] + d["cards"][5]), 0.25)
    # every host-side argument error: the same status and the same message as the _sv sibling
    cases = [
        dict(ev_vars=[0, 0]), dict(ev_vars=[0, 99]), dict(ev_vars=[-1, 3]),
        dict(soft_vars=[2, 3]), dict(soft_vars=[2, 2]), dict(soft_vars=[2, 8]), dict(soft_vars=[-1]),
        dict(dtype=7), dict(rpl=-1), dict(rpl=2 ** 31),
        dict(order=[1, 1]), dict(order=[99]),
    ]
    if fn in ("mpe_batch", "sample_batch", "marginals_batch"):
        cases.append(dict(order=[1, 2]))                    # does not cover every non-evidence variable
    if fn == "marginals_batch":
        cases += [dict(targets=[1, 1]), dict(targets=[99]), dict(targets=[])]
    if fn == "sample_batch":
        cases += [dict(K=0), dict(stride=-1), dict(first=-1), dict(first=2 ** 63 - 1, stride=2 ** 40)]
    null_ctx = []
    for kw in cases:
        a = dict(ev_vars=ev, soft_vars=soft)
        a.update(kw)
        ev_vars, soft_vars = a.pop("ev_vars"), a.pop("soft_vars")
        got = _dv(fn, m, ev_vars, 3, soft_vars, **a)
        want = _sv(fn, m, ev_vars, np.zeros((3, len(ev_vars))), soft_vars, good, **a)
        if want[0] == bnpp.ERR_NO_DEVICE or "context" in want[1]:
            null_ctx.append(kw)                             # only a device can tell (the plan): both get that far
            assert got[0] == want[0] and ("context" in got[1] or got[0] == bnpp.ERR_NO_DEVICE), (kw, got, want)
        else:
            assert got == want and got[0] != bnpp.OK, (kw, got, want)
    assert all(set(kw) <= {"dtype", "rpl", "order"} for kw in null_ctx), null_ctx
    # n_rows, the null model, the null arrays and outputs
    assert _dv(fn, m, ev, 0, soft) == _sv(fn, m, ev, np.zeros((0, 2)), soft, np.zeros((0, 4)))
    assert _dv(fn, None, ev, 3, soft) == _sv(fn, None, ev, rows, soft, good)
    rc, msg = _dv(fn, m, ev, 3, soft, ev=None)
    assert rc == bnpp.ERR_INVALID and msg == "bad evidence arrays"
    rc, msg = _dv(fn, m, ev, 3, soft, lik=None)
    assert rc == bnpp.ERR_INVALID and msg == "bad soft evidence arrays"
    assert _dv(fn, m, ev, 3, soft, out=None) == _sv(fn, m, ev, rows, soft, good, null_out=True)
    rc, msg = _dv(fn, m, ev, 3, soft, lik_dtype=5)
    assert rc == bnpp.ERR_INVALID and "lik_dtype" in msg
    # a valid call gets as far as the missing context (or the missing device), as the sibling does
    for e_, p_, s_ in ((ev, None, soft), (ev, [0, 3], soft), ([], None, soft), (ev, None, [])):
        got = _dv(fn, m, e_, 3, s_, partial=p_)
        want = _sv(fn, m, e_, np.zeros((3, len(e_))), s_, good[:, :4 if s_ else 1], partial=p_)
        assert got == want and ((got[0] == bnpp.ERR_INVALID and "context" in got[1]) or got[0] == bnpp.ERR_NO_DEVICE)


def test_single_step_argument_checks_without_a_device():
    L = bnpp._lib
    cards = _ints([2, 3])
    err = lambda: L.bnpp_last_error().decode()
    f = P(FAKE)
    assert L.bnpp_stage_evidence_rows(None, None, 2, cards, None, 4, 0, 4, f, f, None) == bnpp.ERR_INVALID
    assert L.bnpp_stage_evidence_rows(None, None, 2, cards, None, 0, 0, 4, f, f, f) == bnpp.ERR_INVALID and "n_rows" in err()
    assert L.bnpp_stage_evidence_rows(None, None, 2, cards, None, 4, 4, 4, f, f, f) == bnpp.ERR_INVALID and "row0" in err()
    assert L.bnpp_stage_evidence_rows(None, None, 2, cards, None, 4, 0, 0, f, f, f) == bnpp.ERR_INVALID and "R must" in err()
    assert L.bnpp_stage_evidence_rows(None, None, 2, _ints([2, 0]), None, 4, 0, 4, f, f, f) == bnpp.ERR_INVALID and "card" in err()
    assert L.bnpp_stage_evidence_rows(None, None, 321, _ints([2] * 321), None, 4, 0, 4, f, f, f) == bnpp.ERR_UNSUPPORTED
    assert L.bnpp_stage_evidence_rows(None, None, 2, cards, None, 4, 0, 4, f, f, f) == bnpp.ERR_INVALID and "context" in err()
    assert L.bnpp_stage_likelihoods(None, None, 0, 0, 2, cards, 4, 0, 4, f, f, None, f) == bnpp.ERR_INVALID
    assert L.bnpp_stage_likelihoods(None, None, 3, 0, 2, cards, 4, 0, 4, f, f, f, f) == bnpp.ERR_INVALID and "dtype" in err()
    assert L.bnpp_stage_likelihoods(None, None, 0, 3, 2, cards, 4, 0, 4, f, f, f, f) == bnpp.ERR_INVALID and "dtype" in err()
    assert L.bnpp_stage_likelihoods(None, None, 0, 1, 2, cards, 4, 0, 4, f, f, f, f) == bnpp.ERR_INVALID and "context" in err()
    assert L.bnpp_emit_row_scalars(None, None, 0, f, 1, None, None, 0, 4, None, None) == bnpp.ERR_INVALID and "output" in err()
    assert L.bnpp_emit_row_scalars(None, None, 0, f, 1, None, None, 0, 4, f, None) == bnpp.ERR_INVALID and "context" in err()
    col, wr = _ints([0, -1]), (C.c_ubyte * 2)(0, 1)
    assert L.bnpp_emit_row_states(None, None, 0, 2, col, wr, 2, 4, 0, 4, f, f, 0, None, 0, None, 0, f, None) == bnpp.ERR_INVALID
    assert "K must be 1" in err()
    assert L.bnpp_emit_row_states(None, None, 0, 2, col, wr, 1, 4, 0, 5, f, f, 0, None, 0, None, 0, f, None) == bnpp.ERR_INVALID
    assert "rows_live" in err()
    assert L.bnpp_emit_row_states(None, None, 0, 2, col, wr, 1, 4, 0, 4, f, None, 0, None, 0, None, 0, f, None) == bnpp.ERR_INVALID
    assert "evidence table" in err()
    assert L.bnpp_emit_row_states(None, None, 1, 2, col, wr, 3, 4, 0, 4, f, f, 0, None, 0, f, 2, f, f) == bnpp.ERR_INVALID
    assert "context" in err()


LIK_MODES = ("wide", "ones", "one_hot", "zero_block", "subnormal")


def _lik(mode, n, cards, seed=3):
    rng = np.random.default_rng(seed)
    ws = sum(cards)
    if mode == "wide":                                      # magnitudes over 2^+-1000
        return np.ldexp(rng.uniform(0.5, 1.0, (n, ws)), rng.integers(-1000, 1001, (n, ws)).astype(np.int32))
    if mode == "ones":
        return np.ones((n, ws))
    if mode == "subnormal":
        return np.ldexp(rng.uniform(0.5, 1.0, (n, ws)), rng.integers(-1074, -1022, (n, ws)).astype(np.int32))
    a = np.zeros((n, ws))
    w = 0
    for i, k in enumerate(cards):
        if not (mode == "zero_block" and i == 0):
            a[np.arange(n), w + rng.integers(0, k, n)] = np.ldexp(1.0, rng.integers(-40, 40, n).astype(np.int32))
        w += k
    return a


@pytest.mark.parametrize("mode", LIK_MODES)
@pytest.mark.parametrize("cards", [[3], [1], [300, 2], [2] * 17])
def test_stage_lik_restatement_properties(cards, mode):
    n, R, row0 = 11, 8, 8                                   # the second launch: 3 live rows, 5 padding
    lik = _lik(mode, n, cards)
    out, e_row, status = ref.stage_lik(lik, cards, row0, R, np.float64)
    assert status == ref.NONE and out.shape == (sum(cards), R)
    rows = ref.launch_rows(n, row0, R)
    assert list(rows) == [8, 9, 10, 10, 10, 10, 10, 10], "the padding rule"
    w, e_sum = 0, np.zeros(R, dtype=np.int64)
    for k in cards:
        blk = lik[rows, w:w + k]
        top = out[w:w + k].max(axis=0)
        nz = blk.max(axis=1) > 0
        assert ((top[nz] >= 0.5) & (top[nz] < 1.0)).all(), "every non-zero block's top lies in [0.5, 1)"
        assert (out[w:w + k][:, ~nz] == 0).all()
        e = np.where(nz, np.frexp(blk.max(axis=1))[1], 0)
        # ldexp(staged, e) reproduces lik exactly in fp64 (an entry 2^-1075 or more below a top underflows: none here
        # but in "wide", where the restatement's own rounding is the statement)
        back = np.ldexp(out[w:w + k], e[None, :].astype(np.int32)).T
        exact = (np.ldexp(blk, -e[:, None].astype(np.int32)) >= np.ldexp(1.0, -1022)) | (blk == 0)
        assert np.array_equal(back[exact], blk[exact]) and exact.any()
        e_sum += e
        w += k
    assert np.array_equal(e_row, e_sum)
    assert np.array_equal(out[:, 2], out[:, 7]) and e_row[2] == e_row[7], "padding rows copy the last row"
    # fp32 output: one rounding of the same values; fp32 input widens exactly
    out32, e32, _ = ref.stage_lik(lik, cards, row0, R, np.float32)
    assert np.array_equal(out32, out.astype(np.float32)) and np.array_equal(e32, e_row)
    with np.errstate(under="ignore"):
        l32 = np.minimum(lik, 1e38).astype(np.float32)
    a, ea, _ = ref.stage_lik(l32, cards, row0, R, np.float64)
    b, eb, _ = ref.stage_lik(l32.astype(np.float64), cards, row0, R, np.float64)
    assert np.array_equal(a, b) and np.array_equal(ea, eb)


def test_stage_restatements_name_the_first_invalid_cell():
    cards, partial = [2, 300, 3], [0, 0, 1]
    ev = np.array([[0, 299, -1], [1, 0, 2], [1, 5, 0], [0, 7, 1], [1, 1, 1]], dtype=np.int32)
    t, status = ref.stage_rows(ev, cards, partial, 2, 4)
    assert status == ref.NONE and t.shape == (3, 4) and np.array_equal(t[:, 2], t[:, 3]), "row 4 pads the launch"
    assert np.array_equal(t[:, 0], ev[2]) and np.array_equal(ref.stage_rows(ev, cards, partial, 0, 2)[0][:, 0], [0, 299, -1])
    for (r, j, x) in ((1, 0, -1), (1, 2, -2), (0, 1, 300), (1, 2, 3)):
        bad = ev.copy()
        bad[r, j] = x
        bad[1, 2] = x if (r, j) == (1, 2) else bad[1, 2]
        bad[4, 0] = 2                                       # a later invalid cell: not the first
        t, status = ref.stage_rows(bad, cards, partial, 0, 8)
        assert status == r * 3 + j and t[j, r] == 0 and t[0, 4] == 0
        assert ref.stage_rows(bad, cards, partial, 4, 8)[1] == 12, "a launch names the cells of its own rows"
    lik = np.full((5, 5), 0.5)
    for x in (np.nan, np.inf, -np.inf, -1e-300):
        bad = lik.copy()
        bad[3, 4] = bad[4, 1] = x
        out, e_row, status = ref.stage_lik(bad, [2, 3], 0, 5, np.float64)
        assert status == 3 * 5 + 4 and out[4, 3] == 0 and out[1, 4] == 0 and np.isfinite(out).all()
