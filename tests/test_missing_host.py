"""CPU tests of missing values in batched evidence: the exported _mv symbols,
partial = None / all zero being the old plan, the plans of partial sets (the
mask factor rule, the masked gather key, every level key instantiated), the
argument checks made before a device is looked at, the .evid loader over
differing variable sets, and missing_ref itself."""
import ctypes as C

import numpy as np
import pytest

import bnpp
import missing_ref
from bnpp import synth
from conftest import model_path
from counts_ref import EV_VARS
from missing_ref import MISSING

IP, DP, UBP = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
MASK_KEY = (1 << 24) + 32768
PLANS = {
    "batch": lambda m, ev, **kw: bnpp.plan_batch(m, ev, **kw),
    "mpe": lambda m, ev, **kw: bnpp.plan_mpe_batch(m, ev, **kw),
    "sample": lambda m, ev, **kw: bnpp.plan_sample_batch(m, ev, **kw),
    "counts": lambda m, ev, **kw: bnpp.plan_counts(m, ev, **kw),
    "marginals": lambda m, ev, **kw: bnpp.plan_marginals_batch(m, ev, **kw),
}


def _load(name):
    return bnpp.Model.load(model_path(name + ".uai")), synth.read_uai(model_path(name + ".uai"))


def test_symbols_are_exported_and_bound():
    for name in ("partition_batch", "posterior_batch", "mpe_batch", "sample_batch", "expected_counts", "marginals_batch",
                 "plan_batch", "plan_mpe_batch", "plan_sample_batch", "plan_counts", "plan_marginals_batch",
                 "condition_batch", "evidence_load_batch"):
        assert "bnpp_%s_mv" % name in bnpp.EXPORTED and hasattr(bnpp._lib, "bnpp_%s_mv" % name)
    assert bnpp.MISSING == MISSING == -1 and bnpp.COND_BATCH_MASK_KEY == MASK_KEY
    assert bnpp.COND_BATCH_MASK_KEY > bnpp.MARG_ROWS_KEY, "the next free key after the emit step's"


@pytest.mark.parametrize("name", ["asia", "alarm", "ising6x6"])
@pytest.mark.parametrize("kind", sorted(PLANS))
def test_partial_none_or_all_zero_is_the_old_plan(name, kind):
    m, _ = _load(name)
    ev = EV_VARS[name]
    old = PLANS[kind](m, ev, rows_per_launch=64)
    zero = PLANS[kind](m, ev, rows_per_launch=64, partial=[])
    assert zero[-1] == [-1] * len(ev), "no variable carries a mask"
    assert zero[0] == old[0] and zero[1] == old[1], "stats and groups of the entry without the argument"
    assert tuple(zero[2:-1]) == tuple(old[2:])
    assert all(g["key"] != MASK_KEY for g in old[1])


@pytest.mark.parametrize("name", sorted(EV_VARS))
def test_mask_factor_obeys_the_rule_and_masked_steps_have_their_key(name):
    m, d = _load(name)
    ev = EV_VARS[name]
    for part in [[v] for v in ev] + [list(ev), ev[:2]]:
        st, groups, beliefs, no_b, mf = bnpp.plan_counts(m, ev, rows_per_launch=8, partial=part)
        assert mf == missing_ref.mask_factors(d, ev, part), (part, mf)
        carriers = {f for f in mf if f >= 0}
        masked = [g for g in groups if g["key"] == MASK_KEY]
        assert len(masked) == len(carriers) > 0 and all(g["level"] == 0 and g["n_desc"] == 1 for g in masked)
        hard = [v for v in ev if v not in part]
        n_hard_only = sum(1 for f, s in enumerate(d["scopes"]) if f not in carriers and any(v in hard for v in s))
        assert sum(g["key"] == bnpp.COND_BATCH_KEY for g in groups) == n_hard_only
        assert st["gather_steps"] == n_hard_only + len(carriers)
        # a partial variable is conditioned away nowhere: every factor's belief keeps it; a hard one never is kept
        for f, s in enumerate(d["scopes"]):
            kept = [v for v in beliefs[f] if v != m.n_vars]
            assert sorted(kept) == sorted(v for v in s if v not in hard), (f, s, kept)
        assert no_b
        # ... and it is eliminated: the plan is the plan of the hard variables with more gather steps in front
        sh, gh, bh, _ = bnpp.plan_counts(m, hard, rows_per_launch=8)
        assert st["width"] == sh["width"], "the width of a call without the partial variables as evidence"


def test_mask_goes_to_a_factor_that_is_gathered_anyway():
    # factors: (0, 1) with 6 entries, (1, 2) with 6, (1) with 3; variable 1 partial
    d = dict(type="MARKOV", cards=[2, 3, 2], scopes=[[0, 1], [1, 2], [1]],
             values=[[1.0] * 6, [1.0] * 6, [1.0, 2.0, 3.0]])
    m = bnpp.Model.from_dict(d)
    assert bnpp.plan_batch(m, [1], partial=[1], rows_per_launch=4)[-1] == [2], "fewest entries: the unary factor"
    assert bnpp.plan_batch(m, [1, 2], partial=[1], rows_per_launch=4)[-1] == [1, -1], "a hard variable's factor wins"
    assert bnpp.plan_batch(m, [0, 1, 2], partial=[1], rows_per_launch=4)[-1] == [-1, 0, -1], "ties: the lowest index"
    assert missing_ref.mask_factors(d, [0, 1, 2], [1]) == [-1, 0, -1]
    # a partial variable in no factor carries no mask and adds no step
    d2 = dict(d, cards=[2, 3, 2, 4])
    st, groups, scope, mf = bnpp.plan_batch(bnpp.Model.from_dict(d2), [3], partial=[3], rows_per_launch=4)
    assert mf == [-1] and st["gather_steps"] == 0


def test_explicit_order_must_cover_the_partial_variables():
    m, _ = _load("asia")
    full = [7, 6, 5, 4, 2, 1]
    bnpp.plan_mpe_batch(m, [0, 3], order=full, rows_per_launch=4)
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_mpe_batch(m, [0, 3], order=full, rows_per_launch=4, partial=[3])
    assert e.value.status == bnpp.ERR_INVALID and "cover every non-evidence variable" in str(e.value)
    st, groups, mf = bnpp.plan_mpe_batch(m, [0, 3], order=full + [3], rows_per_launch=4, partial=[3])
    assert mf[0] == -1 and mf[1] >= 0


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_level_keys_of_the_partial_plans_are_instantiated(dt):
    dtype = bnpp.F64 if dt == "f64" else bnpp.F32
    have = set()
    for fam in (0, 1, 2, 4):
        have |= set(bnpp.kernel_keys(dtype, fam, level=True))
    executor = {bnpp.COND_BATCH_KEY, MASK_KEY, bnpp.MARG_ROWS_KEY, bnpp.COUNTS_KEY, bnpp.SAMPLE_BATCH_KEY,
                bnpp.MPE_DECODE_BATCH_KEY}
    for name in sorted(EV_VARS):
        m, _ = _load(name)
        ev = EV_VARS[name]
        for part in [[v] for v in ev] + [list(ev)]:
            for R in (1, 7, 64, 256):
                for kind in sorted(PLANS):
                    groups = PLANS[kind](m, ev, dtype=dtype, rows_per_launch=R, partial=part)[1]
                    assert any(g["key"] == MASK_KEY for g in groups)
                    for g in groups:
                        assert g["key"] in have or g["key"] in executor, (name, part, R, kind, g)


def _raw(m, ev_vars, rows, partial, dtype=bnpp.F64, fn="partition"):
    """An _mv run entry with a NULL context: the arguments are checked first."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.intc).reshape(-1, max(len(ev_vars), 1))[:, :len(ev_vars)])
    vs = (C.c_int * max(len(ev_vars), 1))(*ev_vars)
    pf = None if partial is None else (C.c_ubyte * max(len(ev_vars), 1))(*[1 if v in partial else 0 for v in ev_vars])
    buf = np.zeros(4096)
    xs = np.zeros(4096, dtype=np.intc)
    L = bnpp._lib
    head = (None, m.handle, len(ev_vars), vs, len(rows), rows.ctypes.data_as(IP), pf)
    if fn == "partition":
        rc = L.bnpp_partition_batch_mv(*head, bnpp.MIN_FILL, None, 0, dtype, 0, buf.ctypes.data_as(DP), None, None)
    elif fn == "posterior":
        rc = L.bnpp_posterior_batch_mv(*head, bnpp.MIN_FILL, 1, dtype, 0, buf.ctypes.data_as(DP), None)
    elif fn == "mpe":
        rc = L.bnpp_mpe_batch_mv(*head, bnpp.MIN_FILL, None, 0, dtype, 0, buf.ctypes.data_as(DP), xs.ctypes.data_as(IP), None)
    elif fn == "sample":
        rc = L.bnpp_sample_batch_mv(*head, bnpp.MIN_FILL, None, 0, dtype, 0, 1, 0, 1, 7, C.c_void_p(xs.ctypes.data), None,
                                    None, None)
    elif fn == "counts":
        rc = L.bnpp_expected_counts_mv(*head, None, bnpp.MIN_FILL, None, 0, dtype, 0, buf.ctypes.data_as(DP), None, None,
                                       None)
    else:
        rc = L.bnpp_marginals_batch_mv(*head, bnpp.MIN_FILL, None, 0, 0, None, dtype, 0, buf.ctypes.data_as(DP), None, None)
    return rc, L.bnpp_last_error().decode()


@pytest.mark.parametrize("fn", ["partition", "posterior", "mpe", "sample", "counts", "marginals"])
def test_argument_checks_without_a_device(fn):
    m, d = _load("asia")
    ev = [0, 3]
    # -1 in a column that is not partial: INVALID, naming the row and the variable -- partial NULL included
    for partial in (None, [], [0]):
        rc, msg = _raw(m, ev, [[0, 1], [1, MISSING]], partial, fn=fn)
        assert rc == bnpp.ERR_INVALID and "row 1" in msg and "variable 3" in msg, (partial, msg)
    # -2, and the card, in a partial column
    rc, msg = _raw(m, ev, [[0, 1], [1, -2]], [3], fn=fn)
    assert rc == bnpp.ERR_INVALID and "row 1" in msg and "variable 3" in msg
    rc, msg = _raw(m, ev, [[0, d["cards"][3]], [1, 0]], [3], fn=fn)
    assert rc == bnpp.ERR_INVALID and "row 0" in msg and "variable 3" in msg
    # a valid call with missing values gets as far as the missing context (or the missing device)
    for partial, rows in (([3], [[0, MISSING], [1, 0]]), ([0, 3], [[MISSING, MISSING], [1, MISSING]])):
        rc, msg = _raw(m, ev, rows, partial, fn=fn)
        assert (rc == bnpp.ERR_INVALID and "context" in msg) or rc == bnpp.ERR_NO_DEVICE, (fn, partial, msg)
    # a posterior target may not be listed as evidence, partial or not
    if fn == "posterior":
        rc, msg = _raw(m, [1, 3], [[MISSING, 0]], [1], fn=fn)
        assert rc == bnpp.ERR_INVALID and "target 1" in msg


def test_python_partial_argument():
    m, _ = _load("asia")
    rows = np.array([[0, MISSING], [1, 0]])
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.partition_batch(None, m, [0, 3], rows)
    assert "row 0" in str(e.value) and "variable 3" in str(e.value), "None is the call of today"
    for partial in ("auto", [3], (0, 3)):
        with pytest.raises(bnpp.BnppError) as e:
            bnpp.partition_batch(None, m, [0, 3], rows, partial=partial)
        assert "context" in str(e.value), partial
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.partition_batch(None, m, [0, 3], rows, partial=[0])
    assert "variable 3" in str(e.value)
    with pytest.raises(ValueError):
        bnpp.partition_batch(None, m, [0, 3], rows, partial=[5])
    with pytest.raises(ValueError):
        bnpp.partition_batch(None, m, [0, 3], rows, partial="all")
    f = bnpp._partial_flags([0, 3, 6], "auto", np.array([[0, MISSING, 1], [MISSING, MISSING, 0]]))
    assert list(f) == [1, 1, 0]


def test_loader_reads_differing_variable_sets(tmp_path):
    p = tmp_path / "mixed.evid"
    p.write_text("4\n2 3 1 0 0\n1 6 1\n0\n3 0 1 6 0 3 0\n")
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.load_evidence_batch(str(p))
    assert e.value.status == bnpp.ERR_UNSUPPORTED, "the loader of today stays as it is"
    vs, rows, partial = bnpp.load_evidence_batch(str(p), missing=True)
    assert vs == [0, 3, 6] and partial == [0, 3, 6]
    assert rows.tolist() == [[0, 1, MISSING], [MISSING, MISSING, 1], [MISSING, MISSING, MISSING], [1, 0, 0]]
    same = tmp_path / "same.evid"
    same.write_text("2\n2 3 1 0 0\n2 0 1 3 1\n")
    vs, rows, partial = bnpp.load_evidence_batch(str(same), missing=True)
    assert vs == [0, 3] and partial == [] and rows.tolist() == [[0, 1], [1, 1]]
    one = tmp_path / "one.evid"
    one.write_text("2\n2 3 1 0 0\n1 0 1\n")
    assert bnpp.load_evidence_batch(str(one), missing=True)[2] == [3]
    # the capacity protocol of bnpp_evidence_load_batch: too small a capacity reports the sizes
    n_ev, n_rows = C.c_int(), C.c_int64()
    rc = bnpp._lib.bnpp_evidence_load_batch_mv(str(p).encode(), 0, 0, C.byref(n_ev), None, C.byref(n_rows), None, None)
    assert rc == bnpp.ERR_INVALID and (n_ev.value, n_rows.value) == (3, 4)
    short = tmp_path / "short.evid"
    short.write_text("2\n1 0 1\n1 0\n")
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.load_evidence_batch(str(short), missing=True)
    assert e.value.status == bnpp.ERR_IO
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.load_evidence_batch(str(tmp_path / "absent.evid"), missing=True)
    assert e.value.status == bnpp.ERR_IO


def test_masked_gather_reference_on_a_known_table():
    cards = [3, 2, 4]
    src = np.arange(1.0, 25.0)
    t = src.reshape(3, 2, 4)
    # variable 1 hard, variable 2 partial: out over (0, 2, b)
    ev = np.array([[1, 0, 1, 0], [MISSING, 2, 9, 0]])
    out = missing_ref.masked_gather(src, cards, [0, 1, 2], [1, 2], [2], ev).reshape(3, 4, 4)
    assert np.array_equal(out[:, :, 0], t[:, 1, :]), "missing: the whole slice"
    want = np.zeros((3, 4))
    want[:, 2] = t[:, 0, 2]
    assert np.array_equal(out[:, :, 1], want), "observed: the other digits are 0"
    assert not out[:, :, 2].any(), "a value >= the card matches nothing"
    assert np.array_equal(out[:, 0, 3], t[:, 0, 0]) and not out[:, 1:, 3].any()
    # [p] alone, all missing: the source for every row
    out = missing_ref.masked_gather(np.arange(3.0), [3], [0], [0], [0], np.full((1, 5), MISSING)).reshape(3, 5)
    assert all(np.array_equal(out[:, b], np.arange(3.0)) for b in range(5))
    # no partial variable in the scope: batch_ref's gather
    import batch_ref
    ev = np.array([[1, 0, 1, 1, 0]])
    assert np.array_equal(missing_ref.masked_gather(src, cards, [0, 1, 2], [1], [], ev),
                          batch_ref.gather(src, cards, [0, 1, 2], [1], ev))


def test_brute_force_sums_over_the_missing_variables():
    d = synth.read_uai(model_path("cancer.uai"))
    ev = [0, 3]
    z, marg, counts = missing_ref.brute(d, ev, [[1, MISSING], [MISSING, MISSING], [1, 0], [1, 1]])
    assert np.isclose(z[0], z[2] + z[3]) and np.isclose(z[1], missing_ref.joint(d).sum())
    assert np.array_equal(marg[0][0], [0, 1]) and np.allclose(marg[3][0], [z[2] / z[0], z[3] / z[0]])
    for f, s in enumerate(d["scopes"]):
        assert np.isclose(counts[f].sum(), 4.0), "every possible row counts once in every factor"
    # the masked model of a row has the row's Z with the hard evidence only
    mf = missing_ref.mask_factors(d, ev, [3])
    for row in ([1, MISSING], [1, 0], [0, 1]):
        mm = missing_ref.masked_model(d, ev, mf, row)
        zm, _, _ = missing_ref.brute(mm, [0], [[row[0]]])
        zr, _, _ = missing_ref.brute(d, ev, [row])
        assert np.isclose(zm[0], zr[0], rtol=1e-14)
    rng = np.random.default_rng(3)
    p = missing_ref.punch(rng, np.zeros((1000, 2), dtype=int), 0.3, cols=[1])
    assert (p[:, 0] == 0).all() and 200 < (p[:, 1] == MISSING).sum() < 400


def test_stand_alone_plan_check_program(tmp_path):
    """tests/cpp/missing_plan_check.cpp against the library as built: the program the host code is run under ASan
    and UBSan with (linked against `make sanitize`'s library instead)."""
    import os
    import subprocess
    from conftest import REPO
    LIB = os.path.join(REPO, "bn-pp_amd", "lib")
    exe = str(tmp_path / "missing_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests", "cpp", "missing_plan_check.cpp"),
                    "-I" + os.path.join(REPO, "include"), "-L" + LIB, "-lbnpp", "-Wl,-rpath," + LIB, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    args = []
    for name in ("asia", "alarm"):
        args += [model_path(name + ".uai"), str(len(EV_VARS[name]))] + [str(v) for v in EV_VARS[name]]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    word, plans, checks = p.stdout.split()
    assert word == "OK" and int(plans) == (5 + 4) * 6 * 5 and int(checks) > 0


@pytest.mark.parametrize("name", ["asia", "cancer"])
def test_restatement_meets_the_bound_on_the_distribution_inputs(name):
    """The numpy restatement alone (sample_ref.run on the row's masked model with the hard evidence) for the rows, K
    and seed of test_gpu_missing.py's distribution test: were one of its frequencies outside sample_ref.bound,
    that test would fail on the reference's own noise."""
    import sample_batch_ref as sbr
    import sample_ref
    assert name in sbr.DIST_MODELS
    path = model_path(name + ".uai")
    d = synth.read_uai(path)
    ev, rows, part = missing_ref.dist_case(d)
    assert (rows[::2, 2] == MISSING).all() and (rows[1::2] >= 0).all() and part == [ev[2]]
    hard = ev[:2]
    mf = missing_ref.mask_factors(d, ev, part)
    order, _ = bnpp.ordering(bnpp.Model.load(path), {v: 0 for v in hard}, "mf")
    x = np.zeros((8, sbr.DIST_K, len(d["cards"])), dtype=np.uint8)
    for b, row in enumerate(rows):
        mm = missing_ref.masked_model(d, ev, mf, row)
        x[b], deg = sample_ref.run(mm, {v: int(row[j]) for j, v in enumerate(hard)}, order, sbr.DIST_K,
                                   missing_ref.DIST_SEED, np.float64, first=b * sbr.DIST_K)
        assert deg == 0
        obs = row >= 0
        assert (x[b][:, np.array(ev)[obs]] == row[obs]).all(), "the mask keeps the observed value"
    assert len({int(v) for v in x[0][:, ev[2]]}) == 2, "a missing variable is drawn"
    bad = missing_ref.frequency_violations(d, ev, rows, x)
    assert not bad, bad[:3]
