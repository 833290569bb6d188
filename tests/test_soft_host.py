"""CPU tests of soft evidence in batched calls: the exported _sv symbols, the
argument checks made before a device is looked at, the plans of soft sets (the
likelihood factor rule, the weighted gather key, every level key instantiated,
soft = None being the plan recorded before the feature), the job key, the
likelihood file loader, and soft_ref itself."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bnpp
import missing_ref
import soft_ref
from bnpp import synth
from conftest import model_path
from counts_ref import EV_VARS

IP, DP, UBP = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
SOFT_KEY = (1 << 24) + 36864
MASK_KEY = (1 << 24) + 32768
PLANS = {
    "batch": lambda m, ev, **kw: bnpp.plan_batch(m, ev, **kw),
    "mpe": lambda m, ev, **kw: bnpp.plan_mpe_batch(m, ev, **kw),
    "sample": lambda m, ev, **kw: bnpp.plan_sample_batch(m, ev, **kw),
    "counts": lambda m, ev, **kw: bnpp.plan_counts(m, ev, **kw),
    "marginals": lambda m, ev, **kw: bnpp.plan_marginals_batch(m, ev, **kw),
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft_parent_plans.json")


def _load(name):
    return bnpp.Model.load(model_path(name + ".uai")), synth.read_uai(model_path(name + ".uai"))


def _free(d, ev, n=3):
    """The first n variables that are no evidence variables and sit in a factor."""
    used = {v for s in d["scopes"] for v in s}
    return [v for v in range(len(d["cards"])) if v not in ev and v in used][:n]


def test_symbols_are_exported_and_bound():
    for name in ("partition_batch", "posterior_batch", "mpe_batch", "sample_batch", "expected_counts", "marginals_batch",
                 "plan_batch", "plan_mpe_batch", "plan_sample_batch", "plan_counts", "plan_marginals_batch",
                 "condition_batch"):
        assert "bnpp_%s_sv" % name in bnpp.EXPORTED and hasattr(bnpp._lib, "bnpp_%s_sv" % name)
    assert "bnpp_likelihood_load" in bnpp.EXPORTED
    assert bnpp.COND_BATCH_SOFT_KEY == SOFT_KEY == bnpp.COND_BATCH_MASK_KEY + 4096, "the next free key after the masked step's"
    assert bnpp._lib.bnpp_version() == 205, "symbols are added, the version stays"


@pytest.mark.parametrize("name", soft_ref.PLAN_MODELS)
def test_soft_none_is_the_plan_recorded_before_the_feature(name):
    """golden/soft_parent_plans.json (soft_ref.plan_record says what it holds and how it was written): all five plans
    as the commit before soft evidence planned them, rows_per_launch 64, hard evidence and the first evidence
    variable partial, both dtypes."""
    with open(GOLDEN) as f:
        gold = json.load(f)
    m, _ = _load(name)
    ev = EV_VARS[name]
    cases = soft_ref.plan_cases(bnpp, ev)
    assert len(cases) == 20 and len(gold) == 20 * len(soft_ref.PLAN_MODELS)
    for tag, fn, kw in cases:
        want = gold[name + "/" + tag]
        for soft in (None, []):
            r = fn(m, ev, soft=soft, **kw)
            if soft is not None:
                assert r[-1] == [], "no soft variable: no likelihood factor"
                r = r[:-1]
            got = soft_ref.plan_record(r, bnpp.PLAN_GROUP_FIELDS)
            assert got["stats"] == want["stats"], (tag, soft)
            assert got["keys"] == want["keys"], (tag, soft)
            assert got == want, (tag, soft, "the group rows, or what else the plan function returns")
            assert all(g["key"] != SOFT_KEY for g in r[1])


@pytest.mark.parametrize("name", ["asia", "alarm"])
def test_lam_factor_obeys_the_rule_and_weighted_steps_have_their_key(name):
    m, d = _load(name)
    ev = EV_VARS[name]
    free = _free(d, ev, 4)
    for part in ([], [ev[0]]):
        for soft in [[v] for v in free] + [free, free[::-1][:2]]:
            r = bnpp.plan_counts(m, ev, rows_per_launch=8, partial=part or None, soft=soft)
            st, groups, beliefs, lf = r[0], r[1], r[2], r[-1]
            assert lf == soft_ref.lam_factors(d, ev, part, soft), (part, soft, lf)
            carriers = set(lf)
            weighted = [g for g in groups if g["key"] == SOFT_KEY]
            assert len(weighted) == len(carriers) > 0 and all(g["level"] == 0 and g["n_desc"] == 1 for g in weighted)
            hard = [v for v in ev if v not in part]
            mf = [f for f in (r[-2] if part else []) if f >= 0]
            n_masked = len({f for f in mf if f not in carriers})
            n_plain = sum(1 for f, s in enumerate(d["scopes"])
                          if f not in carriers and f not in mf and any(v in hard for v in s))
            assert sum(g["key"] == MASK_KEY for g in groups) == n_masked, "masks on a weighted step ride with it"
            assert sum(g["key"] == bnpp.COND_BATCH_KEY for g in groups) == n_plain
            assert st["gather_steps"] == n_plain + n_masked + len(carriers)
            # a soft variable is conditioned away nowhere, and the plan keeps the width of the hard variables' plan
            for f, s in enumerate(d["scopes"]):
                kept = [v for v in beliefs[f] if v != m.n_vars]
                assert sorted(kept) == sorted(v for v in s if v not in hard), (f, s, kept)
            assert st["width"] == bnpp.plan_counts(m, hard, rows_per_launch=8)[0]["width"]


def test_likelihoods_go_to_a_factor_that_is_gathered_anyway():
    # factors: (0, 1) with 6 entries, (1, 2) with 6, (1) with 3; variable 1 soft
    d = dict(type="MARKOV", cards=[2, 3, 2], scopes=[[0, 1], [1, 2], [1]],
             values=[[1.0] * 6, [1.0] * 6, [1.0, 2.0, 3.0]])
    m = bnpp.Model.from_dict(d)
    assert bnpp.plan_batch(m, [], soft=[1], rows_per_launch=4)[-1] == [2], "fewest entries: the unary factor"
    assert bnpp.plan_batch(m, [2], soft=[1], rows_per_launch=4)[-1] == [1], "a hard variable's factor wins"
    assert bnpp.plan_batch(m, [0, 2], soft=[1], rows_per_launch=4)[-1] == [0], "ties: the lowest index"
    assert soft_ref.lam_factors(d, [0, 2], [], [1]) == [0]
    st, groups, scope, lf = bnpp.plan_batch(m, [], soft=[1, 0, 2], rows_per_launch=4)
    assert lf == [2, 0, 1] and st["gather_steps"] == 3 and sum(g["key"] == SOFT_KEY for g in groups) == 3
    # one factor may carry several weights, and a mask beside them
    st, groups, scope, mf, lf = bnpp.plan_batch(m, [2, 0], partial=[0], soft=[1], rows_per_launch=4)
    assert lf == [1] and mf == [-1, 0]
    d3 = dict(type="MARKOV", cards=[2, 3, 2], scopes=[[0, 1, 2]], values=[[1.0] * 12])
    st, groups, scope, mf, lf = bnpp.plan_batch(bnpp.Model.from_dict(d3), [0], partial=[0], soft=[1, 2], rows_per_launch=4)
    assert lf == [0, 0] and mf == [0] and [g["key"] for g in groups if g["level"] == 0] == [SOFT_KEY]
    # a soft variable in no factor: UNSUPPORTED, naming it
    d2 = dict(d, cards=[2, 3, 2, 4])
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_batch(bnpp.Model.from_dict(d2), [0], soft=[3], rows_per_launch=4)
    assert e.value.status == bnpp.ERR_UNSUPPORTED and "soft variable 3" in str(e.value) and "no factor" in str(e.value)


def test_nine_unmerged_dims_are_unsupported():
    # one factor over ten binary variables: eight soft dims, never merged, leave the ninth and tenth as one run -> 9 rest dims
    cards = [2] * 10
    d = dict(type="MARKOV", cards=cards, scopes=[list(range(10))], values=[[1.0] * 1024])
    m = bnpp.Model.from_dict(d)
    st, groups, scope, lf = bnpp.plan_batch(m, [], soft=[0, 1, 2, 3, 4, 5, 6], rows_per_launch=4)
    assert lf == [0] * 7, "seven soft dims and one merged run of three: eight rest dims"
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_batch(m, [], soft=[0, 1, 2, 3, 4, 5, 6, 7], rows_per_launch=4)
    assert e.value.status == bnpp.ERR_UNSUPPORTED and "separate runs" in str(e.value) and "at most 8" in str(e.value)
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_batch(m, [], soft=[0, 2, 4, 6, 8], rows_per_launch=4)
    assert e.value.status == bnpp.ERR_UNSUPPORTED, "five soft dims with four single free dims between and one after"


def test_job_key_ignores_values_and_is_unchanged_without_soft():
    m, d = _load("asia")
    ev = EV_VARS["asia"]
    free = _free(d, ev)
    base = bnpp.batch_job_key(m, ev)
    assert bnpp.batch_job_key(m, ev, soft=None) == base == bnpp.batch_job_key(m, ev, soft=[]), "nothing is mixed in"
    k1 = bnpp.batch_job_key(m, ev, soft=free[:1])
    assert k1 != base and k1 == bnpp.batch_job_key(m, ev, soft=free[:1]), "the variables decide, no value is seen"
    assert len({base, k1, bnpp.batch_job_key(m, ev, soft=free[:2]), bnpp.batch_job_key(m, ev, soft=free[:2][::-1]),
                bnpp.batch_job_key(m, ev, partial=[ev[0]]), bnpp.batch_job_key(m, ev, partial=[ev[0]], soft=free[:1])}) == 6


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_level_keys_of_the_soft_plans_are_instantiated(dt):
    dtype = bnpp.F64 if dt == "f64" else bnpp.F32
    have = set()
    for fam in (0, 1, 2, 4):
        have |= set(bnpp.kernel_keys(dtype, fam, level=True))
    assert SOFT_KEY not in have, "the weighted step is the executor's: in no family a census enumerates"
    executor = {bnpp.COND_BATCH_KEY, MASK_KEY, SOFT_KEY, bnpp.MARG_ROWS_KEY, bnpp.COUNTS_KEY, bnpp.SAMPLE_BATCH_KEY,
                bnpp.MPE_DECODE_BATCH_KEY}
    for name in sorted(EV_VARS):
        m, d = _load(name)
        ev = EV_VARS[name]
        for soft in [[v] for v in ev] + [list(ev)]:         # each evidence variable of the catalogue soft instead
            hard = [v for v in ev if v not in soft]
            for R in (1, 7, 64, 256):
                for kind in sorted(PLANS):
                    groups = PLANS[kind](m, hard, dtype=dtype, rows_per_launch=R, soft=soft)[1]
                    assert any(g["key"] == SOFT_KEY for g in groups)
                    for g in groups:
                        assert g["key"] in have or g["key"] in executor, (name, soft, R, kind, g)


def _raw(m, ev_vars, rows, soft_vars, lik, partial=None, dtype=bnpp.F64, fn="partition", target=1):
    """An _sv run entry with a NULL context: the arguments are checked first."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.intc).reshape(len(rows), len(ev_vars)))
    vs = (C.c_int * max(len(ev_vars), 1))(*ev_vars)
    sv = (C.c_int * max(len(soft_vars), 1))(*soft_vars)
    lik = np.ascontiguousarray(lik, dtype=np.float64)
    pf = None if partial is None else (C.c_ubyte * max(len(ev_vars), 1))(*[1 if v in partial else 0 for v in ev_vars])
    buf = np.zeros(4096)
    xs = np.zeros(4096, dtype=np.intc)
    L = bnpp._lib
    head = (None, m.handle, len(ev_vars), vs, len(rows), rows.ctypes.data_as(IP), pf, len(soft_vars), sv,
            lik.ctypes.data_as(DP))
    if fn == "partition":
        rc = L.bnpp_partition_batch_sv(*head, bnpp.MIN_FILL, None, 0, dtype, 0, buf.ctypes.data_as(DP), None, None)
    elif fn == "posterior":
        rc = L.bnpp_posterior_batch_sv(*head, bnpp.MIN_FILL, target, dtype, 0, buf.ctypes.data_as(DP), None)
    elif fn == "mpe":
        rc = L.bnpp_mpe_batch_sv(*head, bnpp.MIN_FILL, None, 0, dtype, 0, buf.ctypes.data_as(DP), xs.ctypes.data_as(IP), None)
    elif fn == "sample":
        rc = L.bnpp_sample_batch_sv(*head, bnpp.MIN_FILL, None, 0, dtype, 0, 1, 0, 1, 7, C.c_void_p(xs.ctypes.data), None,
                                    None, None)
    elif fn == "counts":
        rc = L.bnpp_expected_counts_sv(*head, None, bnpp.MIN_FILL, None, 0, dtype, 0, buf.ctypes.data_as(DP), None, None,
                                       None)
    else:
        rc = L.bnpp_marginals_batch_sv(*head, bnpp.MIN_FILL, None, 0, 0, None, dtype, 0, buf.ctypes.data_as(DP), None, None)
    return rc, L.bnpp_last_error().decode()


@pytest.mark.parametrize("fn", ["partition", "posterior", "mpe", "sample", "counts", "marginals"])
def test_argument_checks_without_a_device(fn):
    m, d = _load("asia")
    ev, soft = [0, 3], [2, 5]
    rows = [[0, 1], [1, 0], [1, 1]]
    ws = d["cards"][2] + d["cards"][5]
    good = np.full((3, ws), 0.25)
    good[2, :] = [3e9, 0.0, 0.0, 1e-300][:ws]               # no upper bound; zeros are values
    # a NaN, an inf and a negative value: INVALID, naming the row and the variable
    for bad in (np.nan, np.inf, -np.inf, -1e-9):
        lik = good.copy()
        lik[1, d["cards"][2]] = bad                         # row 1, the first value of variable 5
        rc, msg = _raw(m, ev, rows, soft, lik, fn=fn)
        assert rc == bnpp.ERR_INVALID and "row 1" in msg and "soft variable 5" in msg, (bad, msg)
    # a variable both evidence and soft, a duplicate, an id out of range
    rc, msg = _raw(m, ev, rows, [2, 3], good, fn=fn)
    assert rc == bnpp.ERR_INVALID and "variable 3 is both" in msg
    rc, msg = _raw(m, ev, rows, [2, 2], good, fn=fn)
    assert rc == bnpp.ERR_INVALID and "soft variable 2 is listed twice" in msg
    for v in (-1, 8):
        rc, msg = _raw(m, ev, rows, [2, v], good, fn=fn)
        assert rc == bnpp.ERR_INVALID and "soft variable %d out of range" % v in msg
    # a valid call gets as far as the missing context (or the missing device), with partial and with n_ev = 0
    for e_, r_, p_ in ((ev, rows, None), (ev, [[0, -1], [1, 0], [-1, -1]], [0, 3]), ([], np.zeros((3, 0)), None)):
        rc, msg = _raw(m, e_, r_, soft, good, partial=p_, fn=fn, target=1)
        assert (rc == bnpp.ERR_INVALID and "context" in msg) or rc == bnpp.ERR_NO_DEVICE, (fn, e_, msg)
    if fn == "posterior":                                   # the target may not be soft, as it may not be evidence
        rc, msg = _raw(m, ev, rows, soft, good, fn=fn, target=5)
        assert rc == bnpp.ERR_INVALID and "target 5 is a soft variable" in msg


def test_a_soft_variable_in_no_factor_is_unsupported_before_the_context():
    d = dict(type="MARKOV", cards=[2, 3, 2, 4], scopes=[[0, 1], [1, 2]], values=[[1.0] * 6, [1.0] * 6])
    m = bnpp.Model.from_dict(d)
    for fn in ("partition", "mpe", "sample", "counts", "marginals"):
        rc, msg = _raw(m, [0], [[0], [1]], [3], np.ones((2, 4)), fn=fn)
        assert rc == bnpp.ERR_UNSUPPORTED and "soft variable 3" in msg and "no factor" in msg, (fn, msg)


def test_python_soft_argument():
    m, d = _load("asia")
    rows = np.array([[0, 1], [1, 0]])
    ok = np.full((2, 4), 0.5)
    for soft in (([2, 5], ok), ([2, 5], [ok[:, :2], ok[:, 2:]]), ([2, 5], ok.tolist())):
        with pytest.raises(bnpp.BnppError) as e:
            bnpp.partition_batch(None, m, [0, 3], rows, soft=soft)
        assert "context" in str(e.value)
    # a wrong shape is a ValueError that says the shape wanted
    for lik in (np.ones((2, 3)), np.ones((3, 4)), np.ones(8), [ok[:, :2], ok[:1, 2:]]):
        with pytest.raises(ValueError) as e:
            bnpp.marginals_batch(None, m, [0, 3], rows, soft=([2, 5], lik))
        assert "(2, " in str(e.value)
    with pytest.raises(ValueError):
        bnpp.partition_batch(None, m, [0, 3], rows, soft=[2, 5, 7])
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.posterior_batch(None, m, [0, 3], rows, 5, soft=([2, 5], ok))
    assert "target 5 is a soft variable" in str(e.value)
    # the plan functions take the ids alone, or what the run calls take, tuple or list
    want = bnpp.plan_batch(m, [0, 3], soft=[2, 5], rows_per_launch=4)
    for soft in (([2, 5], ok), [[2, 5], ok], ([2, 5], None), (2, 5), np.array([2, 5])):
        assert bnpp.plan_batch(m, [0, 3], soft=soft, rows_per_launch=4) == want
    # learn passes it through
    from bnpp import learn
    with pytest.raises(bnpp.BnppError) as e:
        learn.classify(None, m, [0, 3], rows, [1], soft=([2, 5], ok))
    assert "context" in str(e.value)
    with pytest.raises(bnpp.BnppError) as e:
        learn.impute(None, m, [0, 3], rows, soft=([2, 5], -ok))
    assert "row 0" in str(e.value) and "soft variable 2" in str(e.value)


def test_likelihood_file_round_trip(tmp_path):
    m, d = _load("asia")
    rng = np.random.default_rng(5)
    soft = [5, 2]
    lik = soft_ref.random_lik(rng, d["cards"], soft, 7, lo_exp=-60)
    lik[3] = [0.0, 1e300, 5e-324, 1.0]
    p = str(tmp_path / "rows.lik")
    synth.write_likelihoods(soft, lik, p)
    vs, back = bnpp.load_likelihoods(m, p)
    assert vs == soft and back.dtype == np.float64 and np.array_equal(back, lik), "the same doubles"
    ns, nr = C.c_int(), C.c_int64()
    rc = bnpp._lib.bnpp_likelihood_load(m.handle, p.encode(), 0, 0, C.byref(ns), None, C.byref(nr), None)
    assert rc == bnpp.ERR_INVALID and (ns.value, nr.value) == (2, 7), "too small a capacity reports the sizes"
    for text in ("2 5 2\n3\n1 1 1 1\n", "1 9\n1\n1 1\n", "1 2\n1\n0.5 x\n", ""):
        bad = tmp_path / "bad.lik"
        bad.write_text(text)
        with pytest.raises(bnpp.BnppError) as e:
            bnpp.load_likelihoods(m, str(bad))
        assert e.value.status == bnpp.ERR_IO, text
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.load_likelihoods(m, str(tmp_path / "absent.lik"))
    assert e.value.status == bnpp.ERR_IO


def test_cli_refuses_soft_without_a_batch_mode(tmp_path):
    import subprocess
    from conftest import REPO
    exe = os.path.join(REPO, "bn-pp_amd", "bin", "bnpp")
    p = subprocess.run([exe, model_path("asia.uai"), "-pr", "-soft", str(tmp_path / "rows.lik")], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode != 0 and "-soft needs a batch mode" in p.stderr


def test_weighted_gather_reference_on_a_known_table():
    cards = [3, 2, 4]
    src = np.arange(1.0, 25.0)
    t = src.reshape(3, 2, 4)
    # variable 1 hard, variables 0 and 2 soft: out over (0, 2, b)
    ev = np.array([[1, 0]])
    lam = np.array([[1, 2], [1, 3], [1, 5], [1, 7], [1, 11], [1, 13], [1, 17]], dtype=np.float64)   # (Ws = 3 + 4, R = 2)
    out = soft_ref.weighted_gather(src, cards, [0, 1, 2], [1], [], ev, [0, 2], lam).reshape(3, 4, 2)
    assert np.array_equal(out[:, :, 0], t[:, 1, :]), "all ones: the gathered slice"
    want = t[:, 0, :] * np.array([2, 3, 5.0])[:, None] * np.array([7, 11, 13, 17.0])[None, :]
    assert np.array_equal(out[:, :, 1], want)
    # the listed order names the rows of lam, the scope's order the order of the products
    lam2 = np.concatenate([lam[3:], lam[:3]])
    assert np.array_equal(soft_ref.weighted_gather(src, cards, [0, 1, 2], [1], [], ev, [2, 0], lam2).reshape(3, 4, 2), out)
    # in fp32 the order of two roundings shows: (s * a) * b against (s * b) * a
    rng = np.random.default_rng(11)
    s32 = rng.uniform(0.5, 1, 12).astype(np.float32)
    l32 = rng.uniform(0.5, 1, (7, 64)).astype(np.float32)
    got = soft_ref.weighted_gather(s32, [3, 4], [0, 1], [], [], np.zeros((0, 64)), [0, 1], l32).reshape(3, 4, 64)
    a, b = l32[:3].reshape(3, 1, 64), l32[3:].reshape(1, 4, 64)
    first = (s32.reshape(3, 4, 1) * a).astype(np.float32) * b
    other = (s32.reshape(3, 4, 1) * b).astype(np.float32) * a
    assert got.dtype == np.float32 and np.array_equal(got, first) and not np.array_equal(got, other)
    # one-hot and all-ones weights are the masked gather's observed and missing values
    onehot = np.zeros((4, 3))
    onehot[[2, 0, 3], [0, 1, 2]] = 1
    evp = np.array([[1, 0, 1], [2, 0, 3]])
    assert np.array_equal(soft_ref.weighted_gather(src, cards, [0, 1, 2], [1], [], evp[:1], [2], onehot),
                          missing_ref.masked_gather(src, cards, [0, 1, 2], [1, 2], [2], evp))
    assert np.array_equal(soft_ref.weighted_gather(src, cards, [0, 1, 2], [1], [], evp[:1], [2], np.ones((4, 3))),
                          missing_ref.masked_gather(src, cards, [0, 1, 2], [1, 2], [2], np.array([[1, 0, 1], [-1] * 3])))
    # a soft variable outside the scope changes nothing
    assert np.array_equal(soft_ref.weighted_gather(src, cards + [5], [0, 1, 2], [1], [], evp[:1], [3], np.full((5, 3), 9.0)),
                          missing_ref.masked_gather(src, cards, [0, 1, 2], [1], [], evp[:1]))


def test_brute_force_soft_model_and_scaling():
    d = synth.read_uai(model_path("cancer.uai"))
    ev, soft = [0], [3, 1]
    rng = np.random.default_rng(2)
    lik = soft_ref.random_lik(rng, d["cards"], soft, 4)
    lik[1] = [1, 0, 1, 1]                                   # variable 3 observed to be 0, variable 1 unknown
    lik[2, :2] = 0                                          # an all-zero block: an impossible row
    rows = [[1], [0], [1], [0]]
    z, marg, counts = soft_ref.brute(d, ev, rows, soft, lik)
    zh, mh, _ = missing_ref.brute(d, [0, 3], [[0, 0]])
    assert np.isclose(z[1], zh[0], rtol=1e-14) and np.allclose(marg[1][1], mh[1][0]), "a one-hot block is hard evidence"
    assert z[2] == 0 and np.isnan(marg[1][2]).all()
    for f in range(len(d["scopes"])):
        assert np.isclose(counts[f].sum(), 3.0), "every possible row counts once in every factor"
    # the soft model of a row has the row's Z with the hard evidence only, in both dtypes' arithmetic
    lf = soft_ref.lam_factors(d, ev, [], soft)
    for b in (0, 1, 3):
        zm, _, _ = missing_ref.brute(soft_ref.soft_model(d, soft, lf, lik[b]), ev, [rows[b]])
        assert np.isclose(zm[0], z[b], rtol=1e-13)
        z32, _, _ = missing_ref.brute(soft_ref.soft_model(d, soft, lf, lik[b], np.float32), ev, [rows[b]])
        assert np.isclose(z32[0], z[b], rtol=1e-5)
    # the scaling is exact, leaves the largest entry of a block in [0.5, 1) and an all-zero block alone
    sc, e = soft_ref.scale_blocks(d["cards"], soft, lik * 2.0 ** 40)
    assert np.array_equal(np.ldexp(sc[:, :2], 0), sc[:, :2]) and e[2] - 40 == np.frexp(lik[2, 2:].max())[1]
    for i in (0, 2):
        top = sc[:, i:i + 2].max(axis=1)
        assert ((top >= 0.5) & (top < 1) | (top == 0)).all()
    zs, _, _ = soft_ref.brute(d, ev, rows, soft, sc)
    assert np.array_equal(np.ldexp(zs, e)[[0, 1, 3]] > 0, [True] * 3) and np.allclose(np.ldexp(zs, e), z * 2.0 ** 80, rtol=1e-13)


def test_stand_alone_plan_check_program(tmp_path):
    """tests/cpp/soft_plan_check.cpp against the library as built: the program the host code is run under ASan and
    UBSan with (linked against `make sanitize`'s library instead)."""
    import subprocess
    from conftest import REPO
    LIB = os.path.join(REPO, "bn-pp_amd", "lib")
    exe = str(tmp_path / "soft_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests", "cpp", "soft_plan_check.cpp"),
                    "-I" + os.path.join(REPO, "include"), "-L" + LIB, "-lbnpp", "-Wl,-rpath," + LIB, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    args = []
    for name in ("asia", "alarm"):
        args += [model_path(name + ".uai"), str(len(EV_VARS[name]))] + [str(v) for v in EV_VARS[name]]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    word, plans, checks = p.stdout.split()
    assert word == "OK" and int(plans) == 2 * 4 * 2 * 6 * 5 and int(checks) == 2 * 4 * 2 * 7 * 6


@pytest.mark.parametrize("name", ["asia", "cancer"])
def test_restatement_meets_the_bound_on_the_distribution_inputs(name):
    """The numpy restatement alone (sample_ref.run on the row's soft model) for the rows, K and seed of
    test_gpu_soft.py's distribution test: were one of its frequencies outside sample_ref.bound, that test would
    fail on the reference's own noise."""
    import sample_batch_ref as sbr
    import sample_ref
    assert name in sbr.DIST_MODELS
    path = model_path(name + ".uai")
    d = synth.read_uai(path)
    ev, rows, soft, lik = soft_ref.dist_case(d)
    lf = soft_ref.lam_factors(d, ev, [], soft)
    order, _ = bnpp.ordering(bnpp.Model.load(path), {v: 0 for v in ev}, "mf")
    x = np.zeros((rows.shape[0], sbr.DIST_K, len(d["cards"])), dtype=np.uint8)
    for b, row in enumerate(rows):
        sm = soft_ref.soft_model(d, soft, lf, lik[b])
        x[b], deg = sample_ref.run(sm, {v: int(row[j]) for j, v in enumerate(ev)}, order, sbr.DIST_K,
                                   soft_ref.DIST_SEED, np.float64, first=b * sbr.DIST_K)
        assert deg == 0
    assert (x[3][:, soft[0]] == d["cards"][soft[0]] - 1).all(), "a one-hot block pins the variable"
    assert len({int(v) for v in x[0][:, soft[0]]}) == d["cards"][soft[0]], "a soft variable is drawn"
    bad = soft_ref.frequency_violations(d, ev, rows, soft, lik, x)
    assert not bad, bad[:3]
