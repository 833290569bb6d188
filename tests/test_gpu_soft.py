"""GPU tests of soft evidence in batched calls (the _sv entries).

  * the weighted gather alone (bnpp_condition_batch_sv) against
    soft_ref.weighted_gather, bit for bit in both dtypes between guard bands:
    the products come in the scope's order, each rounded once; and the three
    forms of the gather against each other on one table.
  * whole runs against a brute-force joint with the likelihoods as unary
    factors, within the project's own tolerances: 1e-12 (fp64) and 1e-5 (fp32)
    relative for Z, posteriors and marginals, n x those for counts.
  * against the engine's own calls on the per-row soft model (the
    likelihood-carrying factors times the row's weights in the call's dtype):
    fp64 z bit for bit, log10_z within 4 ulp, MPE assignments and sample bytes
    equal in both dtypes.
  * independence of rows per launch / grid cap / split, the job cache, a hidden
    Markov chain against forward, forward-backward and Viterbi written here,
    sampling frequencies, learn.em with noisy labels.
"""
import numpy as np
import pytest
import torch

import bnpp
import missing_ref
import soft_ref
from bnpp import learn, synth
from conftest import model_path
from counts_ref import EV_VARS
from missing_ref import MISSING

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"f64": torch.float64, "f32": torch.float32}
ND = {"f64": np.float64, "f32": np.float32}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
TOL = {"f64": 1e-12, "f32": 1e-5}
GUARD = 16

# cards, scope, evidence variables (rows of the evidence table), the partial ones among them, the soft variables (in
# the order of their blocks of lam)
OPS = [
    dict(name="s_alone", cards=[3], scope=[0], ev=[], partial=[], soft=[0]),                              # rest 3
    dict(name="s_card1", cards=[1], scope=[0], ev=[], partial=[], soft=[0]),                              # rest 1
    dict(name="s_card300", cards=[300, 2], scope=[1, 0], ev=[], partial=[], soft=[0]),                    # rest 600
    dict(name="hard_s", cards=[4, 32], scope=[0, 1], ev=[0], partial=[], soft=[1]),                       # s fastest, rest 32
    dict(name="s_hard", cards=[33, 3], scope=[0, 1], ev=[1], partial=[], soft=[0]),                       # s slowest, rest 33
    dict(name="s_free_hard_free_t", cards=[2, 5, 3, 7, 1], scope=[0, 1, 2, 3, 4], ev=[2], partial=[], soft=[4, 0]),   # rest 70
    dict(name="s_t_adjacent", cards=[3, 4], scope=[0, 1], ev=[], partial=[], soft=[0, 1]),                # rest 12, the order
    dict(name="soft_partial_adjacent", cards=[3, 4, 2], scope=[0, 1, 2], ev=[1, 2], partial=[1], soft=[0]),   # rest 12
    dict(name="partial_soft_hard", cards=[2, 3, 2], scope=[0, 1, 2], ev=[0, 2], partial=[0], soft=[1]),   # rest 6
    dict(name="s_outside_scope", cards=[3, 2, 4], scope=[0, 1], ev=[1], partial=[], soft=[2]),            # the unmasked kernel
]
# one table for the three forms of the gather against each other: R = 5 takes the narrow path, R = 260 the wide one
THREE_FORMS = dict(name="three_forms", cards=[3, 2, 4], scope=[0, 1, 2], ev=[1], partial=[1], soft=[0])
ROWS = [1, 63, 64, 65, 257]
LAMS = ["random", "ones", "onehot", "zeros"]


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


def _load(name):
    return bnpp.Model.load(model_path(name + ".uai")), synth.read_uai(model_path(name + ".uai"))


def _op_lam(op, R, rng, mode, dt):
    """(Ws, R) weights: random in [2^-20, 1], all ones, one-hot per (variable, row), or random with about 40% zeros."""
    cards = op["cards"]
    ws = sum(cards[v] for v in op["soft"])
    lam = np.exp2(rng.uniform(-20, 0, (ws, R)))
    if mode == "ones":
        lam[:] = 1.0
    elif mode == "zeros":
        lam[rng.random((ws, R)) < 0.4] = 0.0
    elif mode == "onehot":
        lam[:] = 0.0
        at = 0
        for v in op["soft"]:
            lam[at + rng.integers(0, cards[v], R), np.arange(R)] = 1.0
            at += cards[v]
    return lam.astype(ND[dt])


def _op_ev(op, R, rng):
    ev = np.stack([rng.integers(0, op["cards"][v], R) for v in op["ev"]]).astype(np.int32) if op["ev"] \
        else np.zeros((0, R), dtype=np.int32)
    for j, v in enumerate(op["ev"]):
        if v in op["partial"]:
            ev[j][rng.random(R) < 0.35] = MISSING
    return ev


def _gather(ctx, stream, op, dt, R, src, ev, lam, partial=None, soft=True, ev_vars=None):
    """The engine's gather of one op between guard bands."""
    cards, scope = op["cards"], op["scope"]
    ev_vars = op["ev"] if ev_vars is None else ev_vars
    partial = op["partial"] if partial is None else partial
    kept = [v for v in scope if v not in ev_vars or v in partial]
    size = int(np.prod([cards[v] for v in kept])) * R
    t_src = torch.tensor(src, dtype=TD[dt], device=DEV)
    t_ev = torch.tensor(np.asarray(ev).reshape(-1), dtype=torch.int32, device=DEV) if len(ev_vars) else None
    t_lam = torch.tensor(lam.reshape(-1), dtype=TD[dt], device=DEV) if soft else None
    buf = torch.full((size + 2 * GUARD,), -7.0, dtype=TD[dt], device=DEV)
    bnpp.condition_batch(ctx, DT[dt], cards, t_src.data_ptr(), scope, ev_vars, R, t_ev.data_ptr() if t_ev is not None else 0,
                         buf[GUARD:].data_ptr(), stream=stream, partial=partial or None,
                         soft=(op["soft"], t_lam.data_ptr()) if soft else None)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == -7.0).all() and (got[GUARD + size:] == -7.0).all(), ("guard band written", op["name"])
    return got[GUARD:GUARD + size]


def _run_op(ctx, stream, op, dt, R, seed, mode="random"):
    cards, scope = op["cards"], op["scope"]
    rng = np.random.default_rng(seed)
    src = rng.uniform(0.05, 1.0, int(np.prod([cards[v] for v in scope]))).astype(ND[dt])
    ev = _op_ev(op, R, rng)
    lam = _op_lam(op, R, rng, mode, dt)
    want = soft_ref.weighted_gather(src, cards, scope, op["ev"], op["partial"], ev, op["soft"], lam)
    return _gather(ctx, stream, op, dt, R, src, ev, lam), want


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), (what, np.flatnonzero(_bits(got) != _bits(want))[:8])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("R", ROWS)
def test_weighted_gather_bit_for_bit(ctx, stream, dt, R):
    for i, op in enumerate(OPS):
        for k, mode in enumerate(LAMS):
            got, want = _run_op(ctx, stream, op, dt, R, 100 + 10 * i + k, mode)
            _same(got, want, (op["name"], dt, R, mode))
            assert not np.signbit(got).any(), "a zero is +0"
        assert want.size == R * int(np.prod([op["cards"][v] for v in op["scope"] if v not in op["ev"] or v in op["partial"]]))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_weighted_gather_wide_path_over_several_row_blocks(ctx, stream, grid_cap, dt):
    """R = 1024 is a multiple of V and spans several blocks of 256 * V rows: the V-wide loads and stores with more than
    one row block, on the full grid and on one workgroup."""
    for cap in (0, 1):
        grid_cap(cap)
        for i, op in enumerate(OPS):
            got, want = _run_op(ctx, stream, op, dt, 1024, 800 + i, "zeros" if i % 2 else "random")
            _same(got, want, (op["name"], dt, 1024, cap))


def test_the_product_order_is_the_scopes(ctx, stream):
    """fp32, two soft dims: (s * a) * b and (s * b) * a differ in some entries; the kernel gives the first."""
    op = OPS[6]
    rng = np.random.default_rng(3)
    src = rng.uniform(0.5, 1, 12).astype(np.float32)
    lam = rng.uniform(0.5, 1, (7, 64)).astype(np.float32)
    got = _gather(ctx, stream, op, "f32", 64, src, np.zeros((0, 64)), lam).reshape(3, 4, 64)
    a, b = lam[:3].reshape(3, 1, 64), lam[3:].reshape(1, 4, 64)
    first = (src.reshape(3, 4, 1) * a).astype(np.float32) * b
    other = (src.reshape(3, 4, 1) * b).astype(np.float32) * a
    assert not np.array_equal(first, other), "the inputs tell the orders apart"
    assert np.array_equal(got, first)
    # listed the other way round the blocks of lam swap, the order of the products stays
    op2 = dict(op, soft=[1, 0])
    got2 = _gather(ctx, stream, op2, "f32", 64, src, np.zeros((0, 64)), np.concatenate([lam[3:], lam[:3]])).reshape(3, 4, 64)
    assert np.array_equal(got2, first)


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_weighted_gather_under_a_capped_grid(ctx, stream, grid_cap, cap):
    grid_cap(cap)
    for dt in ("f64", "f32"):
        for i, op in enumerate(OPS):
            got, want = _run_op(ctx, stream, op, dt, 257, 500 + i)
            _same(got, want, (op["name"], dt, cap))
            got, want = _run_op(ctx, stream, op, dt, 64, 600 + i, "zeros")
            _same(got, want, (op["name"], dt, cap, 64))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_hot_and_all_ones_are_the_masked_gather(ctx, stream, dt):
    """A one-hot block gives the bits of the masked gather with that value observed, an all-ones block those of
    the value missing: hard and missing values are the corners of soft evidence."""
    for i, (op, rows) in enumerate([(op, (64, 65)) for op in OPS[:8]] + [(THREE_FORMS, (5, 260))]):
        for R in rows:
            rng = np.random.default_rng(700 + i)
            cards, scope = op["cards"], op["scope"]
            src = rng.uniform(0.05, 1.0, int(np.prod([cards[v] for v in scope]))).astype(ND[dt])
            ev = _op_ev(op, R, rng)
            vals = np.stack([rng.integers(0, cards[v], R) for v in op["soft"]]).astype(np.int32)
            vals[:, rng.random(R) < 0.3] = MISSING              # these rows: all ones
            if op is THREE_FORMS:
                vals[:, 1:] = MISSING                           # all but the first row: the all-ones corner on its own
            lam = np.zeros((sum(cards[v] for v in op["soft"]), R), dtype=ND[dt])
            at = 0
            for j, v in enumerate(op["soft"]):
                for b in range(R):
                    if vals[j, b] < 0:
                        lam[at:at + cards[v], b] = 1.0
                    else:
                        lam[at + vals[j, b], b] = 1.0
                at += cards[v]
            got = _gather(ctx, stream, op, dt, R, src, ev, lam)
            ev2 = np.concatenate([ev, vals]) if len(op["ev"]) else vals
            masked = _gather(ctx, stream, op, dt, R, src, ev2, None, partial=op["partial"] + op["soft"], soft=False,
                             ev_vars=op["ev"] + op["soft"])
            _same(got, masked, (op["name"], dt, R))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("R", [5, 260])
def test_masked_with_nothing_missing_is_the_plain_gather(ctx, stream, dt, R):
    """One source over cards (3, 2, 4): the masked form with no value missing is the plain gather at the observed digit
    and +0 at the other.  (The weighted form against the masked one on this table: the test above.)"""
    op = THREE_FORMS
    rng = np.random.default_rng(900 + R)
    src = rng.uniform(0.05, 1.0, 24).astype(ND[dt])
    ev = rng.integers(0, 2, (1, R)).astype(np.int32)
    plain = _gather(ctx, stream, op, dt, R, src, ev, None, partial=[], soft=False).reshape(3, 4, R)
    masked = _gather(ctx, stream, op, dt, R, src, ev, None, soft=False)
    want = np.zeros((3, 2, 4, R), dtype=ND[dt])
    for b in range(R):
        want[:, ev[0, b], :, b] = plain[:, :, b]
    assert np.array_equal(plain, src.reshape(3, 2, 4)[:, ev[0], :].transpose(0, 2, 1)), "the plain gather itself"
    _same(masked, want.reshape(-1), ("masked against plain", dt, R))


def test_nine_rest_dims_are_unsupported(ctx, stream):
    cards = [2] * 9
    t = torch.zeros(512 * 4, dtype=torch.float64, device=DEV)
    lam = torch.ones(18 * 4, dtype=torch.float64, device=DEV)
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.condition_batch(ctx, bnpp.F64, cards, t.data_ptr(), list(range(9)), [], 4, 0, t.data_ptr(), stream=stream,
                             soft=(list(range(9)), lam.data_ptr()))
    assert e.value.status == bnpp.ERR_UNSUPPORTED and "separate runs" in str(e.value)


# ---- whole runs against brute force ----

def _rows_of(d, ev, n, seed, frac=0.0, cols=None):
    rng = np.random.default_rng(seed)
    full = np.stack([rng.integers(0, d["cards"][v], n) for v in ev], axis=1) if ev else np.zeros((n, 0), dtype=np.int64)
    return missing_ref.punch(rng, full, frac, cols) if frac else full


def _close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= tol * np.maximum(1.0, np.abs(want[ok]))), \
        (what, np.max(np.abs(got[ok] - want[ok])))


def _free(d, ev, n):
    used = {v for s in d["scopes"] for v in s}
    return [v for v in range(len(d["cards"])) if v not in ev and v in used][:n]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["asia", "cancer", "earthquake", "ising4x4"])
def test_whole_runs_against_brute_force(ctx, name, dt):
    m, d = _load(name)
    tol = TOL[dt]
    ev0 = EV_VARS[name]
    # (rows, evidence variables, partial ones, soft variables): beside hard and partial evidence, and with n_ev = 0
    for n, ev, part, n_soft in ((1, ev0, [], 1), (5, ev0, ev0[-1:], 2), (130, ev0, ev0[-1:], 3), (130, [], [], 2),
                                (5, [], [], 1)):
        free = _free(d, ev0, len(d["cards"]))
        soft = free[:min(n_soft, len(free) - 1)]                # (cancer: two, so that a posterior target is left)
        rng = np.random.default_rng(31 * n + n_soft)
        rows = _rows_of(d, ev, n, 7 * n + n_soft, frac=0.3 if part else 0.0, cols=[ev.index(v) for v in part])
        lik = soft_ref.random_lik(rng, d["cards"], soft, n) * np.exp2(rng.integers(-30, 30, (n, 1)))
        z, marg, counts = soft_ref.brute(d, ev, rows, soft, lik)
        kw = dict(dtype=DT[dt], partial=part or None, soft=(soft, lik))
        lz, gz, _ = bnpp.partition_batch(ctx, m, ev, rows, **kw)
        print(name, dt, n, len(ev), n_soft, "max rel z err", np.max(np.abs(gz - z) / np.maximum(z, 1e-300)))
        assert np.all(np.abs(gz - z) <= tol * z), (name, n)
        ok = z > 0
        assert np.all(np.abs(lz[ok] - np.log10(z[ok])) <= tol * np.maximum(1.0, np.abs(np.log10(z[ok])))), (name, n)
        t = next(v for v in range(m.n_vars) if v not in ev0 and v not in soft)
        post, _ = bnpp.posterior_batch(ctx, m, ev, rows, t, **kw)
        _close(post, marg[t], tol, (name, "posterior", n))
        out, lz2 = bnpp.marginals_batch(ctx, m, ev, rows, **kw)
        _close(out, np.concatenate(marg, axis=1), tol, (name, "marginals", n))
        assert np.array_equal(_bits(lz2), _bits(lz))
        w = rng.uniform(0.5, 2.0, n)
        _, _, wcounts = soft_ref.brute(d, ev, rows, soft, lik, w)
        got, lz3, n_imp = bnpp.expected_counts(ctx, m, ev, rows, weights=w, **kw)
        assert n_imp == int((z == 0).sum())
        for f, c in enumerate(bnpp.split_counts(d, got)):
            assert np.all(np.abs(c - wcounts[f]) <= n * tol * np.maximum(1.0, np.abs(wcounts[f]))), (name, f, n)
            assert abs(c.sum() - w[ok].sum()) <= n * tol * max(1.0, w.sum()), "each factor's counts sum to the possible rows' weight"


def test_an_all_zero_block_makes_the_row_impossible_and_leaves_its_neighbours_alone(ctx):
    m, d = _load("asia")
    ev = EV_VARS["asia"]
    soft = _free(d, ev, 2)
    rng = np.random.default_rng(4)
    rows = _rows_of(d, ev, 9, 11)
    lik = soft_ref.random_lik(rng, d["cards"], soft, 9)
    z0, _, _ = soft_ref.brute(d, ev, rows, soft, lik)
    assert (z0 > 0).all()
    lik2 = lik.copy()
    lik2[4, :d["cards"][soft[0]]] = 0.0
    keep = np.arange(9) != 4
    for dt in ("f64", "f32"):
        kw, kw2 = dict(dtype=DT[dt], soft=(soft, lik)), dict(dtype=DT[dt], soft=(soft, lik2))
        lz, z, _ = bnpp.partition_batch(ctx, m, ev, rows, **kw)
        lz2, z2, _ = bnpp.partition_batch(ctx, m, ev, rows, **kw2)
        assert z2[4] == 0 and np.isneginf(lz2[4])
        assert np.array_equal(_bits(z2[keep]), _bits(z[keep])) and np.array_equal(_bits(lz2[keep]), _bits(lz[keep]))
        out, _ = bnpp.marginals_batch(ctx, m, ev, rows, **kw)
        out2, _ = bnpp.marginals_batch(ctx, m, ev, rows, **kw2)
        blocks = bnpp.split_marginals(d["cards"], None, out2)
        assert np.isnan(blocks[soft[0]][4]).all() and np.array_equal(_bits(out2[keep]), _bits(out[keep]))
        _, _, n_imp = bnpp.expected_counts(ctx, m, ev, rows, **kw2)
        assert n_imp == 1
        lv, x, _ = bnpp.mpe_batch(ctx, m, ev, rows, **kw)
        lv2, x2, _ = bnpp.mpe_batch(ctx, m, ev, rows, **kw2)
        assert np.isneginf(lv2[4]) and np.array_equal(x2[keep], x[keep]) and np.array_equal(_bits(lv2[keep]), _bits(lv[keep]))
        s, _, deg = bnpp.sample_batch(ctx, m, ev, rows, 3, seed=5, **kw)
        s2, slz2, deg2 = bnpp.sample_batch(ctx, m, ev, rows, 3, seed=5, **kw2)
        # every draw degenerate: each of the 3 draws counts every sampled variable (all but the hard evidence)
        assert deg2[4] == 3 * (m.n_vars - len(ev)) and np.isneginf(slz2[4]) and not deg2[keep].any() and np.array_equal(s2[keep], s[keep])


# ---- against the engine's own calls on the per-row soft model ----

def _ulp_close(a, b, n=4):
    return abs(a - b) <= n * np.spacing(abs(b))


@pytest.mark.parametrize("name", ["alarm", "ising6x6", "potts4x5k3"])
def test_rows_equal_the_single_calls_on_the_soft_model(ctx, name):
    m, d = _load(name)
    ev = EV_VARS[name]
    hard, soft = ev[:1], ev[1:]                             # one hard variable, the others given as likelihoods
    rows = _rows_of(d, hard, 6, 21)
    rng = np.random.default_rng(17)
    lik = soft_ref.random_lik(rng, d["cards"], soft, 6)
    lf = bnpp.plan_batch(m, hard, soft=soft)[-1]
    assert lf == soft_ref.lam_factors(d, hard, [], soft)
    seed, K = 9, 4
    got = {}
    for dt in ("f64", "f32"):
        kw = dict(dtype=DT[dt], soft=(soft, lik))
        lz, z, _ = bnpp.partition_batch(ctx, m, hard, rows, **kw)
        lv, x, _ = bnpp.mpe_batch(ctx, m, hard, rows, **kw)
        s, slz, deg = bnpp.sample_batch(ctx, m, hard, rows, K, seed=seed, **kw)
        cnt, _, _ = bnpp.expected_counts(ctx, m, hard, rows, **kw)
        mar, _ = bnpp.marginals_batch(ctx, m, hard, rows, **kw)
        got[dt] = (lz, z, x, s, cnt, mar)
    # one row's block times 2^40: its log10 Z moves by what the exponent gives, and nothing else anywhere
    lik40 = lik.copy()
    lik40[2, :d["cards"][soft[0]]] *= 2.0 ** 40
    lz40, z40, _ = bnpp.partition_batch(ctx, m, hard, rows, soft=(soft, lik40))
    lz, z = got["f64"][0], got["f64"][1]
    pm, pe = np.frexp(z[2])
    assert lz40[2] == np.log10(pm) + float(pe + 40) * np.log10(2.0), "log10_scaled of the same mantissa, the exponent 40 up"
    assert z40[2] == np.ldexp(z[2], 40)
    others = np.arange(6) != 2
    assert np.array_equal(_bits(lz40[others]), _bits(lz[others])) and np.array_equal(_bits(z40[others]), _bits(z[others]))
    mar40, _ = bnpp.marginals_batch(ctx, m, hard, rows, soft=(soft, lik40))
    assert np.array_equal(_bits(mar40), _bits(got["f64"][5])), "marginals do not see the scale"
    cnt40, _, _ = bnpp.expected_counts(ctx, m, hard, rows, soft=(soft, lik40))
    assert np.array_equal(_bits(cnt40), _bits(got["f64"][4])), "counts do not see the scale"
    s40, _, deg40 = bnpp.sample_batch(ctx, m, hard, rows, K, seed=seed, soft=(soft, lik40))
    assert np.array_equal(s40, got["f64"][3]) and not deg40.any(), "nor do the samples"
    _, x40, _ = bnpp.mpe_batch(ctx, m, hard, rows, soft=(soft, lik40))
    assert np.array_equal(x40, got["f64"][2])
    total = {dt: np.zeros_like(got[dt][4]) for dt in got}
    for b, row in enumerate(rows):
        hev = {v: int(row[hard.index(v)]) for v in hard}
        hrow = [[hev[v] for v in hard]]
        for dt in ("f64", "f32"):
            sm = bnpp.Model.from_dict(soft_ref.soft_model(d, soft, lf, lik[b], ND[dt]))
            lz, z, x, s, cnt, mar = got[dt]
            if dt == "f64":
                lz1, z1, _ = bnpp.partition(ctx, sm, hev)
                assert z[b] == z1 and _bits(z[b:b + 1])[0] == _bits(np.array([z1]))[0], (name, b, z[b], z1)
                assert _ulp_close(lz[b], lz1), (name, b, lz[b], lz1)
            _, x1, _ = bnpp.mpe(ctx, sm, hev, dtype=DT[dt])
            assert list(x[b]) == list(x1), (name, dt, b)
            s1, _, _ = bnpp.sample(ctx, sm, K, hev, seed=seed, first_sample=b * K, dtype=DT[dt])
            assert np.array_equal(s[b], s1), (name, dt, b)
            c1, _, _ = bnpp.expected_counts(ctx, sm, hard, hrow, dtype=DT[dt])
            total[dt] += c1
            m1, _ = bnpp.marginals_batch(ctx, sm, hard, hrow, dtype=DT[dt])
            _close(mar[b], m1[0], TOL[dt], (name, dt, b, "marginals"))
    for dt in got:
        cnt = got[dt][4]
        assert np.all(np.abs(cnt - total[dt]) <= len(rows) * TOL[dt] * np.maximum(1.0, np.abs(total[dt]))), (name, dt)


# ---- independence of the launch shape, the job cache ----

def test_results_do_not_depend_on_the_launch_shape_and_the_job_is_cached(ctx, grid_cap):
    m, d = _load("alarm")
    ev = EV_VARS["alarm"]
    hard, soft = ev[:1], ev[1:]
    rows = _rows_of(d, hard, 70, 5)
    rng = np.random.default_rng(6)
    lik = soft_ref.random_lik(rng, d["cards"], soft, 70) * np.exp2(rng.integers(-40, 40, (70, 1)))
    kw = dict(soft=(soft, lik))
    lz, z, _ = bnpp.partition_batch(ctx, m, hard, rows, **kw)
    mar, _ = bnpp.marginals_batch(ctx, m, hard, rows, **kw)
    cnt, _, _ = bnpp.expected_counts(ctx, m, hard, rows, **kw)
    for R in (1, 3, 64):
        lzr, zr, _ = bnpp.partition_batch(ctx, m, hard, rows, rows_per_launch=R, **kw)
        assert np.array_equal(_bits(zr), _bits(z)) and np.array_equal(_bits(lzr), _bits(lz)), R
        marr, _ = bnpp.marginals_batch(ctx, m, hard, rows, rows_per_launch=R, **kw)
        assert np.array_equal(_bits(marr), _bits(mar)), R
        cr, _, _ = bnpp.expected_counts(ctx, m, hard, rows, rows_per_launch=R, **kw)
        assert np.array_equal(_bits(cr), _bits(cnt)), R
    for cap in (1, 2, 3):
        grid_cap(cap)
        lzr, zr, _ = bnpp.partition_batch(ctx, m, hard, rows, **kw)
        assert np.array_equal(_bits(zr), _bits(z)), cap
        marr, _ = bnpp.marginals_batch(ctx, m, hard, rows, **kw)
        assert np.array_equal(_bits(marr), _bits(mar)), cap
        cr, _, _ = bnpp.expected_counts(ctx, m, hard, rows, **kw)
        assert np.array_equal(_bits(cr), _bits(cnt)), cap
    grid_cap(0)
    # a split of the rows over two calls with other likelihoods over the same variables: the second call hits the
    # cached job
    a = bnpp.partition_batch(ctx, m, hard, rows[:30], rows_per_launch=16, soft=(soft, lik[:30]))
    plan_a = bnpp.last_timing()["plan_ms"]
    b = bnpp.partition_batch(ctx, m, hard, rows[30:], rows_per_launch=16, soft=(soft, lik[30:]))
    assert bnpp.last_timing()["plan_ms"] == 0 and plan_a > 0, "the second call reuses the job"
    assert np.array_equal(_bits(np.concatenate([a[1], b[1]])), _bits(z))
    ma, _ = bnpp.marginals_batch(ctx, m, hard, rows[:30], rows_per_launch=16, soft=(soft, lik[:30]))
    mb, _ = bnpp.marginals_batch(ctx, m, hard, rows[30:], rows_per_launch=16, soft=(soft, lik[30:]))
    assert np.array_equal(_bits(np.concatenate([ma, mb])), _bits(mar))
    bnpp.partition_batch(ctx, m, hard, rows[30:], rows_per_launch=16, soft=(soft[:1], lik[30:, :d["cards"][soft[0]]]))
    assert bnpp.last_timing()["plan_ms"] > 0, "another soft variable set is another plan"


# ---- a hidden Markov chain: every state soft, no evidence variable ----

HMM_T, HMM_K = 8, 3


def _hmm(seed):
    """A chain of HMM_T states of card HMM_K: a prior factor, HMM_T - 1 transition factors."""
    rng = np.random.default_rng(seed)
    prior = rng.dirichlet(np.ones(HMM_K))
    trans = [rng.dirichlet(np.ones(HMM_K) * 2.0, HMM_K) for _ in range(HMM_T - 1)]     # trans[t][i, j] = P(x_t+1 = j | x_t = i)
    d = dict(type="MARKOV", cards=[HMM_K] * HMM_T, scopes=[[0]] + [[t, t + 1] for t in range(HMM_T - 1)],
             values=[prior.tolist()] + [a.reshape(-1).tolist() for a in trans])
    return d, prior, trans


def _emissions(seed, n):
    """Gaussian emission likelihoods N(y_t; mu_k, 1) of seeded observations -> (n, HMM_T, HMM_K)."""
    rng = np.random.default_rng(seed)
    mu = np.array([-2.0, 0.0, 2.5])
    states = rng.integers(0, HMM_K, (n, HMM_T))
    y = mu[states] + rng.normal(0, 1.0, (n, HMM_T))
    return np.exp(-0.5 * (y[:, :, None] - mu[None, None, :]) ** 2) / np.sqrt(2 * np.pi)


def _forward_backward(prior, trans, em):
    """-> (log10 Z, the (T, K) state marginals, the (T - 1, K, K) pairwise marginals), scaled per step."""
    T = em.shape[0]
    alpha, c = np.zeros((T, HMM_K)), np.zeros(T)
    a = prior * em[0]
    for t in range(T):
        if t:
            a = (alpha[t - 1] @ trans[t - 1]) * em[t]
        c[t] = a.sum()
        alpha[t] = a / c[t]
    beta = np.ones((T, HMM_K))
    for t in range(T - 2, -1, -1):
        beta[t] = trans[t] @ (em[t + 1] * beta[t + 1]) / c[t + 1]
    gamma = alpha * beta
    xi = np.stack([alpha[t][:, None] * trans[t] * (em[t + 1] * beta[t + 1])[None, :] / c[t + 1] for t in range(T - 1)])
    return np.log10(c).sum(), gamma, xi


def _viterbi(prior, trans, em):
    """-> (log of the best path's weight, the path, the gap to the second-best path's log weight)."""
    import itertools
    T = em.shape[0]
    lp, back = np.log(prior) + np.log(em[0]), []
    for t in range(1, T):
        cand = lp[:, None] + np.log(trans[t - 1]) + np.log(em[t])[None, :]
        back.append(np.argmax(cand, axis=0))
        lp = cand.max(axis=0)
    path = [int(np.argmax(lp))]
    for bk in reversed(back):
        path.append(int(bk[path[-1]]))
    path = path[::-1]
    # the second-best path: all K^T of them (6561), in plain numpy
    paths = np.array(list(itertools.product(range(HMM_K), repeat=T)))
    lw = np.log(prior)[paths[:, 0]] + np.log(em[0])[paths[:, 0]]
    for t in range(1, T):
        lw = lw + np.log(trans[t - 1])[paths[:, t - 1], paths[:, t]] + np.log(em[t])[paths[:, t]]
    top = np.sort(lw)
    assert list(paths[np.argmax(lw)]) == path and np.isclose(top[-1], lp.max())
    return lp.max(), path, top[-1] - top[-2]


@pytest.mark.parametrize("n", [5, 130])
def test_hidden_markov_chain(ctx, n):
    d, prior, trans = _hmm(40)
    m = bnpp.Model.from_dict(d)
    em = _emissions(41 + n, n)
    soft = list(range(HMM_T))
    lik = em.reshape(n, HMM_T * HMM_K)
    ref = [_forward_backward(prior, trans, em[b]) for b in range(n)]
    vit = [_viterbi(prior, trans, em[b]) for b in range(n)]
    # a condition on the inputs, met by the numpy code alone: no sequence has two best paths within 1e-6
    assert min(v[2] for v in vit) > 1e-6, "the seeded emissions leave a gap between the best and the second-best path"
    rows = np.zeros((n, 0), dtype=np.int64)
    for dt in ("f64", "f32"):
        tol = TOL[dt]
        kw = dict(dtype=DT[dt], soft=(soft, lik))
        lz, z, _ = bnpp.partition_batch(ctx, m, [], rows, **kw)
        want_lz = np.array([r[0] for r in ref])
        assert np.all(np.abs(lz - want_lz) <= tol * np.maximum(1.0, np.abs(want_lz))), (dt, np.max(np.abs(lz - want_lz)))
        out, lz2 = bnpp.marginals_batch(ctx, m, [], rows, **kw)
        _close(out, np.stack([r[1].reshape(-1) for r in ref]), tol, (dt, "forward-backward"))
        lv, x, _ = bnpp.mpe_batch(ctx, m, [], rows, **kw)
        assert np.array_equal(x, np.array([v[1] for v in vit])), (dt, "Viterbi")
        want_lv = np.array([v[0] for v in vit]) / np.log(10.0)
        assert np.all(np.abs(lv - want_lv) <= tol * np.maximum(1.0, np.abs(want_lv)))
        cnt, _, n_imp = bnpp.expected_counts(ctx, m, [], rows, **kw)
        assert n_imp == 0
        got = bnpp.split_counts(d, cnt)
        _close(got[0], sum(r[1][0] for r in ref), n * tol, (dt, "the first state's counts"))
        for t in range(HMM_T - 1):
            _close(got[1 + t], sum(r[2][t] for r in ref), n * tol, (dt, "expected transitions", t))


# ---- sampling frequencies ----

@pytest.mark.parametrize("name", ["asia", "cancer"])
def test_sampling_distribution_with_a_soft_variable(ctx, name):
    """8 rows, one soft variable beside the evidence, 4096 draws each from disjoint streams: every single-variable
    frequency of every row within sample_ref.bound of the brute-force posterior with the row's likelihoods.
    (test_soft_host.py puts the same bound on the numpy restatement alone.)"""
    import sample_batch_ref as sbr
    m, d = _load(name)
    ev, rows, soft, lik = soft_ref.dist_case(d)
    x, lz, deg = bnpp.sample_batch(ctx, m, ev, rows, sbr.DIST_K, seed=soft_ref.DIST_SEED, soft=(soft, lik))
    assert not deg.any() and np.isfinite(lz).all()
    for b in range(rows.shape[0]):
        assert (x[b][:, np.array(ev)] == rows[b]).all()
    assert (x[3][:, soft[0]] == d["cards"][soft[0]] - 1).all(), "a one-hot block pins the variable"
    bad = soft_ref.frequency_violations(d, ev, rows, soft, lik, x)
    assert not bad, bad[:3]


# ---- learn.em with noisy labels ----

def test_em_with_noisy_label_likelihoods(ctx):
    m, d = _load("cancer")
    nv = m.n_vars
    n = 200
    full, _, _ = bnpp.sample(ctx, m, n, seed=3)
    noisy = 1                                               # this variable is known only through a noisy label
    ev = [v for v in range(nv) if v != noisy]
    rows = full[:, ev].astype(np.int64)
    rng = np.random.default_rng(8)
    k = d["cards"][noisy]
    flip = rng.random(n) < 0.2
    label = np.where(flip, rng.integers(0, k, n), full[:, noisy])
    lik = np.full((n, k), 0.2 / k)
    lik[np.arange(n), label] += 0.8                         # P(label | value)
    cur, lls = d, []
    for it in range(3):
        counts, lz, n_imp = bnpp.expected_counts(ctx, bnpp.Model.from_dict(cur), ev, rows, soft=([noisy], lik))
        z, _, want = soft_ref.brute(cur, ev, rows, [noisy], lik)
        for f, c in enumerate(bnpp.split_counts(cur, counts)):
            assert np.all(np.abs(c - want[f]) <= n * 1e-12 * np.maximum(1.0, np.abs(want[f]))), (it, f)
        assert np.allclose(lz[z > 0], np.log10(z[z > 0]), rtol=1e-12, atol=1e-12)
        lls.append(float(lz[np.isfinite(lz)].sum()))
        cur = learn.m_step(cur, counts)
    fit, lls2 = learn.em(ctx, d, ev, rows, 3, soft=([noisy], lik))
    assert np.allclose(lls2, lls, rtol=1e-12)
    # "does not decrease" up to the rounding of the sum: n rows, each log10 Z within the project's fp64 tolerance
    slack = n * 1e-12 * max(1.0, float(np.max(np.abs(lz[np.isfinite(lz)]))))
    assert all(b >= a - slack for a, b in zip(lls, lls[1:])), lls
    assert np.allclose(np.concatenate(fit["values"]), np.concatenate(cur["values"]), rtol=1e-12, atol=1e-300)
    # classify reads a soft target's posterior with its likelihoods included; impute draws it
    lab, out = learn.classify(ctx, m, ev, rows, [noisy], soft=([noisy], lik))
    _, marg, _ = soft_ref.brute(d, ev, rows, [noisy], lik)
    _close(out, marg[noisy], 1e-12, "a soft target")
    s = learn.impute(ctx, m, ev, rows, k=2, seed=4, soft=([noisy], lik))
    assert np.array_equal(s[:, 0, :][:, ev], rows) and (s[:, :, noisy] < k).all()


# ---- front ends ----

def _front_end_case(tmp_path):
    ev = EV_VARS["asia"]
    rows = np.array([[0, 1, MISSING, 0], [MISSING, MISSING, 1, 1], [MISSING, MISSING, MISSING, MISSING],
                     [1, 0, 0, MISSING], [1, 1, 1, 0]])
    soft = [5, 2]
    lik = soft_ref.random_lik(np.random.default_rng(12), [2] * 8, soft, 5) * 3.0
    evid = tmp_path / "mixed.evid"
    lines = [str(len(rows))]
    for row in rows:
        obs = [(v, int(x)) for v, x in zip(ev, row) if x >= 0]
        lines.append(" ".join([str(len(obs))] + ["%d %d" % p for p in obs]))
    evid.write_text("\n".join(lines) + "\n")
    likf = tmp_path / "rows.lik"
    synth.write_likelihoods(soft, lik, str(likf))
    return ev, rows, soft, lik, str(evid), str(likf)


def test_cli_with_soft(ctx, tmp_path):
    import os
    import subprocess
    from conftest import REPO
    m, d = _load("asia")
    ev, rows, soft, lik, evid, likf = _front_end_case(tmp_path)
    assert bnpp.load_likelihoods(m, likf)[0] == soft
    exe = os.path.join(REPO, "bn-pp_amd", "bin", "bnpp")
    base = str(tmp_path / "out")
    p = subprocess.run([exe, model_path("asia.uai"), evid, "-pr-batch", "-mar-batch", "-missing", "-soft", likf, "-mf",
                        "-uai", base], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lz, _, _ = bnpp.partition_batch(ctx, m, ev, rows, partial=ev, soft=(soft, lik))
    pr = open(base + ".PR").read().split()
    assert pr[:2] == ["PR", "5"] and np.array_equal(_bits(np.array([float(x) for x in pr[2:]])), _bits(lz))
    lz0, _, _ = bnpp.partition_batch(ctx, m, ev, rows, partial=ev)
    assert not np.array_equal(_bits(lz0), _bits(lz)), "the likelihoods count"
    out, _ = bnpp.marginals_batch(ctx, m, ev, rows, partial=ev, soft=(soft, lik))
    lines = open(base + ".MAR").read().split("\n")
    assert lines[:2] == ["MAR", "5"]
    for b in range(5):
        f = lines[2 + b].split()
        vals, at = [], 1
        for c in d["cards"]:
            assert int(f[at]) == c
            vals += [float(x) for x in f[at + 1:at + 1 + c]]
            at += 1 + c
        assert np.array_equal(_bits(np.array(vals)), _bits(out[b])), b
    short = tmp_path / "short.lik"
    synth.write_likelihoods(soft, lik[:4], str(short))
    p = subprocess.run([exe, model_path("asia.uai"), evid, "-pr-batch", "-missing", "-soft", str(short)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "4 rows of likelihoods for 5 evidence rows" in p.stderr


def test_cpp_mirror_overloads(ctx, tmp_path):
    import os
    import subprocess
    from conftest import REPO
    LIB = os.path.join(REPO, "bn-pp_amd", "lib")
    exe = str(tmp_path / "soft_check")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests", "cpp", "soft_check.cpp"),
                    "-I" + os.path.join(REPO, "include"), "-L" + LIB, "-lbnpp", "-Wl,-rpath," + LIB, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    m, d = _load("asia")
    ev, rows, soft, lik, evid, likf = _front_end_case(tmp_path)
    p = subprocess.run([exe, model_path("asia.uai"), evid, likf], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    got = p.stdout.strip().split("\n")
    kw = dict(partial=ev, soft=(soft, lik))
    out, lz = bnpp.marginals_batch(ctx, m, ev, rows, **kw)
    _, x, _ = bnpp.mpe_batch(ctx, m, ev, rows, **kw)
    s, _, _ = bnpp.sample_batch(ctx, m, ev, rows, 1, seed=5, **kw)
    cnt, _, _ = bnpp.expected_counts(ctx, m, ev, rows, **kw)
    post, _ = bnpp.posterior_batch(ctx, m, ev, rows, 1, **kw)
    for b in range(5):
        f = got[b].split()
        assert f[0] == "Z" and f[2] == "|"
        assert np.array_equal(_bits(np.array([float(f[1])] + [float(v) for v in f[3:]])),
                              _bits(np.concatenate([[lz[b]], out[b]]))), b
        assert got[5 + b].split() == ["X"] + [str(int(v)) for v in x[b]]
        assert got[10 + b].split() == ["S"] + [str(int(v)) for v in s[b, 0]]
        assert np.array_equal(_bits(np.array([float(v) for v in got[15 + b].split()[1:]])), _bits(post[b]))
    flat = [float(v) for line in got[20:] for v in line.split()[1:]]
    assert len(got) == 20 + m.n_factors and np.array_equal(_bits(np.array(flat)), _bits(cnt))
