"""Message-sliced bucket-tree marginals (bnpp_marginals_tree_sliced)
in in-process worlds of R = 2..16 ranks (tests/sliced_world.py: one thread and
one context per rank, a Python collective), so that every exchange kernel of
xchg.hip runs with real, non-identical rank data under a numerical assertion:
the 8-way and the runtime-R (R = 16) transposes, the scalar branches behind
inner % 4 != 0 and the fp32 vector tail of the same-order pack, the per-block
ldexp / clamp_shift / all-zero-block arithmetic with ranks at different
scales, and the two-lane schedule under a stream-ordered exchange.
tests/test_host.py::test_plan_tree_sliced_shapes_the_world_tests_rely_on pins
the plan shapes that put these cases on those branches.

Tolerances (largest absolute difference over all marginal entries):
  * a sliced result against the one-rank bnpp.marginals_tree of the same order
    and dtype: 2e-6 (fp32), 1e-12 (fp64) -- tests/test_gpu_sliced.py's, for its
    reason (the slice variables are summed last, across ranks, in fp64);
  * fp32 sliced against the fp64 one-rank tree: max(2e-6, 4 d), d the distance
    of the fp32 one-rank tree from the fp64 one -- set by the reference pair;
  * fp64 against the CPU oracle (refcpu, per-target VE) at four targets of the
    smallest models: 1e-12.

Not reached by the planner on any column-sweep grid (see the host test): the
mode-1 unpack (xchg_unpack_kernel with x_t < 0).  The transposing pack with an
inner size that is no multiple of 4 is reached (FAST_SLICE_WORLDS).
"""
import threading

import pytest

import bnpp
import refcpu
import sliced_world as sw
from bnpp import synth

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(bnpp.F32, id="f32"), pytest.param(bnpp.F64, id="f64")]
TOL = {bnpp.F32: 2e-6, bnpp.F64: 1e-12}

_models = {}      # key -> (dict, bnpp.Model, rows, cols)
_trees = {}       # (key, dtype, evidence) -> one-rank bucket-tree marginals
_worlds = {}      # (key, R, dtype, evidence) -> (results, record) of a staged run


def _key(x):
    return tuple(tuple(p) if isinstance(p, (list, dict)) else p for p in x)


def _model(kind, *args):
    """("ising", rows, cols) / ("mixed", row_cards, cols) / ("peaked", rows, cols)
    / ("tilt", rows, cols, R, log2) / ("tiltmixed", row_cards, cols, log2) / ("zero", rows, cols, R)
    -> (key, dict, Model, rows, cols)"""
    key = _key((kind,) + args)
    if key not in _models:
        if kind == "ising":
            rows, cols = args
            d = synth.ising_grid(rows, cols, seed=5)
        elif kind == "mixed":
            rows, cols = len(args[0]), args[1]
            d = sw.mixed_grid(list(args[0]), cols)
        elif kind == "peaked":
            rows, cols = args
            d = synth.peaked_grid(rows, cols, log2_eps=10)
        elif kind == "tilt":
            rows, cols, R, log2 = args
            base = synth.ising_grid(rows, cols, seed=5)
            tilt_rows = _slice_rows(base, rows, cols, R)
            d = sw.with_unary(base, {i * cols + j: [1.0, 2.0 ** -log2] for i in tilt_rows for j in range(cols)})
        elif kind == "tiltmixed":
            row_cards, cols, log2 = list(args[0]), args[1], args[2]
            rows = len(row_cards)
            d = sw.mixed_grid(row_cards, cols, unary={i * cols + j: [1.0, 2.0 ** -log2] for i in range(rows)
                                                      if row_cards[i] == 2 for j in range(cols)})
        elif kind == "zero":
            rows, cols, R = args
            base = synth.ising_grid(rows, cols, seed=5)
            d = sw.with_unary(base, {_slice_var(base, rows, cols, R): [1.0, 0.0]})
        else:
            raise ValueError(kind)
        _models[key] = (d, bnpp.Model.from_dict(d), rows, cols)
    return (key,) + _models[key]


def _slice_targets(d, rows, cols, R):
    """The variables the plan delivers as slice variables (host-only plan)."""
    sb, _ = bnpp.plan_tree_sliced(bnpp.Model.from_dict(d), 0, R, order=sw.column_order(rows, cols))
    return [v for v, b in enumerate(sb) if b >= 0]


def _slice_rows(d, rows, cols, R):
    return sorted({v // cols for v in _slice_targets(d, rows, cols, R)})


def _slice_var(d, rows, cols, R):
    sl = _slice_targets(d, rows, cols, R)
    return sl[len(sl) // 2]


def _tree(ctx, key, m, rows, cols, dtype, ev=None):
    k = (key, dtype, _key(sorted((ev or {}).items())))
    if k not in _trees:
        _trees[k], _ = bnpp.marginals_tree(ctx, m, ev or {}, "mf", dtype, order=sw.column_order(rows, cols, ev))
    return _trees[k]


def _staged(key, m, rows, cols, R, dtype, ev=None):
    k = (key, R, dtype, _key(sorted((ev or {}).items())))
    if k not in _worlds:
        _worlds[k] = sw.run_world(m, R, dtype, sw.column_order(rows, cols, ev), ev, "staged")
    return _worlds[k]


def _check(ctx, key, d, m, rows, cols, R, dtype, ev=None, skip=()):
    """The staged world's combined marginals against the one-rank tree(s) ->
    (marginals, record)."""
    res, rec = _staged(key, m, rows, cols, R, dtype, ev)
    assert rec["calls"] > 0 and len(rec["sync"]) > 0
    for rk in res:
        for t, v in rk[0][0].items():
            assert all(x == x and 0.0 <= x < float("inf") for x in v), (t, v)
    got = sw.combine(m, res)
    same = sw.max_abs_diff(got, _tree(ctx, key, m, rows, cols, dtype, ev), skip)
    print("R=%d dtype=%d: %d exchanges, |sliced - tree| = %.3g" % (R, dtype, rec["calls"], same))
    assert same <= TOL[dtype], same
    if dtype == bnpp.F32:
        t64 = _tree(ctx, key, m, rows, cols, bnpp.F64, ev)
        dist = sw.max_abs_diff(_tree(ctx, key, m, rows, cols, bnpp.F32, ev), t64, skip)
        far = sw.max_abs_diff(got, t64, skip)
        print("  |tree32 - tree64| = %.3g, |sliced32 - tree64| = %.3g" % (dist, far))
        assert far <= max(2e-6, 4 * dist), (far, dist)
    return got, rec


def _oracle_spot(d, got, targets):
    om = refcpu.Model.from_dict(d)
    for t in targets:
        ref = om.marginal(t)
        worst = max(abs(x - y) for x, y in zip(got[t], ref))
        assert worst <= 1e-12, (t, worst)


# ---- (a) world sizes ----

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,R", sw.ISING_WORLDS)
def test_world_sizes(ctx, rows, cols, R, dtype):
    """Ising grids (seed 5) at R = 2, 4, 8 and 16 -- the 8-way vector
    transposes and, at R = 16, the runtime-R kernels (blocks=16, 4096-entry
    messages); 10x10 at R = 2 and 11x11 at R = 4 reach inner sizes 4 and 1 and
    are also checked against the CPU oracle at a corner, a slice-row variable,
    a centre variable and a last-column variable."""
    key, d, m, rows, cols = _model("ising", rows, cols)
    got, _ = _check(ctx, key, d, m, rows, cols, R, dtype)
    if rows < 16 and dtype == bnpp.F64:
        centre = (rows // 2) * cols + cols // 2
        _oracle_spot(d, got, [0, _slice_var(d, rows, cols, R), centre, (rows // 2) * cols + cols - 1])


# ---- (b) inner sizes that are no multiple of 4 ----

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_cards,cols,R", sw.MIXED_WORLDS + sw.FAST_SLICE_WORLDS)
def test_mixed_grids(ctx, row_cards, cols, R, dtype):
    """Card-3 rows beside the binary slice rows.  MIXED_WORLDS: same-order
    packs of 13122 / 4374 entries (an fp32 vector tail of 2) and unpacks whose
    inner sizes 13122, 4374, 1458 and 18 take the scalar branch, beside
    46656-entry unpacks on the vector branch.  FAST_SLICE_WORLDS: a transposing
    pack with inner sizes 4374, 729 and 162.  The R = 2 model is spot-checked
    against the CPU oracle (its slice variables live in the two binary rows)."""
    key, d, m, rows, cols = _model("mixed", row_cards, cols)
    got, _ = _check(ctx, key, d, m, rows, cols, R, dtype)
    if (row_cards, R) == sw.MIXED_WORLDS[0][::2] and dtype == bnpp.F64:
        _oracle_spot(d, got, [0, (rows - 1) * cols + cols // 2, (rows // 2) * cols + cols // 2,
                              (rows // 2) * cols + cols - 1])


# ---- (c) ranks at diverging scales ----

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R", [4, 8])
def test_tilted_ranks_rescale_across_a_wide_spread(ctx, R, dtype):
    """Every unary table of the rows that supply slice variables is
    [1, 2^-40] (12x14 Ising grid): a rank's block shrinks by 2^-40 per set bit,
    so the gathered exp2_r differ widely and the pack / unpack shifts are
    large and different per source block.  Coverage: some exchange gathers
    exp2_r with a spread >= 20.  Observed on an MI355X (record["sync"]): a
    largest spread of 85 at R = 4 (fp32 and fp64), 124 (fp32) and 128 (fp64)
    at R = 8; no gathered E_r is -2^40."""
    key, d, m, rows, cols = _model("tilt", 12, 14, R, 40)
    _, rec = _check(ctx, key, d, m, rows, cols, R, dtype)
    spread = sw.exp2_spread(rec["sync"])
    print("tilted R=%d dtype=%d: exp2 spread %d" % (R, dtype, spread))
    assert spread >= 20, spread


@pytest.mark.parametrize("dtype", DTYPES)
def test_tilted_ranks_on_the_scalar_branches(ctx, dtype):
    """The tilt on a card-3 grid (MIXED_WORLDS[2] at R = 8, [1, 2^-40] on every
    binary row, the only rows that can supply slice variables): the wide
    per-block shifts also go through the scalar unpack (inner 1458) and the
    same-order pack with an fp32 tail.  Coverage: an exp2 spread >= 20."""
    row_cards, cols, R = sw.MIXED_WORLDS[2]
    key, d, m, rows, cols = _model("tiltmixed", row_cards, cols, 40)
    _, rec = _check(ctx, key, d, m, rows, cols, R, dtype)
    spread = sw.exp2_spread(rec["sync"])
    print("tilted mixed R=%d dtype=%d: exp2 spread %d" % (R, dtype, spread))
    assert spread >= 20, spread


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R", [4, 8])
def test_zero_block_rank(ctx, R, dtype):
    """One slice-row variable v has the unary table [1, 0] (a factor value, not
    evidence): the ranks whose bit of v is 1 hold all-zero blocks while v is a
    slice variable, so xchg_sync_kernel reports E_r = -2^40 (kNoExp) and the
    common exponent must come from the other ranks.  v's marginal is exactly
    [1, 0]; all others meet the tolerances.  Observed on an MI355X: one gather
    holds E_r = -2^40 (of 32 at R = 4, of 34 at R = 8), in both dtypes."""
    key, d, m, rows, cols = _model("zero", 12, 14, R)
    v = _slice_var(synth.ising_grid(12, 14, seed=5), 12, 14, R)
    assert d["values"][v] == [1.0, 0.0]
    got, rec = _check(ctx, key, d, m, rows, cols, R, dtype, skip=(v,))
    n_zero = sum(1 for pairs in rec["sync"] if any(e == bnpp.NO_EXP for e, _ in pairs))
    print("zero block R=%d dtype=%d: %d of %d gathers hold E_r = -2^40" % (R, dtype, n_zero, len(rec["sync"])))
    assert n_zero > 0
    assert got[v] == [1.0, 0.0], got[v]


@pytest.mark.parametrize("R", [4, 8])
def test_deep_tilt_flushes_small_blocks_fp32(ctx, R):
    """[1, 2^-200] on the same rows in fp32: the small blocks lie below what
    fp32 holds beside the large ones and flush to zero; every share stays
    finite and non-negative (checked for every run in _check) and the
    marginals meet the fp32-against-fp64 bound.  Coverage: some gathered E_r
    is -2^40 (a flushed block).  Observed on an MI355X: 13 of 32 gathers at
    R = 4 and 13 of 34 at R = 8 hold E_r = -2^40; among the non-zero blocks the
    exp2 spread is 8 and 9."""
    key, d, m, rows, cols = _model("tilt", 12, 14, R, 200)
    _, rec = _check(ctx, key, d, m, rows, cols, R, bnpp.F32)
    n_zero = sum(1 for pairs in rec["sync"] if any(e == bnpp.NO_EXP for e, _ in pairs))
    print("deep tilt R=%d: exp2 spread %d, %d of %d gathers hold E_r = -2^40"
          % (R, sw.exp2_spread(rec["sync"]), n_zero, len(rec["sync"])))
    assert n_zero > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_peaked_grid_carries_large_rescales(ctx, dtype):
    """synth.peaked_grid(12, 14, log2_eps=10) at R = 4: every fused run rescales
    by hundreds of binary orders, and the exchanges carry those exponents."""
    key, d, m, rows, cols = _model("peaked", 12, 14)
    _, rec = _check(ctx, key, d, m, rows, cols, 4, dtype)
    print("peaked: exp2 from %d to %d" % (min(x for p in rec["sync"] for _, x in p),
                                          max(x for p in rec["sync"] for _, x in p)))


# ---- (d) stream-ordered exchange ----

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,shape,cols,R", [("ising", 16, 16, 4), ("ising", 16, 16, 8),
                                               ("mixed", sw.MIXED_WORLDS[2][0], 14, 8)])
def test_stream_ordered_exchange_is_bit_identical(kind, shape, cols, R, dtype):
    """The exchange as RCCL shapes it: enqueued on the lane's stream, ordered
    by cross-context events, no host wait on the GPU -- the two lanes'
    alternating windows (lane_order.hpp) run ahead of the data.  The data and
    the arithmetic are those of the staged run, so every rank's mantissas and
    exponents are bit-identical to it."""
    key, d, m, rows, cols = _model(kind, shape, cols)
    staged, _ = _staged(key, m, rows, cols, R, dtype)
    streamed, rec = sw.run_world(m, R, dtype, sw.column_order(rows, cols), None, "stream")
    assert rec["calls"] > 0
    for r in range(R):
        assert streamed[r][0][1] == staged[r][0][1], r        # exponents
        assert streamed[r][0][0] == staged[r][0][0], r        # mantissas


# ---- (e) relaunch ----

@pytest.mark.parametrize("collective", ["staged", "stream"])
def test_relaunch_of_the_planned_job(collective):
    """The identical call again on every rank of a world of 8 relaunches the
    planned job (plan_ms == 0.0) and returns identical bits."""
    key, d, m, rows, cols = _model("ising", 16, 16)
    res, _ = sw.run_world(m, 8, bnpp.F32, sw.column_order(rows, cols), None, collective, calls=2)
    for r in range(8):
        (m1, e1, p1), (m2, e2, p2) = res[r]
        assert p1 > 0.0 and p2 == 0.0, (r, p1, p2)
        assert m2 == m1 and e2 == e1, r


# ---- (f) evidence ----

def test_evidence_world_of_8(ctx):
    """tests/test_gpu_sliced.py's evidence case (12x20, fp64, evidence that
    keeps the column sweep a chain) taken from 4 to 8 ranks."""
    ev = {220: 1, 239: 0}
    key, d, m, rows, cols = _model("ising", 12, 20)
    _check(ctx, key, d, m, rows, cols, 8, bnpp.F64, ev)


# ---- (g) a failing collective ----

def test_failing_collective_ends_every_rank(ctx):
    """Rank 1's callback raises on its third call (a host-side error return; no
    GPU work fails): the barrier is aborted, every rank's call ends with an
    exception well inside the barrier timeout, the library reports "the
    exchange collective failed" on every rank's thread, and a normal world run
    straight afterwards in the same process passes."""
    import time
    key, d, m, rows, cols = _model("ising", 11, 11)
    R, order = 4, sw.column_order(11, 11)
    t0 = time.monotonic()
    with pytest.raises(sw.WorldError) as e:
        sw.run_world(m, R, bnpp.F64, order, None, "staged", fail=(1, 3))
    assert time.monotonic() - t0 < sw.BARRIER_TIMEOUT_S / 2
    errs = e.value.errors
    assert isinstance(errs[1], sw.InjectedFailure) and isinstance(e.value.__cause__, sw.InjectedFailure)
    for r in range(R):
        assert errs[r] is not None, r
        assert r == 1 or isinstance(errs[r], threading.BrokenBarrierError), errs
        assert "the exchange collective failed" in e.value.last_error[r], e.value.last_error
    res, _ = sw.run_world(m, R, bnpp.F64, order, None, "staged")
    assert sw.max_abs_diff(sw.combine(m, res), _tree(ctx, key, m, rows, cols, bnpp.F64)) <= 1e-12
