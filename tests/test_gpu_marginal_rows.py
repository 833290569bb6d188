"""GPU tests of the batched-marginals emit kernel alone: bnpp_bucket_marginal_rows
on caller-owned buffers against the numpy restatement
(marginals_batch_ref.emit_rows), bit for bit in fp64 and fp32, with guard bands
around `out` that must stay untouched."""
import numpy as np
import pytest
import torch

import bnpp
import marginals_batch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"f64": torch.float64, "f32": torch.float32}
ND = {"f64": np.float64, "f32": np.float32}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
GUARD = 24

# kind per target: "b" a belief with the row dimension, "n" a belief without, "e" evidence, "f" free.
# The emit kernel's tile holds 16 columns and its four waves split the targets: W = 2 (one wave), 11, 80 (every
# wave, several tiles each), 300 (one target through the tile in 19 chunks) and a list of every kind
LISTS = {
    "one": ([2], "b"),
    "three": ([3, 1, 7], "bbb"),
    "forty": ([2] * 40, "b" * 40),
    "wide": ([300], "b"),
    "mixed": ([4, 3, 2, 6, 5, 64, 3, 17, 2], "bnefbbenb"),
}
ROWS = [1, 63, 64, 65, 257]


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


def _run(ctx, stream, name, dt, R, seed, live=None, zero=None, wild_ev=False):
    cards, kinds = LISTS[name]
    rng = np.random.default_rng(seed)
    live = R if live is None else live
    W = sum(cards)
    n_ev = max(kinds.count("e"), 1)
    ev = np.stack([rng.integers(0, 2, R) for _ in range(n_ev)]).astype(np.int32)
    tables, has_b, ev_row, e = [], [], [], 0
    for k, kind in zip(cards, kinds):
        if kind in "bn":
            t = rng.uniform(0.05, 1.0, k * (R if kind == "b" else 1)).astype(ND[dt])
            if dt == "f32":
                t *= np.float32(2.0 ** -100)                # a table's scale cancels; fp32 values convert exactly
            tables.append(t)
            has_b.append(kind == "b")
            ev_row.append(-1)
        else:
            tables.append(None)
            has_b.append(False)
            ev_row.append(e if kind == "e" else -1)
            if kind == "e":
                ev[e] = rng.integers(0, k, R)
                if wild_ev:                                 # out of range: clamped
                    ev[e][::3] = k + 5
                    ev[e][1::3] = -2
                e += 1
    if zero is not None:                                    # (target, row): its column of that target all 0
        j, b = zero
        tables[j].reshape(cards[j], R)[:, b] = 0
    want = marginals_batch_ref.emit_rows(np.full((R, W), -7.0), cards, tables, has_b, ev_row, R, live, ev)
    dev = [torch.tensor(t, dtype=TD[dt], device=DEV) if t is not None else None for t in tables]
    t_ev = torch.tensor(ev.reshape(-1), dtype=torch.int32, device=DEV)
    buf = torch.full((R * W + 2 * GUARD,), -7.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    bnpp.bucket_marginal_rows(ctx, DT[dt], cards, [t.data_ptr() if t is not None else 0 for t in dev], has_b, ev_row, R,
                              live, t_ev.data_ptr() if "e" in kinds else 0, buf[GUARD:].data_ptr(), stream=stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == -7.0).all() and (got[GUARD + R * W:] == -7.0).all(), ("guard band written", name, dt, R)
    return got[GUARD:GUARD + R * W].reshape(R, W), want


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want))[:8])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("R", ROWS)
def test_emit_bit_for_bit(ctx, stream, dt, R):
    for i, name in enumerate(LISTS):
        for live in sorted({R, R - 1, 0}):
            got, want = _run(ctx, stream, name, dt, R, 100 + i, live=live)
            _same(got, want, (name, dt, R, live))
            assert (got[live:] == -7.0).all(), "padding rows are not written"
            if live:
                cards, kinds = LISTS[name]
                assert np.abs(got[:live].sum(axis=1) - len(cards)).max() < 1e-9, "every block sums to 1"


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_a_zero_column_is_nan_there_and_only_there(ctx, stream, dt):
    cards, _ = LISTS["mixed"]
    at = sum(cards[:4])                                     # target 4 (card 5, with the row dimension), row 70
    got, want = _run(ctx, stream, "mixed", dt, 130, 7, zero=(4, 70))
    _same(got, want, ("zero column", dt))
    nan = np.isnan(got)
    assert nan[70, at:at + 5].all() and nan.sum() == 5


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_an_evidence_value_out_of_range_is_clamped(ctx, stream, dt):
    got, want = _run(ctx, stream, "mixed", dt, 65, 9, wild_ev=True)
    _same(got, want, ("clamped", dt))
    cards, _ = LISTS["mixed"]
    at = sum(cards[:2])                                     # target 2: evidence, card 2
    assert (got[0::3, at + 1] == 1.0).all() and (got[1::3, at] == 1.0).all()
    assert ((got[:, at:at + 2] == 0) | (got[:, at:at + 2] == 1)).all() and (got[:, at:at + 2].sum(axis=1) == 1).all()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_capped_grid(ctx, stream, grid_cap, dt):
    ref, want = _run(ctx, stream, "mixed", dt, 257, 11)
    _same(ref, want, ("uncapped", dt))
    for cap in (1, 2, 3):
        grid_cap(cap)
        got, _ = _run(ctx, stream, "mixed", dt, 257, 11)
        _same(got, ref, ("grid cap", cap, dt))
