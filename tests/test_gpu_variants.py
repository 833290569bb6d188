"""GPU parity of every reachable single-op kernel: the catalogue of
variant_catalogue.py (the smallest bucket per instantiated key, under one wave
and over two workgroups with a ragged last one) run through
bnpp_bucket_eliminate / bnpp_divide, and the same buckets as one-bucket models
through bnpp_variable_elimination (the level kernels).

Inputs (variant_catalogue.make_inputs): uniform in [0.5, 2), about 10 % exact
zeros, one input times 2^-20, rounded to the dtype before the oracle sees them.

  * fp64: values == the oracle's bucket / product / divide, permuted to the
    planned layout; for the first size of a key, out_sum == its partition.
  * fp32: values bit-identical to the float32 restatement of the kernels' loop
    (variant_catalogue.restate: acc = 0; per summed value p = 1, p *= in_i in
    input order, acc += p, one rounded numpy operation at a time).  Every
    family -- generic, stream and slab -- is bit-identical; no family needs the
    derived (n_in + k - 2) 2^-24 bound.
  * guard bands: the output sits inside a NaN-filled tensor with 64 entries
    before and after it; the bands stay NaN and no output entry does.
  * instrument: right before each launch bnpp.plan_single of the same
    arguments reports the catalogue's key.
"""
import numpy as np
import pytest
import torch

import bnpp
import refcpu
import variant_catalogue as vc

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"f64": torch.float64, "f32": torch.float32}
ND = {"f64": np.float64, "f32": np.float32}
DT = {"f64": bnpp.F64, "f32": bnpp.F32}
FAM = {"generic": 0, "stream": 1, "slab": 2}
GUARD = 64


@pytest.fixture(scope="module")
def entries():
    return vc.load()


@pytest.fixture(scope="module")
def stream():
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    return s.cuda_stream


@pytest.fixture
def grid_cap(ctx):
    """ctx.set_max_grid for one test: the default grids are restored after it."""
    yield ctx.set_max_grid
    ctx.set_max_grid(0)


def _select(entries, family, dt):
    return [(i, e) for i, e in enumerate(entries) if e["family"] == family and e["dtype"] == dt]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("family", ["generic", "stream", "slab"])
def test_single_op_variants(ctx, entries, stream, monkeypatch, family, dt):
    sel = _select(entries, family, dt)
    assert sel
    for i, e in sel:
        ins = vc.make_inputs(e, i)
        want64, part = vc.oracle(refcpu, e, ins)
        want = want64 if dt == "f64" else vc.restate(e, ins, np.float32)
        n = vc.size_of(e["cards"], e["out"])
        assert len(want) == n
        tabs = [torch.tensor(v, dtype=TD[dt], device=DEV) for v in ins]
        buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=TD[dt], device=DEV)
        out = buf[GUARD:GUARD + n]
        psum = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
        with_sum = e["size"] == "a"
        monkeypatch.setenv("BNPP_NO_O32", "1" if e["no_o32"] else "0")
        info = bnpp.plan_single(DT[dt], e["cards"], e["scopes"], e["elim"], e["out"], divide=e["divide"])
        assert (info["family"], info["key"]) == (FAM[family], e["key"]), (e, info)
        if e["divide"]:
            bnpp.divide(ctx, DT[dt], e["cards"], tabs[0].data_ptr(), e["scopes"][0], tabs[1].data_ptr(), e["scopes"][1],
                        out.data_ptr(), e["out"], stream=stream, out_sum=psum.data_ptr() if with_sum else None)
        else:
            bnpp.bucket_eliminate(ctx, DT[dt], e["cards"], [t.data_ptr() for t in tabs], e["scopes"], e["elim"],
                                  out.data_ptr(), e["out"], stream=stream, out_sum=psum.data_ptr() if with_sum else None)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + n:]).all(), ("guard band written", e)
        vals = got[GUARD:GUARD + n]
        assert not np.isnan(vals).any(), ("output entry not written", e)
        assert np.array_equal(vals, want.astype(ND[dt])), (e, int((vals != want).sum()), n)
        if with_sum and dt == "f64":
            assert psum.item() == part, (e, psum.item(), part)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("family,cap", [pytest.param("generic", 0, id="generic"), pytest.param("stream", 0, id="stream"),
                                        pytest.param("slab", 0, id="slab"),
                                        pytest.param("generic", 1, id="generic-cap1"),
                                        pytest.param("stream", 1, id="stream-cap1")])
def test_level_twins(ctx, entries, monkeypatch, grid_cap, family, cap, dt):
    """Every catalogue bucket with a summed variable (found for either dtype),
    run in `dt`, as a model -- with the default grids (cap 0) and again on a
    context capped at one workgroup (bnpp_ctx_set_max_grid), which then walks
    every virtual block of the launch in the kernel's grid-stride loop; the
    slab family's grid is flat (one workgroup per virtual block: the cap does
    not touch it), so it has no capped run.  Its inputs are
    the factors and bnpp_variable_elimination sums the variable out, so the
    bucket runs on a level kernel (uploaded and rescaled by powers of two only:
    runtime.cpp upload_sources, kernels.cuh kScale).  values * 2^exp2 == the
    oracle's variable_elimination in fp64, == the float32 restatement of
    BN::variable_elimination in fp32 (values in [2^-21, 2): no underflow)."""
    grid_cap(cap)
    done = 0
    for i, e in _select(entries, family, "f64") + _select(entries, family, "f32"):
        if e["elim"] < 0 or e["divide"]:
            continue
        ins = vc.make_inputs(e, i, "f32")                 # exact in both dtypes
        d = {"type": "MARKOV", "cards": e["cards"], "scopes": e["scopes"], "values": [v.tolist() for v in ins]}
        monkeypatch.setenv("BNPP_NO_O32", "1" if e["no_o32"] else "0")
        m = bnpp.Model.from_arrays(e["cards"], e["scopes"], np.concatenate(ins))
        n = vc.size_of(e["cards"], e["out"])
        scope, vals, e2 = bnpp.variable_elimination(ctx, m, [e["elim"]], "given", DT[dt], cap_values=n)
        ref = refcpu.Model.from_dict(d).variable_elimination([e["elim"]], "given")
        assert scope == ref.scope, e
        got = np.ldexp(np.array(vals, dtype=np.float64), e2)
        if dt == "f64":
            want = np.array(ref.values, dtype=np.float64)
        else:
            want = vc.restate_ve(e, ins, np.float32, scope).astype(np.float64)
        assert len(got) == len(want) == n
        assert np.array_equal(got, want), (e, int((got != want).sum()), n)
        done += 1
    assert done


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_variable_elimination_result_in_reference_scope_order(ctx, dt):
    """bnpp_variable_elimination returns its result in the reference's scope
    order (the chain's union minus the summed variable), not in the canonical
    layout the planner gives the last message: one factor over [2, 1, 0],
    variable 2 summed out -> [1, 0]; with a second factor over [0, 3] that
    holds no summed variable and so leads the chain -> [0, 3, 1]."""
    cards = [4, 2, 3, 2]
    for scopes, want_scope in (([[2, 1, 0]], [1, 0]), ([[2, 1, 0], [0, 3]], [0, 3, 1])):
        e = {"cards": cards, "scopes": scopes, "elim": 2, "out": want_scope, "dtype": "f32", "divide": False}
        ins = vc.make_inputs(e, 7)
        m = bnpp.Model.from_arrays(cards, scopes, np.concatenate(ins))
        scope, vals, e2 = bnpp.variable_elimination(ctx, m, [2], "given", DT[dt], cap_values=64)
        assert scope == want_scope
        want = vc.restate_ve(e, ins, ND[dt], want_scope).astype(np.float64)
        assert np.array_equal(np.ldexp(np.array(vals, dtype=np.float64), e2), want)
