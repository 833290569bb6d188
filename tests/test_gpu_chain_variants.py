"""GPU parity of every reachable chain-run kernel: the cases of
chain_catalogue.py (the smallest model per dtype, chain key and one-run /
multi-run kernel, and the one with the most virtual blocks) run through
bnpp_variable_elimination, bnpp_partition and bnpp_marginals_tree.

  * instrument: right before each launch bnpp.plan_groups of the same call
    holds the case's key with the case's run count (one descriptor: the
    one-run kernel, several: the multi-run kernel).
  * forward forms (kChainFwd, kChainFwdV, kChainFwdS, kChainFwdSD), "ve" cases:
    under BNPP_VE_CHAIN=1 every column but the last is eliminated, so the
    sweep's last message comes back entry by entry.  fp64: values * 2^exp2 ==
    the oracle's variable_elimination, scope and every entry.  fp32:
    bit-identical to the same call under BNPP_NO_CHAIN=1 (one bucket per
    launch: kernels test_gpu_variants.py pins to the float32 restatement) and
    within 1e-5 relative of the fp64 oracle.
  * summing runs (kChainSum) and "pr" cases: fp64 z == the scalar the oracle's
    variable_elimination of every variable in the same order leaves; log10 Z
    bit-identical to BNPP_NO_CHAIN=1 in the case's dtype.
  * backward forms and fused beliefs, "tree" / "part" cases: the tree
    marginals bit-identical to BNPP_NO_CHAIN=1 (belief keys: also to
    BNPP_NO_BEL_FUSE=1) and within 1e-12 (fp64) / 1e-5 (fp32) of the oracle's
    marginals -- the tolerances of test_gpu_bucket_tree.py.
  * tile loops: every key's case with the most virtual blocks again on a
    context capped (bnpp_ctx_set_max_grid) at 1, 2 and 3 workgroups, so that a
    workgroup walks several tiles and, in a multi-run launch, crosses from one
    run into the next: results == the uncapped ones, and the checks above.
    A cap is used where it makes some workgroup walk several tiles: cap 1
    from 2 virtual blocks, cap 2 and 3 from 2 cap + 1 (a walk of >= 3 tiles),
    and cap 3 on the 4-block belief cases (walks of 2, 1, 1).
"""
import json

import numpy as np
import pytest

import bnpp
import chain_catalogue as cc
import refcpu

pytestmark = pytest.mark.gpu

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
TOL = {"f64": 1e-12, "f32": 1e-5}
ENTRIES = cc.load()


def _id(e):
    return "%s-%d-%s-%s" % (e["dtype"], e["key"], e["runs"], e["size"])


class Case:
    """One model spec: engine and oracle models, oracle results computed once."""
    _all = {}

    @classmethod
    def of(cls, spec):
        k = json.dumps(spec, sort_keys=True)
        if k not in cls._all:
            cls._all[k] = cls(spec)
        return cls._all[k]

    def __init__(self, spec):
        self.spec = spec
        self.d, self.ev, self.order = cc.build_model(spec)
        self.dc = cc.conditioned(self.d, self.ev)
        self.m = bnpp.Model.from_dict(self.d)
        self.mc = bnpp.Model.from_dict(self.dc) if self.ev else self.m
        self.vars = cc.ve_vars(spec, self.ev, self.order)
        self.cap_values = spec["k"] ** spec["rows"]
        self._o = {}

    def oracle(self, what):
        if what not in self._o:
            if what == "ve":
                f = refcpu.Model.from_dict(self.dc).variable_elimination(self.vars, "given")
                self._o[what] = (f.scope, np.array(f.values, dtype=np.float64))
            elif what == "z":
                f = refcpu.Model.from_dict(self.dc).variable_elimination([v for v in self.order if v not in self.ev], "given")
                assert f.scope == []
                self._o[what] = f.values[0]
            else:
                self._o[what] = refcpu.Model.from_dict(self.d).marginals(self.ev, "mf")[0]
        return self._o[what]


def run(ctx, case, e, extra=None):
    """The case's call -> ("ve": (scope, values as float64), "pr": (log10 Z, z), tree: {var: marginal})."""
    kn = dict(e["knobs"])
    kn.update(extra or {})
    dtype, p = DT[e["dtype"]], e["plan"]
    with cc.knobs(kn):
        if p == "ve":
            scope, vals, e2 = bnpp.variable_elimination(ctx, case.mc, case.vars, "given", dtype, cap_values=case.cap_values)
            return scope, np.ldexp(np.array(vals, dtype=np.float64), e2)
        if p == "pr":
            return bnpp.partition(ctx, case.m, case.ev, "mf", dtype, order=case.order)[:2]
        part, n_parts = (int(p[4:]), 2) if p.startswith("part") else (0, 1)
        return bnpp.marginals_tree(ctx, case.m, case.ev, "mf", dtype, order=case.order, part=part, n_parts=n_parts)[0]


def same(a, b):
    if isinstance(a, tuple) and isinstance(a[1], np.ndarray):
        return a[0] == b[0] and np.array_equal(a[1], b[1])
    return a == b


def planned(e, case):
    """The instrument: the plan about to be launched holds the case's key and run count."""
    g = cc.find_group(cc.plan(bnpp, e, model=case.mc if e["plan"] == "ve" else case.m,
                              built=(case.d, case.ev, case.order)), e["key"], e["runs"])
    assert g is not None and g["n_desc"] == e["n_desc"] and g["vblocks"] == e["vblocks"], (e, g)
    return g


def check(ctx, case, e, got):
    """The parity checks of a case's result (module docstring)."""
    dt, p = e["dtype"], e["plan"]
    bel = cc.key_fields(e["key"])[4]
    plain = run(ctx, case, e, {"BNPP_NO_CHAIN": 1})
    if p == "ve":
        scope, want = case.oracle("ve")
        assert got[0] == scope, (e, got[0], scope)
        assert len(got[1]) == len(want)
        if dt == "f64":
            assert np.array_equal(got[1], want), (e, int((got[1] != want).sum()), len(want))
        else:
            assert same(got, plain), (e, int((got[1] != plain[1]).sum()), len(want))
            err = np.abs(got[1] - want) / np.abs(want)
            print("%s: fp32 max relative error %.3g" % (_id(e), err.max()))
            assert err.max() <= 1e-5, (e, err.max())
    elif p == "pr":
        if dt == "f64":
            assert got[1] == case.oracle("z"), (e, got, case.oracle("z"))
        assert got[0] == plain[0], (e, got, plain)
    else:
        assert got == plain, e
        if bel:
            assert got == run(ctx, case, e, {"BNPP_NO_BEL_FUSE": 1}), e
        want = case.oracle("marginals")
        assert got, e
        worst = max(abs(x - y) for t in got for x, y in zip(got[t], want[t]))
        print("%s: max marginal error %.3g" % (_id(e), worst))
        for t in got:
            assert all(abs(x - y) <= TOL[dt] for x, y in zip(got[t], want[t])), (e, t, got[t], want[t])


@pytest.mark.parametrize("e", [e for e in ENTRIES if e["size"] == "small"], ids=_id)
def test_chain_key(ctx, e):
    """Every catalogue key on its smallest case, default grids."""
    case = Case.of(e["model"])
    planned(e, case)
    check(ctx, case, e, run(ctx, case, e))


def walks(vblocks, cap):
    """Tiles each of min(vblocks, cap) workgroups takes (grid-stride)."""
    g = min(vblocks, cap)
    return [len(range(w, vblocks, g)) for w in range(g)]


def loop_cases():
    """(case, cap) for the tile loops: per (dtype, key, runs) the case with
    the most virtual blocks, and every cap of 1, 2, 3 under which some
    workgroup walks several tiles (module docstring)."""
    best = {}
    for e in ENTRIES:
        k = (e["dtype"], e["key"], e["runs"])
        if k not in best or e["vblocks"] > best[k]["vblocks"]:
            best[k] = e
    out = []
    for k in sorted(best):
        e = best[k]
        for cap in (1, 2, 3):
            vb = e["vblocks"]
            if vb >= 2 * cap + 1 or (vb >= 2 and cap == 1) or (vb == 4 and cap == 3):
                out.append(pytest.param(e, cap, id="%s-cap%d" % (_id(e), cap)))
    return out


@pytest.mark.parametrize("e,cap", loop_cases())
def test_chain_key_tile_loops(ctx, e, cap):
    """The same call on a context capped at `cap` workgroups == the uncapped
    result, and passes the same oracle checks."""
    case = Case.of(e["model"])
    g = planned(e, case)
    w = walks(g["vblocks"], cap)
    assert max(w) >= 2
    if cap > 1:
        assert g["vblocks"] >= 2 * cap + 1 or (g["vblocks"] == 4 and cap == 3), (g, cap)
        assert max(w) >= 3 or w == [2, 1, 1], w
    free = run(ctx, case, e)
    ctx.set_max_grid(cap)
    try:
        capped = run(ctx, case, e)
        assert same(capped, free), (e, cap)
        check(ctx, case, e, capped)
    finally:
        ctx.set_max_grid(0)
