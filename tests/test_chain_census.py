"""Chain-run census (CPU): which chain (sweep) kernels the planner can reach,
checked against the instantiation lists of chain.cuh and chainsplit.cuh.

The instruments are the planner's own reports: bnpp.plan_groups (the launch
groups of a plan: key, run descriptors, virtual blocks), bnpp.kernel_keys
family 3 (the dispatch switches' X-macro lists, fused-belief keys included)
and bnpp.chain_key_supported (the predicate build_desc asks).
chain_catalogue.py keeps the smallest case per dtype, key and one-run /
multi-run kernel, and the one with the most virtual blocks;
test_gpu_chain_variants.py runs them on the device.
"""
import pytest

import bnpp
import chain_catalogue as cc

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
FWD, BWD, SUM, FWDV, FWDS, BWDS, FWDSD, BWDSD = 1, 2, 3, 4, 5, 6, 7, 8
NEXT, PREV, ANY = 0, 1, 2


@pytest.fixture(scope="module")
def entries():
    return cc.load()


# Instantiated chain keys no enumerated plan holds, with the reason.  None was
# deleted from the lists.
R_SUM_ANY2 = ("plan.cpp:350-365 (ChainDep): a summing run has no new variables (chain_n[p] = -1, skipped at "
              "plan.cpp:359), so bucket j's G can only count as varying with a later slot p > j; with F = 2 that is "
              "slot j + 1 alone, which is dep next -- dep any needs a slot >= j + 2, so F >= 3 (reached)")
R_BWD_NEXT = ("plan.cpp:350-365 (ChainDep): in a backward run slot p < j already holds column c's variable n_p and "
              "slot p > j still holds the message's variable x_p of column c + 1; a bucket's factors join its own "
              "pair (x_j, n_j) to column c only (vertical, hop and diagonal factors all have an end in the bucket's "
              "column), i.e. to slots p < j: dep prev or any.  dep next needs a factor from bucket j to x_(j+1) of "
              "the other column and none to n_(j-1); the same factor gives a forward bucket two new variables, "
              "which emit_chain rejects (plan.cpp:1117-1122), and the chain bucket tree plans chain-shaped sweeps "
              "only (plan_bucket_tree_chain).  No plan of any enumerated model family holds these keys; the F = 2 "
              "keys are reached because a run of two whose second bucket has no vertical factor counts as next")
UNREACHED = {
    "f32": {**{cc.chain_key(BWD, 2, f, NEXT): R_BWD_NEXT for f in (3, 4, 5, 6)},
            cc.chain_key(BWD, 4, 3, NEXT): R_BWD_NEXT,
            **{cc.chain_key(form, 2, f, NEXT): R_BWD_NEXT for form in (BWDS, BWDSD) for f in (5, 6, 7, 8)},
            **{cc.chain_key(BWDSD, 2, f, NEXT, bel=True): R_BWD_NEXT for f in (5, 6, 7, 8)},
            cc.chain_key(SUM, 2, 2, ANY): R_SUM_ANY2, cc.chain_key(SUM, 4, 2, ANY): R_SUM_ANY2},
    "f64": {**{cc.chain_key(BWD, 2, f, NEXT): R_BWD_NEXT for f in (3, 4, 5)},
            **{cc.chain_key(form, 2, f, NEXT): R_BWD_NEXT for form in (BWDS, BWDSD) for f in (5, 6, 7, 8)},
            **{cc.chain_key(BWDSD, 2, f, NEXT, bel=True): R_BWD_NEXT for f in (5, 6, 7)},
            cc.chain_key(SUM, 2, 2, ANY): R_SUM_ANY2, cc.chain_key(SUM, 4, 2, ANY): R_SUM_ANY2},
}
# keys whose multi-run kernel (several run descriptors in one launch) no plan
# holds: backward runs.  The chain bucket tree's backward pass handles its
# components and segments one after the other (plan_bucket_tree_chain), so two
# backward runs never share a level; only forward and summing runs of two
# components or of the two halves of an evidence-cut grid do.
MULTI_FORMS = (FWD, SUM, FWDV, FWDS, FWDSD)


def test_catalogue_cases_still_plan_to_their_keys(entries):
    """Drift: every frozen case still launches its key with its run count and
    virtual blocks (a changed planner condition moves it; regenerate() then
    finds another case or the key joins UNREACHED with its reason)."""
    moved, models = [], {}
    for e in entries:
        spec = tuple(sorted(e["model"].items()))
        if spec not in models:
            built = cc.build_model(e["model"])
            models[spec] = (built, bnpp.Model.from_dict(built[0]), bnpp.Model.from_dict(cc.conditioned(built[0], built[1])))
        built, full, cond = models[spec]
        g = cc.find_group(cc.plan(bnpp, e, model=cond if e["plan"] == "ve" else full, built=built), e["key"], e["runs"])
        if g is None or (g["n_desc"], g["vblocks"]) != (e["n_desc"], e["vblocks"]):
            moved.append((e["dtype"], e["key"], e["runs"], e["size"], g))
        assert e["model"]["rows"] <= cc.MAX_ROWS[e["model"]["k"]] and e["model"]["cols"] <= cc.MAX_COLS
    assert not moved, moved[:5]


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_catalogue_covers_instantiated_chain_keys(entries, dt):
    """catalogue keys U UNREACHED == the dispatch switch's keys, disjoint; every
    split key's one-run kernel is reached, and the multi-run kernel of every
    forward and summing split key."""
    inst = set(bnpp.kernel_keys(DT[dt], 3, level=True))
    got = {e["key"] for e in entries if e["dtype"] == dt}
    unreached = set(UNREACHED[dt])
    assert not (got & unreached), sorted(got & unreached)
    assert got | unreached == inst, (sorted(inst - got - unreached), sorted((got | unreached) - inst))
    one = {e["key"] for e in entries if e["dtype"] == dt and e["runs"] == "one"}
    multi = {e["key"] for e in entries if e["dtype"] == dt and e["runs"] == "multi"}
    assert one == got
    assert all(cc.key_fields(k)[0] in MULTI_FORMS for k in multi)
    split_fwd = {k for k in got if cc.key_fields(k)[0] in (FWDS, FWDSD) and cc.key_fields(k)[3] == NEXT}
    assert split_fwd and split_fwd <= multi, sorted(split_fwd - multi)
    print("chain census %s: %d instantiated, %d reached (%d also by the multi-run kernel), %d unreached"
          % (dt, len(inst), len(got), len(multi), len(unreached)))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_kernel_keys_are_what_the_planner_accepts(dt):
    """bnpp.kernel_keys family 3 == the keys chain_supported accepts, probed
    over the whole chain key range; chain runs are level launches only."""
    keys = bnpp.kernel_keys(DT[dt], 3, level=True)
    assert len(keys) == len(set(keys)) == {"f32": 92, "f64": 70}[dt]
    assert set(keys) == {k for k in range(8192, 16384) if bnpp.chain_key_supported(DT[dt], k)}
    assert not any(bnpp.chain_key_supported(DT[dt], k) for k in list(range(0, 8192, 7)) + list(range(16384, 32768, 7)))
    assert bnpp.kernel_keys(DT[dt], 3) == []
    assert bnpp.FAMILIES[3] == "chain"
    assert all(cc.chain_key(*cc.key_fields(k)) == k for k in keys)


def test_enumerated_plans_hold_only_instantiated_keys():
    """Every chain key in the plans of a slice of the enumeration (every model
    family, both orders, every switch combination) is instantiated for its
    dtype, and none is an UNREACHED one (regenerate() asserts the first over
    the whole enumeration)."""
    inst = {dt: set(bnpp.kernel_keys(DT[dt], 3, level=True)) for dt in DT}
    seen = {"f32": set(), "f64": set()}
    specs = [{"kind": kind, "rows": 11, "cols": 3, "k": 2, "hop": 2 if kind == "hop" else 0, "order": order}
             for kind in ("ising", "two", "hop", "diag", "diagv") for order in ("down", "up")]
    specs += [{"kind": kind, "rows": 5, "cols": 3, "k": 4, "hop": 0, "order": "down"} for kind in ("potts", "diagv")]
    for spec in specs:
        _, s = cc.scan_model(spec)
        for dt in s:
            seen[dt] |= s[dt]
    for dt in DT:
        assert seen[dt] and seen[dt] <= inst[dt], (dt, sorted(seen[dt] - inst[dt]))
        assert not (seen[dt] & set(UNREACHED[dt])), (dt, sorted(seen[dt] & set(UNREACHED[dt])))


def test_plan_groups_rejects_bad_arguments():
    m = bnpp.Model.from_dict(cc.build_model({"kind": "ising", "rows": 4, "cols": 3, "k": 2, "hop": 0, "order": "down"})[0])
    assert bnpp.plan_groups(m, 0)
    for kw in ({"kind": 4}, {"kind": 0, "n_parts": 2}, {"kind": 3, "part": 2, "n_parts": 2}):
        with pytest.raises(bnpp.BnppError):
            bnpp.plan_groups(m, **kw)
    groups = bnpp.plan_groups(m, 3, part=1, n_parts=2)
    assert all(set(g) == set(bnpp.PLAN_GROUP_FIELDS) and g["n_desc"] >= 1 and g["vblocks"] >= 1 for g in groups)


def test_loop_kinds_have_a_capped_case(entries):
    """The persistent tile loops of chainsplit.cuh each have a catalogue case
    with enough virtual blocks for the capped reruns of
    test_gpu_chain_variants.py (a workgroup walks >= 3 tiles at cap 2 or 3
    when the launch has >= 7 virtual blocks)."""
    def has(dt, forms, fs, runs="one", bel=False, min_vb=7):
        return [e for e in entries if e["dtype"] == dt and e["runs"] == runs and e["vblocks"] >= min_vb and
                cc.key_fields(e["key"])[0] in forms and cc.key_fields(e["key"])[2] in fs and
                cc.key_fields(e["key"])[4] == bel]
    # fp32 forward runs: the next tile staged through LDS
    assert has("f32", (FWDS, FWDSD), (5, 6, 7, 8))
    # fp64 runs of 8 (ALIAS: two register sets, unrolled twice): 16 blocks give walks of 16 (cap 1), 8 (cap 2)
    # and 6, 5, 5 (cap 3): both exits of the unrolled loop
    alias = has("f64", (FWDS, FWDSD), (8,))
    assert alias and any(e["vblocks"] % 2 == 0 and (e["vblocks"] // 3) % 2 != ((e["vblocks"] + 2) // 3) % 2 for e in alias)
    # fp64 runs of 5 to 7.  With BNPP_F64_ALIAS = 1 (the default, chainsplit.cuh) every fp64 one-run forward kernel
    # takes the ALIAS loop too; the AHEAD2 loop (fp64 forward, not aliased) is compiled into no default kernel and
    # so cannot be planned -- these cases walk the ALIAS loop at F = 5, 6, 7
    assert all(has("f64", (FWDS, FWDSD), (f,)) for f in (5, 6, 7))
    # backward runs with a fused belief (bel_sum one tile late), both dtypes: 4 blocks (caps 1 and 3)
    assert has("f32", (BWDSD,), (5, 6, 7, 8), bel=True, min_vb=4) and has("f64", (BWDSD,), (5, 6, 7), bel=True, min_vb=4)
    # the multi-run kernel: a capped workgroup walks from one run into the next
    assert has("f32", (FWDS, FWDSD), (5, 6, 7, 8), runs="multi") and has("f64", (FWDS, FWDSD), (5, 6, 7, 8), runs="multi")
    # the one-thread forms' grid-stride loop
    assert has("f32", (FWD, BWD, SUM, FWDV), range(2, 7)) and has("f64", (FWD, BWD, SUM, FWDV), range(2, 7))
