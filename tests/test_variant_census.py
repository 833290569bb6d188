"""Kernel-variant census (CPU): which single-op and level kernels the planner
can reach, checked against the instantiation lists.

The instrument is the planner's own report: bnpp.plan_single (the family and
dispatch key run_single launches, through the same code) and the key= field of
the BNPP_DUMP_PLAN bucket lines.  bnpp.kernel_keys lists what the dispatch
switches hold (generated from their X-macro lists).  variant_catalogue.py keeps
the smallest bucket found per instantiated single-op key; test_gpu_variants.py
runs those buckets on the device.
"""
import os
import random
import re
import time

import numpy as np
import pytest

import batch_catalogue
import bnpp
import refcpu
import variant_catalogue as vc
from conftest import evidence_of, model_path

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
FAM = {"generic": 0, "stream": 1, "slab": 2}


@pytest.fixture(scope="module")
def entries():
    return vc.load()


# key formulas of bnpp_device.h (variant_key, stream_key, slab_key), for the tables below
def gkey(nin, v1, v2):
    return [nin * 64 + v1 * 8 + v2, 1024 + nin * 64 + v1 * 8 + v2]


def skey(bc, v1, v2):
    return [4096 + bc * 256 + v1 * 16 + v2, 4096 + 2048 + bc * 256 + v1 * 16 + v2]


def lkey(k, c0, v, h=1, r=1, n8=False):
    return 16384 + (8192 if n8 else 0) + k * 1024 + (512 if r == 4 else 256 if r == 2 else 0) + c0 * 16 + v + (8 if h == 2 else 0)


ROW, COL, FULL, DIRECT, ONE, INTER2, INTER4 = 1, 2, 3, 4, 5, 6, 7

# Instantiated single-op keys no caller can reach, with the build_desc
# condition that keeps them out (bn-pp_amd/csrc/plan.cpp).  None was deleted
# from the lists: the level launches share them (BNPP_ALL, BNPP_STREAM_*,
# BNPP_SLAB_*), and the tuning builds' knobs reach the slab ones.
R_6X1 = ("plan.cpp:894-896 asks for v1 == 1 and c0 == 6 with aligned(0, 2), but plan.cpp:598-599 has then "
         "already chosen v1 = 2 (6 % 2 == 0 and aligned(0, 2)): the 6x1 whole-dim row is never picked")
R_CLASS = ("plan.cpp:872-876: Row needs v1 > 1, Col needs v2 > 1, Full needs both; a bucket whose tile lacks "
           "that width takes One or Direct")
R_INTER64 = ("plan.cpp:831-833: broadcast-row tiles hold at most max_ts = 8 entries in fp64, so 8x2 and 4x4 are "
             "halved to 4x2 and 2x4 (the instantiations exist for fp32's 16)")
R_SLABV = ("plan.cpp:701: c0 = 4 (fp32) and c0 = 2 (fp64) get one slow-dim entry per tile; V = 2 only through "
           "the BNPP_SLAB_V knob (plan.cpp:704), which release builds compile out (plan.hpp tuning_knob)")
R_LANES = ("plan.cpp:738: a 32-B tile row always takes two lanes (H = 2); H = 1 only through the "
           "BNPP_SLAB_LANES knob, which release builds compile out")
_CLASS_KEYS = [k for bc, tiles in ((ROW, [(1, 1)]), (COL, [(1, 1), (2, 1), (4, 1)]), (FULL, [(1, 1), (2, 1), (4, 1)]))
               for t in tiles for k in skey(bc, *t)]
UNREACHED = {
    ("f64", "generic"): {k: R_6X1 for nin in (1, 2, 4, 8) for k in gkey(nin, 6, 1)},
    ("f32", "generic"): {k: R_6X1 for nin in (1, 2, 4, 8) for k in gkey(nin, 6, 1)},
    ("f64", "stream"): {**{k: R_CLASS for k in _CLASS_KEYS},
                        **{skey(bc, *t)[0]: R_INTER64 for bc in (INTER2, INTER4) for t in ((8, 2), (4, 4))}},
    ("f32", "stream"): {k: R_CLASS for k in _CLASS_KEYS},
    ("f64", "slab"): {**{lkey(k, 2, 2, h): R_SLABV for k in (1, 2, 3, 4) for h in (1, 2)},
                      **{lkey(k, 4, 1, 1): R_LANES for k in (1, 2, 3, 4)}},
    ("f32", "slab"): {lkey(k, 4, 2, h): R_SLABV for k in (1, 2, 3, 4) for h in (1, 2)},
}


def test_catalogue_entries_still_plan_to_their_keys(entries):
    """Drift: every frozen bucket still reaches the kernel it was recorded for
    (a changed planner condition moves it; regenerate() then finds a new bucket
    or the key joins UNREACHED with its reason)."""
    moved = []
    for e in entries:
        info = vc.plan(bnpp, DT[e["dtype"]], e, e["no_o32"])
        if (info["family"], info["key"], info["n_tiles"]) != (FAM[e["family"]], e["key"], e["n_tiles"]) or not info["instantiated"]:
            moved.append((e["dtype"], e["family"], e["key"], e["size"], info))
    assert not moved, moved[:5]


def test_catalogue_size_classes(entries):
    """Every key has a bucket under one wave where its family allows it
    (generic) and one spanning two workgroups with a ragged last one."""
    by_key = {}
    for e in entries:
        by_key.setdefault((e["dtype"], e["family"], e["key"]), []).append(e)
    for key, es in by_key.items():
        per_block = 256
        if key[1] == "slab":
            per_block = 256 // max(1, vc.plan(bnpp, DT[key[0]], es[0], es[0]["no_o32"])["lanes"])
        assert any(e["n_tiles"] > per_block and e["n_tiles"] % per_block for e in es), key
        if key[1] == "generic":
            assert any(e["n_tiles"] < 64 for e in es), key
        assert all(vc.size_of(e["cards"], e["out"]) <= vc.MAX_OUT for e in es)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("family", ["generic", "stream", "slab"])
def test_catalogue_covers_instantiated_single_keys(entries, dt, family):
    """catalogue keys U UNREACHED == the dispatch switch's keys, disjoint."""
    inst = set(bnpp.kernel_keys(DT[dt], FAM[family]))
    got = {e["key"] for e in entries if e["dtype"] == dt and e["family"] == family}
    unreached = set(UNREACHED[(dt, family)])
    assert not (got & unreached), sorted(got & unreached)
    assert got | unreached == inst, (sorted(inst - got - unreached), sorted((got | unreached) - inst))
    if family == "generic":                       # both offset widths of every reached tile
        assert {k + 1024 for k in got if k < 1024} == {k for k in got if k >= 1024}


def _fuzz_bucket(rng):
    nv = rng.randint(1, 10)
    cards = [rng.randint(1, 8) for _ in range(nv)]
    divide = rng.random() < 0.08
    n_in = 2 if divide else rng.randint(1, 8)
    scopes = [rng.sample(range(nv), min(nv, rng.randint(0, 6))) for _ in range(n_in)]
    if rng.random() < 0.5:
        for s in scopes:
            s.sort()
    ev = {}
    if not divide and rng.random() < 0.25:        # conditioned views
        for v in rng.sample(range(nv), rng.randint(1, min(3, nv))):
            ev[v] = rng.randrange(cards[v])
    live = [[v for v in s if v not in ev] for s in scopes]
    union = vc.out_scope(live, -1)
    r = rng.random()
    if divide or r < 0.2 or not union:
        elim = -1
    elif r < 0.3:                                 # a variable no input holds: a copy
        free = [v for v in range(nv) if v not in union]
        elim = rng.choice(free) if free else -1
    else:
        elim = rng.choice(union)
    out = vc.out_scope(live, elim)
    if rng.random() < 0.6:
        rng.shuffle(out)
    return cards, scopes, elim, out, divide, ev


FUZZ_BUCKETS = 20000


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_planner_only_picks_instantiated_kernels(dt):
    """Seeded fuzz: every bucket bnpp_plan_single accepts -- 1-8 inputs, cards
    1-8, widths 0-6, permuted outputs, the summed variable present, absent or
    -1, divides, conditioned views, both offset widths -- reports a key its
    family's dispatch switch holds; an uninstantiated key would fail the call
    with "kernel launch: invalid value".  20000 buckets per dtype take about
    2 s here (the issue's count; not lowered)."""
    rng = random.Random(987 + DT[dt])
    t0 = time.time()
    accepted, fams, bad = 0, set(), []
    for it in range(FUZZ_BUCKETS):
        cards, scopes, elim, out, divide, ev = _fuzz_bucket(rng)
        os.environ["BNPP_NO_O32"] = "1" if it % 4 == 3 else "0"
        try:
            info = bnpp.plan_single(DT[dt], cards, scopes, elim, out, divide=divide, evidence=ev)
        except bnpp.BnppError:
            continue
        finally:
            del os.environ["BNPP_NO_O32"]
        accepted += 1
        fams.add(info["family"])
        if not info["instantiated"]:
            bad.append((cards, scopes, elim, out, divide, ev, info))
    print("fuzz %s: %d accepted of %d in %.1f s" % (dt, accepted, FUZZ_BUCKETS, time.time() - t0))
    assert not bad, bad[:3]
    assert accepted >= FUZZ_BUCKETS * 0.9 and fams == {0, 1, 2}, (accepted, fams)


def test_restatement_matches_oracle(entries):
    """The numpy restatement the fp32 GPU checks compare with, run in float64,
    equals the oracle bit for bit on the catalogue's small buckets."""
    n = 0
    for i, e in enumerate(entries):
        if vc.size_of(e["cards"], e["out"]) > 512 or e["dtype"] != "f64":
            continue
        ins = vc.make_inputs(e, i)
        want, _ = vc.oracle(refcpu, e, ins)
        got = vc.restate(e, ins, np.float64)
        assert np.array_equal(got, want), e
        n += 1
        if e["elim"] >= 0 and not e["divide"]:    # the level twin's restatement of BN::variable_elimination
            d = {"type": "MARKOV", "cards": e["cards"], "scopes": e["scopes"], "values": [v.tolist() for v in ins]}
            ref = refcpu.Model.from_dict(d).variable_elimination([e["elim"]], "given")
            assert np.array_equal(vc.restate_ve(e, ins, np.float64, ref.scope), np.array(ref.values)), e
    assert n >= 60


# ------------------------------------------------------------- level census
GRIDS = [("potts", 5, 5, 3, 5), ("ising", 9, 7, 2, 6), ("ising", 8, 12, 2, 8), ("ising", 20, 20, 2, 9),
         ("ising", 10, 10, 2, 0), ("ising", 7, 7, 2, 1), ("ising", 6, 9, 2, 11), ("ising", 7, 11, 2, 12),
         ("ising", 10, 13, 2, 5), ("potts", 5, 7, 4, 3), ("ising", 16, 6, 2, 13), ("noisy_or", 14, 18, 3, 7)]
FAST_PR = ["grid3x3.uai", "network.uai", "asia.uai", "potts6x6.uai", "potts4x5k3.uai", "ising4x4.uai", "ising5x5.uai",
           "ising6x6.uai", "ising8x8.uai", "ising10x10.uai", "ising12x12.uai", "cancer.uai", "earthquake.uai",
           "child.uai", "alarm.uai", "insurance.uai", "hailfinder.uai", "noisyor_30_40.uai", "pathfinder.uai",
           "Water.uai", "hepar2.uai", "win95pts.uai", "andes.uai"]


def _family_of(key):
    return "slab" if key >= 16384 else "stream" if 4096 <= key < 8192 else "generic" if key < 4096 else None


def collect_level_keys(entries, golden_ve, capfd, monkeypatch):
    """{dtype: set of generic / stream / slab level keys} over (a) a one-bucket
    model of every catalogue entry (its summed variable eliminated, or the plain
    product), with both offset widths for the generic ones, and (b) the models
    the GPU suite runs: the FAST_PR cases and the synthetic grids of
    test_gpu_bucket_tree.py as partitions and bucket trees."""
    from bnpp import synth
    monkeypatch.setenv("BNPP_DUMP_PLAN", "1")
    keys = {"f64": set(), "f32": set()}

    def run(dt, fn):
        capfd.readouterr()
        fn()
        for m in re.finditer(r" key=(\d+)", capfd.readouterr().err):
            if _family_of(int(m.group(1))):
                keys[dt].add(int(m.group(1)))

    for e in entries:
        if e.get("divide"):
            continue
        vals = np.ones(sum(vc.size_of(e["cards"], s) for s in e["scopes"]))
        m = bnpp.Model.from_arrays(e["cards"], e["scopes"], vals)
        monkeypatch.setenv("BNPP_NO_O32", "1" if e["no_o32"] else "0")
        order = [e["elim"]] if e["elim"] >= 0 else []
        run(e["dtype"], lambda: bnpp.plan_stats(m, 2, None, dtype=DT[e["dtype"]], order=order))
    monkeypatch.delenv("BNPP_NO_O32")
    for dt in ("f64", "f32"):
        for case in golden_ve["pr"]:
            if case["model"] in FAST_PR:
                m = bnpp.Model.load(model_path(case["model"]))
                run(dt, lambda: bnpp.plan_stats(m, 0, evidence_of(case["evidence"]), case["heuristic"], DT[dt]))
        for kind, r, c, k, seed in GRIDS:
            d = (synth.ising_grid(r, c, seed=seed) if kind == "ising" else synth.potts_grid(r, c, k=k, seed=seed)
                 if kind == "potts" else synth.noisy_or_bn(r, c, k, seed=seed))
            m = bnpp.Model.from_dict(d)
            for pk in (0, 3):
                run(dt, lambda: bnpp.plan_stats(m, pk, None, "mf", DT[dt]))
    return keys


# the level keys those plans hold (frozen; a planner change that moves a bucket
# of these models onto another kernel shows here)
LEVEL_KEYS = {
    "f64": [
        73, 81, 84, 89, 97, 98, 105, 121, 145, 148, 153, 161, 162, 169, 265, 273, 274, 276, 281, 289, 290,
        297, 313, 521, 529, 530, 532, 537, 545, 553, 569, 1097, 1105, 1108, 1113, 1121, 1122, 1129, 1145,
        1161, 1169, 1170, 1172, 1177, 1185, 1186, 1193, 1289, 1297, 1298, 1300, 1305, 1313, 1314, 1321, 1337,
        1545, 1553, 1554, 1556, 1561, 1569, 1577, 1593, 4385, 4417, 4642, 4674, 4898, 4900, 4930, 5137, 5153,
        5154, 5156, 5185, 5186, 5393, 5409, 5410, 5412, 5665, 5666, 5761, 6017, 6465, 6690, 6692, 6722, 6948,
        6978, 7185, 7202, 7204, 7233, 7234, 17425, 17426, 17441, 17481, 17682, 18449, 18450, 18505, 18706,
        19473, 19730, 20497, 20553, 20754, 25617],
    "f32": [
        73, 81, 84, 88, 89, 97, 98, 105, 121, 145, 146, 152, 153, 161, 162, 164, 169, 265, 273, 274, 276, 280,
        281, 289, 290, 292, 297, 313, 521, 529, 530, 532, 537, 545, 548, 553, 569, 1097, 1105, 1108, 1112,
        1113, 1121, 1122, 1124, 1129, 1145, 1161, 1169, 1170, 1172, 1176, 1177, 1185, 1186, 1188, 1193, 1289,
        1297, 1298, 1300, 1304, 1305, 1313, 1314, 1316, 1321, 1337, 1545, 1553, 1554, 1556, 1560, 1561, 1569,
        1572, 1577, 1593, 4385, 4417, 4642, 4644, 4674, 4676, 4898, 4900, 4904, 4930, 4932, 5137, 5153, 5154,
        5156, 5160, 5185, 5186, 5188, 5393, 5409, 5410, 5412, 5441, 5442, 5444, 5665, 5666, 5761, 6017, 6433,
        6465, 6690, 7185, 7201, 7202, 7204, 7233, 17425, 17441, 17473, 17684, 18449, 18452, 18708, 19473,
        19732, 20497, 20545, 20756, 26129],
}
# instantiated level keys of the three families that no plan above reaches:
# "condition" ones for the reasons of UNREACHED (the level launches plan with
# the same build_desc), "batched plans only" ones are held by the batched plans
# of batch_catalogue.py (the row variable B as the fastest dimension, in the
# forward sweep of plan_batch or the backward pass of plan_counts and
# plan_marginals_batch: the keys of test_batch_census.BATCH_ONLY_KEYS), "no plan
# found" ones are reachable in
# principle -- the planner owns message layouts, so no caller can ask for them
# directly
UNREACHED_LEVEL = {
    ("f64", "generic"): {
        "condition": [
            113, 177, 305, 561, 1137, 1201, 1329, 1585],
        "batched plans only": [
            82, 137, 146, 185, 546, 1106, 1209, 1570],
        "no plan found": []},
    ("f64", "stream"): {
        "condition": [
            4369, 4625, 4641, 4673, 4881, 4897, 4929, 5700, 5762, 5956, 6018, 6417, 6673, 6689, 6721, 6929,
            6945, 6977],
        "batched plans only": [
            4388, 4418, 4644, 5441, 5442, 6433, 6434, 6436, 6466, 7201, 7441, 7457, 7489],
        "no plan found": [
            4386, 5668, 5697, 5698, 5921, 5922, 5924, 5953, 5954, 6946, 7458, 7460, 7490]},
    ("f64", "slab"): {
        "condition": [
            17442, 17450, 17473, 18466, 18474, 18497, 19490, 19498, 19521, 20514, 20522, 20545, 25873, 25889,
            25929, 26129, 26145, 26185, 26897, 26913, 26953, 27153, 27169, 27209, 27921, 27937, 27977, 28177,
            28193, 28233, 28945, 28961, 29001, 29201, 29217, 29257],
        "batched plans only": [
            19474, 19489, 19529, 20498, 20513, 26641, 27665, 28689],
        "no plan found": [
            18465, 25633, 25673, 26657, 26697, 27681, 27721, 28705, 28745]},
    ("f32", "generic"): {
        "condition": [
            113, 177, 305, 561, 1137, 1201, 1329, 1585],
        "batched plans only": [
            82, 100, 137, 148, 185, 536, 546, 1106, 1209, 1570],
        "no plan found": []},
    ("f32", "stream"): {
        "condition": [
            4369, 4625, 4641, 4673, 4881, 4897, 4929, 6417, 6673, 6689, 6721, 6929, 6945, 6977],
        "batched plans only": [
            4388, 4420, 4648, 6434, 6436, 6466, 6468, 6948, 6978, 6980, 7441, 7457, 7489],
        "no plan found": [
            4386, 4392, 4418, 5416, 5668, 5697, 5698, 5700, 5762, 5921, 5922, 5924, 5953, 5954, 5956,
            6018, 6692, 6722, 6724, 6946, 7234, 7236, 7458, 7460, 7490, 7492]},
    ("f32", "slab"): {
        "condition": [
            17474, 17482, 18498, 18506, 19522, 19530, 20546, 20554],
        "batched plans only": [
            17428, 19476, 19521, 19746, 20500, 20770, 25617, 25873, 26641, 26897, 27153, 27665, 27921, 28177, 28689,
            28945, 29201],
        "no plan found": [
            17442, 17698, 18465, 18466, 18497, 18722, 19489, 19490, 20513, 20514, 25633, 25665,
            25889, 25921, 26145, 26177, 26657, 26689, 26913, 26945, 27169, 27201, 27681, 27713, 27937, 27969,
            28193, 28225, 28705, 28737, 28961, 28993, 29217, 29249]},
}


def test_level_census(entries, golden_ve, capfd, monkeypatch):
    keys = collect_level_keys(entries, golden_ve, capfd, monkeypatch)
    batched = {}
    for e in batch_catalogue.load()["entries"]:
        batched.setdefault((e["dtype"], e["family"]), set()).add(e["key"])
    for dt in ("f64", "f32"):
        assert sorted(keys[dt]) == LEVEL_KEYS[dt], (dt, sorted(keys[dt] ^ set(LEVEL_KEYS[dt])))
        for family in ("generic", "stream", "slab"):
            inst = set(bnpp.kernel_keys(DT[dt], FAM[family], level=True))
            reached = {k for k in keys[dt] if _family_of(k) == family}
            assert reached <= inst, (dt, family, sorted(reached - inst))     # a level key no switch holds
            table = UNREACHED_LEVEL[(dt, family)]
            listed = set(table["condition"]) | set(table["batched plans only"]) | set(table["no plan found"])
            assert listed == inst - reached, (dt, family, sorted(listed ^ (inst - reached)))
            assert len(listed) == len(table["condition"]) + len(table["batched plans only"]) + len(table["no plan found"])
            assert sorted(table["batched plans only"]) == sorted(batched[(dt, family)]), (dt, family)
            assert set(table["condition"]) <= set(UNREACHED[(dt, family)]) | _level_only_conditions(dt, family)
            print("level census %s %s: %d instantiated, %d reached, %d unreached by condition, %d batched plans only, "
                  "%d no plan found" % (dt, family, len(inst), len(reached), len(table["condition"]),
                                        len(table["batched plans only"]), len(table["no plan found"])))


def _level_only_conditions(dt, family):
    """Level-only keys ruled out by a condition: the 8-input-class slab kernels
    take R = 2 or 4 passes per block in fp32 only (plan.cpp:764, eb == 4)."""
    if (dt, family) != ("f64", "slab"):
        return set()
    return {lkey(k, c0, 1, h, r, True) for k in (1, 2, 3, 4) for c0, h in ((1, 1), (2, 1), (4, 2)) for r in (2, 4)}
