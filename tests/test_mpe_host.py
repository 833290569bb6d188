"""CPU tests of MPE's host side: the numpy reference against itself, the
MPE plan (bnpp_plan_mpe_groups: max buckets, one traceback step; arena),
the census of the max kernel family (max_catalogue.py: single ops;
mpe_level_catalogue.py: the same keys as level launches of whole plans, in
both offset widths) and the card limit."""
import json
import math
import os

import pytest

import bnpp
import max_catalogue as mc
import mpe_level_catalogue as ml
import mpe_ref
from bnpp import synth
from conftest import GOLDEN, evidence_of, model_path

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
DECODE_KEY = (1 << 24) + 4096
SMALL = [("ising4x4", "-"), ("grid3x3", "-"), ("grid3x3", "grid3x3-PR.uai.evid"), ("asia", "-"),
         ("asia", "asia.uai.evid"), ("cancer", "-"), ("cancer", "cancer.uai.evid"), ("earthquake", "-"),
         ("earthquake", "earthquake.uai.evid")]


def _golden():
    with open(os.path.join(GOLDEN, "mpe_golden.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name,evf", SMALL)
def test_reference_brute_force_and_max_sum_agree(name, evf):
    m = synth.read_uai(model_path(name + ".uai"))
    ev = evidence_of(evf)
    top, x, gap = mpe_ref.brute_force(m, ev)
    assert gap > 1e-3                                    # a unique maximiser: assignments are comparable
    s, xs = mpe_ref.max_sum(m, ev)
    assert xs == x
    assert abs(s - top) <= 1e-12 * max(1.0, abs(top))
    assert abs(mpe_ref.log_score(m, x) - top) <= 1e-12 * max(1.0, abs(top))
    assert all(x[v] == val for v, val in ev.items())


def test_recorded_reference_of_the_larger_models():
    """golden/mpe_golden.json is mpe_ref.max_sum's output: every record's
    assignment scores its recorded maximum, and the quick models recompute to
    the same maximum (Munin1 takes ~20 s in numpy and is only re-scored)."""
    rec = _golden()
    assert set(rec) == {n for n, _ in mpe_ref.LARGER}
    for name, evf in mpe_ref.LARGER:
        m = synth.read_uai(model_path(name + ".uai"))
        ev = evidence_of(evf) if evf else {}
        r = rec[name]
        assert r["evidence"] == evf
        assert abs(mpe_ref.log_score(m, r["assignment"]) - r["log_max"]) <= 1e-9
        assert all(r["assignment"][v] == val for v, val in ev.items())
        if name not in mpe_ref.SLOW:
            s, x = mpe_ref.max_sum(m, ev)
            assert abs(s - r["log_max"]) <= 1e-9 and x == r["assignment"]


def _separators(m, ev, order):
    """Entries of every eliminating bucket's output (its separator table),
    by a symbolic elimination of `order`."""
    cards = m["cards"]
    rank = {v: i for i, v in enumerate(order)}
    buckets = [[] for _ in order]
    for scope in m["scopes"]:
        s = [v for v in scope if v not in ev]
        if s:
            buckets[min(rank[v] for v in s)].append(s)
    sizes = []
    for i, x in enumerate(order):
        if not buckets[i]:
            continue
        sep = sorted({v for s in buckets[i] for v in s} - {x})
        sizes.append(math.prod(cards[v] for v in sep))
        if sep:
            buckets[min(rank[v] for v in sep)].append(sep)
    return sizes


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["alarm", "ising6x6"])
def test_plan_groups_of_an_mpe_plan(name, dt):
    mm = bnpp.Model.load(model_path(name + ".uai"))
    m = synth.read_uai(model_path(name + ".uai"))
    order, _ = bnpp.ordering(mm, None, "mf")
    groups = bnpp.plan_mpe_groups(mm, None, dtype=DT[dt], order=order)
    max_keys = set(bnpp.kernel_keys(DT[dt], 4, level=True))
    product_keys = set(bnpp.kernel_keys(DT[dt], 0, level=True))
    n_max = 0
    for g in groups:
        assert g["key"] in max_keys or g["key"] in product_keys or g["key"] == DECODE_KEY, g
        n_max += g["n_desc"] if g["key"] in max_keys else 0
    assert [g["key"] for g in groups].count(DECODE_KEY) == 1 and groups[-1]["key"] == DECODE_KEY
    assert groups[-1]["level"] == max(g["level"] for g in groups) and groups[-1]["n_desc"] == 1
    seps = _separators(m, {}, order)
    assert n_max == len(seps)                            # every eliminating bucket is a max bucket
    # arena: every arg table (a byte per separator entry) beside the largest message
    eb = 8 if dt == "f64" else 4
    arena = bnpp.plan_stats(mm, 4, None, dtype=DT[dt], order=order)[1]
    assert arena >= sum(seps) + max(seps) * eb
    assert arena > bnpp.plan_stats(mm, 0, None, dtype=DT[dt], order=order)[1]


def test_plan_is_the_same_for_heuristic_and_given_order():
    mm = bnpp.Model.load(model_path("alarm.uai"))
    ev = evidence_of("alarm.uai.evid")
    order, _ = bnpp.ordering(mm, ev, "mf")
    assert bnpp.plan_mpe_groups(mm, ev) == bnpp.plan_mpe_groups(mm, ev, order=order)
    with pytest.raises(bnpp.BnppError) as e:             # an MPE order covers every free variable
        bnpp.plan_mpe_groups(mm, ev, order=order[:-1])
    assert e.value.status == bnpp.ERR_INVALID


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_census_of_the_max_family(dt, monkeypatch):
    """Every key of the max family's dispatch switch (bnpp_kernel_keys family
    4, single-op and level launches hold the same list) has a catalogue bucket
    that bnpp_plan_max_single plans onto it, and the catalogue holds no other
    key: no key is unreachable, so none is listed as ruled out."""
    ents = [e for e in mc.load() if e["dtype"] == dt]
    single = bnpp.kernel_keys(DT[dt], 4)
    level = bnpp.kernel_keys(DT[dt], 4, level=True)
    assert len(single) == len(set(single)) == 24 and sorted(single) == sorted(level)
    assert bnpp.FAMILIES[mc.FAMILY_MAX] == "max"
    for other in range(4):                               # clear of every sum family's keys
        assert not set(single) & set(bnpp.kernel_keys(DT[dt], other, level=True))
    seen = set()
    for e in ents:
        monkeypatch.setenv("BNPP_NO_O32", "1" if e["no_o32"] else "0")
        info = bnpp.plan_max_single(DT[dt], e["cards"], e["scopes"], e["elim"], e["out"])
        assert info["family"] == mc.FAMILY_MAX and info["instantiated"] == 1
        assert (info["key"], info["v1"], info["v2"], info["k"], info["n_tiles"]) == \
               (e["key"], e["v1"], 1, e["k"], e["n_tiles"]), (e, info)
        assert info["o32"] == (0 if e["no_o32"] else 1)
        seen.add(info["key"])
    assert seen == set(single)
    # the catalogue's own generator gives the recorded entries
    monkeypatch.delenv("BNPP_NO_O32", raising=False)
    assert [e for e in mc.entries_for(bnpp) if e["dtype"] == dt] == ents


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_census_of_the_max_level_kernels(dt):
    """Every max key as the first launch group of a whole MPE plan
    (mpe_level_catalogue.py: the level dispatch, which shares its key list with
    the single-op one, asserted above): the entry's model, eliminated `elim`
    first, plans onto the entry's key under the entry's BNPP_NO_O32, with the
    recorded virtual blocks; the entries hold all 24 keys, 12 with the
    32-bit-offset bit and 12 without, each under one wave ("a") and over
    several workgroups ("b"); under the other switch the same model plans onto
    the key's twin.  Brute force finds one maximiser per entry, at a log gap
    above the catalogue's MIN_GAP, and max-sum in the entry's order agrees."""
    ents = ml.load()                                     # one list: the entries serve both dtypes
    level = set(bnpp.kernel_keys(DT[dt], 4, level=True))
    for e in ents:
        assert max(e["cards"]) <= 256 and all(e["elim"] in s for s in e["scopes"])
        g = ml.first_max_group(bnpp, e, DT[dt])
        assert (g["key"], g["vblocks"], g["level"]) == (e["key"], e["vblocks"], 1), (e["name"], g)
        assert bool(e["key"] & mc.O32) == (not e["no_o32"])
        twin = ml.first_max_group(bnpp, e, DT[dt], no_o32=not e["no_o32"])
        assert twin["key"] == e["key"] ^ mc.O32 and twin["vblocks"] == e["vblocks"]
        d = ml.model_dict(e)
        top, x, gap = mpe_ref.brute_force(d)
        assert gap > ml.MIN_GAP, (e["name"], gap)
        s, xs = mpe_ref.max_sum(d, order=ml.order_of(e))
        assert xs == x and abs(s - top) <= 1e-12 * max(1.0, abs(top))
    held = {e["key"] for e in ents}
    assert held == level and len(held) == 24
    assert len([k for k in held if k & mc.O32]) == len([k for k in held if not k & mc.O32]) == 12
    for key in held:
        vb = sorted(e["vblocks"] for e in ents if e["key"] == key)
        assert len(vb) == 2 and vb[0] == 1 and vb[1] > 3, (key, vb)
    # the catalogue's own generator gives the recorded entries
    if dt == "f64":
        assert ml.entries_for(bnpp) == ents
    assert {e["from"] for e in ents} == {"max_catalogue", "search"}


def test_job_cache_keys_on_the_offset_switch(monkeypatch):
    """A cached job is keyed on BNPP_NO_O32: the key of the same call differs
    between the two widths (bnpp_batch_job_key mixes the same plan switches in
    as the single calls' key does), so a context's cached 32-bit job cannot
    answer for a 64-bit run.  test_gpu_mpe_level.py checks bnpp.mpe itself: a
    switched call plans anew, a repeat does not."""
    mm = bnpp.Model.load(model_path("asia.uai"))
    keys = []
    for flag in ("0", "1", "0"):
        monkeypatch.setenv("BNPP_NO_O32", flag)
        keys.append(bnpp.batch_job_key(mm, [0, 3], rows_per_launch=4))
    assert keys[0] == keys[2] != keys[1]


def test_catalogue_holds_the_named_shapes():
    ents = mc.load()
    for dt in DT:
        es = [e for e in ents if e["dtype"] == dt]
        assert {2, 3, 7} <= {e["k"] for e in es}
        assert {1, 2, 3, 5} <= {len(e["scopes"]) for e in es}
        assert any(e["k"] == 1 for e in es) and any(e["k"] == 256 for e in es)
        assert any(e["no_o32"] for e in es)
        for key in {e["key"] for e in es}:              # a case of several workgroups per key, for the capped reruns
            assert max(e["n_tiles"] for e in es if e["key"] == key) > 3 * 256


def test_card_limit_of_the_maximised_variable():
    for dt in DT.values():
        with pytest.raises(bnpp.BnppError) as e:
            bnpp.plan_max_single(dt, [257, 3], [[0, 1]], 0, [1])
        assert e.value.status == bnpp.ERR_UNSUPPORTED
        assert bnpp.plan_max_single(dt, [256, 3], [[0, 1]], 0, [1])["k"] == 256
        # absent from every input it is a copy (k == 1), whatever its card
        assert bnpp.plan_max_single(dt, [257, 3], [[1]], 0, [1])["k"] == 1
        for card, ok in ((256, True), (257, False)):
            vals = [[1.0 + (i % 7) for i in range(card * 2)], [0.5, 0.25]]
            m = bnpp.Model.from_arrays([card, 2], [[0, 1], [1]], [v for t in vals for v in t])
            if ok:
                assert bnpp.plan_mpe_groups(m, None, dtype=dt)[-1]["key"] == DECODE_KEY
            else:
                with pytest.raises(bnpp.BnppError) as e:
                    bnpp.plan_stats(m, 4, None, dtype=dt)
                assert e.value.status == bnpp.ERR_UNSUPPORTED
                assert bnpp.plan_stats(m, 0, None, dtype=dt)     # the sum path has no such limit
                # as evidence the variable is not maximised
                assert bnpp.plan_mpe_groups(m, {0: 256}, dtype=dt)[-1]["key"] == DECODE_KEY


def test_out_of_memory_names_messages_and_arg_tables(monkeypatch):
    mm = bnpp.Model.load(model_path("ising12x12.uai"))
    monkeypatch.setenv("BNPP_MEM_BUDGET_GB", "0.0001")
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_stats(mm, 4, None)
    assert e.value.status == bnpp.ERR_OOM
    assert "messages" in str(e.value) and "arg tables" in str(e.value)


def test_bad_arguments():
    mm = bnpp.Model.load(model_path("asia.uai"))
    for kind in (4, 5):                                  # plan_groups: the sum plans only (plan_mpe_groups)
        with pytest.raises(bnpp.BnppError):
            bnpp.plan_groups(mm, kind)
    with pytest.raises(bnpp.BnppError):
        bnpp.plan_stats(mm, 5)
    with pytest.raises(bnpp.BnppError):
        bnpp.kernel_keys(bnpp.F64, 5)
    with pytest.raises(bnpp.BnppError):                  # the output scope must be the inputs' minus the variable
        bnpp.plan_max_single(bnpp.F64, [2, 3, 4], [[0, 1], [2]], 0, [1])
    with pytest.raises(bnpp.BnppError):                  # a max bucket names its variable
        bnpp.plan_max_single(bnpp.F64, [2, 3], [[0, 1]], -1, [0, 1])
    assert bnpp.ABI_VERSION == 205
