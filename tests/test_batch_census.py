"""Batched-plan census (CPU): which level kernels only a batched plan reaches.

A batched plan lays the row variable B (cardinality R = rows_per_launch) out as
the fastest dimension of every message evidence reaches, a layout no other
planner produces, so R alone decides tile shape, alignment, the odd-row form
and the slab dimension of those buckets.  The instrument is bnpp.plan_batch
(the launch groups of the plan partition_batch / posterior_batch run, through
the same code).  batch_catalogue.py keeps, per level key that is not in
test_variant_census.LEVEL_KEYS, the smallest batched plan that holds it;
test_gpu_batch_variants.py runs those plans on the device.  The catalogue
sweeps plan_counts, plan_marginals_batch, plan_sample_batch and the product
groups of plan_mpe_batch as well ("call" in an entry; bc.plan dispatches on
it): the backward pass behind counts and marginals reaches further keys.
"""
import zlib

import pytest

import batch_catalogue as bc
import bnpp
from conftest import model_path
from test_variant_census import LEVEL_KEYS

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
FAM = {"generic": 0, "stream": 1, "slab": 2}

# the level keys batched plans reach beyond LEVEL_KEYS (frozen; a planner change
# that moves a B-extended bucket onto another kernel shows here)
BATCH_ONLY_KEYS = {
    "f64": [
        82, 137, 146, 185, 546, 1106, 1209, 1570, 4388, 4418, 4644, 5441, 5442, 6433, 6434, 6436, 6466, 7201,
        7441, 7457, 7489, 19474, 19489, 19529, 20498, 20513, 26641, 27665, 28689],
    "f32": [
        82, 100, 137, 148, 185, 536, 546, 1106, 1209, 1570, 4388, 4420, 4648, 6434, 6436, 6466, 6468, 6948,
        6978, 6980, 7441, 7457, 7489, 17428, 19476, 19521, 19746, 20500, 20770, 25617, 25873, 26641, 26897,
        27153, 27665, 27921, 28177, 28689, 28945, 29201],
}
# the keys a host-only sweep found before the catalogue existed: the least the lists above hold
FIRST_FOUND = {
    "f64": [1209, 1570, 4388, 4418, 5441, 6433, 19474, 20498, 26641, 27665, 28689],
    "f32": [1209, 1570, 4388, 4420, 6978, 19476, 20500, 25873, 26641, 26897, 27153, 27665, 27921, 28177, 28689,
            28945, 29201],
}
# the keys of plan_batch's own entries (the lists above before the other plan functions were swept), and the
# keys the backward pass of plan_counts / plan_marginals_batch was first seen to reach: the least they add
BATCH_ONLY_BEFORE = {
    "f64": [
        137, 146, 185, 546, 1209, 1570, 4388, 4418, 4644, 5441, 5442, 6433, 7441, 7457, 7489, 19474, 19489,
        19529, 20498, 26641, 27665, 28689],
    "f32": [
        137, 148, 185, 536, 546, 1209, 1570, 4388, 4420, 6466, 6978, 7441, 7457, 7489, 19476, 19521, 19746,
        20500, 25617, 25873, 26641, 26897, 27153, 27665, 27921, 28177, 28689, 28945, 29201],
}
MINIMUM = {"f64": [82, 1106], "f32": [82, 100, 1106, 6948, 6980, 17428]}
# fp32 key 4648 (stream): with plain evidence only plans of Water hold it (R = 2, one evidence variable), and
# those variables' assignments do not pass the fp32 row condition; with that variable partial (a missing cell
# sums it out: its row's Z is large) the rows of Water's variable 11 pass, and the key has an entry.
# fp64 stream 5924 and fp32 stream 5956: only counts / marginals plans of Water hold them, at R = 1 itself, so
# no case has an R = 1 control made of held kernels (batch_catalogue.py, Calls); they stay "no plan found" too.


@pytest.fixture(scope="module")
def cat():
    return bc.load()


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = bnpp.Model.load(model_path(name + ".uai"))
        return cache[name]
    return get


def test_entries_still_plan_to_their_keys(cat, models):
    """Drift: every frozen case still launches the kernel it was recorded for,
    in a plan of the recorded size."""
    moved = []
    for e in cat["entries"]:
        st, groups = bc.plan(bnpp, e, model=models(e["model"]))
        vb = [g["vblocks"] for g in groups if g["key"] == e["key"]]
        if not vb or max(vb) != e["vblocks"] or int(st["arena_bytes"]) != e["arena_bytes"] or st["rows_per_launch"] != e["R"]:
            moved.append((e["dtype"], e["key"], e["model"], e["ev_vars"], e["R"], bc.sum_keys(groups)))
        assert bc.family_of(e["key"]) == e["family"]
    assert not moved, moved[:5]


def test_frozen_keys(cat):
    for dt in ("f64", "f32"):
        got = sorted({e["key"] for e in cat["entries"] if e["dtype"] == dt})
        assert got == BATCH_ONLY_KEYS[dt], (dt, sorted(set(got) ^ set(BATCH_ONLY_KEYS[dt])))
        assert not set(got) & set(LEVEL_KEYS[dt])
        assert set(FIRST_FOUND[dt]) <= set(got), (dt, sorted(set(FIRST_FOUND[dt]) - set(got)))
        # a key plan_batch supplies keeps its plan_batch entry
        calls = {e["key"]: bc.call_of(e) for e in cat["entries"] if e["dtype"] == dt}
        newer = {e["key"] for e in cat["entries"] if e["dtype"] == dt and "call" in e}    # another call or form
        assert newer == set(got) - set(BATCH_ONLY_BEFORE[dt]), dt
        for k in MINIMUM[dt]:                              # the cases the backward pass was first seen to reach
            assert calls[k] in ("counts", "marginals"), (dt, k)
        # one entry per key, but for the fp64 cases added for their impossible row
        plain = [e["key"] for e in cat["entries"] if e["dtype"] == dt and "extra" not in e]
        assert len(plain) == len(set(plain))
    assert len(FIRST_FOUND["f64"]) == 11 and len(FIRST_FOUND["f32"]) == 17


def test_every_swept_key_is_instantiated(cat, models):
    """Every sum-kernel key any plan of the catalogue's sweep held, and every key
    of the entries' plans as they plan now, is in its family's level dispatch
    switch: a batched plan cannot ask for a kernel that does not exist."""
    inst = {dt: {f: set(bnpp.kernel_keys(DT[dt], FAM[f], level=True)) for f in FAM} for dt in DT}
    for dt in DT:
        assert set(BATCH_ONLY_KEYS[dt]) <= set(cat["swept"][dt])
        missing = [k for k in cat["swept"][dt] if k not in inst[dt][bc.family_of(k)]]
        assert not missing, (dt, missing)
    for e in cat["entries"]:
        _, groups = bc.plan(bnpp, e, model=models(e["model"]))
        missing = [k for k in bc.sum_keys(groups) if k not in inst[e["dtype"]][bc.family_of(k)]]
        assert not missing, (e["dtype"], e["model"], e["ev_vars"], e["R"], missing)


def test_rows(cat, models):
    """The stored rows: in range, distinct, n_rows two launches with a padded
    second one; an fp64 partition entry and an fp64 posterior entry hold an
    impossible row beside possible ones."""
    for e in cat["entries"]:
        cards = models(e["model"]).cards
        assert 1 <= len(e["rows"]) <= bc.MAX_DISTINCT and len({tuple(r) for r in e["rows"]}) == len(e["rows"])
        part = e.get("partial") or []
        assert all(len(r) == len(e["ev_vars"]) and all(0 <= x < cards[v] or (x == bc.MISSING and v in part)
                                                         for x, v in zip(r, e["ev_vars"])) for r in e["rows"])
        if part:                                          # seeded missing cells, about a quarter, some observed
            assert set(part) <= set(e["ev_vars"]) and bc.call_of(e) in ("batch", "sample") and e["soft"] is None
            cells = [x for r in e["rows"] for x, v in zip(r, e["ev_vars"]) if v in part]
            assert bc.MISSING in cells and any(x != bc.MISSING for x in cells)
            full = bc.assignments(cards, e["ev_vars"], zlib.crc32(repr((e["model"], e["ev_vars"])).encode()))
            punched = bc.punch(full, [e["ev_vars"].index(v) for v in part], e["miss_seed"])
            assert all(r in punched for r in e["rows"]) and (e["dtype"] == "f32" or e["rows"] == punched)
        assert 1 <= len(e["ev_vars"]) <= 4 and e["target"] not in e["ev_vars"]
        assert e["n_rows"] == bc.n_rows_of(e["R"]) and e["R"] < e["n_rows"] <= 2 * e["R"] + 2
        assert len(bc.rows_of(e)) == e["n_rows"]
    for posterior in (False, True):                   # -inf / 0 of a partition, the NaN row of a posterior
        assert any(e["mixed_launch"] and (e["target"] is not None) == posterior for e in cat["entries"] if e["dtype"] == "f64")
    assert not any(e["mixed_launch"] for e in cat["entries"] if e["dtype"] == "f32")
    for dt in DT:
        for fam in FAM:
            sel = [e for e in cat["entries"] if e["dtype"] == dt and e["family"] == fam]
            assert sel, (dt, fam)
            big = cat["entries"][cat["capped"][dt + " " + fam]]
            assert big in sel and big["vblocks"] == max(e["vblocks"] for e in sel)


def test_fp32_control_is_made_of_compared_kernels(cat, models):
    """R = 1 of every fp32 entry's model, evidence set and target holds only
    keys of LEVEL_KEYS["f32"], kernels the suite already compares bit for bit:
    the fp32 GPU comparison of an entry's R with R = 1 has a known side."""
    for e in cat["entries"]:
        if e["dtype"] == "f32" and "call" not in e:
            _, groups = bc.plan(bnpp, e, model=models(e["model"]), R=1)
            assert set(bc.sum_keys(groups)) <= set(LEVEL_KEYS["f32"]), (e["model"], e["ev_vars"], bc.sum_keys(groups))
    # an entry of another call, in either dtype (its fp64 comparison with R = 1 is the new one): the R = 1 plan
    # of its own plan function holds only LEVEL_KEYS and the keys of plan_batch's entries, which
    # test_gpu_batch_variants.py holds to bits against the single calls
    for e in cat["entries"]:
        if "call" in e:
            ok = set(LEVEL_KEYS[e["dtype"]]) | {x["key"] for x in cat["entries"]
                                                if x["dtype"] == e["dtype"] and "call" not in x}
            _, groups = bc.plan(bnpp, e, model=models(e["model"]), R=1)
            assert set(bc.sum_keys(groups)) <= ok, (e["call"], e["model"], e["ev_vars"], bc.sum_keys(groups))
            assert e["soft"] is None and (e["target"] is None or bc.call_of(e) == "batch")


def test_plans_of_test_gpu_batch_reach_no_other_kernel(models):
    """Today's reach, recorded: the plans tests/test_gpu_batch.py runs -- its
    six models at the automatic R of 67 rows (128), alarm at R = 1, 16, 64 too,
    the posteriors at 128, 16 and 1, the cached-job and CLI calls -- hold only
    keys of LEVEL_KEYS, with one exception: the fp64 posterior of noisyor_30_40
    at R = 1 (the rows-per-launch rerun of test_posterior_batch) holds key 1570.
    Apart from that launch those tests run no level kernel the single-call
    tests do not run; the catalogue's cases do."""
    from bnpp import synth
    import test_gpu_batch as tb
    held = {"f64": set(), "f32": set()}

    def add(name, ev, target, R, dts=("f64", "f32")):
        for dt in dts:
            _, groups, _ = bnpp.plan_batch(models(name), ev, target=target, dtype=DT[dt], rows_per_launch=R)
            held[dt] |= set(bc.sum_keys(groups))

    for name in tb.MODELS:
        if name in tb.EV_VARS:
            ev = tb.EV_VARS[name]
        else:
            ev = sorted(tb._zero_entry(synth.read_uai(model_path(name + ".uai")))[0])
        add(name, ev, None, 128)
        if name == "alarm":
            for R in (1, 16, 32, 64):
                add(name, ev, None, R)
            add(name, [3, 10, 20], None, 32, ("f64",))
            add(name, [], None, 8, ("f64",))
        if name == "asia":
            add(name, ev, None, 4, ("f64",))                 # the CLI's three rows
        if name in tb.TARGET:
            for R in (128, 16, 1):
                add(name, ev, tb.TARGET[name], R, ("f64", "f32") if R == 128 else ("f64",))
    beyond = {"f64": {1570}, "f32": set()}
    for dt in DT:
        assert held[dt] and held[dt] - set(LEVEL_KEYS[dt]) == beyond[dt], (dt, sorted(held[dt] - set(LEVEL_KEYS[dt])))
        print("test_gpu_batch.py plans, %s: %d sum-kernel keys, %d outside LEVEL_KEYS" % (dt, len(held[dt]), len(beyond[dt])))
    _, groups, _ = bnpp.plan_batch(models("noisyor_30_40"), tb.EV_VARS["noisyor_30_40"], target=tb.TARGET["noisyor_30_40"],
                                   rows_per_launch=1)
    assert 1570 in bc.sum_keys(groups)


# the level keys outside LEVEL_KEYS that the whole-run plans of the other batched calls' GPU tests hold today
# (frozen; see the test below)
OTHER_TESTS_BEYOND = {
    "f64": [1209, 1570, 19474, 20498, 26641, 27665],
    "f32": [1209, 1570, 17428, 19476, 20500, 26641, 26897, 27153, 27665, 27921],
}
OTHER_TESTS_R = (1, 3, 7, 8, 16, 32, 64, 128, 256, 512)


def test_plans_of_the_other_batched_tests_reach_these_kernels(models):
    """Today's reach, recorded, of a model of the whole-run plans of
    test_gpu_counts.py, test_gpu_marginals_batch.py, test_gpu_sample_batch.py,
    test_gpu_missing.py and test_gpu_soft.py -- not those tests' own argument
    lists (test_gpu_sample_batch.py takes test_gpu_batch's evidence sets, K in
    {1, 3, 5, 257} and R = 67, 257; test_gpu_soft.py up to three soft variables
    and cases without evidence), so drift in them does not show here: the eight models and evidence variables of
    counts_ref.EV_VARS through plan_counts, plan_marginals_batch,
    plan_sample_batch, plan_mpe_batch and plan_batch, with plain evidence, with
    all, the last and all but the first evidence variable partial, and with the
    lowest non-evidence variable soft (alone and beside all partial), at the
    rows per launch those tests name (1, 3, 7, 8, 16, 32, 64) and the automatic
    ones of their 5 to 257 rows (8 to 512).  Those tests compare whole results
    to 1e-12 / 1e-5; the catalogue's cases hold the kernels to bits.  A planner
    change that moves one of these plans onto another kernel shows here."""
    from counts_ref import EV_VARS
    held, found = {"f64": set(), "f32": set()}, {}
    for name, ev in sorted(EV_VARS.items()):
        m = models(name)
        soft = [min(v for v in range(m.n_vars) if v not in ev)]
        forms = [(None, None), (ev, None), (ev[-1:], None), (ev[1:], None), (None, soft), (ev, soft)]
        for call in bc.CALLS:
            for partial, sv in forms:
                for dt in DT:
                    for R in OTHER_TESTS_R:
                        e = {"dtype": dt, "model": name, "ev_vars": ev, "target": None, "R": R, "no_o32": False,
                             "call": call, "partial": partial, "soft": sv}
                        try:
                            _, groups = bc.plan(bnpp, e, model=m)
                        except bnpp.BnppError:
                            continue
                        held[dt] |= set(bc.sum_keys(groups))
    for dt in DT:
        beyond = sorted(held[dt] - set(LEVEL_KEYS[dt]))
        print("other batched tests' plans, %s: %d sum-kernel keys, outside LEVEL_KEYS: %s" % (dt, len(held[dt]), beyond))
        found[dt] = beyond
    for dt in DT:
        assert held[dt] and found[dt] == OTHER_TESTS_BEYOND[dt], (dt, found[dt])
        assert set(found[dt]) <= set(BATCH_ONLY_KEYS[dt]), dt      # each is held to bits by a catalogue entry
