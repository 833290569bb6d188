"""Catalogue of the smallest batched-evidence plans that launch a level kernel
no single-call plan of the suite launches (a helper, like variant_catalogue.py
and chain_catalogue.py; CPU only).

A batched plan (bnpp.plan_batch) carries the row variable B of cardinality R =
rows_per_launch as the fastest dimension of every message evidence reaches, so
R alone picks tile shapes, the odd-row forms and the slab dimension of those
buckets.  A case is a fixture model, a set of evidence variables, a target (or
None: the partition), R, a dtype and the offset-width switch.  regenerate()
sweeps

  models   MODELS: the fixture models of test_variant_census.FAST_PR with at
           most 80 variables
  evidence every single variable, and seeded random sets of 2, 3 and 4
           variables (SETS_PER_SIZE each); for the Bayesian networks also the
           scope of the first CPT with a zero entry (an impossible assignment)
  queries  the partition, and the posterior of the smallest variable that is
           not evidence
  R        R_LIST
  dtypes   both; BNPP_NO_O32=1 as well, where only generic keys are recorded
           (the switch moves generic launches only)

and reads every plan's launch-group keys.  For every sum-kernel key (generic /
stream / slab) that is not in test_variant_census.LEVEL_KEYS[dtype] it keeps
the case with the smallest arena_bytes (ties: smaller R, then model, evidence
set, partition before posterior) that passes the conditions below, among plans
of at most MAX_ARENA bytes.

Rows.  The distinct assignments of the evidence variables in lexicographic
order, all of them up to 64, else a seeded sample of 64; `rows` holds them and
rows_of() cycles them to n_rows = R + 3 (R <= 256) or R + 1: two launches, the
second padded.

  fp64  every assignment is kept, impossible ones (oracle Z == 0) included;
        regenerate() asserts that a launch of some fp64 partition entry
        and of some fp64 posterior entry holds an impossible row beside
        possible ones, and where no smallest case does, adds one more entry
        ("extra") for it: the smallest case over the scope of a zero CPT entry.
  fp32  only assignments whose oracle (refcpu, fp64) Z is positive and at most
        2^30 below the largest are kept, so a launch stays inside the shared
        scale limit of DESIGN 12.  A case that keeps fewer than four of them
        is skipped -- or fewer than all, where the evidence variables have
        fewer than four assignments in the first place (one binary variable
        has two).  The R = 1 plan of the same model, evidence set and target
        must hold only keys of LEVEL_KEYS["f32"]: the control of the GPU
        comparison is then made of kernels the suite already holds to bits.

Calls.  Beside bnpp.plan_batch the sweep plans the same models, evidence sets,
R, dtypes and offset widths through bnpp.plan_counts, plan_marginals_batch (all
variables as targets), plan_sample_batch (SAMPLE_K = 2 draws) and
plan_mpe_batch (its product groups only: the max keys have their own census,
mpe_level_catalogue.py).  Their forward sweeps are plan_batch's; the backward
pass of the bucket tree (counts, marginals) lays B-carrying buckets out anew.
An entry of those calls has "call" (an entry without it means "batch"),
"partial" and "soft" (both null: see Forms).  A key plan_batch supplies keeps
its plan_batch entry, chosen as before; the other calls add entries only for
the keys plan_batch does not reach, by the same rule (smallest arena; ties:
smaller R, model, evidence set, then the order of CALLS).  Conditions of such
an entry, in both dtypes: the fp32 row condition above (fp32), and the R = 1
plan of the same call holds only keys of LEVEL_KEYS[dtype] and of plan_batch's
entries, which test_gpu_batch_variants.py holds to bits against the single
calls -- the GPU comparison of the entry's R with R = 1 then has a known side.
Found: keys 82 and 1106 (both dtypes), 100 (fp32), 6434 (both), 6466 and 7201
(fp64), 6948, 6980 and 17428 (fp32), all through counts or marginals; the
sample and mpe plans hold no key the others do not.  Not catalogued because no
case passes the R = 1 control (every plan of Water that holds them has an
R = 1 plan with a key outside the held set): fp64 stream 5924 and fp32 stream
5956; they stay "no plan found" in test_variant_census.UNREACHED_LEVEL.

Forms.  Every call is swept with plain evidence (no partial and no soft
variable); plan_batch and plan_sample_batch also with the last evidence
variable partial ("last") and with every one partial ("all"): FORMS.  All five
forms of all five calls take more than ten minutes on 8 cores (a keys-only
probe of the four other forms alone took 588 s), so the forms whose families
hold no key beyond the others' are left out -- by that probe: one soft variable
for plan_batch, plan_sample_batch and plan_mpe_batch; all partial + soft for
every call; every partial or soft form of plan_mpe_batch; all partial for
plan_counts and plan_marginals_batch.  Also left out, though the probe saw a
key there: last-partial and soft evidence for plan_counts and
plan_marginals_batch, whose only keys beyond the catalogue are fp64 5924 and
fp32 5956, held at R = 1 itself by plans of Water (so no R = 1 control can be
made of held kernels, as with plain evidence).

An entry with partial variables has "call", "partial" (the variable ids) and
"miss_seed": its rows are the distinct assignments with each cell of a partial
variable MISSING with probability MISSING_FRAC, drawn by punch() from
random.Random(miss_seed), duplicates dropped; a case needs a missing and an
observed partial cell.  The oracle Z of such a row is that of its observed
entries, and the fp32 row condition and "mixed_launch" use it.  The entries
found: fp64 6436 and 6466 (insurance, both of [0, 8] partial, posterior of 1,
R = 2 and 4; 6466 replaces the larger marginals entry), fp64 20513 (Water, [5]
partial, R = 2), fp32 6436 and 6468 (insurance, as fp64), fp32 20770 (Water,
[4, 31] partial, R = 2) and fp32 4648 (Water, [11] partial, R = 2: with plain
evidence no case of this key passed the fp32 row condition; a missing cell
sums the variable out, and its rows pass).  plan_sample_batch's partial plans
hold 4648 and 20770 too, in larger arenas, so every entry is plan_batch's and
no entry has "call": "sample".  No key the partial sweep found is left out.

batch_catalogue_data.json holds the entries, per dtype every sum-kernel key
any plan of the sweep held ("swept": test_batch_census.py checks them against
the dispatch switches), and per (dtype, family) the index of the entry whose
key's launch group has the most virtual blocks ("capped": the entry
test_gpu_batch_variants.py reruns on capped grids).
"""
import itertools
import json
import os
import random
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "batch_catalogue_data.json")
R_LIST = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 20, 24, 32, 63, 64, 65, 66, 67, 96, 100, 128, 256, 512, 1000, 1024)
MAX_VARS = 80
MAX_ARENA = 8 << 20
MAX_DISTINCT = 64
SETS_PER_SIZE = 8
KEEP = 24                      # candidates kept per key for the second pass
SPAN_LOG2 = 30
FAMILIES = ("generic", "stream", "slab")


def load():
    with open(DATA) as f:
        return json.load(f)


def family_of(key):
    """The sum-kernel family of a launch-group key, or None (gather steps, chain keys)."""
    return "slab" if 16384 <= key < (1 << 24) else "stream" if 4096 <= key < 8192 else "generic" if 0 <= key < 4096 else None


def sum_keys(groups):
    return sorted({g["key"] for g in groups if family_of(g["key"])})


class no_o32:
    """BNPP_NO_O32 set for a with-block (read by the planner at every call)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("BNPP_NO_O32")
        os.environ["BNPP_NO_O32"] = "1" if self.on else "0"

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["BNPP_NO_O32"]
        else:
            os.environ["BNPP_NO_O32"] = self.old


CALLS = ("batch", "counts", "marginals", "sample", "mpe")
SAMPLE_K = 2                   # draws per row of the "sample" entries
MAX_KEY_BASE = 65536           # the max family's keys start here (plan_mpe_batch: product groups only are recorded)


def call_of(e):
    return e.get("call", "batch")


def plan(bnpp, e, model=None, R=None):
    """The plan function of a catalogue entry's call (at another R if given) -> (stats, groups):
    bnpp.plan_batch (an entry without "call"), plan_counts, plan_marginals_batch (all variables),
    plan_sample_batch (SAMPLE_K draws) or plan_mpe_batch, whose max groups are left out."""
    from conftest import model_path
    m = model or bnpp.Model.load(model_path(e["model"] + ".uai"))
    kw = dict(dtype=bnpp.F32 if e["dtype"] == "f32" else bnpp.F64, rows_per_launch=e["R"] if R is None else R,
              partial=e.get("partial"), soft=e.get("soft"))
    call = call_of(e)
    with no_o32(e["no_o32"]):
        if call == "batch":
            res = bnpp.plan_batch(m, e["ev_vars"], target=e["target"], **kw)
        elif call == "counts":
            res = bnpp.plan_counts(m, e["ev_vars"], **kw)
        elif call == "marginals":
            res = bnpp.plan_marginals_batch(m, e["ev_vars"], **kw)
        elif call == "sample":
            res = bnpp.plan_sample_batch(m, e["ev_vars"], SAMPLE_K, **kw)
        else:
            assert call == "mpe", call
            res = bnpp.plan_mpe_batch(m, e["ev_vars"], **kw)
    groups = res[1] if call != "mpe" else [g for g in res[1] if not MAX_KEY_BASE <= g["key"] < (1 << 24)]
    return res[0], groups


def rows_of(e):
    """The (n_rows, n_ev) evidence rows of an entry: its distinct assignments, cycled."""
    return [e["rows"][i % len(e["rows"])] for i in range(e["n_rows"])]


def n_rows_of(R):
    return R + 3 if R <= 256 else R + 1


# -------------------------------------------------------------------- sweep
def models():
    import bnpp
    from conftest import model_path
    from test_variant_census import FAST_PR
    out = []
    for f in FAST_PR:
        if bnpp.Model.load(model_path(f)).n_vars <= MAX_VARS:
            out.append(f[:-len(".uai")])
    return out


def zero_scope(d):
    """The scope of the first CPT of 2-4 variables with an entry that is exactly 0, or None."""
    for s, v in zip(d["scopes"], d["values"]):
        if 2 <= len(s) <= 4 and any(x == 0 for x in v):
            return sorted(s)
    return None


def ev_sets(name, d):
    n = len(d["cards"])
    rng = random.Random(zlib.crc32(name.encode()))
    sets = [[v] for v in range(n)]
    for size in (2, 3, 4):
        if size < n:
            for _ in range(SETS_PER_SIZE):
                sets.append(sorted(rng.sample(range(n), size)))
    if d["type"] == "BAYES":
        z = zero_scope(d)
        if z is not None and len(z) < n:
            sets.append(z)
    out = []
    for s in sets:
        if s not in out:
            out.append(s)
    return out


# the evidence forms swept per call (Forms in the module docstring): "last" the last evidence variable
# partial, "all" every one
FORMS = {"batch": ("plain", "last", "all"), "counts": ("plain",), "marginals": ("plain",),
         "sample": ("plain", "last", "all"), "mpe": ("plain",)}
MISSING = -1                   # bnpp.MISSING (BNPP_MISSING)
MISSING_FRAC = 0.25


def scan_model(task):
    """Every plan of one model, call and evidence form: ({(dtype, key): [(cost, case)]}, the same
    for the cases over a zero entry's scope alone, {dtype: keys held by any plan})."""
    name, call, form = task
    plain = call == "batch" and form == "plain"          # the sweep as it was before the other calls and forms
    import bnpp
    from bnpp import synth
    from conftest import model_path
    from test_variant_census import LEVEL_KEYS
    path = model_path(name + ".uai")
    m, d = bnpp.Model.load(path), synth.read_uai(path)
    known = {dt: set(LEVEL_KEYS[dt]) for dt in LEVEL_KEYS}
    cand, zero, swept = {}, {}, {"f64": set(), "f32": set()}
    zscope = zero_scope(d) if d["type"] == "BAYES" else None
    for ev in ev_sets(name, d):
        free = [v for v in range(m.n_vars) if v not in ev]
        for target in ((None, free[0]) if call == "batch" else (None,)):
            for dt in ("f64", "f32"):
                for o32off in (False, True):
                    control = None               # batch, fp32: does the R = 1 plan hold LEVEL_KEYS keys only?
                    r1 = None                    # the other calls: the R = 1 plan's keys (regenerate() judges them)
                    for R in R_LIST:
                        e = {"dtype": dt, "model": name, "ev_vars": ev, "target": target, "R": R, "no_o32": o32off}
                        if not plain:
                            e.update(call=call, partial=None if form == "plain" else ev[-1:] if form == "last" else ev,
                                     soft=None)
                        try:
                            st, groups = plan(bnpp, e, model=m)
                        except bnpp.BnppError:
                            continue
                        if R == 1:
                            control = not plain or set(sum_keys(groups)) <= known["f32"]
                            r1 = sum_keys(groups)
                        for key in sum_keys(groups):
                            fam = family_of(key)
                            if o32off and fam != "generic":
                                continue
                            swept[dt].add(key)
                            if key in known[dt] or st["arena_bytes"] > MAX_ARENA or (dt == "f32" and not control):
                                continue
                            if not plain and r1 is None:
                                continue
                            vb = max(g["vblocks"] for g in groups if g["key"] == key)
                            cost = (not plain, int(st["arena_bytes"]), R, name, ev, target is not None, o32off,
                                    CALLS.index(call), FORMS[call].index(form))
                            case = dict(e, key=key, family=fam, arena_bytes=int(st["arena_bytes"]), vblocks=int(vb))
                            if not plain:
                                case["r1_keys"] = r1
                            if ev == zscope and plain:
                                zero.setdefault((dt, key), []).append((cost, case))
                            lst = cand.setdefault((dt, key), [])
                            lst.append((cost, case))
                            if len(lst) > 4 * KEEP:
                                lst.sort(key=lambda c: c[0])
                                del lst[KEEP:]
    return cand, zero, swept


def search(procs=None):
    import multiprocessing as mp
    cand, zero, swept = {}, {}, {"f64": set(), "f32": set()}
    with mp.Pool(procs or min(16, os.cpu_count() or 4)) as pool:
        for c, z, s in pool.imap_unordered(scan_model, [(n, c, f) for c in CALLS for f in FORMS[c] for n in models()]):
            for dt in s:
                swept[dt] |= s[dt]
            for k, lst in c.items():
                cand.setdefault(k, []).extend(lst)
            for k, lst in z.items():
                zero.setdefault(k, []).extend(lst)
    for lst in cand.values():
        lst.sort(key=lambda c: c[0])
    return cand, zero, swept


# ------------------------------------------------------------ rows, conditions
def assignments(cards, ev_vars, seed):
    """The distinct assignments of ev_vars, lexicographic; over 64, a seeded sample of 64 of them."""
    ranges = [range(cards[v]) for v in ev_vars]
    total = 1
    for r in ranges:
        total *= len(r)
    if total <= MAX_DISTINCT:
        return [list(a) for a in itertools.product(*ranges)]
    picks = sorted(random.Random(seed).sample(range(total), MAX_DISTINCT))
    out = []
    for p in picks:
        a = []
        for r in reversed(ranges):
            p, x = divmod(p, len(r))
            a.insert(0, x)
        out.append(a)
    return out


class Oracle:
    """refcpu's fp64 Z per (model, evidence assignment), computed once."""

    def __init__(self):
        self.models, self.z = {}, {}

    def partition(self, name, ev_vars, a):
        import refcpu
        from conftest import model_path
        k = (name, tuple(ev_vars), tuple(a))
        if k not in self.z:
            if name not in self.models:
                self.models[name] = refcpu.Model.load(model_path(name + ".uai"))
            self.z[k] = self.models[name].partition(dict(zip(ev_vars, a)), "mf")[0]
        return self.z[k]


def punch(rows, cols, seed):
    """The rows with about MISSING_FRAC of the cells of `cols` MISSING (random.Random(seed), row by row, column
    by column), duplicates dropped; None unless some cell of `cols` is missing and some is observed."""
    rng = random.Random(seed)
    out = []
    for r in rows:
        r = list(r)
        for j in cols:
            if rng.random() < MISSING_FRAC:
                r[j] = MISSING
        if r not in out:
            out.append(r)
    cells = [r[j] for r in out for j in cols]
    return out if MISSING in cells and any(x != MISSING for x in cells) else None


def choose_rows(case, cards, oracle):
    """(the distinct assignments an entry runs, their oracle Z) or None when the
    fp32 row condition leaves too few."""
    ev = case["ev_vars"]
    allrows = assignments(cards, ev, zlib.crc32(repr((case["model"], ev)).encode()))
    if case.get("partial"):
        allrows = punch(allrows, [ev.index(v) for v in case["partial"]], case["miss_seed"])
        if allrows is None:
            return None
    z = [oracle.partition(case["model"], [v for v, x in zip(ev, a) if x != MISSING], [x for x in a if x != MISSING])
         for a in allrows]
    if case["dtype"] == "f64":
        return allrows, z
    top = max(z)
    keep = [i for i in range(len(z)) if z[i] > 0 and z[i] * 2.0 ** SPAN_LOG2 > top]
    if len(keep) < min(4, len(allrows)):
        return None
    return [allrows[i] for i in keep], [z[i] for i in keep]


def finish(case, rows, z):
    """The catalogue entry of a case: its rows, and whether one of its two launches
    holds an impossible row (oracle Z == 0) beside possible ones."""
    e = dict(case, rows=rows, n_rows=n_rows_of(case["R"]))
    zs = [z[i % len(z)] for i in range(e["n_rows"])]
    launches = (zs[:case["R"]], zs[case["R"]:])
    e["mixed_launch"] = bool(case["dtype"] == "f64" and any(min(l) == 0 and max(l) > 0 for l in launches))
    return e


def control_ok(bnpp, case, model):
    """fp32: the R = 1 plan of the case holds only keys the suite already compares bit for bit."""
    from test_variant_census import LEVEL_KEYS
    _, groups = plan(bnpp, case, model=model, R=1)
    return set(sum_keys(groups)) <= set(LEVEL_KEYS["f32"])


def regenerate(path=DATA):
    """Rebuild the frozen table (needs the built library and the oracle; 206 s on 8 cores)."""
    import bnpp
    from bnpp import synth
    from conftest import model_path
    from test_variant_census import LEVEL_KEYS
    cand, zero, swept = search()
    oracle = Oracle()
    loaded = {}
    entries, dropped = [], []
    # plan_batch's keys first: a key plan_batch supplies keeps its plan_batch entry, and those keys, with
    # LEVEL_KEYS, are the kernels the R = 1 control of another call's entry may hold
    order = sorted(cand, key=lambda k: (cand[k][0][0][0], k))
    held = {dt: set(LEVEL_KEYS[dt]) for dt in LEVEL_KEYS}
    for (dt, key) in order:
        chosen = None
        for cost, case in cand[(dt, key)]:
            if cost[0]:                          # a call other than plan_batch
                held_now = held[dt] | {e["key"] for e in entries if e["dtype"] == dt and "call" not in e}
                case = dict(case)
                if not set(case.pop("r1_keys")) <= held_now:
                    dropped.append((dt, key, case["model"], case["ev_vars"], case["R"],
                                    "%s %s R = 1 control" % (case["call"], case["partial"])))
                    continue
            name = case["model"]
            if name not in loaded:
                p = model_path(name + ".uai")
                loaded[name] = (bnpp.Model.load(p), synth.read_uai(p))
            m, d = loaded[name]
            if dt == "f32" and "call" not in case and not control_ok(bnpp, case, m):
                dropped.append((dt, key, name, case["ev_vars"], case["R"], "R = 1 control"))
                continue
            if case.get("partial"):
                case = dict(case, miss_seed=zlib.crc32(repr((name, case["ev_vars"], case["partial"])).encode()))
            got = choose_rows(case, d["cards"], oracle)
            if got is None:
                dropped.append((dt, key, name, case["ev_vars"], case["R"], "rows"))
                continue
            rows, z = got
            chosen = finish(case, rows, z)
            break
        if chosen is None:                       # stays "no plan found" in the level census
            dropped.append((dt, key, "-", [], 0, "no case of this key passes the conditions"))
            continue
        entries.append(chosen)
    for posterior in (False, True):
        # a partition and a posterior with an impossible row (-inf / 0, a NaN row): where no smallest case
        # holds one, one more fp64 entry, the smallest case over a zero entry's scope whose launch mixes
        # an impossible row with possible ones
        if any(e["mixed_launch"] and (e["target"] is not None) == posterior for e in entries
               if e["dtype"] == "f64" and "call" not in e):
            continue
        for _, case in sorted((c for k, lst in zero.items() if k[0] == "f64" for c in lst), key=lambda c: c[0]):
            if (case["target"] is not None) != posterior or "call" in case:
                continue
            d = synth.read_uai(model_path(case["model"] + ".uai"))
            e = finish(case, *choose_rows(case, d["cards"], oracle))
            if e["mixed_launch"]:
                entries.append(dict(e, extra="impossible row"))
                break
    for posterior in (False, True):
        assert any(e["mixed_launch"] and (e["target"] is not None) == posterior for e in entries
                   if e["dtype"] == "f64" and "call" not in e), \
            "no fp64 entry mixes an impossible row with possible ones"
    entries.sort(key=lambda e: (e["dtype"], e["key"], "extra" in e))
    capped = {}
    for i, e in enumerate(entries):
        k = e["dtype"] + " " + e["family"]
        if k not in capped or e["vblocks"] > entries[capped[k]]["vblocks"]:
            capped[k] = i
    for dt, dtype in (("f64", bnpp.F64), ("f32", bnpp.F32)):
        for fi, fam in enumerate(FAMILIES):
            inst = set(bnpp.kernel_keys(dtype, fi, level=True))
            held = {k for k in swept[dt] if family_of(k) == fam}
            assert held <= inst, ("a batched plan holds a key no dispatch switch has", dt, fam, sorted(held - inst))
    with open(path, "w") as f:
        f.write('{"capped": %s,\n' % json.dumps(capped, sort_keys=True))
        f.write('"swept": %s,\n' % json.dumps({dt: sorted(swept[dt]) for dt in sorted(swept)}, sort_keys=True))
        f.write('"entries": [\n')
        f.write(",\n".join(json.dumps(e, sort_keys=True) for e in entries))
        f.write("\n]}\n")
    return entries, dropped


if __name__ == "__main__":
    import sys
    import time
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401  (puts the package and the oracle on sys.path)
    t0 = time.time()
    ents, drop = regenerate()
    for x in drop:
        print("skipped", x)
    print(len(ents), "entries in %.0f s" % (time.time() - t0))
