"""Catalogue of the smallest models that reach every instantiated chain-run
kernel (a helper, like variant_catalogue.py; CPU only).

A case is a small grid model, an elimination order, planning switches and a
plan kind.  bnpp.plan_groups (bnpp_plan_groups: the launch groups of the plan
the call builds, through the same code) tells which chain keys the plan
launches and with how many run descriptors: a split key is backed by a one-run
kernel (one descriptor) and a multi-run kernel (several).  regenerate()
enumerates

  models  ising / peaked / potts (k = 4) grids, two disconnected grids, a grid
          cut in two by a column of evidence, grids with extra "hop" factors
          (a factor to the variable `hop` rows below: ChainDep any), grids with
          anti-diagonal factors (r, c)-(r - 1, c + 1) instead of the vertical
          ones ("diag": ChainDep prev going forward) or beside them ("diagv")
  orders  column sweeps top-down ("down") and bottom-up ("up")
  knobs   BNPP_CHAIN_RUN_MAX 2..8, BNPP_SPLIT_MIN_F, BNPP_NO_DENSE,
          BNPP_NO_CHAIN_FWDV, BNPP_NO_SPLIT, BNPP_KEEP_LOG2, BNPP_TREE_SLOTS,
          BNPP_NO_BEL_FUSE
  plans   "pr" the partition (kind 0), "ve" bnpp_variable_elimination of every
          column but the last under BNPP_VE_CHAIN=1 (kind 2: the sweep's last
          message entry by entry), "tree" the bucket tree (kind 3), "part" one
          of two tree parts

within rows <= 18 (K = 2) / 9 (K = 4) and <= 6 columns, and freezes per
(dtype, key, one-run or multi-run) two cases in chain_catalogue_data.json:

  "small"  the fewest variables (then the fewest switches)
  "big"    the most virtual blocks in the key's launch: the case the capped
           reruns use, so that a workgroup walks several tiles

Forward keys are taken from "ve" plans where one exists (else "pr"), summing
keys from "pr", backward and belief keys from "tree" / "part".
test_chain_census.py asserts that every case still plans to its key and that
the keys cover the instantiation lists; test_gpu_chain_variants.py runs them.
"""
import json
import math
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "chain_catalogue_data.json")
MAX_ROWS = {2: 18, 4: 9}
MAX_COLS = 6
KNOBS = ("BNPP_CHAIN_RUN_MAX", "BNPP_SPLIT_MIN_F", "BNPP_NO_DENSE", "BNPP_NO_CHAIN_FWDV", "BNPP_NO_SPLIT",
         "BNPP_KEEP_LOG2", "BNPP_TREE_SLOTS", "BNPP_NO_BEL_FUSE", "BNPP_VE_CHAIN", "BNPP_NO_CHAIN")
FWD_FORMS, SUM_FORM, BWD_FORMS = (1, 4, 5, 7), 3, (2, 6, 8)
BEL = 128


def load():
    with open(DATA) as f:
        return json.load(f)["entries"]


# ---------------------------------------------------------------- chain keys
def key_fields(key):
    """(form, k, f, dep, belief) of a chain dispatch key (bnpp_device.h chain_key)."""
    r = key - 8192
    dep, r = divmod(r, 2048)
    form, r = divmod(r, 256)
    if form == 0:                                         # form 8 * 256 carries into the dep field
        form, dep = 8, dep - 1
    bel, r = divmod(r, BEL)
    return form, r // 16, r % 16, dep, bool(bel)


def chain_key(form, k, f, dep, bel=False):
    return 8192 + dep * 2048 + form * 256 + k * 16 + f + (BEL if bel else 0)


def is_chain(key):
    return 8192 <= key < 16384


# -------------------------------------------------------------------- models
def build_model(spec):
    """(model dict, evidence, order) of a case's model spec
    {"kind", "rows", "cols", "k", "hop", "order"}; seeds follow from the shape."""
    from bnpp import synth
    R, C, kind = spec["rows"], spec["cols"], spec["kind"]
    seed = 1000 + 16 * R + C
    ev = {}
    if kind == "peaked":
        d = synth.peaked_grid(R, C, log2_eps=10, seed=seed)
    elif spec["k"] != 2:
        d = synth.potts_grid(R, C, k=spec["k"], seed=seed)
    else:
        d = synth.ising_grid(R, C, seed=seed)
    if kind in ("diag", "diagv"):
        # a factor from (r, c) to (r - 1, c + 1): on a top-down sweep G_j then varies with the variable
        # the previous bucket brought in (ChainDep prev); "diag" has them instead of the vertical pairs
        # (prev alone), "diagv" beside them (next and prev: any)
        rng = random.Random(seed + 2)
        k = spec["k"]
        if kind == "diag":
            keep = R * C + R * (C - 1)
            d["scopes"], d["values"] = d["scopes"][:keep], d["values"][:keep]
        for c in range(C - 1):
            for r in range(1, R):
                j = rng.uniform(-0.5, 0.5)
                e, ne = round(math.exp(j), 6), round(math.exp(-j), 6)
                d["scopes"].append([r * C + c, (r - 1) * C + c + 1])
                d["values"].append([e if x == y else ne for x in range(k) for y in range(k)])
    if kind == "hop":
        rng = random.Random(seed + 1)
        hop = spec["hop"]
        for c in range(C):
            for r in range(R - hop):
                j = rng.uniform(-0.5, 0.5)
                e, ne = round(math.exp(j), 6), round(math.exp(-j), 6)
                d["scopes"].append([r * C + c, (r + hop) * C + c])
                d["values"].append([e, ne, ne, e])
    if kind == "cut":
        ev = {r * C + C // 2: r % 2 for r in range(R)}
    rows = range(R) if spec["order"] == "down" else range(R - 1, -1, -1)
    col = [r * C + c for c in range(C) for r in rows]
    order = col
    if kind == "two":
        b = synth.ising_grid(R, C, seed=seed + 7)
        n = R * C
        d = {"type": "MARKOV", "cards": d["cards"] + b["cards"],
             "scopes": d["scopes"] + [[v + n for v in s] for s in b["scopes"]], "values": d["values"] + b["values"]}
        order = col + [v + n for v in col]
    return d, ev, order


def conditioned(d, ev):
    """The model with `ev` applied to its factors (what variable_elimination,
    which takes the factors as given, is handed for a model with evidence):
    every factor restricted to the evidence values, its scope without the
    evidence variables."""
    if not ev:
        return d
    scopes, values = [], []
    for s, vals in zip(d["scopes"], d["values"]):
        keep = [v for v in s if v not in ev]
        strides, n = [], 1
        for v in reversed(s):
            strides.insert(0, n)
            n *= d["cards"][v]
        base = sum(ev[v] * st for v, st in zip(s, strides) if v in ev)
        ks = [(d["cards"][v], st) for v, st in zip(s, strides) if v not in ev]
        out = [base]
        for card, st in ks:
            out = [o + x * st for o in out for x in range(card)]
        scopes.append(keep)
        values.append([vals[o] for o in out])
    return {"type": d["type"], "cards": d["cards"], "scopes": scopes, "values": values}


def ve_vars(spec, ev, order):
    """The variables the "ve" plan eliminates: the order without the last
    column swept (of the second grid for "two") and without evidence."""
    return [v for v in order[:len(order) - spec["rows"]] if v not in ev]


class knobs:
    """Planning switches of a case set in os.environ for a with-block."""

    def __init__(self, kn):
        self.kn = {k: str(v) for k, v in kn.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.kn)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def plan(bnpp, e, model=None, built=None, extra=None):
    """bnpp.plan_groups of a case: the launch groups of the plan its call builds."""
    d, ev, order = built or build_model(e["model"])
    dtype = bnpp.F32 if e["dtype"] == "f32" else bnpp.F64
    kn = dict(e["knobs"])
    kn.update(extra or {})
    p = e["plan"]
    with knobs(kn):
        if p == "ve":
            m = model or bnpp.Model.from_dict(conditioned(d, ev))
            return bnpp.plan_groups(m, 2, None, dtype=dtype, order=ve_vars(e["model"], ev, order))
        m = model or bnpp.Model.from_dict(d)
        if p == "pr":
            return bnpp.plan_groups(m, 0, ev, dtype=dtype, order=order)
        if p == "tree":
            return bnpp.plan_groups(m, 3, ev, dtype=dtype, order=order)
        return bnpp.plan_groups(m, 3, ev, dtype=dtype, order=order, part=int(p[4:]), n_parts=2)


def find_group(groups, key, runs):
    """The launch group of `key` with one descriptor ("one") or several
    ("multi") that has the most virtual blocks, or None."""
    best = None
    for g in groups:
        if g["key"] == key and (g["n_desc"] > 1) == (runs == "multi"):
            if best is None or g["vblocks"] > best["vblocks"]:
                best = g
    return best


# -------------------------------------------------------------------- search
RUN_MAX = (None, 2, 3, 4, 5, 6, 7, 8)
EXTRA = ({}, {"BNPP_NO_DENSE": 1}, {"BNPP_NO_CHAIN_FWDV": 1}, {"BNPP_NO_SPLIT": 1}, {"BNPP_SPLIT_MIN_F": 6},
         {"BNPP_SPLIT_MIN_F": 7}, {"BNPP_SPLIT_MIN_F": 8}, {"BNPP_NO_DENSE": 1, "BNPP_NO_CHAIN_FWDV": 1})
TREE = ({}, {"BNPP_TREE_SLOTS": 3}, {"BNPP_TREE_SLOTS": 3, "BNPP_KEEP_LOG2": 8}, {"BNPP_TREE_SLOTS": 3, "BNPP_KEEP_LOG2": 9},
        {"BNPP_TREE_SLOTS": 3, "BNPP_KEEP_LOG2": 8, "BNPP_NO_BEL_FUSE": 1})


def model_specs(rows2=range(4, 19), rows4=range(3, 10), cols=(3, 4, 6)):
    for order in ("down", "up"):
        for C in cols:
            for R in rows2:
                for kind in ("ising", "peaked", "two", "cut"):
                    if kind == "cut" and C < 3:
                        continue
                    yield {"kind": kind, "rows": R, "cols": C, "k": 2, "hop": 0, "order": order}
                for kind in ("diag", "diagv"):
                    yield {"kind": kind, "rows": R, "cols": C, "k": 2, "hop": 0, "order": order}
                for hop in (2, 3):
                    if hop < R:
                        yield {"kind": "hop", "rows": R, "cols": C, "k": 2, "hop": hop, "order": order}
            for R in rows4:
                for kind in ("potts", "diag", "diagv"):
                    yield {"kind": kind, "rows": R, "cols": C, "k": 4, "hop": 0, "order": order}


def knob_sets(p):
    for rm in RUN_MAX:
        base = {} if rm is None else {"BNPP_CHAIN_RUN_MAX": rm}
        for ex in (EXTRA[:1] if p == "part" else EXTRA if p != "tree" else [x for x in EXTRA if "BNPP_NO_CHAIN_FWDV" not in x]):
            for tr in (TREE if p in ("tree", "part") else TREE[:1]):
                if p == "part" and not tr:
                    continue
                kn = dict(base)
                kn.update(ex)
                kn.update(tr)
                if p == "ve":
                    kn["BNPP_VE_CHAIN"] = 1
                yield kn


KIND_RANK = ("ising", "two", "cut", "hop", "diag", "diagv", "potts", "peaked")   # ties: the plainer model


def allowed(form, p):
    if form in FWD_FORMS:
        return p in ("ve", "pr")
    return p == "pr" if form == SUM_FORM else p in ("tree", "part0", "part1")


def scan_model(spec):
    """Every plan of one model spec: {(dtype, key, runs, plan class): {"small": (cost, entry), "big": ...}}
    and the set of chain keys seen per dtype."""
    import bnpp
    built = build_model(spec)
    d, ev, order = built
    full = bnpp.Model.from_dict(d)
    cond = bnpp.Model.from_dict(conditioned(d, ev)) if ev else full
    best, seen = {}, {"f32": set(), "f64": set()}
    nv = len(d["cards"])
    big_table = spec["k"] ** spec["rows"]
    for p in ("ve", "pr", "tree", "part0", "part1"):
        if p == "ve" and spec["cols"] < 2:
            continue
        for kn in knob_sets("part" if p.startswith("part") else p):
            for dt in ("f32", "f64"):
                e = {"dtype": dt, "model": spec, "knobs": kn, "plan": p}
                try:
                    groups = plan(bnpp, e, model=cond if p == "ve" else full, built=built)
                except bnpp.BnppError:
                    continue
                for g in groups:
                    if not is_chain(g["key"]):
                        continue
                    seen[dt].add(g["key"])
                    form = key_fields(g["key"])[0]
                    if not allowed(form, p):
                        continue
                    runs = "multi" if g["n_desc"] > 1 else "one"
                    cls = "ve" if p == "ve" else "x"
                    slot = best.setdefault((dt, g["key"], runs, cls), {})
                    ent = dict(e, key=g["key"], runs=runs, n_desc=g["n_desc"], vblocks=g["vblocks"], level=g["level"])
                    cost = (nv, big_table, KIND_RANK.index(spec["kind"]), len(kn), json.dumps(kn, sort_keys=True), p,
                            spec["order"])
                    if "small" not in slot or cost < slot["small"][0]:
                        slot["small"] = (cost, ent)
                    bcost = (-g["vblocks"],) + cost
                    if "big" not in slot or bcost < slot["big"][0]:
                        slot["big"] = (bcost, ent)
    return best, seen


def search(specs=None, procs=None):
    """Merged scan of all model specs: ({(dtype, key, runs): {"small": entry, "big": entry}}, seen keys)."""
    import multiprocessing as mp
    specs = list(model_specs() if specs is None else specs)
    best, seen = {}, {"f32": set(), "f64": set()}
    with mp.Pool(procs or min(16, os.cpu_count() or 4)) as pool:
        for b, s in pool.imap_unordered(scan_model, specs, chunksize=4):
            for dt in s:
                seen[dt] |= s[dt]
            for k, slot in b.items():
                mine = best.setdefault(k, {})
                for size, (cost, ent) in slot.items():
                    if size not in mine or cost < mine[size][0]:
                        mine[size] = (cost, ent)
    out = {}
    for (dt, key, runs, cls), slot in best.items():
        # forward keys: the "ve" plan's case where one exists
        if cls == "x" and (dt, key, runs, "ve") in best:
            continue
        out[(dt, key, runs)] = {size: ent for size, (cost, ent) in slot.items()}
    return out, seen


def regenerate(path=DATA):
    """Rebuild the frozen table (needs the built library; minutes on 8 cores)."""
    import bnpp
    best, seen = search()
    for dt, dtype in (("f32", bnpp.F32), ("f64", bnpp.F64)):
        inst = set(bnpp.kernel_keys(dtype, 3, level=True))
        assert seen[dt] <= inst, (dt, sorted(seen[dt] - inst))
    entries = []
    for k in sorted(best):
        for size in ("small", "big"):
            ent = dict(best[k][size], size=size)
            if size == "big" and ent["vblocks"] <= best[k]["small"]["vblocks"]:
                continue                                  # the smallest case already has the most blocks
            entries.append(ent)
    with open(path, "w") as f:
        f.write('{"entries": [\n')
        f.write(",\n".join(json.dumps(e, sort_keys=True) for e in entries))
        f.write("\n]}\n")
    return entries


if __name__ == "__main__":
    import sys
    import time
    sys.path.insert(0, os.path.join(HERE, "..", "bn-pp_amd", "python"))
    t0 = time.time()
    print(len(regenerate()), "entries in %.0f s" % (time.time() - t0))
