"""Catalogue of the smallest buckets that reach every instantiated single-op
kernel (a helper, like sliced_world.py; CPU only).

A bucket is cards, input scopes, the summed variable, the output layout and
whether it is a divide.  bnpp.plan_single (bnpp_plan_single: the planner's own
report of the family and dispatch key a call launches) maps it to a kernel;
regenerate() searches seeded random buckets around shape templates -- the ones
the parity tests use and what build_desc's conditions ask for -- and keeps, per
dtype and key, the smallest output found in two size classes:

  "a"  generic family: n_tiles under one wave (< 64).  Stream and slab buckets
       start at 1024 tiles (plan.cpp build_desc: d.n_tiles >= 1024), so their
       "a" entry is simply the smallest bucket found.
  "b"  at least two workgroups with a ragged last one: n_tiles > 256 and
       n_tiles % 256 != 0 (slab: the tiles one block takes, 256 / lanes).

When the smallest bucket of a key is already ragged only "a" is kept.  Generic
keys are reached with 32-bit offsets and, under BNPP_NO_O32=1, without.  The
result is frozen in variant_catalogue_data.json (test data, not a reference
fixture); test_variant_census.py asserts that every entry still plans to its
key and that the keys cover the instantiation lists, test_gpu_variants.py runs
them.
"""
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "variant_catalogue_data.json")
FAMILIES = ("generic", "stream", "slab")
MAX_OUT = 1 << 16            # output entries of the larger size: a few times 10^4
MAX_IN = 1 << 18             # entries of the largest input
SEED = 20261019


def load():
    with open(DATA) as f:
        return json.load(f)["entries"]


def size_of(cards, scope):
    n = 1
    for v in scope:
        n *= cards[v]
    return n


def out_scope(scopes, elim):
    u = []
    for s in scopes:
        u += [v for v in s if v not in u]
    return [v for v in u if v != elim]


def plan(bnpp, dtype, b, no_o32=False):
    """bnpp.plan_single of a catalogue bucket (BNPP_NO_O32 set around the call)."""
    old = os.environ.get("BNPP_NO_O32")
    os.environ["BNPP_NO_O32"] = "1" if no_o32 else "0"
    try:
        return bnpp.plan_single(dtype, b["cards"], b["scopes"], b["elim"], b["out"], divide=b.get("divide", False))
    finally:
        if old is None:
            del os.environ["BNPP_NO_O32"]
        else:
            os.environ["BNPP_NO_O32"] = old


# ------------------------------------------------------------ shape templates
def _t_random(rng):
    """Small buckets of 1-8 inputs: the generic tiles by alignment and merging."""
    nv = rng.randint(1, 6)
    cards = [rng.choice([1, 2, 2, 2, 3, 4, 4, 5, 6, 7, 8]) for _ in range(nv)]
    n_in = rng.randint(1, 8)
    divide = rng.random() < 0.1
    if divide:
        n_in = 2
    scopes = [rng.sample(range(nv), rng.randint(0, min(nv, 4))) for _ in range(n_in)]
    if rng.random() < 0.6:                       # natural layouts: dims merge, tiles widen
        for s in scopes:
            s.sort()
    union = out_scope(scopes, -1)
    elim = -1 if divide or not union or rng.random() < 0.3 else rng.choice(union)
    out = out_scope(scopes, elim)
    r = rng.random()
    if r < 0.5:
        out.sort()
    elif r < 0.8:
        rng.shuffle(out)
    return {"cards": cards, "scopes": scopes, "elim": elim, "out": out, "divide": divide}


def _t_rows(rng):
    """Generic 2-D tiles and whole-dim rows: a fastest output dim of a chosen
    card that cannot merge with the next one (an input holds one but not the other)."""
    c0 = rng.choice([2, 2, 4, 3, 5, 6, 7])
    c1 = rng.choice([2, 4, 8, 3, 6, 12, 16])
    rest = [rng.choice([1, 2, 3, 4, 5]) for _ in range(rng.randint(0, 3))]
    k = rng.choice([1, 2, 3, 4])
    cards = [k, c0, c1] + rest                   # x = 0, a = 1 (fastest), b = 2
    rv = list(range(3, 3 + len(rest)))
    n_in = rng.randint(1, 8)
    pool = [[1], [2, 1], [0, 1], [0, 2], [2], [0], rv + [2, 1], rv + [2], [0] + rv + [2, 1], rv + [1], rv[:1] + [0, 1],
            [2, 0, 1], rv + [2, 0, 1], rv + [2, 1, 0]]
    scopes = [list(rng.choice(pool)) for _ in range(n_in)]
    elim = 0 if k > 1 and rng.random() < 0.7 else -1
    out = [v for v in rv + [2, 1] if any(v in s for s in scopes)]
    if elim < 0 and any(0 in s for s in scopes):
        out = [0] + out
    return {"cards": cards, "scopes": scopes, "elim": elim, "out": out, "divide": False}


def _t_stream(rng):
    """One input past the LDS limit (4096 entries), the others small: the stream
    big classes by where the summed variable and the output's fastest dims sit in
    the big input; variables only the small inputs hold give Col / One / broadcast rows."""
    k = rng.choice([1, 2, 2, 3, 4, 4])
    fast = [rng.choice([2, 2, 4, 4, 8, 3, 6, 9]) for _ in range(rng.randint(1, 2))]
    mid = []
    n = k
    for c in fast:
        n *= c
    while n <= 4096 or (rng.random() < 0.3 and n < MAX_OUT // 2):
        c = rng.choice([2, 2, 2, 3, 4, 5])
        mid.append(c)
        n *= c
    extra = [rng.choice([2, 4, 2, 3, 8, 9]) for _ in range(rng.randint(0, 2))]   # 9: no tile, no whole-dim row
    cards = [k] + mid + fast + extra             # x = 0, then mid (slow), fast, extras
    x = 0
    mv = list(range(1, 1 + len(mid)))
    fv = list(range(1 + len(mid), 1 + len(mid) + len(fast)))
    ev = list(range(1 + len(mid) + len(fast), len(cards)))
    elim = x if k > 1 else -1
    where = rng.choice(["first", "last", "mid", "absent"]) if k > 1 else "absent"
    big = mv + fv
    if where == "first":
        big = [x] + big
    elif where == "last":
        big = big + [x]
    elif where == "mid":
        big = mv + [x] + fv
    near = fv + ev + mv[-1:] + mv[:1] + ([x] if k > 1 else [])
    n_small = rng.randint(0 if where != "absent" or k == 1 else 1, 7)
    smalls = []
    for _ in range(n_small):
        s = rng.sample(near, rng.randint(0, min(3, len(near))))
        if size_of(cards, s) <= 4096:
            smalls.append(s)
    if k > 1 and where == "absent":
        smalls.append([x] + rng.sample(fv + ev, rng.randint(0, 1)))
    at = rng.randint(0, len(smalls))
    scopes = smalls[:at] + [big] + smalls[at:]
    if len(scopes) > 8:
        return None
    used = [v for v in ev if any(v in s for s in scopes)]
    out = mv + fv
    for v in used:                               # a small-only variable: fastest, slowest or second
        pos = rng.choice([0, len(out), len(out) - 1, len(out) - len(fv)])
        out.insert(max(0, pos), v)
    if rng.random() < 0.15 and len(out) > 2:
        i, j = rng.sample(range(len(out)), 2)
        out[i], out[j] = out[j], out[i]
    if elim < 0 and k > 1:
        return None
    return {"cards": cards, "scopes": scopes, "elim": elim, "out": out, "divide": False}


def _t_slab(rng):
    """Slab form: the big input holds the summed variable as its slowest dim (k
    slabs contiguous along the output's slow index S), small inputs depend on
    (x, y) only, the output is (S..., y) with y absent, one dim of card 2 / 4,
    or two binary dims (rows over two dims)."""
    k = rng.choice([1, 2, 3, 4])
    ys = rng.choice([[], [2], [4], [2, 2]])
    scards = []
    n = 1
    odd = rng.random() < 0.3                     # an odd slab dim: one entry per lane
    while n * max(1, size_of(ys, range(len(ys)))) < 4200 or (rng.random() < 0.3 and n < MAX_OUT // 8):
        c = rng.choice([3, 5, 3, 7] if odd else [2, 2, 2, 3, 4, 5])
        scards.append(c)
        n *= c
    cards = [k] + ys + scards
    x = 0
    yv = list(range(1, 1 + len(ys)))
    S = list(range(1 + len(ys), len(cards)))
    big = ([x] if k > 1 else []) + S
    pool = [[x] + yv, yv, [x], yv[::-1] + [x], yv[:1], [x] + yv[-1:], []] if k > 1 else [yv, yv[:1], yv[::-1], [], yv[-1:]]
    n_small = rng.randint(0 if not yv else 1, 7)
    smalls = [list(rng.choice(pool)) for _ in range(n_small)]
    if yv and not all(any(v in s for s in smalls) for v in yv):
        smalls.append(list(yv))
    at = rng.randint(0, len(smalls))
    scopes = smalls[:at] + [big] + smalls[at:]
    if len(scopes) > 8:
        return None
    out = S + yv[::-1] if rng.random() < 0.8 else S + yv
    return {"cards": cards, "scopes": scopes, "elim": x if k > 1 else -1, "out": out, "divide": False}


def _t_divide(rng):
    """bnpp_divide at sizes past one workgroup (never the stream form: plan.cpp !b.divide)."""
    nv = rng.randint(2, 7)
    cards = [rng.choice([2, 2, 3, 4, 5, 6, 7, 8]) for _ in range(nv)]
    a = sorted(rng.sample(range(nv), rng.randint(1, nv)))
    b = sorted(rng.sample(range(nv), rng.randint(0, min(3, nv))))
    out = out_scope([a, b], -1)
    if rng.random() < 0.6:
        out.sort()
    return {"cards": cards, "scopes": [a, b], "elim": -1, "out": out, "divide": True}


TEMPLATES = ((_t_random, 40000), (_t_rows, 40000), (_t_divide, 4000), (_t_stream, 80000), (_t_slab, 30000))


def size_class(info):
    """"b" when the launch spans two workgroups with a ragged last one, "a" when
    it is under one wave (generic) / any size (stream, slab), else None."""
    per_block = 256 // max(1, info["lanes"]) if info["family"] == 2 else 256
    nt = info["n_tiles"]
    ragged = nt > per_block and nt % per_block != 0
    small = nt < 64 if info["family"] == 0 else True
    return small, ragged


def search(bnpp, templates=TEMPLATES, seed=SEED):
    """{(dtype, family, key, no_o32, cls): (out_size, bucket)}: smallest per key and size class."""
    rng = random.Random(seed)
    best = {}
    for tmpl, count in templates:
        for _ in range(count):
            b = tmpl(rng)
            if b is None:
                continue
            osz = size_of(b["cards"], b["out"])
            if osz > MAX_OUT or max(size_of(b["cards"], s) for s in b["scopes"]) > MAX_IN:
                continue
            for dtype in (bnpp.F64, bnpp.F32):
                for no_o32 in (False, True):
                    try:
                        info = plan(bnpp, dtype, b, no_o32)
                    except bnpp.BnppError:
                        break
                    if no_o32 and info["family"] != 0:
                        break                    # the switch only moves generic launches
                    small, ragged = size_class(info)
                    for cls, ok in (("a", small), ("b", ragged)):
                        if not ok:
                            continue
                        k = (dtype, info["family"], info["key"], no_o32, cls)
                        cost = (osz, sum(size_of(b["cards"], s) for s in b["scopes"]))
                        if k not in best or cost < best[k][0]:
                            best[k] = (cost, b, info["n_tiles"])
    return best


def regenerate(path=DATA):
    """Rebuild the frozen table (needs the built library; about a minute)."""
    import bnpp
    best = search(bnpp)
    entries = []
    for (dtype, fam, key, no_o32, cls) in sorted(best):
        cost, b, nt = best[(dtype, fam, key, no_o32, cls)]
        if cls == "b" and (dtype, fam, key, no_o32, "a") in best and best[(dtype, fam, key, no_o32, "a")][1] == b:
            continue                             # the smallest bucket is already the ragged one
        e = {"dtype": "f32" if dtype == bnpp.F32 else "f64", "family": FAMILIES[fam], "key": key, "no_o32": no_o32,
             "size": cls, "n_tiles": nt}
        e.update(b)
        entries.append(e)
    with open(path, "w") as f:
        f.write('{"entries": [\n')
        f.write(",\n".join(json.dumps(e, sort_keys=True) for e in entries))
        f.write("\n]}\n")
    return entries


# ------------------------------------------------- inputs and restatements
def make_inputs(e, seed, dtype=None):
    """One float64 array per input, already rounded to `dtype` (the entry's own by default):
    uniform in [0.5, 2), about 10 % exact zeros, one input times 2^-20 (exact),
    so a dropped or doubled factor cannot hide.  A divide's divisor keeps no
    zeros (x / 0 and 0 / 0 are inf and NaN in the kernel and the oracle alike,
    and NaN is what the tests' unwritten-output check looks for)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    dt = np.float32 if (dtype or e["dtype"]) == "f32" else np.float64
    scaled = int(rng.integers(len(e["scopes"])))
    ins = []
    for i, s in enumerate(e["scopes"]):
        n = size_of(e["cards"], s)
        v = rng.uniform(0.5, 2.0, n).astype(dt)
        zero = rng.random(n) < 0.1
        if not (e.get("divide") and i == 1):
            v[zero] = 0
        if i == scaled:
            v = v * dt(2.0 ** -20)
        ins.append(v.astype(np.float64))
    return ins


def _bview(np, vals, scope, cards, layout):
    """vals (row-major over scope, last fastest) as an array broadcastable
    over `layout` (a list of variables; absent ones become axes of length 1)."""
    keep = [v for v in scope if v in layout]      # a variable the layout lacks has card 1
    a = vals.reshape([cards[v] for v in keep])
    a = a.transpose([keep.index(v) for v in layout if v in keep])
    return a.reshape([cards[v] if v in keep else 1 for v in layout])


def restate(e, ins, dt, scopes=None, elim=None, out=None, divide=None):
    """The kernels' arithmetic one operation at a time in numpy type `dt`:
    acc = 0; per value of the summed variable p = 1, p *= in_i in input order
    (p /= in_1 for a divide), acc += p (kernels.cuh compute_tile,
    factor.cpp:131-143, 199-205).  Flat, in the layout `out`."""
    import numpy as np
    cards = e["cards"]
    scopes = e["scopes"] if scopes is None else scopes
    elim = e["elim"] if elim is None else elim
    out = e["out"] if out is None else out
    divide = e.get("divide", False) if divide is None else divide
    has = elim >= 0 and any(elim in s for s in scopes)
    k = cards[elim] if has else 1
    lay = ([elim] if has else []) + list(out)
    views = [_bview(np, np.asarray(v).astype(dt), s, cards, lay) for v, s in zip(ins, scopes)]
    shape = [cards[v] for v in out]
    acc = np.zeros(shape, dtype=dt)
    for x in range(k):
        p = np.ones(shape, dtype=dt)
        for i, v in enumerate(views):
            t = v[x if v.shape[0] > 1 else 0] if has else v
            p = p / t if divide and i == 1 else p * t
        acc = acc + p
    return acc.reshape(-1)


def restate_ve(e, ins, dt, result_scope):
    """BN::variable_elimination of the entry's summed variable over its inputs
    as a model (model.cpp:394-439): the factors without the variable multiplied
    into the result in order, then the bucket's message; flat over result_scope."""
    import numpy as np
    x = e["elim"]
    inb = [i for i, s in enumerate(e["scopes"]) if x in s]
    rest = [i for i, s in enumerate(e["scopes"]) if x not in s]
    mscope = out_scope([e["scopes"][i] for i in inb], x)
    msg = restate(e, [ins[i] for i in inb], dt, scopes=[e["scopes"][i] for i in inb], out=mscope)
    cards = e["cards"]
    res = np.ones([cards[v] for v in result_scope], dtype=dt)
    for i in rest:
        res = res * _bview(np, np.asarray(ins[i]).astype(dt), e["scopes"][i], cards, result_scope)
    res = res * _bview(np, msg, mscope, cards, result_scope)
    return res.reshape(-1)


def oracle(refcpu, e, ins):
    """The fp64 oracle's table of the entry in the layout e["out"], and its partition sum."""
    import numpy as np
    cards = {v: c for v, c in enumerate(e["cards"])}
    fs = [refcpu.Factor.new(s, cards, v.tolist()) for s, v in zip(e["scopes"], ins)]
    if e.get("divide"):
        ref = fs[0].divide(fs[1])
    elif e["elim"] >= 0:
        ref = refcpu.bucket(fs, e["elim"], e["cards"][e["elim"]])
    else:
        ref = fs[0]
        for f in fs[1:]:
            ref = ref.product(f)
    sc = ref.scope
    assert sorted(sc) == sorted(e["out"]), (sc, e["out"])
    t = np.array(ref.values, dtype=np.float64).reshape([e["cards"][v] for v in sc])
    lay = [v for v in e["out"] if v in sc]
    return t.transpose([sc.index(v) for v in lay]).reshape(-1), ref.partition


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(HERE, "..", "bn-pp_amd", "python"))
    print(len(regenerate()), "entries")
