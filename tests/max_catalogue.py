"""Catalogue of max buckets (bnpp_bucket_max): for every key of the max kernel
family (bnpp_kernel_keys family 4: input classes 1/2/4/8 x tiles 1x1 2x1 4x1 x
32/64-bit offsets, per dtype) one smallest bucket that reaches it ("a": under
one wave) and a larger one ("b": several workgroups with a ragged last one,
for the capped reruns of the tile loop), plus the shapes the tests name:
k in {2, 3, 7}, 1/2/3/5 inputs, an output of three unmergeable dims, a view
at an offset, k == 1 and a card-256 variable.

The entries live in max_catalogue_data.json (written by `python
tests/max_catalogue.py`, which asks bnpp_plan_max_single for each key -- host
only); test_mpe_host.py checks the file against the library's key lists.
Variable 0 is the maximised one; the output scope is slowest first.
"""
import json
import os

import numpy as np

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "max_catalogue_data.json")
MAX_KEY_BASE = 65536
O32 = 1024
FAMILY_MAX = 4

# input scope templates over variable 0 (maximised) and the output variables
# 1, 2, 3 (3 fastest): in this order a bucket of n inputs takes the first n.
# From two inputs on, no two output dims merge (input 1 holds them permuted);
# the one-input buckets read [1, 0, 2, 3], where dims 2 and 3 merge.
TEMPLATES = ([0, 1, 2, 3], [3, 0, 1], [2, 0, 3], [1, 3], [0], [2, 1, 0], [3], [0, 2])


def key_of(n_in, v1, o32):
    cls = 1 if n_in <= 1 else 2 if n_in <= 2 else 4 if n_in <= 4 else 8
    return MAX_KEY_BASE + cls * 64 + v1 * 8 + 1 + (O32 if o32 else 0)


def specs():
    """(name, cards, scopes, elim, out, no_o32) of every catalogue bucket."""
    out = []
    for n_in in (1, 2, 3, 5):
        for c3, v1 in ((3, 1), (2, 2), (4, 4)):
            k = {1: 2, 2: 3, 4: 7}[v1]
            for no_o32 in (0, 1):
                # "a": 5 * 3 * c3 entries; "b": 4-5 virtual blocks, the last ragged
                for size, c1, c2 in (("a", 5, 3), ("b", 7 * 17 * v1, 11)):
                    cards = [k, c1, c2, c3]
                    out.append(("n%d_v%d_%s%s" % (n_in, v1, size, "_o64" if no_o32 else ""), cards,
                                [list(t) for t in TEMPLATES[:n_in]] if n_in > 1 else [[1, 0, 2, 3]], 0, [1, 2, 3],
                                no_o32))
    # the maximised variable absent from every input: a copy, arg 0 (k == 1)
    out.append(("k1_copy", [3, 5, 4], [[1, 2], [2]], 0, [1, 2], 0))
    # a card-256 variable: the largest arg value a byte holds
    out.append(("card256", [256, 3, 2], [[1, 0, 2], [0]], 0, [1, 2], 0))
    # output laid out against the inputs (a transposed output scope)
    out.append(("out_perm", [3, 4, 5, 2], [[0, 1, 2, 3], [3, 1]], 0, [3, 1, 2], 0))
    return out


def entries_for(bnpp):
    """Plan every spec for both dtypes (host only)."""
    ents = []
    for dt_name, dt in (("f64", bnpp.F64), ("f32", bnpp.F32)):
        for name, cards, scopes, elim, out, no_o32 in specs():
            os.environ["BNPP_NO_O32"] = "1" if no_o32 else "0"
            info = bnpp.plan_max_single(dt, cards, scopes, elim, out)
            ents.append({"name": name, "dtype": dt_name, "cards": cards, "scopes": scopes, "elim": elim, "out": out,
                         "no_o32": no_o32, "key": info["key"], "v1": info["v1"], "k": info["k"],
                         "n_tiles": info["n_tiles"]})
    os.environ.pop("BNPP_NO_O32", None)
    return ents


def load():
    with open(DATA) as f:
        return json.load(f)["entries"]


def size_of(cards, scope):
    n = 1
    for v in scope:
        n *= cards[v]
    return n


def make_inputs(e, seed, ties=False):
    """One float64 array per input (row-major over its scope), exact in fp32.
    Default: uniform in [0.5, 2) rounded to fp32, about 10 % exact zeros, one
    input times 2^-20.  ties: entries from {0, 0.5, 1}, and input 0 zero for
    every value of the maximised variable at about 10 % of the output entries,
    so that many maxima tie (all-zero rows included)."""
    rng = np.random.default_rng(1000 + seed)
    ins = []
    for i, s in enumerate(e["scopes"]):
        n = size_of(e["cards"], s)
        if ties:
            v = rng.choice(np.array([0.0, 0.5, 1.0]), size=n, p=[0.3, 0.35, 0.35])
            if i == 0 and e["elim"] in s:                # input 0 holds every variable: zero ~10 % of the rows
                a = np.moveaxis(v.reshape([e["cards"][x] for x in s]), s.index(e["elim"]), 0)
                a[:, rng.random(a.shape[1:]) < 0.1] = 0.0
        else:
            v = rng.uniform(0.5, 2.0, size=n).astype(np.float32).astype(np.float64)
            v[rng.random(n) < 0.1] = 0.0
            if i == len(e["scopes"]) - 1:
                v = v * 2.0 ** -20
        ins.append(v)
    return ins


def restate(e, ins, dtype):
    """The max kernels' loop in numpy, one rounded operation at a time:
    per value v of the maximised variable p = ((1 * in_0) * in_1) ...; best
    starts at v = 0 and a later v replaces it only when strictly greater.
    -> (values, args) flat over the output scope."""
    cards, out = e["cards"], e["out"]
    shape = [cards[v] for v in out]
    k = cards[e["elim"]] if any(e["elim"] in s for s in e["scopes"]) else 1
    best, arg = None, np.zeros(shape, dtype=np.uint8)
    for v in range(k):
        p = np.ones(shape, dtype=dtype)
        for s, t in zip(e["scopes"], ins):
            a = np.asarray(t, dtype=dtype).reshape([cards[x] for x in s])
            if e["elim"] in s:
                a = np.take(a, v, axis=s.index(e["elim"]))
            rest = [x for x in s if x != e["elim"]]
            pos = [out.index(x) for x in rest]
            order = sorted(range(len(rest)), key=lambda i: pos[i])
            a = np.transpose(a, order) if rest else a
            bshape = [1] * len(out)
            for i in order:
                bshape[pos[i]] = cards[rest[i]]
            p = (p * a.reshape(bshape)).astype(dtype)
        if best is None:
            best = p.copy()
        else:
            up = p > best
            best = np.where(up, p, best)
            arg = np.where(up, np.uint8(v), arg)
    return best.reshape(-1), arg.reshape(-1)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bn-pp_amd", "python"))
    os.environ.setdefault("BNPP_NO_TORCH", "1")
    import bnpp
    with open(DATA, "w") as f:
        json.dump({"entries": entries_for(bnpp)}, f, indent=0, separators=(",", ":"))
        f.write("\n")
