"""numpy reference for MPE (most probable explanation), independent of the
engine: a brute force over the joint for small models and a log-domain
max-sum bucket elimination with traceback for larger ones.

Models are the dicts of bnpp.synth.read_uai ({"cards", "scopes", "values"});
evidence is {var: value}.  Scores are natural logs of the unnormalised
probability, -inf for a zero entry.
"""
import math

import numpy as np

BRUTE_MAX_STATES = 1 << 20


def _log_tables(model, evidence):
    """The evidence-conditioned factors as (vars, log table) pairs."""
    cards = model["cards"]
    out = []
    for scope, vals in zip(model["scopes"], model["values"]):
        t = np.asarray(vals, dtype=np.float64).reshape([cards[v] for v in scope] or [1])
        if not scope:
            t = t.reshape(())
        idx = tuple(evidence[v] if v in evidence else slice(None) for v in scope)
        t = t[idx] if scope else t
        with np.errstate(divide="ignore"):
            lt = np.log(t)
        out.append(([v for v in scope if v not in evidence], lt))
    return out


def _expand(vars_, table, all_vars):
    """`table` over `vars_` as a broadcastable view over `all_vars` (in that order)."""
    pos = [all_vars.index(v) for v in vars_]
    order = sorted(range(len(vars_)), key=lambda i: pos[i])
    t = np.transpose(table, order) if vars_ else table
    shape = [1] * len(all_vars)
    for i in order:
        shape[pos[i]] = table.shape[i]
    return t.reshape(shape)


def log_score(model, x):
    """The log of the unnormalised probability of the full assignment x (fp64,
    from the model's factor entries, added in factor order)."""
    cards = model["cards"]
    s = 0.0
    for scope, vals in zip(model["scopes"], model["values"]):
        off = 0
        for v in scope:
            off = off * cards[v] + x[v]
        p = vals[off]
        if p <= 0.0:
            return -math.inf
        s += math.log(p)
    return s


def free_states(model, evidence):
    n = 1
    for v, c in enumerate(model["cards"]):
        if v not in evidence:
            n *= c
    return n


def brute_force(model, evidence=None):
    """-> (log max, assignment, log gap to the runner-up) over the joint of the
    non-evidence variables (at most BRUTE_MAX_STATES states).  The assignment
    is the first maximiser in row-major order of the variables (lowest values
    first); the gap is 0 when the maximum is not unique."""
    evidence = dict(evidence or {})
    cards = model["cards"]
    free = [v for v in range(len(cards)) if v not in evidence]
    assert free_states(model, evidence) <= BRUTE_MAX_STATES
    joint = np.zeros([cards[v] for v in free] or [1], dtype=np.float64)
    for vars_, lt in _log_tables(model, evidence):
        joint = joint + (_expand(vars_, lt, free) if free else lt)
    flat = joint.reshape(-1)
    best = int(np.argmax(flat))
    x = [0] * len(cards)
    for v, val in evidence.items():
        x[v] = val
    idx = np.unravel_index(best, joint.shape)
    for v, i in zip(free, idx):
        x[v] = int(i)
    top = float(flat[best])
    if flat.size > 1:
        second = float(np.partition(flat, flat.size - 2)[flat.size - 2])
        gap = top - second if second > -math.inf else math.inf
    else:
        gap = math.inf
    return top, x, gap


def min_fill_order(model, evidence):
    """A greedy min-fill elimination order of the non-evidence variables (ties:
    the smaller resulting table, then the lower id)."""
    cards = model["cards"]
    adj = {v: set() for v in range(len(cards)) if v not in evidence}
    for scope in model["scopes"]:
        s = [v for v in scope if v not in evidence]
        for a in s:
            adj[a].update(b for b in s if b != a)
    order = []
    while adj:
        best, best_key = None, None
        for v, nb in adj.items():
            nbl = sorted(nb)
            fill = 0
            for i, a in enumerate(nbl):
                aa = adj[a]
                for b in nbl[i + 1:]:
                    if b not in aa:
                        fill += 1
            w = 1.0
            for a in nbl:
                w *= cards[a]
            key = (fill, w * cards[v], v)
            if best_key is None or key < best_key:
                best, best_key = v, key
        nb = adj.pop(best)
        for a in nb:
            adj[a].discard(best)
            adj[a].update(b for b in nb if b != a)
        order.append(best)
    return order


def max_sum(model, evidence=None, order=None):
    """Log-domain max-sum bucket elimination with traceback ->
    (log max, assignment).  Ties resolve to the lowest value (np.argmax)."""
    evidence = dict(evidence or {})
    cards = model["cards"]
    if order is None:
        order = min_fill_order(model, evidence)
    rank = {v: i for i, v in enumerate(order)}
    buckets = [[] for _ in order]
    total = 0.0
    for vars_, lt in _log_tables(model, evidence):
        if vars_:
            buckets[min(rank[v] for v in vars_)].append((vars_, lt))
        else:
            total += float(lt)
    records = []                                     # (var, separator vars, argmax table)
    for i, x in enumerate(order):
        if not buckets[i]:
            records.append((x, [], None))
            continue
        scope = [x]
        for vars_, _ in buckets[i]:
            scope += [v for v in vars_ if v not in scope]
        acc = np.zeros([cards[v] for v in scope], dtype=np.float64)
        for vars_, lt in buckets[i]:
            acc = acc + _expand(vars_, lt, scope)
        sep = scope[1:]
        arg = np.argmax(acc, axis=0)
        msg = np.max(acc, axis=0)
        records.append((x, sep, arg))
        if sep:
            buckets[min(rank[v] for v in sep)].append((sep, msg))
        else:
            total += float(msg)
    xs = [0] * len(cards)
    for v, val in evidence.items():
        xs[v] = val
    for x, sep, arg in reversed(records):
        if arg is not None:
            xs[x] = int(arg[tuple(xs[v] for v in sep)]) if sep else int(arg)
    return total, xs


# The larger models of test_gpu_mpe.py: (model, evidence file or None).  Their
# max-sum results are recorded in golden/mpe_golden.json (`python
# tests/mpe_ref.py` rewrites it; Munin1 alone takes ~20 s in numpy), and
# test_mpe_host.py recomputes the quick ones against the record.
LARGER = (("alarm", None), ("Munin1", None), ("potts4x5k3", None), ("ising12x12", None),
          ("noisyor_50_80", "noisyor_50_80.uai.evid"), ("ising12x32", None))
SLOW = ("Munin1",)

if __name__ == "__main__":
    import json
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "..", "bn-pp_amd", "python"))
    os.environ.setdefault("BNPP_NO_TORCH", "1")
    from bnpp import synth
    rec = {}
    for name, evf in LARGER:
        m = synth.read_uai(os.path.join(here, "golden", "models", name + ".uai"))
        ev = synth.read_evidence(os.path.join(here, "golden", "models", evf)) if evf else {}
        top, x = max_sum(m, ev)
        rec[name] = {"evidence": evf, "log_max": top, "assignment": x}
    with open(os.path.join(here, "golden", "mpe_golden.json"), "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
