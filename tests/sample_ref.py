"""numpy restatement of posterior sampling (include/bnpp.h bnpp_bucket_sample,
bnpp_sample), independent of the engine.

  philox / uniform   Philox4x32-10 and the u in [0, 1) a draw uses
  draw               one draw per sample, the unit of the arithmetic
  run                the whole run: forward elimination, then the draws in
                     reverse elimination order
  joint              the brute-force posterior of a small model

Models are the dicts of bnpp.synth.read_uai ({"cards", "scopes", "values"});
evidence is {var: value}; x is uint8[n_vars][n], variable-major.

run() is unscaled where the engine stores messages scaled by exact powers of
two.  With at most 8 inputs per bucket (no materialised prefix products) and
no subnormal message entry -- both asserted -- the scaling changes no bit of
a message's significand, and every p_v of one draw shares the scale, so no
draw changes: run() is then bit for bit what bnpp.sample returns in fp64.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
MAX_IN = 8


def philox(counter, key):
    """Philox4x32-10 on python ints -> (r0, r1, r2, r3)."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(seed, g, var):
    """u of the draw of variable `var` in the samples with global indices g
    (an integer array) -> float64 array in [0, 1)."""
    g = np.asarray(g, dtype=np.uint64)
    m32 = np.uint64(MASK)
    s32 = np.uint64(32)
    c0, c1 = g & m32, g >> s32
    c2 = np.full(g.shape, var, dtype=np.uint64)
    c3 = np.zeros(g.shape, dtype=np.uint64)
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return (((c0 << s32) | c1) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def weights(ins, scopes, cards, var, x, dtype):
    """p_v of one draw for every sample -> array [k][n] of `dtype`: the chain
    product ((1 * in_0) * in_1) ..., each product rounded in `dtype`, the other
    scope variables read from x."""
    n = x.shape[1]
    k = cards[var]
    p = np.ones((k, n), dtype=dtype)
    vs = np.arange(k, dtype=np.int64)[:, None]
    for t, scope in zip(ins, scopes):
        t = np.asarray(t, dtype=dtype).reshape(-1)
        off = np.zeros((1, n), dtype=np.int64)
        stride = 1
        for v in reversed(scope):
            off = off + (vs if v == var else x[v].astype(np.int64)[None, :]) * stride
            stride *= cards[v]
        p = p * t[np.broadcast_to(off, (k, n))]
    return p


def pick(p, u):
    """The walk of one draw: p [k][n], u [n] -> (values uint8 [n], degenerate
    draws).  c_v accumulates in fp64 in order of v; the value is the lowest v
    with c_v > u * c_{k-1} (strict); none: 0, counted."""
    c = np.cumsum(p.astype(np.float64), axis=0)                  # sequential, c_0 = 0.0 + p_0
    with np.errstate(invalid="ignore"):
        hit = c > (u * c[-1])[None, :]
    none = ~hit.any(axis=0)
    return np.where(none, 0, np.argmax(hit, axis=0)).astype(np.uint8), int(none.sum())


def draw(ins, scopes, cards, var, x, seed, first, dtype, u=None):
    """One draw per sample (bnpp_bucket_sample): ins are whole tables in the
    order of their scopes -> (row of `var`, n_degenerate).  u: forced uniforms
    (tests), else Philox at the global indices first + s."""
    if u is None:
        u = uniform(seed, first + np.arange(x.shape[1], dtype=np.uint64), var)
    return pick(weights(ins, scopes, cards, var, x, dtype), np.asarray(u, dtype=np.float64))


def conditioned(model, evidence, dtype):
    """The evidence-conditioned sources as (vars, table of `dtype`) pairs."""
    cards = model["cards"]
    out = []
    for scope, vals in zip(model["scopes"], model["values"]):
        t = np.asarray(vals, dtype=np.float64).astype(dtype).reshape([cards[v] for v in scope] or [1])
        if scope:
            t = t[tuple(evidence[v] if v in evidence else slice(None) for v in scope)]
        out.append(([v for v in scope if v not in evidence], np.ascontiguousarray(t)))
    return out


def _expand(vars_, table, all_vars):
    pos = [all_vars.index(v) for v in vars_]
    order = sorted(range(len(vars_)), key=lambda i: pos[i])
    t = np.transpose(table, order) if vars_ else table
    shape = [1] * len(all_vars)
    for i in order:
        shape[pos[i]] = table.shape[i]
    return t.reshape(shape)


def _chain(ins, dtype, cards):
    """Chain product by broadcasting in input order -> (scope, table); the
    scope is the inputs' union in order of first appearance."""
    scope = []
    for vars_, _ in ins:
        scope += [v for v in vars_ if v not in scope]
    p = np.ones([cards[v] for v in scope] or [1], dtype=dtype)
    for vars_, t in ins:
        p = p * (_expand(vars_, t, scope) if scope else t.reshape([1]))
    return scope, p


def forward(model, evidence, order, dtype):
    """The forward pass -> (rows, Z factors): rows[i] = (order[i], the inputs of
    its bucket).  Each source goes to the first bucket in the order that holds
    one of its variables, in factor order; messages are appended as produced
    and go to the first later bucket; a message is the sequential sum over the
    eliminated value of the chain product.  Asserts that no bucket has more
    than 8 inputs and that no message entry is subnormal."""
    cards = model["cards"]
    rank = {v: i for i, v in enumerate(order)}
    buckets = [[] for _ in order]
    rest = []
    for vars_, t in conditioned(model, evidence, dtype):
        (buckets[min(rank[v] for v in vars_)] if vars_ else rest).append((vars_, t))
    rows = []
    tiny = np.finfo(dtype).tiny
    for i, xv in enumerate(order):
        ins = buckets[i]
        assert len(ins) <= MAX_IN, ("bucket of %d inputs" % len(ins), xv)
        rows.append((xv, ins))
        if not ins:
            continue
        scope, p = _chain(ins, dtype, cards)
        ax = scope.index(xv)
        msg = np.zeros([c for j, c in enumerate(p.shape) if j != ax] or [1], dtype=dtype)
        for v in range(cards[xv]):
            msg = msg + np.take(p, v, axis=ax).reshape(msg.shape)
        assert not ((msg > 0) & (msg < tiny)).any(), ("subnormal message entry", xv)
        sep = [v for v in scope if v != xv]
        (buckets[min(rank[v] for v in sep)] if sep else rest).append((sep, msg))
    return rows, rest


def run(model, evidence, order, n, seed, dtype=np.float64, first=0):
    """The whole run (bnpp_sample) -> (samples uint8 [n][n_vars], n_degenerate)."""
    evidence = dict(evidence or {})
    cards = model["cards"]
    rows, _ = forward(model, evidence, order, dtype)
    x = np.zeros((len(cards), n), dtype=np.uint8)
    for v, val in evidence.items():
        x[v] = val
    deg = 0
    for xv, ins in reversed(rows):
        x[xv], d = draw([t for _, t in ins], [vars_ for vars_, _ in ins], cards, xv, x, seed, first, dtype)
        deg += d
    return x.T, deg


def joint(model, evidence=None):
    """Brute force -> (free variables, P(free | evidence) as an array over
    them); at most 2^16 joint states."""
    evidence = dict(evidence or {})
    cards = model["cards"]
    free = [v for v in range(len(cards)) if v not in evidence]
    states = 1
    for v in free:
        states *= cards[v]
    assert states <= 1 << 16
    j = np.ones([cards[v] for v in free] or [1], dtype=np.float64)
    for vars_, t in conditioned(model, evidence, np.float64):
        j = j * (_expand(vars_, t, free) if free else t.reshape([1]))
    return free, j / j.sum()


def bound(p, n):
    """The statistical bound on |p_hat - p| for a frequency over n independent
    samples: five standard deviations of a binomial proportion, plus up to
    four stray hits on an entry with tiny p."""
    p = np.asarray(p, dtype=np.float64)
    return 5.0 * np.sqrt(np.clip(p * (1.0 - p), 0.0, None) / n) + 4.0 / n


def check_frequencies(samples, cards, marginals=None, joint_of=None, scopes=()):
    """Compare sample frequencies against exact probabilities under bound():
    single-variable frequencies against `marginals` ({var: [p_0 ..]}) or the
    brute-force joint `joint_of` = joint(...); with the joint also the joint
    frequency over every scope in `scopes` (restricted to free variables).
    -> the list of violations (empty: all within the bound)."""
    n = samples.shape[0]
    bad = []
    if joint_of is not None:
        free, j = joint_of
        for i, v in enumerate(free):
            p = j.sum(axis=tuple(a for a in range(len(free)) if a != i))
            f = np.bincount(samples[:, v], minlength=cards[v])[: cards[v]] / n
            if (np.abs(f - p) > bound(p, n)).any():
                bad.append(("var", v, f.tolist(), p.tolist()))
        for scope in scopes:
            sc = [v for v in scope if v in free]
            if len(sc) < 2:
                continue
            keep = sorted(free.index(v) for v in sc)
            p = j.sum(axis=tuple(a for a in range(len(free)) if a not in keep)).reshape(-1)
            idx = np.zeros(n, dtype=np.int64)
            for a in keep:
                idx = idx * cards[free[a]] + samples[:, free[a]]
            f = np.bincount(idx, minlength=p.size) / n
            if (np.abs(f - p) > bound(p, n)).any():
                bad.append(("scope", list(scope), float(np.abs(f - p).max())))
    else:
        for v, p in marginals.items():
            p = np.asarray(p, dtype=np.float64)
            f = np.bincount(samples[:, v], minlength=cards[v])[: cards[v]] / n
            if (np.abs(f - p) > bound(p, n)).any():
                bad.append(("var", v, f.tolist(), p.tolist()))
    return bad


# The larger models of the distribution tests: (model, evidence file or "-").
# Their exact marginals are recorded in golden/sample_golden.json from the
# engine's fp64 bucket-tree marginals (`python tests/sample_ref.py [path]`
# rewrites it; needs a GPU), so that test_sample_host.py can put the bound on
# this restatement alone, without one.
LARGER = (("alarm", "alarm.uai.evid"), ("noisyor_50_80", "noisyor_50_80.uai.evid"), ("potts4x5k3", "-"),
          ("Munin1", "-"))

if __name__ == "__main__":
    import json
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "..", "bn-pp_amd", "python"))
    import bnpp
    from bnpp import synth
    ctx = bnpp.Context(0)
    rec = {}
    for name, evf in LARGER:
        path = os.path.join(here, "golden", "models", name + ".uai")
        ev = synth.read_evidence(os.path.join(here, "golden", "models", evf)) if evf != "-" else {}
        mm = bnpp.Model.load(path)
        marg, _ = bnpp.marginals_tree(ctx, mm, ev, "mf", bnpp.F64)
        rec[name] = {"evidence": evf, "marginals": {str(v): list(marg[v]) for v in range(mm.n_vars) if v not in ev}}
    ctx.close()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "golden", "sample_golden.json")
    with open(out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
