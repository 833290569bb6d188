"""Numpy restatement of the weighted gather (bnpp_condition_batch_sv), the rule
that picks the factor carrying a soft variable's likelihoods, the per-row
soft model, the runtime's per-block scaling, and a brute-force joint with the
likelihoods as unary factors.

weighted_gather multiplies in the kernel's order -- the soft dims in the order
of the scope, left to right, each product rounded once in the table's dtype --
so the engine's table must equal it bit for bit in both dtypes.

soft_model multiplies the factors in the CALL's dtype: the engine converts a
model's fp64 values to fp32 on upload, so for an fp32 call the factor is
float32(v) * float32(lam) rounded to float32, which a float32 holds exactly and
the upload returns unchanged.
"""
import numpy as np

import missing_ref
from missing_ref import MISSING, condition, joint


def lam_rows(cards, soft_vars):
    """Per soft variable its first row of lam (the blocks in the listed order), and the total Ws."""
    at, out = 0, []
    for v in soft_vars:
        out.append(at)
        at += cards[v]
    return out, at


def weighted_gather(T, cards, scope, ev_vars, partial, ev, soft_vars, lam):
    """missing_ref.masked_gather, then for every soft variable of the scope, in
    scope order, out *= lam[row0_v + digit_v(rest)][b].  lam: (Ws, R) in T's
    dtype.  A soft variable outside the scope is ignored."""
    t = np.asarray(T)
    R = np.asarray(ev).reshape(len(ev_vars), -1).shape[1] if len(ev_vars) else np.asarray(lam).shape[1]
    ev = np.asarray(ev).reshape(len(ev_vars), R) if len(ev_vars) else np.zeros((0, R), dtype=np.int64)
    out = missing_ref.masked_gather(t, cards, scope, ev_vars, partial, ev) if len(ev_vars) else \
        np.repeat(t.reshape(-1, 1), R, axis=1).reshape(-1)
    rest = [v for v in scope if v not in ev_vars or v in set(partial)]
    shape = [cards[v] for v in rest]
    out = out.reshape(shape + [R]).astype(t.dtype)
    lam = np.asarray(lam, dtype=t.dtype)
    row0, _ = lam_rows(cards, soft_vars)
    for d, v in enumerate(rest):                # the scope's order, left to right
        if v in soft_vars:
            r0 = row0[list(soft_vars).index(v)]
            w = lam[r0:r0 + cards[v]].reshape([cards[v] if i == d else 1 for i in range(len(rest))] + [R])
            out = (out * w).astype(t.dtype)     # one rounding per soft dim
    return out.reshape(-1)


def lam_factors(model_dict, ev_vars, partial, soft_vars):
    """Per soft variable the factor that carries its likelihoods, by the rule of
    missing_ref.mask_factors: 1. a factor holding a hard evidence variable;
    2. the fewest entries after conditioning on the hard variables; 3. the
    lowest factor index."""
    cards, scopes = model_dict["cards"], model_dict["scopes"]
    hard = [v for v in ev_vars if v not in set(partial)]
    out = []
    for v in soft_vars:
        cand = []
        for f, s in enumerate(scopes):
            if v in s:
                size = int(np.prod([cards[x] for x in s if x not in hard], dtype=np.int64))
                cand.append((0 if any(x in hard for x in s) else 1, size, f))
        out.append(min(cand)[2] if cand else -1)
    return out


def soft_model(model_dict, soft_vars, lam_factor, lam_row, dtype=np.float64):
    """The model whose likelihood-carrying factors are multiplied by one row's
    weights (lam_row: the row's Ws likelihoods), in `dtype`'s arithmetic, the
    soft variables of one factor in the order of its scope."""
    cards, scopes = model_dict["cards"], model_dict["scopes"]
    values = [np.array(v, dtype=np.float64).astype(dtype).reshape([cards[x] for x in s])
              for s, v in zip(scopes, model_dict["values"])]
    row0, _ = lam_rows(cards, soft_vars)
    lam_row = np.asarray(lam_row, dtype=np.float64).astype(dtype)
    for f, s in enumerate(scopes):
        for d, v in enumerate(s):
            for i, sv in enumerate(soft_vars):
                if sv == v and lam_factor[i] == f:
                    w = lam_row[row0[i]:row0[i] + cards[v]].reshape([-1 if j == d else 1 for j in range(len(s))])
                    values[f] = (values[f] * w).astype(dtype)
    return dict(model_dict, values=[v.astype(np.float64).reshape(-1).tolist() for v in values])


def scale_blocks(cards, soft_vars, lik):
    """The runtime's scaling: every (row, variable) block times the power of two
    that brings its largest entry into [0.5, 1) -> (the scaled array, e[n]: the
    sum of a row's exponents; lik == scaled * 2^e block by block, exactly)."""
    lik = np.array(lik, dtype=np.float64)
    out, e = lik.copy(), np.zeros(lik.shape[0], dtype=np.int64)
    row0, _ = lam_rows(cards, soft_vars)
    for i, v in enumerate(soft_vars):
        blk = lik[:, row0[i]:row0[i] + cards[v]]
        top = blk.max(axis=1)
        ex = np.where(top > 0, np.frexp(np.where(top > 0, top, 1.0))[1], 0)
        out[:, row0[i]:row0[i] + cards[v]] = np.ldexp(blk, -ex[:, None])
        e += ex
    return out, e


def brute(model_dict, ev_vars, rows, soft_vars, lik, w=None):
    """missing_ref.brute with the likelihoods as unary factors -> (z[n],
    marginals per variable (n, card), NaN for Z = 0, counts per factor summed
    over the possible rows with weights w)."""
    cards, scopes = model_dict["cards"], model_dict["scopes"]
    nv = len(cards)
    jt = joint(model_dict)
    lik = np.asarray(lik, dtype=np.float64)
    n = lik.shape[0]
    rows = np.asarray(rows).reshape(n, len(ev_vars))
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    row0, _ = lam_rows(cards, soft_vars)
    z = np.zeros(n)
    marg = [np.full((n, c), np.nan) for c in cards]
    counts = [np.zeros([cards[x] for x in s]) for s in scopes]
    for b in range(n):
        cond = condition(jt, ev_vars, rows[b])
        for i, v in enumerate(soft_vars):
            cond = cond * lik[b, row0[i]:row0[i] + cards[v]].reshape([-1 if j == v else 1 for j in range(nv)])
        z[b] = cond.sum()
        if z[b] == 0:
            continue
        post = cond / z[b]
        for v in range(nv):
            marg[v][b] = np.einsum(post, list(range(nv)), [v])
        for f, s in enumerate(scopes):
            counts[f] += w[b] * np.einsum(post, list(range(nv)), list(s))
    return z, marg, counts


def random_lik(rng, cards, soft_vars, n, lo_exp=-20):
    """(n, Ws) likelihoods, log-uniform in [2^lo_exp, 1]."""
    _, ws = lam_rows(cards, soft_vars)
    return np.exp2(rng.uniform(lo_exp, 0.0, size=(n, ws)))


# the sampling distribution test: sample_batch_ref's case with one more variable soft.  The first candidate
# seed; test_soft_host.py asserts that the numpy restatement alone stays within sample_ref.bound under it
DIST_SEED = 20261021


def dist_case(model):
    """-> (ev_vars, rows, soft_vars, lik): sample_batch_ref.dist_case's 8 rows and the lowest non-evidence
    variable soft, with likelihoods in [1/4, 1] (row 3: a one-hot block, row 5: all ones)."""
    import sample_batch_ref as sbr
    ev_vars, rows = sbr.dist_case(model)
    s = min(v for v in range(len(model["cards"])) if v not in ev_vars)
    k = model["cards"][s]
    lik = np.random.default_rng(7).uniform(0.25, 1.0, size=(rows.shape[0], k))
    lik[3] = np.eye(k)[k - 1]
    lik[5] = 1.0
    return ev_vars, rows, [s], lik


def frequency_violations(model, ev_vars, rows, soft_vars, lik, samples):
    """sample_ref.check_frequencies per row against the joint with the row's likelihoods."""
    import sample_ref as sr
    cards = model["cards"]
    nv = len(cards)
    row0, _ = lam_rows(cards, soft_vars)
    bad = []
    for b, row in enumerate(rows):
        ev = {v: int(x) for v, x in zip(ev_vars, row) if x >= 0}
        free, jt = sr.joint(model, ev)
        for i, v in enumerate(soft_vars):
            jt = jt * np.asarray(lik[b, row0[i]:row0[i] + cards[v]]).reshape(
                [-1 if j == free.index(v) else 1 for j in range(len(free))])
        for x in sr.check_frequencies(samples[b], cards, joint_of=(free, jt / jt.sum())):
            bad.append((b,) + tuple(x))
    return bad


# ---- the plans without soft evidence, as recorded from the commit before the feature ----
# golden/soft_parent_plans.json: per (model, planner, dtype, hard / first evidence variable partial) the stats in
# full, the launch-group keys run-length encoded ([key, repeats]) and a sha256 prefix of all group rows and of
# whatever else the plan function returns.  plan_record uses nothing the commit before lacked: to rewrite the file,
# copy this module into a checkout of that commit, build it and run `python tests/soft_ref.py`.
PLAN_MODELS = ("asia", "alarm", "ising6x6")


def plan_record(result, fields):
    """One plan function's result -> the record kept in the golden file."""
    import hashlib
    import json
    stats, groups = result[0], [[g[k] for k in fields] for g in result[1]]
    keys = []
    for g in result[1]:
        if keys and keys[-1][0] == g["key"]:
            keys[-1][1] += 1
        else:
            keys.append([g["key"], 1])
    sha = lambda x: hashlib.sha256(json.dumps(x, sort_keys=True).encode()).hexdigest()[:16]
    return {"stats": stats, "keys": keys, "groups_sha": sha(groups), "rest_sha": sha(list(result[2:]))}


def plan_cases(bnpp, ev):
    """-> [(tag, planner, kwargs)] of the recorded cases for one model's evidence variables."""
    plans = {"batch": bnpp.plan_batch, "mpe": bnpp.plan_mpe_batch, "sample": bnpp.plan_sample_batch,
             "counts": bnpp.plan_counts, "marginals": bnpp.plan_marginals_batch}
    out = []
    for kind in sorted(plans):
        for dt, dtype in (("f64", bnpp.F64), ("f32", bnpp.F32)):
            for tag, part in (("hard", None), ("partial", [ev[0]])):
                out.append(("%s/%s/%s" % (kind, dt, tag), plans[kind], dict(dtype=dtype, rows_per_launch=64, partial=part)))
    return out


if __name__ == "__main__":
    import json
    import os
    import bnpp
    from conftest import model_path
    from counts_ref import EV_VARS
    rec = {}
    for name in PLAN_MODELS:
        m = bnpp.Model.load(model_path(name + ".uai"))
        for tag, fn, kw in plan_cases(bnpp, EV_VARS[name]):
            rec[name + "/" + tag] = plan_record(fn(m, EV_VARS[name], **kw), bnpp.PLAN_GROUP_FIELDS)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft_parent_plans.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(rec[k], sort_keys=True) for k in sorted(rec)) + "\n}\n")
    print(path, len(rec))
