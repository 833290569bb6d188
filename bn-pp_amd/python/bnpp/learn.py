"""Parameter learning on top of expected_counts: the M step of a Bayesian
network's CPTs and a small EM driver; imputation (sample_batch) and
maximum-posterior-marginal decoding (marginals_batch) of the rows.

All rows of one call share their evidence variables.  Rows with different
missing patterns are the caller's to group by pattern: counts add, so call
expected_counts once per pattern, sum the counts and pass the sum to m_step.
There is no "missing" evidence value.
"""
from typing import List, Sequence, Tuple

import numpy as np

from . import F64, Context, Model, expected_counts, marginals_batch, sample_batch, split_counts, split_marginals


def m_step(model_dict: dict, counts, prior: float = 0.0) -> dict:
    """New CPTs from expected counts: theta = (N + prior) / sum over the child.

    model_dict is a BAYES model (type, cards, scopes, values): each factor is
    a CPT whose child is the LAST variable of its scope (the UAI convention).
    counts is the flat array of expected_counts, or its split_counts.  A
    parent configuration whose total is zero keeps its old row.  MARKOV models
    raise ValueError (iterative fitting is out of scope).
    """
    if model_dict.get("type") != "BAYES":
        raise ValueError("m_step fits the CPTs of a BAYES model; Markov networks need iterative fitting")
    per = counts if isinstance(counts, (list, tuple)) else split_counts(model_dict, counts)
    if len(per) != len(model_dict["scopes"]):
        raise ValueError("one count table per factor is needed")
    values = []
    for scope, old, n in zip(model_dict["scopes"], model_dict["values"], per):
        k = model_dict["cards"][scope[-1]] if len(scope) else 1
        old = np.asarray(old, dtype=np.float64).reshape(-1, k)
        num = np.asarray(n, dtype=np.float64).reshape(-1, k) + float(prior)
        tot = num.sum(axis=1, keepdims=True)
        new = np.where(tot > 0, num / np.where(tot > 0, tot, 1.0), old)
        values.append(new.reshape(-1).tolist())
    out = dict(model_dict)
    out["values"] = values
    return out


def em(ctx: Context, model_dict: dict, ev_vars: Sequence[int], rows, iters: int, weights=None, dtype: int = F64,
       prior: float = 0.0, partial=None, soft=None) -> Tuple[dict, List[float]]:
    """`iters` EM iterations on the rows -> (the fitted model_dict, the
    weighted log-likelihood in log10 of the model each iteration started from).

    Every iteration builds a new Model, takes its expected counts (the E step,
    on the device) and refits the CPTs with m_step.  Impossible rows (Z = 0)
    count nowhere and are left out of the log-likelihood.  All rows share
    ev_vars; group rows with different missing patterns by pattern yourself
    (see the module docstring) -- or pass `partial` (the variables that hold
    bnpp.MISSING in some row, or "auto"): every row then keeps its own pattern
    in one plan (expected_counts, missing values).  soft: (soft_vars, lik),
    per-row likelihoods of variables known only as noisy labels or scores
    (expected_counts, soft evidence); the log-likelihood then includes them.
    """
    w = None if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    cur, lls = model_dict, []
    for _ in range(int(iters)):
        counts, lz, _ = expected_counts(ctx, Model.from_dict(cur), ev_vars, rows, weights=w, dtype=dtype,
                                        partial=partial, soft=soft)
        ok = np.isfinite(lz)
        lls.append(float(np.sum((lz if w is None else w * np.where(ok, lz, 0.0))[ok])))
        cur = m_step(cur, counts, prior)
    return cur, lls


def impute(ctx: Context, model: Model, ev_vars: Sequence[int], rows, k: int = 1, seed: int = 0, dtype: int = F64,
           partial=None, soft=None):
    """k completions of every row, drawn from P(x | the row) (sample_batch with
    disjoint streams) -> uint8 (n, k, n_vars): the observed variables keep
    their values, the others are one exact joint draw.  Multiple imputation,
    the E step of a stochastic EM, posterior-predictive checks.  An impossible
    row (Z = 0) comes back with its observed values and zeros elsewhere.
    partial: the variables that may be bnpp.MISSING in a row (or "auto"); a
    row's observed entries keep their values, its missing ones are drawn.
    soft: (soft_vars, lik), per-row likelihoods; a soft variable is drawn."""
    return sample_batch(ctx, model, ev_vars, rows, int(k), seed=seed, dtype=dtype, partial=partial, soft=soft)[0]


def argmax_marginals(cards: Sequence[int], targets, out) -> np.ndarray:
    """The per-row argmax of every target's block of a marginals_batch array ->
    an (n, len(targets)) int array; the lowest value wins a tie (and a block of
    NaN, an impossible row's, reads 0)."""
    blocks = split_marginals(cards, targets, np.asarray(out))
    if not blocks:
        return np.zeros((np.asarray(out).shape[0], 0), dtype=np.int64)
    return np.stack([np.argmax(b, axis=1) for b in blocks], axis=1).astype(np.int64)


def classify(ctx: Context, model: Model, ev_vars: Sequence[int], rows, targets, dtype: int = F64, partial=None,
             soft=None):
    """Maximum-posterior-marginal decoding: for every row the most probable
    value of each target on its own, argmax_x P(X_t = x | the row) -> (an
    (n, len(targets)) int array, lowest value on ties; the (n, W) marginals of
    marginals_batch).  Unlike the MPE (mpe_batch) the targets are decoded one by
    one, which minimises the expected number of wrong labels.  partial: as
    marginals_batch's (rows with bnpp.MISSING entries); soft: (soft_vars, lik),
    per-row likelihoods (a soft target reads its posterior with them included)."""
    targets = [int(t) for t in targets]
    out, _ = marginals_batch(ctx, model, ev_vars, rows, targets=targets, dtype=dtype, partial=partial,
                             soft=soft)
    return argmax_marginals(model.cards, targets, out), out
