"""numpy restatement of batched posterior sampling (include/bnpp.h
bnpp_sample_batch), independent of the engine: sample (b, s) is
sample_ref.run's draw for evidence row b at the global index first + b *
row_stride + s; an impossible row (Z = 0, the product of the forward pass's
scalars) has every draw degenerate and every sampled value 0, the contract's
rule for it.  Also the inputs of the distribution tests, built without a
device so that the CPU suite can put the bound on this restatement alone.
"""
import itertools

import numpy as np

import sample_ref as sr

# the distribution tests (test_sample_batch_host.py, test_gpu_sample_batch.py)
DIST_MODELS = ("asia", "cancer")
DIST_K = 4096
DIST_FIRST = 0
# One seed for both models.  The first candidate; test_sample_batch_host.py asserts that
# the restatement stays within sample_ref.bound under it (were it not to, the
# next seed would be searched there, as ASIA_BRUTE_SEED was).
DIST_SEED = 20261020


def run(model, ev_vars, rows, order, k, seed, first=0, row_stride=None, dtype=np.float64):
    """-> (samples uint8 [n_rows][k][n_vars], n_degenerate int64 [n_rows])."""
    stride = k if row_stride is None else row_stride
    rows = np.asarray(rows).reshape(len(rows), len(ev_vars))
    out = np.zeros((len(rows), k, len(model["cards"])), dtype=np.uint8)
    deg = np.zeros(len(rows), dtype=np.int64)
    for b, row in enumerate(rows):
        ev = dict(zip(ev_vars, (int(v) for v in row)))
        if partition(model, ev, order, dtype) > 0:
            out[b], deg[b] = sr.run(model, ev, order, k, seed, dtype, first=first + b * stride)
        else:                                               # impossible: zeros beside the evidence, every draw counted
            out[b][:, ev_vars] = row
            deg[b] = k * len(order)
    return out, deg


def partition(model, evidence, order, dtype=np.float64):
    """Z of the forward pass: the product of the scalars no bucket takes."""
    _, rest = sr.forward(model, evidence, order, dtype)
    z = 1.0
    for _, t in rest:
        z *= float(np.asarray(t, dtype=np.float64).reshape(-1)[0])
    return z


def dist_case(model):
    """The evidence of a distribution test -> (ev_vars, rows): the first three
    binary variables (in lexicographic order of the triples) whose 8 joint
    values are all possible, and those 8 rows."""
    cards = model["cards"]
    free, j = sr.joint(model)
    assert free == list(range(len(cards)))
    for ev_vars in itertools.combinations(range(len(cards)), 3):
        if any(cards[v] != 2 for v in ev_vars):
            continue
        p = j.sum(axis=tuple(a for a in range(len(cards)) if a not in ev_vars))
        if (p > 0).all():
            return list(ev_vars), np.array(list(itertools.product((0, 1), repeat=3)), dtype=np.int64)
    raise AssertionError("no three binary variables with 8 possible joint values")


def frequency_violations(model, ev_vars, rows, samples):
    """Every single-variable frequency of every row against the brute-force
    posterior under sample_ref.bound -> the list of violations."""
    bad = []
    for b, row in enumerate(rows):
        ev = dict(zip(ev_vars, (int(v) for v in row)))
        for v in sr.check_frequencies(samples[b], model["cards"], joint_of=sr.joint(model, ev)):
            bad.append((b,) + tuple(v))
    return bad
