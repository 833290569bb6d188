"""GPU test of the job cache under the batched calls: calls of different kinds
with the same evidence variable set and rows per launch never pick up one
another's cached job.

One context, asia, two evidence variables, 5 rows at rows_per_launch=4 (two
launches, the second padded).  partition_batch, posterior_batch, mpe_batch,
sample_batch (K = 2) and expected_counts run in that order and then in reverse
order with the same arguments: every second answer equals the first, and each
equals what the same call gives in a fresh context of a child process that
runs with BNPP_NO_JOB_CACHE set (no call there meets a cached job).  Equalities
are of bits.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EV_VARS = [2, 5]
ROWS = [[0, 0], [0, 1], [1, 0], [1, 1], [0, 1]]
R = 4
KINDS = ("partition", "posterior", "mpe", "sample", "counts")


def _call(bnpp, ctx, m, kind):
    """The answer of one batched call as a tuple of numpy arrays (no timings)."""
    if kind == "partition":
        lz, z, _ = bnpp.partition_batch(ctx, m, EV_VARS, ROWS, rows_per_launch=R)
        return lz, z
    if kind == "posterior":
        return (bnpp.posterior_batch(ctx, m, EV_VARS, ROWS, 0, rows_per_launch=R)[0],)
    if kind == "mpe":
        lv, x, _ = bnpp.mpe_batch(ctx, m, EV_VARS, ROWS, rows_per_launch=R)
        return lv, x
    if kind == "sample":
        return bnpp.sample_batch(ctx, m, EV_VARS, ROWS, 2, seed=7, rows_per_launch=R)
    counts, lz, n_impossible = bnpp.expected_counts(ctx, m, EV_VARS, ROWS, rows_per_launch=R)
    return counts, lz, np.array([n_impossible])


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
                                    for x, y in zip(a, b))


if __name__ == "__main__":                      # the child: a fresh context, every call plans afresh
    import conftest
    import bnpp
    assert os.environ.get("BNPP_NO_JOB_CACHE")
    model = bnpp.Model.load(conftest.model_path("asia.uai"))
    c = bnpp.Context(0)
    out = {}
    for kd in KINDS:
        for i, a in enumerate(_call(bnpp, c, model, kd)):
            out["%s_%d" % (kd, i)] = np.ascontiguousarray(a)
    c.close()
    np.savez(sys.argv[1], **out)
    sys.exit(0)

import pytest  # noqa: E402

import bnpp  # noqa: E402
from conftest import model_path  # noqa: E402

pytestmark = pytest.mark.gpu


def test_kinds_do_not_share_a_cached_job(ctx, tmp_path):
    m = bnpp.Model.load(model_path("asia.uai"))
    first = {kd: _call(bnpp, ctx, m, kd) for kd in KINDS}
    second = {kd: _call(bnpp, ctx, m, kd) for kd in reversed(KINDS)}
    for kd in KINDS:
        assert _same(first[kd], second[kd]), (kd, first[kd], second[kd])
    out = str(tmp_path / "fresh.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, BNPP_NO_JOB_CACHE="1"),
                       cwd=HERE, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    with np.load(out) as z:
        for kd in KINDS:
            fresh = tuple(z["%s_%d" % (kd, i)] for i in range(len(first[kd])))
            assert _same(tuple(np.ascontiguousarray(a) for a in first[kd]), fresh), (kd, first[kd], fresh)
