"""bench.py's plain run on the device, in this process: the record's fields,
--steps, and --dump-outputs against the same sums in torch."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu


def _run(capsys, argv):
    import bench
    bench.main(argv)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_plain_run_record_and_dump(tmp_path, capsys, dtype):
    """k = 4, w = 6 (16,384 outputs: dumped whole).  The dump is what the
    bucket's caller receives: bit-equal to the products and sums of the seeded
    inputs taken in the reference's order, and identical from run to run."""
    import torch
    k, w = 4, 6
    S = k ** w
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--k", str(k), "--w", str(w), "--dtype", dtype]
    rec = _run(capsys, argv + ["--dump-outputs", str(tmp_path / "a")])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["dtype"] == dtype and rec["full"] is False
    assert rec["unit"] == "factor-entries/s" and rec["higher_is_better"] is True
    assert rec["ms_per_step"] > 0
    assert abs(rec["value"] - k ** (w + 2) / (rec["ms_per_step"] * 1e-3)) <= 1e-9 * rec["value"]
    for leg in ("cpu_baseline", "mar", "mar_f64", "fp64_bucket"):
        assert rec[leg] is None, leg
    assert "checksum_ok" not in rec
    a = np.load(tmp_path / "a" / "bucket_out.npy")
    tdt = torch.float32 if dtype == "f32" else torch.float64
    assert a.shape == (S * k,) and a.dtype == (np.float32 if dtype == "f32" else np.float64)

    g = torch.Generator(device="cuda:0").manual_seed(1234)
    m_t = torch.rand(k * S, generator=g, device="cuda:0", dtype=tdt) * 1.5 + 0.5
    f_t = torch.rand(k * k, generator=g, device="cuda:0", dtype=tdt) * 1.5 + 0.5
    M, F = m_t.reshape(k, S), f_t.reshape(k, k)
    acc = torch.zeros(S, k, device="cuda:0", dtype=tdt)
    for x in range(k):
        acc = acc + M[x][:, None] * F[x][None, :]
    assert np.array_equal(a, acc.reshape(-1).cpu().numpy())

    _run(capsys, argv + ["--dump-outputs", str(tmp_path / "b")])
    assert np.array_equal(a, np.load(tmp_path / "b" / "bucket_out.npy"))
