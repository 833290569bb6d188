"""CPU tests of posterior sampling's host side: the Philox known answers, the
numpy restatement (sample_ref.py) against exact probabilities, the sampling
plan (bnpp.plan_sample) and the argument checks."""
import json
import os

import numpy as np
import pytest

import bnpp
import sample_ref as sr
from bnpp import synth
from conftest import GOLDEN, evidence_of, model_path

DT = {"f64": bnpp.F64, "f32": bnpp.F32}
SEED = 20261019                                          # test_gpu_sample.py's
N_DIST = 65536
SMALL = [("asia", "-"), ("asia", "asia.uai.evid"), ("cancer", "-"), ("cancer", "cancer.uai.evid"),
         ("earthquake", "-"), ("earthquake", "earthquake.uai.evid"), ("grid3x3", "-"),
         ("grid3x3", "grid3x3-PR.uai.evid"), ("ising4x4", "-")]
# the forward pass of Munin1 alone takes ~15 s in numpy: its draws run at n = 8192
LARGER = [("alarm", "alarm.uai.evid", N_DIST), ("noisyor_50_80", "noisyor_50_80.uai.evid", N_DIST),
          ("potts4x5k3", "-", N_DIST), ("Munin1", "-", 8192)]


def test_philox_known_answers():
    """Random123's published vectors, and the draw of variable 3 in sample 5 under seed 42."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            "d16cfe09 94fdcceb 5001e420 24126ea1"),
           ((5, 0, 3, 0), (42, 0), "39b5e818 2fa9cf5e c8119bbf 370136f6")]
    for ctr, key, want in kat:
        assert " ".join("%08x" % w for w in sr.philox(ctr, key)) == want
    assert sr.uniform(42, [5], 3)[0] == 0.22543192472918527
    # the vectorised form is the scalar one, 64-bit seeds and indices included
    seed, g = 0x299F31D0A4093822, np.array([0, 5, 0x85A308D3243F6A88, 2 ** 64 - 1], dtype=np.uint64)
    for i, gi in enumerate(g.tolist()):
        r = sr.philox((gi & sr.MASK, gi >> 32, 7, 0), (seed & sr.MASK, seed >> 32))
        assert sr.uniform(seed, g, 7)[i] == ((r[0] << 32 | r[1]) >> 11) * 2.0 ** -53
    u = sr.uniform(SEED, np.arange(4096), 1)
    assert (u >= 0).all() and (u < 1).all()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_draw_never_returns_a_value_of_zero_weight(dt):
    rng = np.random.default_rng(3)
    cards = [5, 3, 4]
    scopes = [[1, 0], [0, 2]]
    ins = [rng.choice([0.0, 0.5, 1.0], size=15, p=[0.5, 0.25, 0.25]), rng.choice([0.0, 0.5, 1.0], size=20)]
    n = 4096
    x = np.stack([rng.integers(0, c, n).astype(np.uint8) for c in cards])
    p = sr.weights(ins, scopes, cards, 0, x, dt)
    zero_row = ~(p > 0).any(axis=0)
    assert zero_row.any() and (~zero_row).any() and (p[0] == 0).any()
    for u in (None, np.zeros(n), np.full(n, 1.0 - 2.0 ** -53)):
        row, deg = sr.draw(ins, scopes, cards, 0, x, SEED, 0, dt, u=u)
        assert (p[row, np.arange(n)] > 0)[~zero_row].all()
        assert not row[zero_row].any() and deg == int(zero_row.sum())


@pytest.mark.parametrize("name,evf", SMALL)
def test_reference_meets_the_bound_on_small_models(name, evf):
    m = synth.read_uai(model_path(name + ".uai"))
    ev = evidence_of(evf)
    order, _ = bnpp.ordering(bnpp.Model.load(model_path(name + ".uai")), ev)
    for dt in (np.float64, np.float32):
        x, deg = sr.run(m, ev, order, N_DIST, SEED, dt)
        assert deg == 0 and all((x[:, v] == val).all() for v, val in ev.items())
        bad = sr.check_frequencies(x, m["cards"], joint_of=sr.joint(m, ev), scopes=m["scopes"])
        assert not bad, bad[:3]


@pytest.mark.parametrize("name,evf,n", LARGER)
def test_reference_meets_the_bound_on_larger_models(name, evf, n):
    """Against the recorded fp64 bucket-tree marginals (golden/sample_golden.json,
    written by `python tests/sample_ref.py` on a GPU)."""
    with open(os.path.join(GOLDEN, "sample_golden.json")) as f:
        rec = json.load(f)[name]
    assert rec["evidence"] == evf
    m = synth.read_uai(model_path(name + ".uai"))
    ev = evidence_of(evf)
    order, _ = bnpp.ordering(bnpp.Model.load(model_path(name + ".uai")), ev)
    x, deg = sr.run(m, ev, order, n, SEED, np.float64)
    assert deg == 0
    marg = {int(v): p for v, p in rec["marginals"].items()}
    assert sorted(marg) == [v for v in range(len(m["cards"])) if v not in ev]
    bad = sr.check_frequencies(x, m["cards"], marginals=marg)
    assert not bad, bad[:3]


@pytest.mark.parametrize("name,evf", [("asia", "-"), ("asia", "asia.uai.evid"), ("alarm", "-"), ("alarm", "alarm.uai.evid")])
def test_the_sampling_plan(name, evf):
    mm = bnpp.Model.load(model_path(name + ".uai"))
    ev = evidence_of(evf)
    for dt in DT.values():
        st, groups = bnpp.plan_sample(mm, 1, ev, dtype=dt)
        assert st["sample_rows"] == mm.n_vars - len(ev)              # one row per non-evidence variable
        assert st["sample_bytes"] == mm.n_vars
        assert groups[-1]["key"] == bnpp.SAMPLE_KEY and groups[-1]["n_desc"] == 1
        # every earlier group is an ordinary sum kernel: generic (< 2048), stream (4096 ..) or slab
        # (16384 .. 32767), never a chain run (8192 .. 16383), a max bucket (65536 ..) or an executor step
        assert all(g["key"] < 8192 or 16384 <= g["key"] < 32768 for g in groups[:-1]), groups
        assert all(g["level"] < groups[-1]["level"] for g in groups[:-1])
        st2, _ = bnpp.plan_sample(mm, 65536, ev, dtype=dt)
        grow = st2["arena_bytes"] - st["arena_bytes"]                # tables are placed at multiples of 256 B
        assert abs(grow - mm.n_vars * 65535) <= 512, grow


def test_card_limit_and_bad_arguments():
    mm = bnpp.Model.load(model_path("asia.uai"))
    for n in (0, -1):
        with pytest.raises(bnpp.BnppError) as e:
            bnpp.plan_sample(mm, n)
        assert e.value.status == bnpp.ERR_INVALID
    for dt in DT.values():
        for card, ok in ((256, True), (257, False)):
            vals = [[1.0 + (i % 7) for i in range(card * 2)], [0.5, 0.25]]
            m = bnpp.Model.from_arrays([card, 2], [[0, 1], [1]], [v for t in vals for v in t])
            if ok:
                assert bnpp.plan_sample(m, 16, dtype=dt)[1][-1]["key"] == bnpp.SAMPLE_KEY
            else:
                with pytest.raises(bnpp.BnppError) as e:
                    bnpp.plan_sample(m, 16, dtype=dt)
                assert e.value.status == bnpp.ERR_UNSUPPORTED
                # as evidence the variable is not sampled
                assert bnpp.plan_sample(m, 16, {0: 256}, dtype=dt)[0]["sample_rows"] == 1


def test_out_of_memory_names_messages_and_samples(monkeypatch):
    mm = bnpp.Model.load(model_path("ising12x12.uai"))
    monkeypatch.setenv("BNPP_MEM_BUDGET_GB", "0.01")
    assert bnpp.plan_sample(mm, 16)
    with pytest.raises(bnpp.BnppError) as e:
        bnpp.plan_sample(mm, 1 << 20)
    assert e.value.status == bnpp.ERR_OOM
    assert "messages" in str(e.value) and "samples" in str(e.value)
