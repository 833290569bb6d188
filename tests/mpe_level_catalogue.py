"""Catalogue of whole models whose first elimination level launches one chosen
key of the max family's LEVEL dispatch (max_level_kernel; a helper like
max_catalogue.py, CPU only).

max_catalogue.py holds one bucket per max key and test_gpu_mpe.py runs each as
a single op (max_single_kernel).  Here the same buckets become models --
bnpp.Model.from_arrays(cards, scopes, values) eliminated in the order `elim`
first, then the other variables ascending -- so that bnpp.mpe runs the bucket
as the first launch group of an MPE plan, through the level kernel, with the
model's own factor tables as inputs (their scopes permuted against the output,
as the templates lay them out).  BNPP_NO_O32 per entry picks the offset width.

Two kinds of catalogue bucket do not carry over, and regenerate() replaces
them by a bucket searched from the same generator (cards k, c1, c2, c3 and the
"a" / "b" sizes of max_catalogue.specs); "from" tells which:

  * five inputs (class 8): max_catalogue's fourth template [1, 3] lacks the
    maximised variable, so in a whole model that factor waits in a later
    bucket and the first bucket has four inputs (class 4).  The replacement
    templates (TEMPLATES) hold variable 0 in every input.
  * the "b" size of the 4x1 tile: its variable 1 has 476 values, more than the
    256 an arg table's byte holds, which bnpp_plan_mpe_groups refuses.  The
    replacement has 238 x 22 x 4 output entries, as many as 476 x 11 x 4.

mpe_level_catalogue_data.json holds per key (one list for both dtypes: the
key and the virtual blocks are the same in fp64 and fp32) an "a" entry (under one
wave) and a "b" entry (11-21 virtual blocks, the last ragged: the capped
reruns) with the key and the virtual blocks bnpp_plan_mpe_groups reports for
the first group (written by `python tests/mpe_level_catalogue.py`, host only;
test_mpe_host.py checks it).  The tables come from max_catalogue.make_inputs
under the entry's seed: the bucket's index in max_catalogue.specs(), plus 100
until brute force over the joint finds one maximiser with a log gap above
MIN_GAP to the runner-up.  MIN_GAP is argued from the rounding of an fp32
product chain (see its comment), not measured as an fp32 margin on a device.
"""
import json
import os

import numpy as np

import max_catalogue as mc
import mpe_ref

# the log gap between the maximum and the runner-up that an entry's tables must show: an fp32 product of at
# most 9 tables (5 inputs, then the messages) is within 9 * 2^-24 = 5.4e-7 of exact, relative, so two
# assignments 1e-5 apart in log keep their order in fp32 (the "b" joints have 1.5e5 states: their two best lie
# about 1e-5 apart, a gap like the small models' 1e-3 does not exist there)
MIN_GAP = 1e-5
MAX_TRIES = 20
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mpe_level_catalogue_data.json")
# max_catalogue.TEMPLATES with the maximised variable 0 in every input
TEMPLATES = ([0, 1, 2, 3], [3, 0, 1], [2, 0, 3], [1, 0, 3], [0], [2, 1, 0], [0, 3], [0, 2])


def load():
    with open(DATA) as f:
        return json.load(f)["entries"]


def order_of(e):
    """The elimination order of an entry's model: `elim` first, the rest ascending."""
    return [e["elim"]] + [v for v in range(len(e["cards"])) if v != e["elim"]]


def model_dict(e):
    """The entry as a model dict (cards, scopes, values per factor): what mpe_ref takes."""
    return {"cards": e["cards"], "scopes": e["scopes"], "values": [v.tolist() for v in mc.make_inputs(e, e["seed"])]}


def model_of(bnpp, e):
    return bnpp.Model.from_arrays(e["cards"], e["scopes"], np.concatenate(mc.make_inputs(e, e["seed"])))


def first_max_group(bnpp, e, dtype, no_o32=None):
    """The first launch group of the entry's MPE plan under its offset switch (or the given one)."""
    old = os.environ.get("BNPP_NO_O32")
    os.environ["BNPP_NO_O32"] = "1" if (e["no_o32"] if no_o32 is None else no_o32) else "0"
    try:
        groups = bnpp.plan_mpe_groups(model_of(bnpp, e), None, dtype=dtype, order=order_of(e))
    finally:
        if old is None:
            del os.environ["BNPP_NO_O32"]
        else:
            os.environ["BNPP_NO_O32"] = old
    return groups[0]


def searched(n_in, v1, size):
    """(cards, scopes) of the replacement bucket for a class and tile."""
    k, c3 = {1: (2, 3), 2: (3, 2), 4: (7, 4)}[v1]
    c1, c2 = (5, 3) if size == "a" else (7 * 17 * min(v1, 2), 11 * (2 if v1 == 4 else 1))
    return [k, c1, c2, c3], ([list(t) for t in TEMPLATES[:n_in]] if n_in > 1 else [[1, 0, 2, 3]])


def entries_for(bnpp):
    """Per max key the "a" and the "b" bucket as a model: max_catalogue's where its
    plan's first group has the key, else the searched one (host only).  The max
    family's keys do not depend on the dtype: an entry serves both, and the fp32
    plan is asserted to report the fp64 plan's group (test_mpe_host.py too)."""
    ents = []
    for dt in (bnpp.F64,):
        for seed, (name, cards, scopes, elim, out, no_o32) in enumerate(mc.specs()):
            if not name.startswith("n"):
                continue
            n_in, v1, size = int(name[1]), int(name[4]), name[6]
            want = mc.key_of(n_in, v1, not no_o32)
            for source, (c, s) in (("max_catalogue", (cards, scopes)), ("search", searched(n_in, v1, size))):
                e = {"name": name, "cards": c, "scopes": s, "elim": elim, "no_o32": no_o32, "key": want,
                     "seed": seed, "from": source}
                try:
                    g = first_max_group(bnpp, e, dt)
                except bnpp.BnppError:
                    continue
                if g["key"] == want:
                    g32 = first_max_group(bnpp, e, bnpp.F32)
                    assert (g32["key"], g32["vblocks"]) == (g["key"], g["vblocks"]), (name, g, g32)
                    for _ in range(MAX_TRIES):
                        if mpe_ref.brute_force(model_dict(e))[2] > MIN_GAP:
                            break
                        e["seed"] += 100
                    else:
                        raise AssertionError("no seed gives %s a gap above MIN_GAP" % name)
                    ents.append(dict(e, vblocks=int(g["vblocks"])))
                    break
            else:
                raise AssertionError("no bucket of the generator plans onto key %d as a model" % want)
    return ents


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bn-pp_amd", "python"))
    os.environ.setdefault("BNPP_NO_TORCH", "1")
    import bnpp
    with open(DATA, "w") as f:
        f.write('{"entries": [\n' + ",\n".join(json.dumps(e, sort_keys=True) for e in entries_for(bnpp)) + "\n]}\n")
