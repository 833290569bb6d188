"""An in-process world for the message-sliced bucket tree: R ranks
as R threads of one process, each with its own bnpp.Context(0), exchanging
through a Python collective handed to bnpp.marginals_tree_sliced.  The library
keeps its error text and timing per thread and its caches per context, and a
device pointer of any context is valid in the one process, so a world of 16
costs milliseconds where a gloo world costs a process (and a torch import) per
rank.

Two collectives over one threading.Barrier(R, timeout=60):

  staged  synchronous, the shape of TorchCollective's gloo branch: the stream
          is synchronised, the send bytes go through host memory, the 16-byte
          all-gathers (xchg_sync_kernel's (E_r, exp2_r) pairs) are decoded into
          record["sync"].
  stream  stream-ordered, the shape of its RCCL branch: cross-context events
          and device-to-device copies on the engine's own stream, no host wait
          on the GPU; the host barrier only orders event *recording* before
          event *waiting* (a wait on an unrecorded event is a no-op).

A raising callback aborts the barrier: its peers' callbacks then raise
BrokenBarrierError, every rank's call returns an error, run_world joins with a
timeout and raises WorldError -- a hang is bounded and reported as a failure.

This is a plain helper module (no tests, no fixtures).
"""
import math
import random
import threading
import time

import numpy as np

import bnpp

BARRIER_TIMEOUT_S = 60
JOIN_TIMEOUT_S = 120

# The worlds of tests/test_gpu_sliced_world.py, (rows, cols, R) / (row cards,
# cols, R); tests/test_host.py pins the exchange shapes their plans must have.
ISING_WORLDS = [(16, 16, 2), (16, 16, 4), (16, 16, 8), (16, 16, 16), (10, 10, 2), (11, 11, 4)]
# binary slice rows below card-3 rows: same-order (mode 0) packs with an fp32
# vector tail, unpacks whose inner size is no multiple of 4
MIXED_WORLDS = [([3] * 8 + [2] * 2, 12, 2), ([3] * 7 + [2] * 3, 12, 4), ([3] * 6 + [2] * 6, 14, 8),
                ([3, 3] + [2] * 10, 14, 8)]
# binary rows above the card-3 rows and one below: the first re-slice takes
# slice variables that are the message's fastest, a transposing (mode 1) pack
# whose inner size is no multiple of 4 (4374, 729 -- odd -- and 162)
FAST_SLICE_WORLDS = [([2] * 2 + [3] * 7 + [2], 12, 2), ([2] * 3 + [3] * 6 + [2], 12, 4),
                     ([2] * 6 + [3] * 4 + [2], 12, 8)]


class InjectedFailure(RuntimeError):
    """Raised by a rank's callback on the call a test chose (run_world(fail=...))."""


class WorldError(RuntimeError):
    """A world run that did not complete.  errors[r]: rank r's exception or
    None; last_error[r]: the library's error text on rank r's thread."""

    def __init__(self, msg, errors, last_error):
        super().__init__(msg)
        self.errors = errors
        self.last_error = last_error


def _r6(x):
    return float("%.6g" % x)


def mixed_grid(row_cards, cols, seed=0, unary=None):
    """len(row_cards) x cols grid, variable id = i*cols + j with cardinality
    row_cards[i]; the factor list laid out as synth.ising_grid's (unary tables
    row-major, then horizontal pairs, then vertical pairs), every value
    U(0.5, 2) rounded through %.6g, one draw per entry in list order.
    unary: {variable: table} replaces chosen unary tables (after the draws, so
    the other tables do not move)."""
    rng = random.Random(seed)
    rows = len(row_cards)
    n = rows * cols
    cards = [row_cards[v // cols] for v in range(n)]
    scopes = [[v] for v in range(n)]
    scopes += [[i * cols + j, i * cols + j + 1] for i in range(rows) for j in range(cols - 1)]
    scopes += [[i * cols + j, (i + 1) * cols + j] for i in range(rows - 1) for j in range(cols)]
    values = []
    for s in scopes:
        size = 1
        for v in s:
            size *= cards[v]
        values.append([_r6(rng.uniform(0.5, 2.0)) for _ in range(size)])
    for v, tab in (unary or {}).items():
        assert len(tab) == cards[v], (v, tab)
        values[v] = [float(x) for x in tab]
    return {"type": "MARKOV", "cards": cards, "scopes": scopes, "values": values}


def with_unary(model, unary):
    """A copy of a synth model dict with chosen unary tables replaced (factor v
    is variable v's unary table in every grid builder)."""
    values = [list(t) for t in model["values"]]
    for v, tab in unary.items():
        assert model["scopes"][v] == [v] and len(tab) == model["cards"][v], (v, tab)
        values[v] = [float(x) for x in tab]
    return dict(model, values=values)


def column_order(rows, cols, evidence=None):
    ev = evidence or {}
    return [i * cols + j for j in range(cols) for i in range(rows) if i * cols + j not in ev]


class _World:
    def __init__(self, R, fail):
        self.R = R
        self.fail = fail                       # (rank, 1-based call number) or None
        self.barrier = threading.Barrier(R, timeout=BARRIER_TIMEOUT_S)
        self.slots = [None] * R                # staged: each rank's send bytes
        self.sends = [None] * R                # stream: each rank's send tensor
        self.ready = [None] * R                # stream: "send ready" events
        self.done = [None] * R                 # stream: "copies done" events
        self.n_calls = [0] * R
        self.record = {"sync": [], "calls": 0, "bytes": 0}

    def callback(self, rank, ctx, inner):
        def cb(op, send, recv, nbytes, stream):
            try:
                self.n_calls[rank] += 1
                if self.fail == (rank, self.n_calls[rank]):
                    raise InjectedFailure("rank %d, call %d" % (rank, self.n_calls[rank]))
                inner(rank, ctx, op, send, recv, nbytes, stream)
                if rank == 0:
                    self.record["calls"] += 1
                    self.record["bytes"] += nbytes * (self.R - 1)
            except BaseException:
                self.barrier.abort()
                raise
        return cb

    def staged(self, rank, ctx, op, send, recv, nbytes, stream):
        R = self.R
        ctx.synchronize(stream)
        buf = np.empty(nbytes * (R if op == bnpp.COLL_ALLTOALL else 1), dtype=np.uint8)
        bnpp._check(bnpp._lib.bnpp_memcpy_d2h(ctx.handle, buf.ctypes.data, send, buf.size), "d2h")
        self.slots[rank] = buf
        self.barrier.wait()
        if op == bnpp.COLL_ALLGATHER:
            out = np.concatenate(self.slots)
            # the sync step gathers in place: its send pair lies right behind the R gathered ones
            if nbytes == 16 and send == recv + 16 * R and rank == 0:
                pairs = out.view(np.int64).reshape(R, 2)
                self.record["sync"].append([(int(e), int(x)) for e, x in pairs])
        elif op == bnpp.COLL_ALLTOALL:
            out = np.concatenate([self.slots[p][rank * nbytes:(rank + 1) * nbytes] for p in range(R)])
        else:
            raise ValueError("unknown collective op %r" % (op,))
        assert out.size == nbytes * R
        bnpp._check(bnpp._lib.bnpp_memcpy_h2d(ctx.handle, recv, out.ctypes.data, out.size), "h2d")
        self.barrier.wait()                    # nobody overwrites a slot that is still being read

    @staticmethod
    def _device(ptr, nbytes):
        import torch

        class _CAI:
            pass
        o = _CAI()
        o.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3,
                                      "strides": None}
        return torch.as_tensor(o, device="cuda")

    def stream(self, rank, ctx, op, send, recv, nbytes, stream):
        import torch
        R = self.R
        if op not in (bnpp.COLL_ALLGATHER, bnpp.COLL_ALLTOALL):
            raise ValueError("unknown collective op %r" % (op,))
        s = torch.cuda.ExternalStream(stream or ctx.stream())
        self.sends[rank] = self._device(send, nbytes * (R if op == bnpp.COLL_ALLTOALL else 1))
        rt = self._device(recv, nbytes * R)
        ev = torch.cuda.Event()
        ev.record(s)                           # send ready
        self.ready[rank] = ev
        self.barrier.wait()                    # every rank's event is recorded before anyone waits on it
        with torch.cuda.stream(s):
            for p in range(R):
                s.wait_event(self.ready[p])
            for p in range(R):
                src = self.sends[p]
                if op == bnpp.COLL_ALLTOALL:
                    src = src[rank * nbytes:(rank + 1) * nbytes]
                rt[p * nbytes:(p + 1) * nbytes].copy_(src, non_blocking=True)
            dn = torch.cuda.Event()
            dn.record(s)                       # copies done
        self.done[rank] = dn
        self.barrier.wait()
        for p in range(R):                     # a peer's next kernel must not overwrite a send buffer being read
            s.wait_event(self.done[p])


def run_world(model, R, dtype, order, evidence=None, collective="staged", budget_gb=1.0, calls=1, fail=None):
    """R rank threads, each calling bnpp.marginals_tree_sliced `calls` times on
    its own context -> (results, record): results[r][k] = (mant, exps, plan_ms)
    of rank r's k-th call; record["sync"]: the decoded (E_r, exp2_r) pairs of
    every 16-byte all-gather (staged only), record["calls"] / ["bytes"]:
    exchanges and bytes sent by rank 0.  model: a synth dict or a bnpp.Model.
    fail=(rank, n): that rank's callback raises on its n-th call."""
    if collective not in ("staged", "stream"):
        raise ValueError(collective)
    if collective == "stream":
        import torch
        torch.cuda.init()
    m = model if isinstance(model, bnpp.Model) else bnpp.Model.from_dict(model)
    w = _World(R, fail)
    inner = w.staged if collective == "staged" else w.stream
    results = [None] * R
    errors = [None] * R
    last_error = [""] * R

    def body(rank):
        ctx = None
        try:
            if collective == "stream":
                import torch
                torch.cuda.set_device(0)
            ctx = bnpp.Context(0)
            cb = w.callback(rank, ctx, inner)
            out = []
            for _ in range(calls):
                mant, exps, _ = bnpp.marginals_tree_sliced(ctx, m, rank, R, cb, evidence, dtype=dtype, order=order,
                                                           budget_gb=budget_gb)
                out.append((mant, exps, bnpp.last_timing()["plan_ms"]))
            results[rank] = out
        except BaseException as e:
            errors[rank] = e
            last_error[rank] = bnpp._lib.bnpp_last_error().decode()
            w.barrier.abort()
        finally:
            if ctx is not None:
                ctx.close()

    threads = [threading.Thread(target=body, args=(r,), name="rank%d" % r, daemon=True) for r in range(R)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN_TIMEOUT_S
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [t.name for t in threads if t.is_alive()]
    if alive:
        w.barrier.abort()
        raise WorldError("world of %d: still running after %d s: %s" % (R, JOIN_TIMEOUT_S, alive), errors, last_error)
    failed = [r for r in range(R) if errors[r] is not None]
    if failed:
        # the root cause first: a broken barrier is what the other ranks see of it
        root = [r for r in failed if not isinstance(errors[r], threading.BrokenBarrierError)] or failed
        raise WorldError("world of %d: rank %d failed: %r" % (R, root[0], errors[root[0]]), errors,
                         last_error) from errors[root[0]]
    return results, w.record


def combine(model, results, call=0):
    """The marginals of one call from every rank's share mant * 2^exp: aligned
    per target to the largest exponent (bnpp.NO_EXP marks an all-zero share),
    summed with math.fsum and normalised -- bnpp.dist.combine_shares without
    torch."""
    cards = model["cards"] if isinstance(model, dict) else model.cards
    res = {}
    for t in results[0][call][0]:
        emax = max(rk[call][1][t] for rk in results)
        cols = [[] for _ in range(cards[t])]
        for rk in results:
            mant, exps, _ = rk[call]
            if exps[t] == bnpp.NO_EXP:
                continue
            sh = max(exps[t] - emax, -4000)
            for k, v in enumerate(mant[t]):
                cols[k].append(math.ldexp(v, sh))
        v = [math.fsum(c) for c in cols]
        z = math.fsum(v)
        res[t] = [x / z for x in v] if z > 0 else [1.0 / cards[t]] * cards[t]
    return res


def max_abs_diff(a, b, skip=()):
    """Largest absolute difference over all entries of two {var: marginal} maps."""
    assert set(a) == set(b)
    worst = 0.0
    for t, p in a.items():
        if t in skip:
            continue
        assert len(p) == len(b[t]), t
        worst = max(worst, max(abs(x - y) for x, y in zip(p, b[t])))
    return worst


def exp2_spread(sync):
    """Largest max - min of the gathered exp2_r over the exchanges whose ranks
    all hold a non-zero block."""
    best = 0
    for pairs in sync:
        xs = [x for e, x in pairs if e != bnpp.NO_EXP]
        if len(xs) > 1:
            best = max(best, max(xs) - min(xs))
    return best
