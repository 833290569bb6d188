"""The batched calls on torch tensors that stay on the device (the _dv entries of include/bnpp.h).

partition_batch, marginals_batch, mpe_batch and sample_batch take `rows` and
`soft=(soft_vars, lik)` as torch tensors on the context's device and return
torch tensors there; row b's results are the host-array call's for the same
arguments.  Nothing is copied to the host: the rows and likelihoods are staged
and the results unpacked by kernels on the context's stream, which is made to
wait for torch's current stream first.  The call has waited for its own stream
when it returns, so the results are ready for any stream.  A CPU tensor, or a
tensor of another device, is a ValueError (never a silent copy).

log_soft=(soft_vars, loglik) is soft evidence in log space: natural logs of the
likelihoods (a network's logits or log-probabilities; -inf is the likelihood 0),
staged on the device without an exp in torch.  log_partition is ln Z of every
row as a torch.autograd.Function: its gradient with respect to loglik is the
posterior of the soft variables, which the same bucket-tree pass returns.

Tables is the tables of one model rewritten in place on the device, so that a
training loop plans once: expected_counts(tables=...) takes the rows' expected
sufficient statistics under them, m_step refits CPTs from the counts, em is
learn.em's loop made of the two, and log_likelihood is the rows' weighted
log-likelihood as a torch.autograd.Function whose gradient with respect to the
log tables is those counts.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import (F32, F64, LIK_LOG, MISSING, Context, Model, _check, _h, _ints, _lib, _order_args, _P,  # noqa: F401
               _targets_arg)


def _on_device(ctx: Context, t, what: str):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch tensor on the context's device" % what)
    if t.device.type != "cuda" or t.device.index != ctx.device:
        raise ValueError("%s is on %s, not on the context's device cuda:%d" % (what, t.device, ctx.device))
    return t


def _rows(ctx: Context, ev_vars: Sequence[int], rows):
    """(n_ev, ev_vars as c ints, n, the rows as a contiguous int32 tensor of the device)."""
    ev_vars = [int(v) for v in ev_vars]
    rows = _on_device(ctx, rows, "rows")
    if rows.dtype.is_floating_point or rows.dtype == torch.bool:
        raise ValueError("rows must be an integer tensor")
    if rows.dim() != 2 or rows.shape[1] != len(ev_vars):
        raise ValueError("rows must have shape (n, %d), not %s" % (len(ev_vars), tuple(rows.shape)))
    return len(ev_vars), _ints(ev_vars), rows.shape[0], rows.to(torch.int32).contiguous()


def _partial(ev_vars: Sequence[int], partial, rows):
    """partial as the entries take it: None, "auto" (evaluated on the device) or a sequence of variable ids."""
    if partial is None:
        return None
    ev_vars = [int(v) for v in ev_vars]
    flags = (C.c_ubyte * max(len(ev_vars), 1))()
    if isinstance(partial, str):
        if partial != "auto":
            raise ValueError('partial must be None, "auto" or a sequence of variable ids')
        for j, f in enumerate((rows == MISSING).any(0).tolist()):
            flags[j] = 1 if f else 0
        return flags
    ids = [int(v) for v in partial]
    for v in ids:
        if v not in ev_vars:
            raise ValueError("partial variable %d is not an evidence variable" % v)
    for j, v in enumerate(ev_vars):
        flags[j] = 1 if v in ids else 0
    return flags


def _soft(ctx: Context, model: Model, soft, n: int, log_soft=None):
    """(n_soft, the ids as c ints, the (n, Ws) tensor or None, its pointer, lik_dtype).  log_soft: the same pair
    with natural logs for likelihoods (lik_dtype | LIK_LOG); one of the two at most."""
    if soft is not None and log_soft is not None:
        raise ValueError("soft and log_soft are mutually exclusive")
    log = LIK_LOG if log_soft is not None else 0
    if log:
        soft = log_soft
    if soft is None:
        return 0, None, None, None, F64
    what = "loglik" if log else "lik"
    if not (isinstance(soft, (tuple, list)) and len(soft) == 2):
        raise ValueError("%s must be (soft_vars, %s)" % ("log_soft" if log else "soft", what))
    ids = [int(v) for v in soft[0]]
    lik = _on_device(ctx, soft[1], what)
    if lik.dtype not in (torch.float64, torch.float32):
        raise ValueError("%s must be a float64 or float32 tensor" % what)
    if all(0 <= v < model.n_vars for v in ids):
        ws = sum(model.cards[v] for v in ids)
        if lik.dim() != 2 or tuple(lik.shape) != (n, ws):
            raise ValueError("%s must have shape (%d, %d): one row per evidence row, the sum of the soft cards wide; "
                             "got %s" % (what, n, ws, tuple(lik.shape)))
    elif lik.dim() != 2 or lik.shape[0] != n:           # a bad id: the library names it
        raise ValueError("%s must have one row per evidence row" % what)
    lik = lik.detach().contiguous()                     # detach only drops the autograd view: the same data and pointer
    return (len(ids), _ints(ids) if ids else (C.c_int * 1)(), lik, _P(lik.data_ptr()),
            (F32 if lik.dtype == torch.float32 else F64) | log)


def _out(ctx: Context, out, shape, dtype, what: str):
    if out is None:
        return torch.empty(shape, dtype=dtype, device="cuda:%d" % ctx.device)
    _on_device(ctx, out, what)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor of shape %s" % (what, dtype, tuple(shape)))
    return out


def _enter(ctx: Context) -> None:
    """The context's stream waits for what torch's current stream has been given so far."""
    torch.cuda.ExternalStream(ctx.stream(), device=ctx.device).wait_stream(torch.cuda.current_stream(ctx.device))


def _ptr(t):
    return _P(t.data_ptr() or None)


def partition_batch(ctx: Context, model: Model, ev_vars: Sequence[int], rows, heuristic: str = "mf", dtype: int = F64,
                    rows_per_launch: int = 0, order: Optional[Sequence[int]] = None, partial=None, soft=None,
                    out=None, log_soft=None):
    """bnpp.partition_batch on device tensors -> (log10_z, z, uptime_ms), float64 tensors of length n.
    out: (log10_z, z) tensors to write instead of new ones.  log_soft: soft evidence as natural logs."""
    ne, ev_v, n, r32 = _rows(ctx, ev_vars, rows)
    ns, sv, lik, lp, ld = _soft(ctx, model, soft, n, log_soft)
    h, oa, no = _order_args(order, heuristic)
    lz = _out(ctx, out[0] if out is not None else None, (n,), torch.float64, "out[0]")
    z = _out(ctx, out[1] if out is not None else None, (n,), torch.float64, "out[1]")
    up = C.c_double()
    _enter(ctx)
    _check(_lib.bnpp_partition_batch_dv(_h(ctx), model.handle, ne, ev_v, n, _ptr(r32), _partial(ev_vars, partial, r32),
                                        ns, sv, lp, ld, h, oa, no, dtype, int(rows_per_launch), _ptr(lz), _ptr(z),
                                        C.byref(up)), "bnpp_partition_batch_dv")
    del r32, lik
    return lz, z, up.value


def marginals_batch(ctx: Context, model: Model, ev_vars: Sequence[int], rows, targets: Optional[Sequence[int]] = None,
                    heuristic: str = "mf", dtype: int = F64, rows_per_launch: int = 0,
                    order: Optional[Sequence[int]] = None, out=None, partial=None, soft=None, log_soft=None):
    """bnpp.marginals_batch on device tensors -> (out, log10_z): an (n, W) float64 tensor (what another model
    takes as soft=(targets, out)) and float64[n].  out: an (n, W) tensor to write instead of a new one.
    log_soft: soft evidence as natural logs."""
    ne, ev_v, n, r32 = _rows(ctx, ev_vars, rows)
    ns, sv, lik, lp, ld = _soft(ctx, model, soft, n, log_soft)
    h, oa, no = _order_args(order, heuristic)
    ts, nt, ta = _targets_arg(model, targets)
    width = sum(model.cards[t] for t in ts if 0 <= t < model.n_vars)
    out = _out(ctx, out, (n, max(width, 1)), torch.float64, "out")
    lz = _out(ctx, None, (n,), torch.float64, "log10_z")
    up = C.c_double()
    _enter(ctx)
    _check(_lib.bnpp_marginals_batch_dv(_h(ctx), model.handle, ne, ev_v, n, _ptr(r32), _partial(ev_vars, partial, r32),
                                        ns, sv, lp, ld, h, oa, no, nt, ta, dtype, int(rows_per_launch), _ptr(out),
                                        _ptr(lz), C.byref(up)), "bnpp_marginals_batch_dv")
    del r32, lik
    return out, lz


def mpe_batch(ctx: Context, model: Model, ev_vars: Sequence[int], rows, heuristic: str = "mf", dtype: int = F64,
              order: Optional[Sequence[int]] = None, rows_per_launch: int = 0, partial=None, soft=None, out=None,
              log_soft=None):
    """bnpp.mpe_batch on device tensors -> (log10_value float64[n], assignment int32 (n, n_vars), uptime_ms).
    out: (log10_value, assignment) tensors to write instead of new ones.  log_soft: soft evidence as natural
    logs (Viterbi decoding from log emission scores)."""
    ne, ev_v, n, r32 = _rows(ctx, ev_vars, rows)
    ns, sv, lik, lp, ld = _soft(ctx, model, soft, n, log_soft)
    h, oa, no = _order_args(order, heuristic)
    lv = _out(ctx, out[0] if out is not None else None, (n,), torch.float64, "out[0]")
    x = _out(ctx, out[1] if out is not None else None, (n, max(model.n_vars, 1)), torch.int32, "out[1]")
    up = C.c_double()
    _enter(ctx)
    _check(_lib.bnpp_mpe_batch_dv(_h(ctx), model.handle, ne, ev_v, n, _ptr(r32), _partial(ev_vars, partial, r32), ns, sv,
                                  lp, ld, h, oa, no, dtype, int(rows_per_launch), _ptr(lv), _ptr(x), C.byref(up)),
           "bnpp_mpe_batch_dv")
    del r32, lik
    return lv, x, up.value


def sample_batch(ctx: Context, model: Model, ev_vars: Sequence[int], rows, n_per_row: int, seed: int = 0,
                 first_sample: int = 0, row_stride: Optional[int] = None, heuristic: str = "mf", dtype: int = F64,
                 order: Optional[Sequence[int]] = None, rows_per_launch: int = 0, partial=None, soft=None, out=None,
                 log_soft=None):
    """bnpp.sample_batch on device tensors -> (samples uint8 (n, n_per_row, n_vars), log10_z float64[n],
    n_degenerate int64[n]).  out: a samples tensor to write instead of a new one.  log_soft: soft evidence as
    natural logs (sampling from logits)."""
    ne, ev_v, n, r32 = _rows(ctx, ev_vars, rows)
    ns, sv, lik, lp, ld = _soft(ctx, model, soft, n, log_soft)
    h, oa, no = _order_args(order, heuristic)
    k = int(n_per_row)
    stride = k if row_stride is None else int(row_stride)
    out = _out(ctx, out, (n, max(k, 1), max(model.n_vars, 1)), torch.uint8, "out")
    lz = _out(ctx, None, (n,), torch.float64, "log10_z")
    deg = _out(ctx, None, (n,), torch.int64, "n_degenerate")
    up = C.c_double()
    _enter(ctx)
    _check(_lib.bnpp_sample_batch_dv(_h(ctx), model.handle, ne, ev_v, n, _ptr(r32), _partial(ev_vars, partial, r32), ns,
                                     sv, lp, ld, h, oa, no, dtype, int(rows_per_launch), k, int(first_sample), stride,
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out), _ptr(lz), _ptr(deg), C.byref(up)),
           "bnpp_sample_batch_dv")
    del r32, lik
    return out, lz, deg


class _LogPartition(torch.autograd.Function):
    """ln Z of every row; d ln Z_b / d loglik[b, w] = the posterior of the soft variables, which the marginals
    plan of the same pass returns (bnpp_log_partition_dv with post)."""

    @staticmethod
    def forward(fctx, loglik, need, ctx, model, ev_vars, rows, soft_vars, partial, heuristic, dtype, rows_per_launch, order):
        ne, ev_v, n, r32 = _rows(ctx, ev_vars, rows)
        ns, sv, lik, lp, ld = _soft(ctx, model, None, n, None if loglik is None else (soft_vars, loglik))
        h, oa, no = _order_args(order, heuristic)
        ln_z = _out(ctx, None, (n,), torch.float64, "ln_z")
        need = need and ns > 0
        post = _out(ctx, None, tuple(lik.shape), torch.float64, "post") if need else None
        up = C.c_double()
        _enter(ctx)
        _check(_lib.bnpp_log_partition_dv(_h(ctx), model.handle, ne, ev_v, n, _ptr(r32), _partial(ev_vars, partial, r32),
                                          ns, sv, lp, ld | LIK_LOG, h, oa, no, dtype, int(rows_per_launch), _ptr(ln_z),
                                          _ptr(post) if need else None, C.byref(up)), "bnpp_log_partition_dv")
        del r32, lik
        if need:
            fctx.save_for_backward(post)
        if loglik is not None:
            fctx.lik_shape, fctx.lik_dtype = tuple(loglik.shape), loglik.dtype
        return ln_z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad_out):
        if not fctx.saved_tensors:                          # no soft variable: an (n, 0) loglik, whose gradient is empty
            return (grad_out.new_zeros(fctx.lik_shape, dtype=fctx.lik_dtype),) + (None,) * 11
        (post,) = fctx.saved_tensors
        return ((grad_out.double()[:, None] * post).to(fctx.lik_dtype),) + (None,) * 11


def log_partition(ctx: Context, model: Model, ev_vars: Sequence[int], rows, log_soft=None, partial=None,
                  heuristic: str = "mf", dtype: int = F64, rows_per_launch: int = 0,
                  order: Optional[Sequence[int]] = None):
    """ln Z of every row -> a float64 tensor of length n, differentiable with respect to the loglik of
    log_soft=(soft_vars, loglik): the gradient of row b is its posterior of the soft variables (with the
    likelihoods included), so an entry of -inf has gradient 0.  Where loglik requires no gradient (or grad mode
    is off) the call runs partition_batch's plan, else marginals_batch's on the soft variables.  An impossible
    row reads -inf and NaN in its gradient row.  No double backward."""
    if log_soft is None:
        loglik, soft_vars = None, ()
    elif isinstance(log_soft, (tuple, list)) and len(log_soft) == 2:
        soft_vars, loglik = [int(v) for v in log_soft[0]], log_soft[1]
    else:
        raise ValueError("log_soft must be (soft_vars, loglik)")
    need = loglik is not None and isinstance(loglik, torch.Tensor) and loglik.requires_grad and torch.is_grad_enabled()
    return _LogPartition.apply(loglik, need, ctx, model, ev_vars, rows, soft_vars, partial, heuristic, dtype,
                               int(rows_per_launch), order)


# ---- device-resident model tables: parameter learning without a trip through the host ----

def _leave(ctx: Context) -> None:
    """torch's current stream waits for what the context's stream has been given (a step that is not waited for)."""
    torch.cuda.current_stream(ctx.device).wait_stream(torch.cuda.ExternalStream(ctx.stream(), device=ctx.device))


def _counts_size(model: Model) -> int:
    total = C.c_int64()
    _check(_lib.bnpp_counts_size(model.handle, C.byref(total)), "bnpp_counts_size")
    return total.value


def _flat(ctx: Context, t, n: int, what: str, dtypes=(torch.float64, torch.float32)):
    """t as a contiguous flat tensor of n entries on the context's device (the same data where it already is one)."""
    t = _on_device(ctx, t, what)
    if t.dtype not in dtypes:
        raise ValueError("%s must be a %s tensor" % (what, " or ".join(str(d).replace("torch.", "") for d in dtypes)))
    if t.numel() != n:
        raise ValueError("%s must have %d entries (the model's tables, flat), not %d" % (what, n, t.numel()))
    return t.detach().contiguous().reshape(-1)


class Tables:
    """The tables of one model on one context in one dtype, rewritten in place on the device (bnpp_tables): the
    calls that take tables= read them instead of the model's own values, from one plan and one job however often
    they are set.  They start as the model's own values.  Keeps its context and its model alive."""

    def __init__(self, ctx: Context, model: Model, dtype: int = F64):
        self._h = _P()
        self.ctx, self.model, self.dtype = ctx, model, dtype
        self.size = _counts_size(model)
        _check(_lib.bnpp_tables_create(_h(ctx), model.handle, dtype, C.byref(self._h)), "bnpp_tables_create")
        own = (C.c_double * max(self.size, 1))()
        _check(_lib.bnpp_model_values(model.handle, own), "bnpp_model_values")
        self.values = torch.tensor(list(own[: self.size]), dtype=torch.float64, device="cuda:%d" % ctx.device)
        self.log = False

    @property
    def handle(self):
        return self._h

    def set(self, values, log: bool = False) -> "Tables":
        """New values for every factor: one flat float64 or float32 tensor of the device in the layout of counts;
        log=True: natural logs (-inf is the value 0).  The first invalid entry raises, naming its factor."""
        v = _flat(self.ctx, values, self.size, "values")
        _enter(self.ctx)
        _check(_lib.bnpp_tables_set_dv(self._h, _ptr(v), (F32 if v.dtype == torch.float32 else F64) | (LIK_LOG if log else 0)),
               "bnpp_tables_set_dv")
        self.values, self.log = values, bool(log)
        return self

    def to_model_dict(self, model_dict: dict) -> dict:
        """model_dict (type, cards, scopes) with the values last set (their exp, for a log form), by one
        device-to-host copy: what Model.from_dict takes, for the calls that take no tables."""
        v = self.values.detach().reshape(-1).double()
        flat = (torch.exp(v) if self.log else v).cpu().tolist()
        out, at = dict(model_dict), 0
        out["values"] = []
        for s in model_dict["scopes"]:
            size = 1
            for x in s:
                size *= model_dict["cards"][x]
            out["values"].append(flat[at:at + size])
            at += size
        if at != len(flat):
            raise ValueError("model_dict does not match the tables' model")
        return out

    def close(self) -> None:
        if self._h:
            _lib.bnpp_tables_free(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _counts_call(ctx, model, ev_vars, rows, weights, tables, partial, soft, log_soft, accumulate, out, heuristic, dtype,
                 rows_per_launch, order, with_counts: bool, with_ln: bool):
    """bnpp_expected_counts_dv -> (counts or None, log10_z, ln_z or None, n_impossible)."""
    ne, ev_v, n, r32 = _rows(ctx, ev_vars, rows)
    ns, sv, lik, lp, ld = _soft(ctx, model, soft, n, log_soft)
    h, oa, no = _order_args(order, heuristic)
    if tables is not None and not isinstance(tables, Tables):
        raise ValueError("tables must be a bnpp.tensor.Tables")
    if dtype is None:
        dtype = tables.dtype if tables is not None else F64
    w = None if weights is None else _flat(ctx, weights, n, "weights", (torch.float64,))
    total = _counts_size(model)
    counts = None
    if with_counts:
        if accumulate and out is None:
            raise ValueError("accumulate=True adds to out: pass the counts tensor of the earlier call")
        counts = _out(ctx, out, (max(total, 1),), torch.float64, "out")
    lz = _out(ctx, None, (n,), torch.float64, "log10_z")
    ln = _out(ctx, None, (n,), torch.float64, "ln_z") if with_ln else None
    ni = _out(ctx, None, (), torch.int64, "n_impossible")
    up = C.c_double()
    _enter(ctx)
    _check(_lib.bnpp_expected_counts_dv(_h(ctx), model.handle, tables.handle if tables is not None else None, ne, ev_v, n,
                                        _ptr(r32), _partial(ev_vars, partial, r32), ns, sv, lp, ld,
                                        _ptr(w) if w is not None else None, 1 if accumulate else 0, h, oa, no, dtype,
                                        int(rows_per_launch), _ptr(counts) if with_counts else None, _ptr(lz),
                                        _ptr(ln) if with_ln else None, _ptr(ni), C.byref(up)), "bnpp_expected_counts_dv")
    del r32, lik, w
    return (counts[:total] if with_counts else None), lz, ln, ni


def expected_counts(ctx: Context, model: Model, ev_vars: Sequence[int], rows, weights=None, tables: Optional[Tables] = None,
                    partial=None, soft=None, log_soft=None, accumulate: bool = False, out=None, heuristic: str = "mf",
                    dtype: Optional[int] = None, rows_per_launch: int = 0, order: Optional[Sequence[int]] = None):
    """bnpp.expected_counts on device tensors -> (counts float64[counts_size], log10_z float64[n], n_impossible, a
    0-dim int64 tensor), all on the device.  tables: a Tables of this model to read instead of its own values
    (dtype then defaults to theirs).  weights: a float64 tensor of n entries.  accumulate=True adds to `out`,
    the counts of an earlier call, continuing its fold; else out (if given) is overwritten."""
    c, lz, _, ni = _counts_call(ctx, model, ev_vars, rows, weights, tables, partial, soft, log_soft, accumulate, out,
                                heuristic, dtype, rows_per_launch, order, True, False)
    return c, lz, ni


def m_step(ctx: Context, model: Model, counts, old_values, prior: float = 0.0, out=None):
    """The M step of a BAYES model on device tensors (bnpp_mstep_dv; learn.m_step with a fixed summation order):
    new = (counts + prior) / its sum over the child, a parent configuration whose sum is 0 keeping its old row.
    counts, old_values: flat float64 tensors; out: the tensor to write (it may be old_values), else a new one."""
    n = _counts_size(model)
    c = _flat(ctx, counts, n, "counts", (torch.float64,))
    old = _flat(ctx, old_values, n, "old_values", (torch.float64,))
    new = _out(ctx, out, (n,), torch.float64, "out")
    _enter(ctx)
    _check(_lib.bnpp_mstep_dv(_h(ctx), None, model.handle, _ptr(c), float(prior), _ptr(old), _ptr(new)), "bnpp_mstep_dv")
    _leave(ctx)
    return new


def em(ctx: Context, model: Model, ev_vars: Sequence[int], rows, iters: int, weights=None, prior: float = 0.0,
       tables: Optional[Tables] = None, partial=None, soft=None, dtype: int = F64):
    """learn.em's loop on the device -> (tables, lls): every iteration is expected_counts(tables=...), m_step and
    tables.set, with no new Model, no plan after the first and no copy to the host; lls[i] is the weighted
    log-likelihood in log10 of the tables iteration i started from, impossible rows left out.  tables: the set to
    start from and to refit (linear form), else a new one holding the model's own values."""
    t = tables if tables is not None else Tables(ctx, model, dtype)
    if t.log:
        raise ValueError("em refits linear tables; these were last set in log form")
    w = None if weights is None else _flat(ctx, weights, rows.shape[0], "weights", (torch.float64,))
    lls = []
    for _ in range(int(iters)):
        counts, lz, _ = expected_counts(ctx, model, ev_vars, rows, weights=w, tables=t, partial=partial, soft=soft)
        ok = torch.isfinite(lz)
        lls.append(torch.sum((lz if w is None else w * torch.where(ok, lz, torch.zeros_like(lz)))[ok]))
        t.set(m_step(ctx, model, counts, t.values.detach().reshape(-1).double(), prior))
    return t, (torch.stack(lls).tolist() if lls else [])


class _LogLikelihood(torch.autograd.Function):
    """ll = sum_b w_b ln Z_b under the tables exp(log_tables); d ll / d log theta_f(x) = N_f(x), the expected counts
    the same bucket-tree pass accumulates (bnpp_expected_counts_dv on log-form tables)."""

    _tables = {}                                            # (context, model, dtype) -> Tables, the few last used

    @classmethod
    def tables_for(cls, ctx: Context, model: Model, dtype: int) -> Tables:
        key = (id(ctx), id(model), dtype)
        t = cls._tables.pop(key, None)                      # a Tables keeps both alive, so the ids stay theirs
        if t is None:
            t = Tables(ctx, model, dtype)
        cls._tables[key] = t
        while len(cls._tables) > 4:
            cls._tables.pop(next(iter(cls._tables)))
        return t

    @staticmethod
    def forward(fctx, log_tables, need, ctx, model, ev_vars, rows, weights, tables, partial, log_soft, heuristic,
                rows_per_launch, order):
        tables.set(log_tables.detach(), log=True)
        counts, _, ln_z, ni = _counts_call(ctx, model, ev_vars, rows, weights, tables, partial, None, log_soft, False, None,
                                           heuristic, None, rows_per_launch, order, need, True)
        ok = torch.isfinite(ln_z)
        terms = ln_z if weights is None else weights.detach().reshape(-1).double() * ln_z
        ll = torch.sum(torch.where(ok, terms, torch.zeros_like(ln_z)))
        if need:
            fctx.save_for_backward(counts)
        fctx.shape, fctx.dtype = tuple(log_tables.shape), log_tables.dtype
        fctx.mark_non_differentiable(ln_z, ni)
        return ll, ln_z, ni

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, g_ll, g_ln, g_ni):
        (counts,) = fctx.saved_tensors
        return ((g_ll.double() * counts).to(fctx.dtype).reshape(fctx.shape),) + (None,) * 12


def log_likelihood(ctx: Context, model: Model, ev_vars: Sequence[int], rows, log_tables, weights=None,
                   tables: Optional[Tables] = None, partial=None, log_soft=None, heuristic: str = "mf",
                   dtype: Optional[int] = None, rows_per_launch: int = 0, order: Optional[Sequence[int]] = None):
    """The weighted log-likelihood of the rows under the tables exp(log_tables) -> (ll, ln_z, n_impossible):
    ll = sum_b w_b ln Z_b over the rows with a finite ln Z_b, a 0-dim float64 tensor differentiable with respect
    to log_tables (one flat tensor of natural logs in the layout of counts); its gradient is the expected counts
    of the rows, which the same pass returns.  ln_z float64[n] and n_impossible are not differentiable.  Where
    log_tables requires no gradient (or grad mode is off) the call runs the batch plan, without the backward
    pass.  tables: the Tables to stage log_tables in (else one kept per context, model and dtype); dtype then
    defaults to theirs, and another one is a ValueError.  weights are not differentiated (that gradient is ln_z
    itself): weights that require grad are a ValueError.  The tables are not normalised: for CPTs, pass log_softmax over the child.  No double backward."""
    if log_soft is not None and isinstance(log_soft, (tuple, list)) and len(log_soft) == 2 and \
            isinstance(log_soft[1], torch.Tensor) and log_soft[1].requires_grad and torch.is_grad_enabled():
        raise ValueError("log_likelihood has no gradient with respect to log_soft (the counts job does not produce the "
                         "rows' posteriors): use log_partition for the soft evidence's gradient")
    if isinstance(weights, torch.Tensor) and weights.requires_grad and torch.is_grad_enabled():
        raise ValueError("log_likelihood has no gradient with respect to weights: it is ln_z, which the call returns "
                         "(detach the weights, or weigh ln_z in torch)")
    if not isinstance(log_tables, torch.Tensor):
        raise ValueError("log_tables must be a torch tensor on the context's device")
    if tables is None:
        tables = _LogLikelihood.tables_for(ctx, model, F64 if dtype is None else dtype)
    elif not isinstance(tables, Tables):
        raise ValueError("tables must be a bnpp.tensor.Tables")
    elif dtype is not None and tables.dtype != dtype:
        raise ValueError("tables are of dtype %d, the call asks for %d" % (tables.dtype, dtype))
    need = log_tables.requires_grad and torch.is_grad_enabled()
    return _LogLikelihood.apply(log_tables, need, ctx, model, ev_vars, rows, weights, tables, partial, log_soft, heuristic,
                                int(rows_per_launch), order)
