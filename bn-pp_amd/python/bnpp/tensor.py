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
