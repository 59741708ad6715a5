"""roll: rolling-window statistics of a series or a panel, alone and against a second panel or
one shared factor (include/sts_roll.h r1 / r2).

roll(ts, op, window, minPeriods=None, other=None) is ONE batched C-ABI call.  ts is a series (T,) or
a panel (S, T); the result has ts's shape and kind, and out[s, t] belongs to the trailing window
[max(0, t - window + 1), t].  op is "sum", "mean", "var", "std", "min", "max" or "zscore" without
`other`, and "cov", "corr" or "beta" (the slope of ts on other) with it; `other` is a panel of ts's
shape and kind or one factor (T,) that every series shares.  minPeriods=None means `window`: fewer
valid (non-NaN) steps in a window give NaN.  Torch GPU tensors take the device path on torch's
current stream, numpy arrays the `_host` path.

Every window is evaluated directly in the header's order, so an output depends on its own window
alone, bit for bit; the numbers are held to exact arithmetic at level 1e9 and on data scaled by
2^400 or 2^-400, where the difference of two cumulative sums returns noise.
"""
from __future__ import annotations

from . import _native
from ._panel import Panel, check, is_torch, ptr
from .errors import IllegalArgumentException

__all__ = ["roll"]


def _panel(v, name, what):
    try:
        return Panel(v, name)
    except (TypeError, ValueError) as e:
        raise IllegalArgumentException("%s: %s" % (what, e))


def _code(fn, op, what):
    c = getattr(_native.lib(), fn)(op.encode() if isinstance(op, str) else op)
    if c < 0:
        raise IllegalArgumentException("roll: op %r is not one of %s" % (op, what))
    return c


def roll(ts, op: str, window: int, minPeriods=None, other=None):
    """The rolling `op` over windows of `window` steps; see the module's text."""
    window = int(window)
    mp = window if minPeriods is None else int(minPeriods)
    what = "roll(%s)" % (op,)
    p = _panel(ts, "ts", what)
    lib = _native.lib()
    if p.S < 1 or p.T < 1:
        raise IllegalArgumentException("%s: an empty %s" % (what, "series" if p.squeeze else "panel"))
    if other is None:
        code = _code("sts_roll_op_from_name", op, _native.ROLL_OPS)
        out = p.empty()
        if p.device:
            st = lib.sts_roll_stat(ptr(p.t), ptr(out), p.S, p.T, p.ld, p.T, window, mp, code, p.stream)
        else:
            st = lib.sts_roll_stat_host(ptr(p.t), ptr(out), p.S, p.T, p.ld, window, mp, code)
        check(st, what)
        return p.out(out)
    code = _code("sts_roll_pair_op_from_name", op, _native.ROLL_PAIR_OPS)
    if is_torch(other) != p.device:
        raise IllegalArgumentException("%s: other must be of ts's kind (numpy with numpy, torch with torch)" % what)
    q = _panel(other, "other", what)
    if p.device and q.t.device != p.t.device:
        raise IllegalArgumentException("%s: other on %s, ts on %s" % (what, q.t.device, p.t.device))
    if q.T != p.T or not (q.S == p.S or q.squeeze):
        raise IllegalArgumentException("%s: other must be a (T,) factor or of ts's shape (%d, %d), got (%d, %d)"
                                       % (what, p.S, p.T, q.S, q.T))
    Sy = 1 if q.squeeze else q.S
    out = p.empty()
    if p.device:
        st = lib.sts_roll_pair(ptr(p.t), ptr(q.t), Sy, q.ld, ptr(out), p.S, p.T, p.ld, p.T, window, mp, code, p.stream)
    else:
        st = lib.sts_roll_pair_host(ptr(p.t), ptr(q.t), Sy, q.ld, ptr(out), p.S, p.T, p.ld, window, mp, code)
    check(st, what)
    return p.out(out)
