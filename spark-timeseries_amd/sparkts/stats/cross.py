"""cov and corr: the covariance and correlation matrices of a panel, or of two panels
(include/sts_cross.h c1).

The reference hands this step to MLlib (toRowMatrix().computeCovariance(), Statistics.corr on the
instants); here it is ONE batched C-ABI call on the series-major panel.  x is a panel (Sx, T) (a
single series (T,) is a panel of one); without y the result is the symmetric (Sx, Sx) matrix, with a
panel y (Sy, T) of x's kind it is (Sx, Sy): series i of x against series j of y.  Torch GPU tensors
take the device path on torch's current stream, numpy arrays the `_host` path, and the result is of
the input's kind.  Wrong shapes and kinds raise IllegalArgumentException before any native call.

The numbers are the corrected two-pass form, held to exact arithmetic, not MLlib's one-pass
(X'X - n m m') / (n - 1).  A series with a non-finite value has NaN in its row (and
column); a bit-constant series has covariance +0.0 and correlation NaN; the diagonal of corr(x) is
exactly 1.0 otherwise.  Every entry depends on its two series and T alone, bit for bit.
"""
from __future__ import annotations

from .. import _native
from .._panel import Panel, check, is_torch, ptr
from ..errors import IllegalArgumentException, MathIllegalArgumentException

__all__ = ["cov", "corr", "cross_moments"]


def _panel(v, name, what):
    try:
        return Panel(v, name)
    except (TypeError, ValueError) as e:
        raise IllegalArgumentException("%s: %s" % (what, e))


def cross_moments(x, y=None, kind: str = "cov"):
    """The matrix of `kind` ("cov" / "corr")."""
    code = _native.lib().sts_cross_kind_from_name(kind.encode() if isinstance(kind, str) else kind)
    if code < 0:
        raise IllegalArgumentException("cross_moments: kind %r is not cov or corr" % (kind,))
    px = _panel(x, "x", kind)
    py = None
    if y is not None:
        if is_torch(y) != px.device:
            raise IllegalArgumentException("%s: y must be of x's kind (numpy with numpy, torch with torch)" % kind)
        py = _panel(y, "y", kind)
        if px.device and py.t.device != px.t.device:
            raise IllegalArgumentException("%s: y on %s, x on %s" % (kind, py.t.device, px.t.device))
        if py.T != px.T:
            raise IllegalArgumentException("%s: y has %d instants, x has %d" % (kind, py.T, px.T))
        if py.S < 1:
            raise IllegalArgumentException("%s: y has no series" % kind)
    if px.S < 1:
        raise IllegalArgumentException("%s: x has no series" % kind)
    if px.T < 2:
        raise MathIllegalArgumentException("%s: %d instants, a covariance needs 2" % (kind, px.T))
    cols = px.S if py is None else py.S
    out = px.empty(S=px.S, T=cols)
    lib = _native.lib()
    yt, ys, yld = (None, 0, 0) if py is None else (ptr(py.t), py.S, py.ld)
    if px.device:
        st = lib.sts_cross_moments(ptr(px.t), px.S, px.T, px.ld, yt, ys, yld, code, ptr(out), cols, None, None,
                                   px.stream)
    else:
        st = lib.sts_cross_moments_host(ptr(px.t), px.S, px.T, px.ld, yt, ys, yld, code, ptr(out), None, None)
    check(st, kind)
    return out


def cov(x, y=None):
    """Sample covariance (divisor T - 1): (Sx, Sx), or (Sx, Sy) against the panel y."""
    return cross_moments(x, y, "cov")


def corr(x, y=None):
    """Pearson correlation, clamped to [-1, 1]: (Sx, Sx), or (Sx, Sy) against the panel y."""
    return cross_moments(x, y, "corr")
