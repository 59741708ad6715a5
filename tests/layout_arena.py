"""Layout arenas for the panel-layout contract of include/sts.h ("Panel layout").

An arena is one flat float64 allocation that holds a series-contiguous panel somewhere in its
middle:

    [ red zone | skew (base_off) | S x ld panel | red zone ]
      red        base_off          S * ld         red          doubles

The start of the skew is 128-B aligned, so `base_off` is the panel's offset (in doubles) inside
a 128-B line.  Everything outside the elements (s, t < T) -- red zones, skew, row padding, the
last row's padding included -- holds a poison value.  The red zones keep a stray access of up
to a halo's width inside the allocation: a layout error shows as a failed assertion, not as a
device fault.

snapshot() / verify_outside() / verify_all() compare BITS (uint64), so a NaN poison with
another payload, or -0.0 for 0.0, counts as a change:

    verify_outside(snap)   an OUTPUT arena: nothing outside (s, t < T) changed
    verify_all(snap)       an INPUT arena: nothing changed at all (inputs are const)

carve() builds a device arena (torch), carve_np() its numpy twin for the `_host` entry points
(optionally inside caller-provided memory, e.g. pinned memory from sts_host_alloc).  This is a
plain module: numpy only, torch is imported by carve() alone.
"""
import numpy as np

LINE = 16                 # doubles per 128-B line
RED = 512                 # default red zone, doubles (a multiple of LINE)

# Every case runs with both poisons.  NaN catches a pad step that reaches a sum, a count or a
# min / max; the finite sentinel catches a pad value that a fill would fill over and a halo leak
# into a filled value.  Output arenas are pre-filled with OUT_FILL, distinct from both.
POISONS = {"nan": float("nan"), "sentinel": 7.0e77}
OUT_FILL = -3.0e55

# name -> (ld_in - T, ld_out - T, base_in, base_out); bases in doubles from a 128-B aligned start
LAYOUTS = {
    "packed": (0, 0, 0, 0),              # control: must pass at the same bar
    "even": (2, 4, 0, 0),                # fast forms with ld != T
    "odd": (1, 3, 0, 0),                 # rows alternate 16-B aligned and misaligned
    "in_fast_out_slow": (2, 2, 0, 1),    # aligned loads, misaligned stores
    "in_slow_out_fast": (2, 2, 1, 0),    # the converse
    "skew": (5, 7, 5, 15),               # rows start at varied offsets inside a 128-B line
}
LAYOUT_NAMES = list(LAYOUTS)


def layout(name, T, T_out=None):
    """(ld_in, ld_out, base_in, base_out) of a named layout for rows of T (out: T_out) steps."""
    pi, po, bi, bo = LAYOUTS[name]
    return T + pi, (T if T_out is None else T_out) + po, bi, bo


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Arena:
    """flat: the whole allocation (1-D, numpy array or torch tensor); view: its (S, T) window
    (strides (ld, 1)); ptr: address of element (0, 0); off: index of element (0, 0) in flat."""

    def __init__(self, flat, S, T, ld, base_off, red, device):
        self.flat, self.S, self.T, self.ld, self.base_off, self.red = flat, S, T, ld, base_off, red
        self.device = device
        self.off = red + base_off
        n = S * ld
        if device:
            self.view = flat[self.off:self.off + n].view(S, ld)[:, :T]
            self.ptr = flat.data_ptr() + 8 * self.off
        else:
            self.view = flat[self.off:self.off + n].reshape(S, ld)[:, :T]
            self.ptr = flat.ctypes.data + 8 * self.off
        assert (self.ptr - 8 * base_off) % 128 == 0

    # ---- contents ----
    def host(self):
        """The whole allocation as a host numpy array (a copy)."""
        if self.device:
            return self.flat.detach().cpu().numpy().copy()
        return self.flat.copy()

    def data(self):
        """The (S, T) elements as a contiguous host array."""
        h = self.host()
        return np.ascontiguousarray(h[self.off:self.off + self.S * self.ld].reshape(self.S, self.ld)[:, :self.T])

    def inside_mask(self):
        m = np.zeros(self.flat.shape[0], dtype=bool)
        m[self.off:self.off + self.S * self.ld].reshape(self.S, self.ld)[:, :self.T] = True
        return m

    # ---- snapshot / verify ----
    def snapshot(self):
        return bits(self.host())

    def _report(self, bad, what):
        i = int(np.flatnonzero(bad)[0])
        n = self.S * self.ld
        if i < self.red:
            where = "front red zone, %d doubles before the skew" % (self.red - i)
        elif i < self.off:
            where = "skew, %d doubles before element (0, 0)" % (self.off - i)
        elif i < self.off + n:
            s, t = divmod(i - self.off, self.ld)
            where = ("row %d padding, column %d (T=%d, ld=%d)" if t >= self.T else "element (%d, %d) (T=%d, ld=%d)") % (
                s, t, self.T, self.ld)
        else:
            where = "back red zone, %d doubles after the panel" % (i - self.off - n)
        raise AssertionError("%s: %d doubles changed, first in the %s" % (what, int(bad.sum()), where))

    def verify_outside(self, snap, what="output arena"):
        """Every element outside (s, t < T) is bit-identical to the snapshot."""
        bad = (self.snapshot() != snap) & ~self.inside_mask()
        if bad.any():
            self._report(bad, what)

    def verify_all(self, snap, what="input arena"):
        """The whole allocation is bit-identical to the snapshot."""
        bad = self.snapshot() != snap
        if bad.any():
            self._report(bad, what)


def _aligned_window(addr, total):
    """First index of a float64 buffer at `addr` whose address is 128-B aligned."""
    assert addr % 8 == 0
    return ((-addr) % 128) // 8


def _size(S, T, ld, base_off, red):
    assert S >= 0 and 0 <= T <= ld and base_off >= 0 and red >= 0 and red % LINE == 0
    return red + base_off + S * ld + red


def carve_np(S, T, ld, base_off, poison, red=RED, data=None, raw=None):
    """numpy arena.  data: optional (S, T) values for the panel elements (else they hold the
    poison too).  raw: optional 1-D float64 array to carve from (needs LINE spare doubles)."""
    n = _size(S, T, ld, base_off, red)
    if raw is None:
        raw = np.empty(n + LINE, dtype=np.float64)
    assert raw.dtype == np.float64 and raw.ndim == 1 and raw.size >= n + LINE
    lead = _aligned_window(raw.ctypes.data, n)
    flat = raw[lead:lead + n]
    flat[:] = poison
    a = Arena(flat, S, T, ld, base_off, red, device=False)
    if data is not None:
        a.view[...] = data
    return a


def carve(S, T, ld, base_off, poison, red=RED, data=None, device="cuda:0"):
    """Device arena (torch).  data: optional (S, T) host values for the panel elements."""
    import torch
    n = _size(S, T, ld, base_off, red)
    raw = torch.empty(n + LINE, dtype=torch.float64, device=device)
    lead = _aligned_window(raw.data_ptr(), n)
    flat = raw[lead:lead + n]
    flat.fill_(poison)
    a = Arena(flat, S, T, ld, base_off, red, device=True)
    if data is not None:
        a.view.copy_(torch.as_tensor(np.ascontiguousarray(data, dtype=np.float64)))
    return a
