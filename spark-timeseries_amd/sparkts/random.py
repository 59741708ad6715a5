"""The generator the models' sample(n, rand) draws from (include/sts_sample.h).

The reference hands `sample` a commons-math3 RandomGenerator and calls nextGaussian() n times.
Here `rand` is a PhiloxGenerator: a seed, the global index of the first series and a position.
Draw t of series g under a seed is a pure function z(seed, g, t) (csrc/sts_normal.hpp), so a
path can be regenerated on any rank from (seed, first_series + j, position); the generator
object only does the bookkeeping a stateful RandomGenerator does implicitly: every sample call
draws at t0 = position and then advances position by n, so two consecutive calls give
independent paths.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native
from ._panel import check, is_torch, ptr
from .errors import IllegalArgumentException


class PhiloxGenerator:
    """PhiloxGenerator(seed, first_series=0): seed in [0, 2^64); series j of a call uses the stream
    of global series first_series + j; `position` is the next unread draw of every stream."""

    def __init__(self, seed, first_series: int = 0):
        seed, first_series = int(seed), int(first_series)
        if not 0 <= seed < 2 ** 64:
            raise IllegalArgumentException("PhiloxGenerator: seed %d outside [0, 2^64)" % seed)
        if first_series < 0:
            raise IllegalArgumentException("PhiloxGenerator: negative first_series %d" % first_series)
        self.seed, self.first_series, self.position = seed, first_series, 0

    def take(self, n: int) -> int:
        """reserve n draws of every stream: -> the position of the first, position += n"""
        n = int(n)
        if n < 0:
            raise IllegalArgumentException("PhiloxGenerator: cannot draw %d values" % n)
        t0 = self.position
        self.position = t0 + n
        return t0

    def normal(self, S: int, n: int, device=None):
        """the raw panel: (S, n) standard normals on the device, row j from stream first_series + j"""
        dev = resolve_device([], device)
        out = new_panel(S, n, dev)
        t0 = self.take(n)
        check(_native.lib().sts_sample_normal(ptr(out), self.first_series, S, n, n, t0, ctypes.c_uint64(self.seed),
                                              current_stream(dev)), "PhiloxGenerator.normal")
        return out

    def __repr__(self):
        return "PhiloxGenerator(seed=%d, first_series=%d, position=%d)" % (self.seed, self.first_series, self.position)


def require_generator(rand, what):
    if not isinstance(rand, PhiloxGenerator):
        raise TypeError("%s: rand must be a sparkts.random.PhiloxGenerator (the device draws from its counter-based "
                        "stream, not from a host RandomGenerator), got %s" % (what, type(rand).__name__))
    return rand


def _shape(v):
    return tuple(v.shape) if is_torch(v) else np.shape(v)


def path_count(params, paths, what):
    """The shape rule of sample(n, rand, paths).  params: (value, name, ndim of ONE series' value)
    -> (S, squeeze): scalar parameters give one path (n,), or `paths` paths of the same model
    (paths, n); per-series parameters give one path per series (S, n) and take no `paths`."""
    per_series = {}
    for value, name, base in params:
        shp = _shape(value)
        if len(shp) == base + 1:
            per_series[name] = shp[0]
        elif len(shp) != base:
            raise ValueError("%s: %s has shape %s" % (what, name, shp))
    if per_series:
        if len(set(per_series.values())) != 1:
            raise ValueError("%s: per-series parameters disagree on the number of series: %s" % (what, per_series))
        if paths is not None:
            raise ValueError("%s: paths is for a model with scalar parameters; %s hold one value per series"
                             % (what, sorted(per_series)))
        return next(iter(per_series.values())), False
    if paths is None:
        return 1, True
    paths = int(paths)
    if paths < 0:
        raise ValueError("%s: negative paths" % what)
    return paths, False


def resolve_device(values, device):
    """the device of the first device-resident parameter, else `device`, else torch's current one"""
    import torch
    dev = None
    if device is not None:
        dev = torch.device(device)
    else:
        for v in values:
            if is_torch(v) and v.device.type == "cuda":
                dev = v.device
                break
    if dev is None or dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise TypeError("samples are made on the GPU (there is no CPU path), got device %s" % dev)
    _native.ensure_device(dev.index)
    return dev


def new_panel(S, n, dev):
    import torch
    if S < 0 or n < 0:
        raise IllegalArgumentException("sample: negative shape (%d, %d)" % (S, n))
    return torch.empty((S, n), dtype=torch.float64, device=dev)


def current_stream(dev):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def per_series(value, S, width, dev):
    """(S,) or (S, width) contiguous device tensor from one series' value or one row per series"""
    import torch
    if is_torch(value):
        v = value.detach().to(device=dev, dtype=torch.float64)
    else:
        v = torch.as_tensor(np.asarray(value, dtype=np.float64), device=dev)
    shape = (S,) if width is None else (S, width)
    return v.expand(shape).contiguous()


def run_sample(what, n, rand, paths, params, device, call):
    """params: (value, name, ndim of one series' value, row width or None); call(out, S, vectors, t0, stream)
    -> status.  Returns (n,), (paths, n) or (S, n) on the device."""
    rand = require_generator(rand, what)
    S, squeeze = path_count([p[:3] for p in params], paths, what)
    dev = resolve_device([p[0] for p in params], device)
    out = new_panel(S, int(n), dev)
    vecs = [per_series(v, S, width, dev) for v, _, _, width in params]
    t0 = rand.take(n)
    check(call(out, S, vecs, t0, current_stream(dev)), what)
    return out[0] if squeeze else out
