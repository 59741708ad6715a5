"""Host mirror of com.cloudera.sparkts.DateTimeIndex and Frequency (S/DateTimeIndex.scala,
S/Frequency.scala), the index semantics of include/sts_index.h.

Everything is UTC and integer milliseconds since the epoch: the reference builds every DateTime it
compares in UTC, where Joda's calendar arithmetic is int64 arithmetic with Java's truncating
division.  A date-time argument may be an int (ms since the epoch), a numpy.datetime64, a
datetime.datetime (naive means UTC) or an ISO string ("2015-04-10", "2015-4-10",
"2015-04-10T09:30:00.000Z"); methods that return a date-time return int ms.  No pandas.

Deviations from the reference, as stated in the header: an irregular index with duplicates returns
the FIRST location of an instant; IrregularDateTimeIndex.slice with absent bounds returns the
instants inside [start, end] (the reference runs an unclamped negative Array.slice); fromString also
reads "hours n", which the reference writes but cannot read; locAtDateTime gives -1 where the
reference's scalar code throws (a weekend earlier than a business-day first).

Lookups of many timestamps: locsAtDateTimes(millis) with a device tensor runs sts_index_locs on the
device; with a host array it runs the numpy restatement below.
"""
from __future__ import annotations

import datetime as _dt
import re

import numpy as np

from . import _native
from .errors import IllegalArgumentException

D = 86400000
H = 3600000
_EPOCH_ORDINAL = 719163   # date(1970, 1, 1).toordinal()

__all__ = ["DayFrequency", "HourFrequency", "BusinessDayFrequency", "DateTimeIndex", "UniformDateTimeIndex",
           "IrregularDateTimeIndex", "uniform", "irregular", "fromString", "nextBusinessDay", "to_millis", "to_iso"]

_ISO = re.compile(r"^(-?\d{1,9})-(\d{1,2})-(\d{1,2})(?:T(\d{1,2})(?::(\d{1,2})(?::(\d{1,2})(?:[.,](\d{1,9}))?)?)?)?"
                  r"(Z|[+-]\d{2}(?::?\d{2})?)?$")


def to_millis(dt) -> int:
    """A date-time argument -> int ms since the epoch, UTC."""
    if isinstance(dt, (bool, np.bool_)):
        raise TypeError("not a date-time: %r" % (dt,))
    if isinstance(dt, (int, np.integer)):
        return int(dt)
    if isinstance(dt, np.datetime64):
        return int(dt.astype("datetime64[ms]").astype(np.int64))
    if isinstance(dt, _dt.datetime):
        if dt.tzinfo is not None:
            dt = dt.astimezone(_dt.timezone.utc).replace(tzinfo=None)
        return ((dt.toordinal() - _EPOCH_ORDINAL) * D + dt.hour * H + dt.minute * 60000 + dt.second * 1000
                + dt.microsecond // 1000)
    if isinstance(dt, _dt.date):
        return (dt.toordinal() - _EPOCH_ORDINAL) * D
    if isinstance(dt, str):
        m = _ISO.match(dt.strip())
        if not m:
            raise IllegalArgumentException("Invalid format: \"%s\"" % dt)
        y, mo, d, hh, mi, ss, frac, zone = m.groups()
        t = (_dt.date(int(y), int(mo), int(d)).toordinal() - _EPOCH_ORDINAL) * D
        t += int(hh or 0) * H + int(mi or 0) * 60000 + int(ss or 0) * 1000 + (int((frac + "00")[:3]) if frac else 0)
        if zone and zone != "Z":
            sign = -1 if zone[0] == "-" else 1
            digits = zone[1:].replace(":", "")
            t -= sign * (int(digits[:2]) * H + int(digits[2:4] or 0) * 60000)
        return t
    raise TypeError("not a date-time: %r" % (dt,))


def to_iso(ms: int) -> str:
    """Joda's DateTime(ms, UTC).toString: 2015-04-10T00:00:00.000Z."""
    days, rem = divmod(int(ms), D)
    d = _dt.date.fromordinal(days + _EPOCH_ORDINAL)
    return "%04d-%02d-%02dT%02d:%02d:%02d.%03dZ" % (d.year, d.month, d.day, rem // H, rem // 60000 % 60,
                                                    rem // 1000 % 60, rem % 1000)


def _millis_array(values) -> np.ndarray:
    """many date-times -> int64 ms (host)"""
    if isinstance(values, np.ndarray) and values.dtype.kind == "M":
        return values.astype("datetime64[ms]").astype(np.int64)
    if isinstance(values, np.ndarray) and values.dtype.kind in "iu":
        return values.astype(np.int64)
    return np.fromiter((to_millis(v) for v in values), dtype=np.int64, count=len(values))


def _tdiv(a, b):
    """Java's truncating division, element-wise on int64 (b > 0)"""
    a = np.asarray(a, dtype=np.int64)
    q = np.abs(a) // b
    return np.where(a < 0, -q, q)


def _dow(t):
    """Monday = 1 .. Sunday = 7"""
    return (np.floor_divide(t, D) + 3) % 7 + 1


class _Frequency:
    """A frequency for a uniform index: advance / difference on int ms (arrays allowed)."""
    kind = None      # the sts_index_kind
    name = None      # the reference's toString prefix
    unit = D

    def __init__(self, n: int):
        self.n = int(n)

    def __eq__(self, other):
        return type(other) is type(self) and other.n == self.n

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((self.name, self.n))

    def __str__(self):
        return "%s %d" % (self.name, self.n)

    __repr__ = __str__

    def advance(self, dt, k):
        """dt advanced by this frequency k times (S/Frequency.scala:43)."""
        return _scalar(np.asarray(to_millis(dt) if not isinstance(dt, np.ndarray) else dt, dtype=np.int64)
                       + np.asarray(k, dtype=np.int64) * (self.n * self.unit))

    def difference(self, dt1, dt2):
        """How often this frequency occurs between the two, rounded toward zero (:55, :62)."""
        a = dt1 if isinstance(dt1, np.ndarray) else to_millis(dt1)
        b = dt2 if isinstance(dt2, np.ndarray) else to_millis(dt2)
        return _scalar(_tdiv(_tdiv(np.asarray(b, dtype=np.int64) - a, self.unit), self.n))


def _scalar(a):
    a = np.asarray(a)
    return int(a) if a.ndim == 0 else a


class DayFrequency(_Frequency):
    kind, name, unit = _native.INDEX_DAYS, "days", D

    def days(self):
        return self.n


class HourFrequency(_Frequency):
    kind, name, unit = _native.INDEX_HOURS, "hours", H

    def hours(self):
        return self.n


class BusinessDayFrequency(_Frequency):
    """S/Frequency.scala:67-106: weekends are skipped; advance from a weekend, and difference whose
    earlier argument is a weekend, raise IllegalArgumentException."""
    kind, name, unit = _native.INDEX_BUSINESS_DAYS, "businessDays", D

    def days(self):
        return self.n

    def advance(self, dt, k):
        t = np.asarray(dt if isinstance(dt, np.ndarray) else to_millis(dt), dtype=np.int64)
        dow = _dow(t)
        if np.any(dow > 5):
            raise IllegalArgumentException("%s is not a business day" % to_iso(int(np.asarray(t)[np.asarray(dow > 5)].flat[0])
                                                                               if t.ndim else int(t)))
        total = np.asarray(k, dtype=np.int64) * self.n
        weeks = _tdiv(total, 5)
        extra = np.where(dow + (total - weeks * 5) > 5, 2, 0)
        return _scalar(t + (total + weeks * 2 + extra) * D)

    def difference(self, dt1, dt2):
        a = np.asarray(dt1 if isinstance(dt1, np.ndarray) else to_millis(dt1), dtype=np.int64)
        b = np.asarray(dt2 if isinstance(dt2, np.ndarray) else to_millis(dt2), dtype=np.int64)
        a, b = np.broadcast_arrays(a, b)
        flip = b < a
        lo, hi = np.where(flip, b, a), np.where(flip, a, b)
        dow = _dow(lo)
        if np.any(dow > 5):
            raise IllegalArgumentException("%s is not a business day" % to_iso(int(lo[dow > 5].flat[0]) if lo.ndim else int(lo)))
        between = _tdiv(hi - lo, D)
        weeks = _tdiv(between, 7)
        extra = np.where(dow + (between - weeks * 7) > 5, 2, 0)
        q = _tdiv(between - weeks * 2 - extra, self.n)
        return _scalar(np.where(flip, -q, q))


class DateTimeIndex:
    """The duck-typing TimeSeriesRDD relies on: len(index); index[a:b] with integer bounds is islice,
    with date-time bounds the date slice (both ends inclusive); index[int array] is the irregular
    index of those instants; index[date-time] is locAtDateTime; integers in [] are always locations
    (index[i] is dateTimeAtLoc(i)); np.asarray(index) is int64 ms; str(index) is the reference's
    toString."""

    def __len__(self):
        return self.size()

    def __array__(self, dtype=None, copy=None):
        a = self.toMillisArray()
        return a if dtype is None else a.astype(dtype)

    def __ne__(self, other):
        return not self == other

    def __repr__(self):
        return self.toString()

    __str__ = __repr__

    def __getitem__(self, key):
        if isinstance(key, slice):
            if key.step is not None:
                raise IllegalArgumentException("a DateTimeIndex slice takes no step")
            ints = [b is None or isinstance(b, (int, np.integer)) for b in (key.start, key.stop)]
            if all(ints):
                lo, hi, _ = key.indices(self.size())
                return self.islice(lo, max(lo, hi))
            start = self.first() if key.start is None else to_millis(key.start)
            stop = self.last() if key.stop is None else to_millis(key.stop)
            return self.slice(start, stop)
        if isinstance(key, (int, np.integer)) and not isinstance(key, (bool, np.bool_)):
            return self.dateTimeAtLoc(int(key) + (self.size() if key < 0 else 0))
        if isinstance(key, (list, tuple, np.ndarray)) or hasattr(key, "cpu"):
            locs = np.asarray(key.cpu().numpy() if hasattr(key, "cpu") else key)
            if locs.dtype == np.bool_:
                locs = np.flatnonzero(locs)
            if locs.size and locs.dtype.kind not in "iu":
                raise TypeError("locations must be integers")
            return IrregularDateTimeIndex(self.toMillisArray()[locs.astype(np.int64)])
        return self.locAtDateTime(key)

    def locsAtDateTimes(self, millis):
        """locAtDateTime of many timestamps (int64 ms).  A device tensor is looked up on the device
        (sts_index_locs, on torch's current stream) and a device tensor comes back; anything else on
        the host."""
        from ._panel import check, is_torch, ptr
        if is_torch(millis) and millis.device.type == "cuda":
            import ctypes
            import torch
            if millis.dtype != torch.int64:
                raise TypeError("timestamps: expected int64 ms, got %s" % millis.dtype)
            m = millis.contiguous().reshape(-1)
            _native.ensure_device(m.device.index if m.device.index is not None else torch.cuda.current_device())
            loc = torch.empty_like(m)
            inst = self._device_instants(m.device)
            st = ctypes.c_void_p(torch.cuda.current_stream(m.device).cuda_stream)
            check(_native.lib().sts_index_locs(ptr(m), m.numel(), *self._c_args(inst), ptr(loc), st), "locAtDateTime")
            return loc.reshape(millis.shape)
        a = np.asarray(millis.cpu().numpy() if is_torch(millis) else millis)
        if a.dtype.kind != "i":
            a = _millis_array(a.reshape(-1)).reshape(a.shape)
        return self._host_locs(a.astype(np.int64))

    # the index as the C ABI takes it: kind, start_ms, periods, step, instants, n_instants
    def _device_instants(self, device):
        return None

    def _c_args(self, inst=None):
        raise NotImplementedError


class UniformDateTimeIndex(DateTimeIndex):
    """S/DateTimeIndex.scala:112-174: date-times at regular intervals, constant space."""

    def __init__(self, start, periods: int, frequency: _Frequency):
        if not isinstance(frequency, _Frequency):
            raise TypeError("frequency: expected a DayFrequency, HourFrequency or BusinessDayFrequency")
        self.start = to_millis(start)
        self.periods = int(periods)
        self.frequency = frequency

    def first(self) -> int:
        return self.start

    def last(self) -> int:
        return self.frequency.advance(self.start, self.periods - 1)

    def size(self) -> int:
        return self.periods

    def dateTimeAtLoc(self, loc: int) -> int:
        return self.frequency.advance(self.start, int(loc))

    def locAtDateTime(self, dt) -> int:
        return int(self._host_locs(np.array([to_millis(dt)], dtype=np.int64))[0])

    def _host_locs(self, t):
        f = self.frequency
        t = np.asarray(t, dtype=np.int64)
        out = np.full(t.shape, -1, dtype=np.int64)
        if self.periods <= 0 or t.size == 0:
            return out
        ok = (t >= self.start) & (t <= self.last())   # outside: absent, or the reference throws
        if isinstance(f, BusinessDayFrequency):
            if _dow(np.int64(self.start)) > 5:
                return out
        tt = t[ok]
        loc = np.asarray(f.difference(np.full(tt.shape, self.start, dtype=np.int64), tt), dtype=np.int64)
        loc_c = np.clip(loc, 0, self.periods - 1)
        hit = (loc == loc_c) & (np.asarray(f.advance(np.full(tt.shape, self.start, dtype=np.int64), loc_c)) == tt)
        out[ok] = np.where(hit, loc, -1)
        return out

    def islice(self, lower: int, upper: int) -> "UniformDateTimeIndex":
        return UniformDateTimeIndex(self.frequency.advance(self.start, int(lower)), int(upper) - int(lower), self.frequency)

    def slice(self, start, end) -> "UniformDateTimeIndex":
        """uniform(start, difference(start, end) + 1, frequency): both ends inclusive (:125-127)."""
        s = to_millis(start)
        return UniformDateTimeIndex(s, self.frequency.difference(s, to_millis(end)) + 1, self.frequency)

    def toMillisArray(self) -> np.ndarray:
        if self.periods <= 0:
            return np.empty(0, dtype=np.int64)
        return np.asarray(self.frequency.advance(np.full(self.periods, self.start, dtype=np.int64),
                                                 np.arange(self.periods, dtype=np.int64)), dtype=np.int64)

    def toString(self) -> str:
        return ",".join(["uniform", to_iso(self.start), str(self.periods), str(self.frequency)])

    def __eq__(self, other):
        return (isinstance(other, UniformDateTimeIndex) and other.start == self.start and other.periods == self.periods
                and other.frequency == self.frequency)

    __hash__ = None

    def _c_args(self, inst=None):
        return (self.frequency.kind, self.start, self.periods, self.frequency.n, None, 0)


class IrregularDateTimeIndex(DateTimeIndex):
    """S/DateTimeIndex.scala:180-232: sorted (non-decreasing) instants, O(log n) lookups."""

    def __init__(self, instants):
        a = _millis_array(instants) if not (isinstance(instants, np.ndarray) and instants.dtype == np.int64) else instants
        a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
        if a.size > 1 and np.any(a[1:] < a[:-1]):
            raise IllegalArgumentException("an irregular index must be sorted")
        self.instants = a
        self._dev = {}

    def first(self) -> int:
        return int(self.instants[0])

    def last(self) -> int:
        return int(self.instants[-1])

    def size(self) -> int:
        return int(self.instants.size)

    def dateTimeAtLoc(self, loc: int) -> int:
        return int(self.instants[int(loc)])

    def locAtDateTime(self, dt) -> int:
        return int(self._host_locs(np.array([to_millis(dt)], dtype=np.int64))[0])

    def _host_locs(self, t):
        t = np.asarray(t, dtype=np.int64)
        pos = np.searchsorted(self.instants, t, side="left")
        inside = pos < self.instants.size
        hit = np.zeros(t.shape, dtype=bool)
        hit[inside] = self.instants[pos[inside]] == t[inside]
        return np.where(hit, pos, -pos - 1).astype(np.int64)

    def islice(self, start: int, end: int) -> "IrregularDateTimeIndex":
        return IrregularDateTimeIndex(self.instants[max(int(start), 0):max(int(end), 0)].copy())

    def slice(self, start, end) -> "IrregularDateTimeIndex":
        lo, hi = self._slice_locs(start, end)
        return IrregularDateTimeIndex(self.instants[lo:hi].copy())

    def _slice_locs(self, start, end):
        """[lo, hi): the instants in [start, end], lower bound of start and upper bound of end"""
        lo = int(np.searchsorted(self.instants, to_millis(start), side="left"))
        hi = int(np.searchsorted(self.instants, to_millis(end), side="right"))
        return lo, max(lo, hi)

    def toMillisArray(self) -> np.ndarray:
        return self.instants.copy()

    def toString(self) -> str:
        return ",".join(["irregular"] + [to_iso(t) for t in self.instants.tolist()])

    def __eq__(self, other):
        return isinstance(other, IrregularDateTimeIndex) and np.array_equal(other.instants, self.instants)

    __hash__ = None

    def _device_instants(self, device):
        """the instants on `device`, uploaded once per device"""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.as_tensor(self.instants, device=device)
        return self._dev[key]

    def _c_args(self, inst=None):
        from ._panel import ptr
        return (_native.INDEX_IRREGULAR, 0, 0, 1, ptr(inst) if self.instants.size else None, int(self.instants.size))


def uniform(start, end=None, periods=None, freq=None) -> UniformDateTimeIndex:
    """DateTimeIndex.uniform: a start and either an inclusive end or a number of periods."""
    if freq is None:
        raise ValueError("Missing frequency")
    if end is None and periods is None:
        raise ValueError("Need an end date or number of periods")
    if end is not None:
        s = to_millis(start)
        return UniformDateTimeIndex(s, freq.difference(s, to_millis(end)) + 1, freq)
    return UniformDateTimeIndex(start, periods, freq)


def irregular(instants) -> IrregularDateTimeIndex:
    """DateTimeIndex.irregular: the given date-times, sorted non-decreasing."""
    return IrregularDateTimeIndex(instants)


def nextBusinessDay(dt) -> int:
    """The next business day at or after dt (S/DateTimeIndex.scala:281-289)."""
    t = to_millis(dt)
    dow = int(_dow(np.int64(t)))
    return t + 2 * D if dow == 6 else (t + D if dow == 7 else t)


_FREQUENCIES = {"days": DayFrequency, "businessDays": BusinessDayFrequency, "hours": HourFrequency}


def fromString(text: str) -> DateTimeIndex:
    """Parse toString's output (S/DateTimeIndex.scala:303-325); also reads "hours n"."""
    tokens = text.strip().split(",")
    if tokens[0] == "uniform":
        name, _, n = tokens[3].partition(" ")
        if name not in _FREQUENCIES:
            raise IllegalArgumentException("Frequency %s not recognized" % name)
        return UniformDateTimeIndex(to_millis(tokens[1]), int(tokens[2]), _FREQUENCIES[name](int(n)))
    if tokens[0] == "irregular":
        return IrregularDateTimeIndex([to_millis(t) for t in tokens[1:]])
    raise IllegalArgumentException("DateTimeIndex type %s not recognized" % tokens[0])


def rebase_plan(source: DateTimeIndex, target: DateTimeIndex):
    """How to rebase a panel from `source` onto `target` (include/sts_index.h, "Rebase"):
    ("shift", start_loc) for two uniform indices, else ("map", int64 host array m) with m[j] the
    first location of target instant j in the source, negative where absent."""
    if isinstance(source, UniformDateTimeIndex) and isinstance(target, UniformDateTimeIndex):
        return "shift", uniform_start_loc(source, target)
    return "map", source._host_locs(target.toMillisArray())


def uniform_start_loc(source: UniformDateTimeIndex, target: UniformDateTimeIndex) -> int:
    """The location of target.first in source (negative: before it).  Unequal frequencies raise, as the
    reference's doc comment requires; so do firsts that are not on a common grid, where the reference
    silently floors."""
    f = source.frequency
    if f != target.frequency:
        raise IllegalArgumentException("rebase: frequencies differ (%s, %s)" % (f, target.frequency))
    early, late = (source.start, target.start) if target.start >= source.start else (target.start, source.start)
    loc = f.difference(early, late)
    if f.advance(early, loc) != late:
        raise IllegalArgumentException("rebase: %s and %s are not on a common %s grid" % (to_iso(source.start),
                                                                                        to_iso(target.start), f))
    return loc if target.start >= source.start else -loc
