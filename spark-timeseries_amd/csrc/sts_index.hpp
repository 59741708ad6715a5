// sts_index.hpp -- the date-time index arithmetic of include/sts_index.h, plain C++ for host and
// device (tests/native/index_harness.cpp compiles it for the host and tests/index_ref.py restates
// it; all three agree).  S/Frequency.scala and S/DateTimeIndex.scala in UTC: int64 milliseconds
// since the epoch and Java's truncating division.
//
// Division.  gfx950 has no 64-bit integer division: a quotient by a run-time divisor is a long
// software sequence.  Everything here divides by compile-time constants (D, H, 7, 5: a multiply-high
// and shifts) except the one division by the frequency's step, div_step(): its dividend is a count
// of days or hours, at most 2^63 / H < 2^42, exact as a double, so trunc((double)d * (1.0 / step)) is
// within one of the quotient and a remainder check makes it exact.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define STS_IX_HD __host__ __device__
#else
#define STS_IX_HD
#endif

namespace sts {
namespace ix {

constexpr int64_t kDay = 86400000;
constexpr int64_t kHour = 3600000;
constexpr int64_t kMaxInstant = (int64_t)1 << 62;   // |first|, |last| of a uniform index
// kinds: the values of sts_index_kind
constexpr int kDays = 0, kHours = 1, kBusinessDays = 2, kIrregular = 3;

// A validated uniform index (make_uniform): first <= last, both within +-kMaxInstant; a
// business-day first is a weekday.  An empty index has last = first - 1: no instant is inside.
struct Uniform {
    int kind;
    int step;
    int dow0;         // business days: day of week of first, 1..5
    int64_t first, last, periods;
    double rstep;     // 1.0 / step
};

STS_IX_HD inline int64_t floor_div(int64_t a, int64_t b) {   // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// ((floor(t / D) + 3) mod 7) + 1, Monday = 1 (1970-01-01 was a Thursday)
STS_IX_HD inline int day_of_week(int64_t t) {
    const int64_t d = floor_div(t, kDay) + 3;
    return (int)(d - floor_div(d, 7) * 7) + 1;
}

// trunc(d / step) for 0 <= d < 2^52, 1 <= step < 2^31
STS_IX_HD inline int64_t div_step(int64_t d, int step, double rstep) {
    int64_t q = (int64_t)((double)d * rstep);
    const int64_t r = d - q * step;
    if (r < 0) q--;
    else if (r >= step) q++;
    return q;
}

// calendar days a business-day advance of `total` >= 0 business days covers from a weekday
// (S/Frequency.scala:76-80)
STS_IX_HD inline int64_t business_span(int dow, int64_t total) {
    const int64_t weeks = total / 5;
    const int rem = (int)(total - weeks * 5);
    return total + weeks * 2 + (dow + rem > 5 ? 2 : 0);
}

// dateTimeAtLoc(loc) = frequency.advance(first, loc), 0 <= loc < periods (so no overflow)
STS_IX_HD inline int64_t instant_at(const Uniform& u, int64_t loc) {
    const int64_t total = loc * u.step;
    if (u.kind == kBusinessDays) return u.first + business_span(u.dow0, total) * kDay;
    return u.first + total * (u.kind == kHours ? kHour : kDay);
}

// locAtDateTime(t).  Outside [first, last] the answer is -1 whatever difference() gives: a
// negative or too large loc, loc 0 with another instant, or the reference's exception (a weekend
// earlier than a business-day first).  Inside, t - first < 2^63.
STS_IX_HD inline int64_t loc_at(const Uniform& u, int64_t t) {
    if (t < u.first || t > u.last) return -1;
    const int64_t unit = u.kind == kHours ? kHour : kDay;
    int64_t units = (t - u.first) / unit;   // daysBetween / hoursBetween
    if (u.kind == kBusinessDays) {          // S/Frequency.scala:87-95
        const int64_t weeks = units / 7;
        const int rem = (int)(units - weeks * 7);
        units -= weeks * 2 + (u.dow0 + rem > 5 ? 2 : 0);
        if (units < 0) return -1;           // a Saturday right after a Friday first: loc <= 0, another instant
    }
    const int64_t loc = div_step(units, u.step, u.rstep);
    return (loc < u.periods && instant_at(u, loc) == t) ? loc : -1;
}

// IrregularDateTimeIndex.locAtDateTime: the first location holding t, else -(insertion point) - 1
STS_IX_HD inline int64_t loc_irregular(const int64_t* instants, int64_t n, int64_t t) {
    int64_t lo = 0, hi = n;   // lower bound
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (instants[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && instants[lo] == t) ? lo : -lo - 1;
}

// Host only: validate a uniform index and fill `u`; nullptr when it is acceptable, else what is
// wrong (include/sts_index.h, "An index as arguments").
inline const char* make_uniform(int kind, int64_t start_ms, int64_t periods, int step, Uniform* u) {
    if (kind != kDays && kind != kHours && kind != kBusinessDays) return "unknown index kind";
    if (step < 1) return "frequency step must be at least 1";
    if (periods < 0) return "negative number of periods";
    if (start_ms < -kMaxInstant || start_ms > kMaxInstant) return "first instant outside [-2^62, 2^62] ms";
    u->kind = kind;
    u->step = step;
    u->rstep = 1.0 / (double)step;
    u->first = start_ms;
    u->periods = periods;
    u->dow0 = day_of_week(start_ms);
    if (kind == kBusinessDays && u->dow0 > 5) return "a business-day index starts on a weekend";
    if (periods == 0) {
        u->last = start_ms - 1;
        return nullptr;
    }
    // last = advance(first, periods - 1) in 128 bits: at most 7/5 * total + 2 units
    const __int128 total = (__int128)(periods - 1) * step;
    __int128 units = total;
    if (kind == kBusinessDays) units = total + (total / 5) * 2 + (u->dow0 + (int)(total % 5) > 5 ? 2 : 0);
    const __int128 last = (__int128)start_ms + units * (kind == kHours ? kHour : kDay);
    if (last > (__int128)kMaxInstant) return "last instant beyond 2^62 ms";
    u->last = (int64_t)last;
    return nullptr;
}

}  // namespace ix
}  // namespace sts
