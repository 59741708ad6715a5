/*
 * sts_index.h -- date-time indices on the device: DateTimeIndex lookups, and the rebasing of
 * panels from one index onto another that TimeSeriesRDD.slice / withIndex / timeSeriesRDD(
 * targetIndex, seriesRDD) are built on (S/DateTimeIndex.scala, S/Frequency.scala,
 * S/TimeSeriesUtils.scala:65-203, S/TimeSeriesRDD.scala:159-172, 446-482).
 *
 * A sibling of sts.h, like sts_transforms.h and sts_sample.h.  The panel layout contract, the
 * stream contract and the error contract of sts.h hold here VERBATIM: series-contiguous fp64 panels
 * with any 8-byte aligned base and any ld >= T; results depend only on the elements (s, t < T);
 * nothing outside the documented output block is written and no input is written; reads stay
 * inside the 128-byte lines the inputs touch; every launch and copy of a call is queued on `stream`
 * (NULL = hipStreamPerThread) and the call returns without waiting (no entry point here takes
 * err_per_series); every function returns an sts_status and sts_last_error() gives the thread-local
 * message.  The guards of sts.h have twins for this header in tests/test_index_cpu.py, the stream
 * rows live in tests/test_index_stream_gpu.py, and the bindings in sparkts/_native.py
 * INDEX_SIGNATURES.
 *
 *   S/ = src/main/scala/com/cloudera/sparkts/ in the reference, as in sts.h.
 *
 * ---- Instants ----
 * An instant is an int64 count of milliseconds since 1970-01-01T00:00:00Z.  Everything is UTC: the
 * reference builds every DateTime it compares in UTC, where Joda's calendar arithmetic is int64
 * arithmetic with Java's truncating division.  D = 86 400 000, H = 3 600 000.  The arithmetic is
 * defined once for host and device in csrc/sts_index.hpp and restated in tests/index_ref.py:
 *   DayFrequency(n)          advance(t, k) = t + k n D;  difference(a, b) = trunc(trunc((b - a) / D) / n)
 *   HourFrequency(n)         the same with H
 *   BusinessDayFrequency(n)  S/Frequency.scala:71-96 as written, with dayOfWeek(t) =
 *                            ((floor(t / D) + 3) mod 7) + 1 (Monday = 1); advance from a weekend and
 *                            difference whose earlier argument is a weekend throw
 *
 * ---- An index as arguments ----
 *   int kind, int64_t start_ms, int64_t periods, int step, const int64_t* instants, int64_t n_instants
 * kind is an sts_index_kind.  A uniform kind (DAYS, HOURS, BUSINESS_DAYS) is UniformDateTimeIndex(
 * start_ms, periods, frequency(step)) and ignores instants / n_instants; STS_INDEX_IRREGULAR is
 * IrregularDateTimeIndex(instants[0 .. n_instants)), a DEVICE array sorted non-decreasing, and
 * ignores start_ms / periods / step.  STS_ERR_BAD_ARG, on the host, before any launch: an unknown
 * kind; step < 1; a negative periods or n_instants; a NULL instants with n_instants > 0; a
 * business-day start on a weekend; a uniform index whose first or last instant lies outside
 * [-2^62, 2^62] ms.
 *
 * ---- locAtDateTime ----
 * Uniform: loc = difference(first, t) if 0 <= loc < periods and advance(first, loc) == t, else -1
 * (S/DateTimeIndex.scala:143-150).  A timestamp on which the reference's scalar code throws (a
 * weekend earlier than a business-day first) gives -1.
 * Irregular: the FIRST location holding t, else -(insertion point) - 1.  For an index without
 * duplicates that is java.util.Arrays.binarySearch bit for bit.  With duplicates it is what the
 * reference's doc comment promises ("returns its first appearance") and what its merge loop
 * (S/TimeSeriesUtils.scala:176-188) does; its binarySearch may return another duplicate.
 *
 * ---- Rebase: one rule for every pair of index kinds ----
 *   out(s, j) = m[j] >= 0 ? in(s, m[j]) : default_value,   m[j] = the first location of target
 *   instant j in the source.
 * Uniform -> uniform is the shift m[j] = j + start_loc (i3); every other pair is a lookup (i2 on the
 * target's instants, then i4).  For irregular sources that is the documented meaning of the
 * reference's rebaserWithIrregularSource, which is only right when at most one source instant
 * precedes the target (it drops -locAtDateTime(first) elements, 1 whenever first is absent) and
 * asserts on duplicates and off-grid instants; all RebaseSuite cases agree with the lookup rule.
 * Uniform -> irregular throws UnsupportedOperationException in the reference and is the same lookup
 * here.
 *
 * All five entry points are pure copies and BIT-EXACT: copied elements keep their bits (NaN
 * payloads, -0.0, infinities, subnormals), default_value is written with its bits, and padding
 * t in [T_out, ld_out) is never written.
 *
 * JNI bindings do not exist for these entry points.
 */
#ifndef STS_INDEX_H
#define STS_INDEX_H

#include "sts.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    STS_INDEX_DAYS = 0,
    STS_INDEX_HOURS = 1,
    STS_INDEX_BUSINESS_DAYS = 2,
    STS_INDEX_IRREGULAR = 3
} sts_index_kind;

/* ---- i1: DateTimeIndex.toMillisArray on the device: out[i] = dateTimeAtLoc(i), i < size (periods
 *      or n_instants int64 entries, a device array). */
int sts_index_instants(int kind, int64_t start_ms, int64_t periods, int step, const int64_t* instants,
                       int64_t n_instants, int64_t* out, void* stream);

/* ---- i2: DateTimeIndex.locAtDateTime for n device timestamps: loc[i] = locAtDateTime(millis[i])
 *      ("locAtDateTime" above), one thread per timestamp.  n < 0 -> STS_ERR_BAD_ARG. */
int sts_index_locs(const int64_t* millis, int64_t n, int kind, int64_t start_ms, int64_t periods, int step,
                   const int64_t* instants, int64_t n_instants, int64_t* loc, void* stream);

/* ---- i3: rebase, uniform -> uniform (S/TimeSeriesUtils.scala:100-129):
 *   out(s, j) = 0 <= j + start_loc < T_in ? in(s, j + start_loc) : default_value,   j < T_out.
 * Any start_loc, fully disjoint ranges included (out is then all default_value).  out must not
 * alias in. */
int sts_rebase_shift(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                     int64_t ld_out, int64_t start_loc, double default_value, void* stream);

/* ---- i4: rebase by lookup, the gather form:
 *   out(s, j) = 0 <= map[j] < T_in ? in(s, map[j]) : default_value,   j < T_out.
 * map: T_out device entries.  An entry < 0 OR >= T_in means absent: no map can cause a read outside
 * a row, and nothing is validated with a synchronisation.  out must not alias in. */
int sts_rebase_map(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                   int64_t ld_out, const int64_t* map, double default_value, void* stream);

/* ---- i5: timeSeriesRDD(targetIndex, seriesRDD) (S/TimeSeriesRDD.scala:446-482) for series that
 *      each have their own uniform index.  Series s is the len_s = offsets[s + 1] - offsets[s] values
 *      starting at values[offsets[s]]:
 *   out(s, j) = 0 <= j + start_loc[s] < len_s ? values[offsets[s] + j + start_loc[s]] : default_value,
 *   j < T_out.
 * offsets: S + 1 device entries, non-decreasing; start_loc: S device entries (i3's start_loc, per
 * series).  A zero-length series gives an all-default row.  Reads stay inside
 * values[0 .. offsets[S]). */
int sts_align_uniform(const double* values, const int64_t* offsets, const int64_t* start_loc, int64_t S,
                      int64_t T_out, double* out, int64_t ld_out, double default_value, void* stream);

/* ---- host-buffer variants of i3 and i4: the staging pipeline of sts.h ("host-buffer variants").
 * in is (S, T_in) with ld; out is packed, ld = T_out; map is a HOST array of T_out entries. ---- */
int sts_rebase_shift_host(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld,
                          int64_t start_loc, double default_value);
int sts_rebase_map_host(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld,
                        const int64_t* map, double default_value);

#ifdef __cplusplus
}
#endif
#endif /* STS_INDEX_H */
