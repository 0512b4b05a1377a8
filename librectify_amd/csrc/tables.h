// What the entries that take a per-call table (warp, prepare, overlay, JPEG) share on the host: reading the caller's
// doubles as integers, the check that no two outputs overlap, sending a table up, and picking a kernel by pixel format.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "context.h"

namespace lramd {

constexpr double kExact = 9007199254740992.0;  // 2^53: integers up to it are doubles

// v as an integer in [lo, hi], if it is one
inline bool table_integer(double v, double lo, double hi, uint64_t* out) {
    if (!(v >= lo && v <= hi) || v != std::floor(v)) return false;
    *out = (uint64_t)v;
    return true;
}

// Sorts the extents [first byte, end).  Returns 0 if no two overlap, otherwise the place (in sorted order, at least 1) of
// one that begins inside the one before it.
inline size_t extents_overlap(std::vector<std::pair<uint64_t, uint64_t>>& extent) {
    std::sort(extent.begin(), extent.end());
    for (size_t b = 1; b < extent.size(); ++b)
        if (extent[b].first < extent[b - 1].second) return b;
    return 0;
}

// The per-call upload of a mirrored buffer on the context's stream, in two parts around the caller's writes to m.h.
// upload_reserve: room for `count` elements (a buffer that must grow, to `grow_to` if that is given, does so after a stream
// synchronise: the previous call's launch may still read the device copy) and `ev` made and waited for (the previous call's
// upload has read the page-locked copy).  upload_send: the first `bytes` go up and `ev` is recorded behind them.
template <class T>
int upload_reserve(lr_context* c, MirroredBuffer<T>& m, Event& ev, size_t count, size_t grow_to = 0) {
    if (count > m.cap()) {
        LR_HIP(hipStreamSynchronize(c->stream));
        if (m.grow(std::max(count, grow_to))) return 1;
    }
    if (ev.ensure(hipEventDisableTiming)) return 1;
    LR_HIP(hipEventSynchronize(ev));
    return 0;
}
template <class T>
int upload_send(lr_context* c, MirroredBuffer<T>& m, Event& ev, size_t bytes) {
    LR_HIP(hipMemcpyAsync(m.d, m.h, bytes, hipMemcpyHostToDevice, c->stream));
    LR_HIP(hipEventRecord(ev, c->stream));
    return 0;
}

// The weights of LR_WARP_CUBIC: row a holds the four taps' weights, at scale 2048, for the
// fraction a / 32 -- the Keys kernel with A = -0.75, c0 = ((A(t+1) - 5A)(t+1) + 8A)(t+1) - 4A, c1 = ((A+2)t - (A+3))t^2 + 1,
// c2 = c1 of 1 - t, c3 = 1 - c0 - c1 - c2, each floor(c * 2048 + 0.5), and what a row then lacks to 2048 (at most 1 either way)
// added to its entry [1] (a <= 16) or [2] (a > 16).  Every row sums to 2048, row 32 - a is row a reversed, the largest sum
// of magnitudes is 2816 (rows 10 .. 12 and 20 .. 22).  tests/numpy_warp_cubic_ref.py computes the table from the formula and
// tests/test_warp_cubic_cpu.py holds these literals against it.
alignas(8) constexpr int16_t kCubicWeights[32][4] = {
    {   0, 2048,    0,    0}, { -45, 2043,   51,   -1}, { -84, 2031,  107,   -6}, {-118, 2009,  169,  -12},
    {-147, 1981,  235,  -21}, {-171, 1946,  305,  -32}, {-190, 1903,  379,  -44}, {-205, 1854,  456,  -57},
    {-216, 1800,  536,  -72}, {-223, 1740,  618,  -87}, {-227, 1676,  702, -103}, {-227, 1607,  787, -119},
    {-225, 1535,  873, -135}, {-220, 1460,  959, -151}, {-213, 1380, 1046, -165}, {-203, 1299, 1131, -179},
    {-192, 1216, 1216, -192}, {-179, 1131, 1299, -203}, {-165, 1046, 1380, -213}, {-151,  959, 1460, -220},
    {-135,  873, 1535, -225}, {-119,  787, 1607, -227}, {-103,  702, 1676, -227}, { -87,  618, 1740, -223},
    { -72,  536, 1800, -216}, { -57,  456, 1854, -205}, { -44,  379, 1903, -190}, { -32,  305, 1946, -171},
    { -21,  235, 1981, -147}, { -12,  169, 2009, -118}, {  -6,  107, 2031,  -84}, {  -1,   51, 2043,  -45},
};

// launch(tag) with tag an std::integral_constant of the pixel format, so that `decltype(tag)::value` names a kernel's
// instantiation (the caller has checked that `format` is one of the three)
template <class Launch>
void launch_by_format(int format, Launch&& launch) {
    if (format == LR_PIX_U8) launch(std::integral_constant<int, LR_PIX_U8>{});
    else if (format == LR_PIX_U8X3) launch(std::integral_constant<int, LR_PIX_U8X3>{});
    else launch(std::integral_constant<int, LR_PIX_F32>{});
}

// launch(tag, rule) for the warp, whose kernels are instantiated per sampling rule as well: rule is std::true_type for
// LR_WARP_CUBIC and std::false_type for the bilinear rule
template <class Launch>
void launch_by_format_and_rule(int format, bool cubic, Launch&& launch) {
    launch_by_format(format, [&](auto fmt) {
        if (cubic) launch(fmt, std::true_type{});
        else launch(fmt, std::false_type{});
    });
}

}  // namespace lramd
