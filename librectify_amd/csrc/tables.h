// What the entries that take a per-call table (warp, prepare, overlay, JPEG) share on the host: reading the caller's
// doubles as integers, the check that no two outputs overlap, sending a table up, and picking a kernel by pixel format.
#pragma once
#include <algorithm>
#include <cmath>
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

// launch(tag) with tag an std::integral_constant of the pixel format, so that `decltype(tag)::value` names a kernel's
// instantiation (the caller has checked that `format` is one of the three)
template <class Launch>
void launch_by_format(int format, Launch&& launch) {
    if (format == LR_PIX_U8) launch(std::integral_constant<int, LR_PIX_U8>{});
    else if (format == LR_PIX_U8X3) launch(std::integral_constant<int, LR_PIX_U8X3>{});
    else launch(std::integral_constant<int, LR_PIX_F32>{});
}

}  // namespace lramd
