// Which bytes of a batch call's pageable host frames are page-locked where they lie (upload.hip: BatchUploader).  Plain C++,
// no HIP: tests/cxx/reg_plan_check.cpp compiles it on its own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lramd {

struct RegPlan {
    uintptr_t lo = 0, hi = 0;  // the whole pages inside the frame (hi <= lo: none worth registering)
    int r_lo = 0, r_hi = 0;    // rows [r_lo, r_hi) lie in them; the rows before and after are staged
};

// The plans of `n` frames of `h` rows of `row_bytes` bytes, `pitch` bytes from one row to the next (pitch >= row_bytes),
// frames[i] addressing frame i's first row; may_register[i] == 0: frame i gets no plan (memory the caller has page-locked
// already, a call that registers nothing).
// No page is ever registered twice.  Frames of one array share the page at each end with their neighbours (an 8-bit
// 1080p frame is 506.25 pages; an fp32 frame too, where the array does not start on a page), and the helpers register
// and release frame by frame, concurrently.  So a frame's range is rounded INWARDS to whole pages: the pages two
// frames share belong to neither, and the rows that reach into them -- at most 4 KB and a row at each end -- go through
// the slot's staging buffer instead.  A frame whose pages overlap an earlier frame's (a frame listed twice, sliding
// windows over one array) is not registered at all: it takes the staging copy, which only reads the caller's memory.
inline std::vector<RegPlan> plan_registrations(const void* const* frames, int n, int h, size_t pitch, size_t row_bytes, uintptr_t page,
                                               const char* may_register) {
    std::vector<RegPlan> plan((size_t)n);
    for (int i = 0; i < n; ++i) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(frames[i]), e = a + (size_t)(h - 1) * pitch + row_bytes;
        const uintptr_t lo = (a + page - 1) / page * page, hi = e / page * page;
        if (hi <= lo) continue;
        const int r_lo = (int)((lo - a + pitch - 1) / pitch);                                // first row that starts at or behind lo
        const int r_hi = hi - a >= row_bytes ? (int)std::min<size_t>((size_t)h, (hi - a - row_bytes) / pitch + 1) : 0;  // rows that end at or before hi
        if (r_hi - r_lo < h / 2) continue;  // (a frame of a few pages: the staging copy)
        bool apart = may_register[i] != 0;  // ... from every earlier frame's pages
        for (int j = 0; j < i && apart; ++j) {
            const RegPlan& q = plan[(size_t)j];
            apart = q.hi <= q.lo || q.hi <= lo || hi <= q.lo;
        }
        if (!apart) continue;
        plan[(size_t)i] = RegPlan{lo, hi, r_lo, r_hi};
    }
    return plan;
}

}  // namespace lramd
