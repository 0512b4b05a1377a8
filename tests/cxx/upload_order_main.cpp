// The host upload path of the library, linked host-only against the model HIP runtime (tests/cxx/model_hip): single host
// frames, the staging crew on its own, batches of host frames, under the schedule named on the command line.
//
//   upload_order <eager|lazy|threaded> <seed> <group>[,<group>...]
//
// Every pixel of every frame encodes (frame index, row, column).  The filter kernel has a behaviour that checks, at the
// moment the model executes a launch, that every image row the launch reads holds the bytes of the frame it should hold.
// After each public call that succeeds the harness asks the model whether anything is still pending on the caller's memory,
// overwrites the caller's frame with a poison value and drains the model: no later check may see the poison.
// The process ends with 0 only if the model's error list is empty.  (LIBRECTIFY_UPLOAD_BAND_KB and
// LIBRECTIFY_REGISTER_FRAMES are read once per process by the library: the test starts a process per setting.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "host.h"
#include "model_hip/model_hip.h"

using namespace lramd;

namespace {

constexpr uint8_t kPoison = 0xEE;
int pix_size(int fmt) { return fmt == LR_PIX_F32 ? 4 : fmt == LR_PIX_U8 ? 1 : 3; }
const char* fmt_name(int fmt) { return fmt == LR_PIX_F32 ? "f32" : fmt == LR_PIX_U8 ? "u8" : "u8x3"; }

uint8_t byte_of(int fidx, int y, int xb) { return (uint8_t)(fidx * 67 + y * 29 + xb * 3 + (xb >> 6) * 5 + (y >> 5) * 11 + 1); }
uint32_t word_of(int fidx, int y, int x) { return 0x40000000u | ((uint32_t)fidx << 22) | ((uint32_t)y << 11) | (uint32_t)x; }
// the bytes of row y of frame fidx (w pixels)
void expected_row(int fmt, int w, int fidx, int y, uint8_t* out) {
    if (fmt == LR_PIX_F32) {
        for (int x = 0; x < w; ++x) {
            const uint32_t v = word_of(fidx, y, x);
            std::memcpy(out + 4 * (size_t)x, &v, 4);
        }
    } else {
        const int n = w * pix_size(fmt);
        for (int xb = 0; xb < n; ++xb) out[xb] = byte_of(fidx, y, xb);
    }
}
// rows [r0, r1) of a packed device frame against frame fidx: the first row that differs, or -1
int first_bad_row(const uint8_t* img, int fmt, int w, int fidx, int r0, int r1) {
    std::vector<uint8_t> row((size_t)w * pix_size(fmt));
    for (int y = r0; y < r1; ++y) {
        expected_row(fmt, w, fidx, y, row.data());
        if (std::memcmp(img + (size_t)y * row.size(), row.data(), row.size()) != 0) return y;
    }
    return -1;
}

// A caller's frame: pageable (malloc) or page-locked (the model's hipHostMalloc, marked as the caller's).
struct HostFrame {
    uint8_t* mem = nullptr;  // row 0 of the image
    void* owner = nullptr;
    size_t owner_bytes = 0;
    bool pinned = false, owns = false;
    int fmt = 0, w = 0, h = 0, stride = 0;  // stride in pixels, as the caller passes it (any sign)
    size_t pitch() const { return (size_t)(stride < 0 ? -stride : stride) * pix_size(fmt); }
    // what the caller passes: with a negative stride the rows are addressed from the other end (no flip)
    const void* arg() const { return stride < 0 ? mem + (size_t)(h - 1) * pitch() : mem; }
    void fill(int fidx) {
        std::vector<uint8_t> row((size_t)w * pix_size(fmt));
        for (int y = 0; y < h; ++y) {
            expected_row(fmt, w, fidx, y, row.data());
            std::memcpy(mem + (size_t)y * pitch(), row.data(), row.size());
        }
    }
    void poison() { std::memset(mem, kPoison, (size_t)(h - 1) * pitch() + (size_t)w * pix_size(fmt)); }
    void release() {
        if (owns && pinned) (void)hipHostFree(owner);
        else if (owns) std::free(owner);
        owner = nullptr;
    }
};
HostFrame make_frame(int fmt, int w, int h, int stride, bool pinned) {
    HostFrame f;
    f.fmt = fmt;
    f.w = w;
    f.h = h;
    f.stride = stride;
    f.pinned = pinned;
    f.owns = true;
    f.owner_bytes = (size_t)(h - 1) * f.pitch() + (size_t)w * pix_size(fmt);
    if (pinned) {
        if (hipHostMalloc(&f.owner, f.owner_bytes) != hipSuccess) std::abort();
        model_hip_mark_caller_memory(f.owner);
    } else {
        f.owner = std::malloc(f.owner_bytes);
    }
    f.mem = static_cast<uint8_t*>(f.owner);
    std::memset(f.mem, kPoison, f.owner_bytes);
    return f;
}
int frames_word(int fmt) { return (fmt + 1) << 8; }

// ---- what the filter launches must find -----------------------------------------------------------------------------------

struct Expect {
    std::atomic<int> mode{0};  // 0: nothing is expected (the launch is counted only), 1: one frame, 2: a batch
    int fmt = 0, w = 0, h = 0, fidx = 0;
    bool follow = true;                   // the filter reads the frame's slot (f32, u8); else it reads the luma plane
    const lr_context* ctx = nullptr;      // mode 1, !follow: whose slot 0 must hold the whole frame
    std::atomic<int> launches{0}, rows{0};
    std::atomic<int> by_hits[64];         // mode 1: launches that covered band row by
    std::atomic<int> frame_hits[16];      // mode 2: whole-frame launches that found frame i
    void reset(int m) {
        launches.store(0);
        rows.store(0);
        for (auto& a : by_hits) a.store(0);
        for (auto& a : frame_hits) a.store(0);
        mode.store(m, std::memory_order_release);
    }
} g_expect;

int decode_fidx(const uint8_t* img, int fmt) {
    if (fmt == LR_PIX_F32) {
        uint32_t v;
        std::memcpy(&v, img, 4);
        return (v >> 30) == 1u ? (int)((v >> 22) & 15u) : -1;
    }
    for (int i = 0; i < 16; ++i)
        if (img[0] == byte_of(i, 0, 0) && img[1] == byte_of(i, 0, 1) && img[2] == byte_of(i, 0, 2)) return i;
    return -1;
}

// filter_lanes_kernel(img, w, h, stride, taps, dx, dy, dmask, cand, cand_count, tile_max, bands_x, band_begin, band_end):
// fourteen parameters, img the first (argument 0), the three band words the last (arguments 11 to 13).
constexpr int kFilterArgs = 14;
void filter_run(void*, void* const* args, void*) {
    Expect& e = g_expect;
    const int mode = e.mode.load(std::memory_order_acquire);
    const uint8_t* img = *static_cast<const uint8_t* const*>(args[0]);
    const int w = *static_cast<const int*>(args[1]), h = *static_cast<const int*>(args[2]), stride = *static_cast<const int*>(args[3]);
    const int bands_x = *static_cast<const int*>(args[11]), band_begin = *static_cast<const int*>(args[12]), band_end = *static_cast<const int*>(args[13]);
    e.launches.fetch_add(1);
    if (mode == 0) return;
    if (w != e.w || h != e.h || stride != e.w || bands_x != (w + 55) / 56 || band_begin % bands_x != 0 || band_end % bands_x != 0 || band_end <= band_begin) {
        model_hip_error("filter-args", "filter launch with w %d h %d stride %d bands_x %d bands [%d, %d) on a frame of %d x %d", w, h, stride, bands_x,
                        band_begin, band_end, e.w, e.h);
        return;
    }
    const int by0 = band_begin / bands_x, by1 = band_end / bands_x;
    const int fb = filter_band_rows();
    if (mode == 1) {
        for (int by = by0; by < by1 && by < 64; ++by) e.by_hits[by].fetch_add(1);
        if (!e.follow) {  // the frame went up whole before its luma launch: the slot must hold all of it by now
            const uint8_t* slot = reinterpret_cast<const uint8_t*>(e.ctx->frames.slot[0].get());
            const int bad = first_bad_row(slot, e.fmt, e.w, e.fidx, 0, e.h);
            if (bad >= 0) model_hip_error("filter-rows", "interleaved frame %d: row %d of the slot does not hold the frame when the filter runs", e.fidx, bad);
            e.rows.fetch_add(e.h);
            return;
        }
        const int r0 = std::max(0, fb * by0 - 4), r1 = std::min(h - 1, filter_band_last_row(by1 - 1)) + 1;
        const int bad = first_bad_row(img, e.fmt, e.w, e.fidx, r0, r1);
        if (bad >= 0)
            model_hip_error("filter-rows", "frame %d (%s %d x %d): the filter launch over band rows [%d, %d) reads image row %d, which does not hold the frame's bytes",
                            e.fidx, fmt_name(e.fmt), e.w, e.h, by0, by1, bad);
        e.rows.fetch_add(r1 - r0);
        return;
    }
    // a batch: the launch covers a whole frame, and its slot must hold exactly one frame, complete
    if (by0 != 0 || by1 != (h + fb - 1) / fb) {
        model_hip_error("filter-args", "batch: a filter launch over band rows [%d, %d) of a frame of %d rows", by0, by1, h);
        return;
    }
    const int fidx = decode_fidx(img, e.fmt);
    const int bad = fidx < 0 ? 0 : first_bad_row(img, e.fmt, e.w, fidx, 0, e.h);
    if (fidx < 0 || bad >= 0) {
        model_hip_error("filter-rows", "batch: the slot at %p holds no complete frame when its filter runs (first pixel says frame %d, row %d differs)",
                        (const void*)img, fidx, bad);
        return;
    }
    e.frame_hits[fidx].fetch_add(1);
    e.rows.fetch_add(h);
}
int filter_writes(void*, void* const* args, model_hip_range* out, int cap) {
    const int w = *static_cast<const int*>(args[1]), h = *static_cast<const int*>(args[2]);
    const size_t npix = (size_t)w * h;
    if (cap < 3) return 0;
    out[0] = model_hip_range{*static_cast<void* const*>(args[5]), npix * 4};
    out[1] = model_hip_range{*static_cast<void* const*>(args[6]), npix * 4};
    out[2] = model_hip_range{*static_cast<void* const*>(args[7]), npix};
    return 3;
}

// ---- bookkeeping ------------------------------------------------------------------------------------------------------------

int g_harness_errors = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++g_harness_errors;                           \
            model_hip_error("harness", __VA_ARGS__);      \
        }                                                 \
    } while (0)

std::string trace_string() {
    uint64_t t[16];
    const int n = model_hip_trace_lengths(t, 16);
    std::string s;
    for (int i = 0; i < std::min(n, 16); ++i) s += (i ? "," : "") + std::to_string(t[i]);
    return s.empty() ? "-" : s;
}
// after a public call that succeeded: nothing may be pending on the caller's frame, which is overwritten at once (the caller
// of this drains the model when it is done looking at what the call left pending)
void after_call(HostFrame& f) {
    model_hip_check_quiescent();
    f.poison();
}

size_t env_band_bytes() {
    const char* e = std::getenv("LIBRECTIFY_UPLOAD_BAND_KB");
    return e ? (size_t)std::max(64, std::atoi(e)) << 10 : (size_t)4 << 20;
}
// upload bands of a single host frame (frame.hip: ctx_find_groups_host)
int upload_bands(int fmt, int w, int h, bool pinned) {
    const size_t row_bytes = (size_t)w * pix_size(fmt);
    const bool band_env = std::getenv("LIBRECTIFY_UPLOAD_BAND_KB") != nullptr;
    const int rpb = (int)std::max<size_t>(1, ((pinned && !band_env) ? (size_t)h * row_bytes : env_band_bytes()) / row_bytes);
    return (h + rpb - 1) / rpb;
}

int g_frame_counter = 0;
int next_fidx() { return g_frame_counter++ & 15; }

// ---- single host frames -----------------------------------------------------------------------------------------------------

void run_single(lr_context* c, const char* name, int fmt, int w, int h, int stride, bool pinned, int threads) {
    HostFrame f = make_frame(fmt, w, h, stride, pinned);
    const int fidx = next_fidx();
    f.fill(fidx);
    Expect& e = g_expect;
    e.fmt = fmt;
    e.w = w;
    e.h = h;
    e.fidx = fidx;
    e.follow = fmt != LR_PIX_U8X3;
    e.ctx = c;
    e.reset(1);
    model_hip_reset_counters();
    std::vector<LineSegment> out(16);
    int n = -1;
    const int rc = lr_find_line_segment_groups_host(c, static_cast<const float*>(f.arg()), w, h, stride, 10.f, frames_word(fmt), threads, out.data(), 16, &n);
    CHECK(rc == 0, "%s: lr_find_line_segment_groups_host failed: %s", name, lr_last_error());
    const std::string trace = trace_string();
    if (rc == 0) after_call(f);
    if (rc == 0 && threads == 2 && stride == w) {  // the whole call, then lr_download: nothing may be left that it does not wait for
        std::vector<uint32_t> label((size_t)w * h);
        CHECK(lr_download(c, LR_BUF_LABEL, label.data(), label.size() * 4) == 0, "%s: lr_download failed: %s", name, lr_last_error());
        const int left = model_hip_pending_work();
        if (left) model_hip_error("pending-after-download", "%s: %d copies, memsets or launches are still pending when lr_download returns", name, left);
    }
    model_hip_drain();
    e.mode.store(0);
    const int band_rows = (h + filter_band_rows() - 1) / filter_band_rows();
    for (int by = 0; by < band_rows && rc == 0; ++by)
        CHECK(e.by_hits[by].load() == 1, "%s: band row %d of %d was filtered %d times", name, by, band_rows, e.by_hits[by].load());
    CHECK(rc != 0 || n == 0, "%s: %d lines from a device that computes nothing", name, n);
    std::printf("case %s fmt=%s w=%d h=%d stride=%d pinned=%d threads=%d follow=%d bands=%d launches=%d rows=%d trace=%s\n", name, fmt_name(fmt), w, h, stride,
                (int)pinned, threads, (int)e.follow, upload_bands(fmt, w, h, pinned), e.launches.load(), e.rows.load(), trace.c_str());
    f.release();
}

void group_single(bool slow_helpers) {
    lr_context* c = nullptr;
    if (lr_context_create(0, &c)) std::abort();
    const int heights[] = {63, 64, 65, 94, 127, 128, 129, 193};
    const struct {
        int fmt, w;
    } kinds[] = {{LR_PIX_F32, 256}, {LR_PIX_U8, 1024}, {LR_PIX_U8X3, 340}};
    if (slow_helpers) model_hip_helper_pause_us(300);
    for (const auto& k : kinds)
        for (int h : heights)
            for (int s = 0; s < 3; ++s)
                for (int pinned = 0; pinned < 2; ++pinned)
                    for (int threads : {1, 2, 8}) {
                        if (slow_helpers && (pinned || threads == 1 || s != 0 || k.fmt == LR_PIX_U8X3)) continue;
                        run_single(c, slow_helpers ? "slow" : "single", k.fmt, k.w, h, s == 0 ? k.w : s == 1 ? k.w + 13 : -k.w, pinned != 0, threads);
                    }
    model_hip_helper_pause_us(0);
    lr_context_destroy(c);
}

// the same context over small -> large -> small -> trim -> large, and nine small frames in a row (the workspace is given back
// by itself after eight): slots, staging buffers and workspace grow and shrink with work behind them
void group_sequence() {
    lr_context* c = nullptr;
    if (lr_context_create(0, &c)) std::abort();
    for (int pinned = 0; pinned < 2; ++pinned) {
        run_single(c, "seq", LR_PIX_F32, 256, 65, 256, pinned != 0, 2);
        run_single(c, "seq", LR_PIX_F32, 512, 300, 512, pinned != 0, 2);
        run_single(c, "seq", LR_PIX_F32, 256, 65, 256, pinned != 0, 2);
        CHECK(lr_context_trim(c) == 0, "lr_context_trim failed: %s", lr_last_error());
        run_single(c, "seq", LR_PIX_U8, 1024, 193, 1024, pinned != 0, 8);
        for (int i = 0; i < 9; ++i) run_single(c, "seq", LR_PIX_F32, 256, 64, 256, pinned != 0, 2);
        run_single(c, "seq", LR_PIX_F32, 512, 300, 525, pinned != 0, 2);
    }
    lr_context_destroy(c);
}

// lr_stage_filter_host: the frame goes up whole (upload_rows) and the call returns without waiting; lr_download is the
// blocking copy behind it
void stage_filter_case(lr_context* c, const char* name, int w, int h, int stride, bool pinned) {
    HostFrame f = make_frame(LR_PIX_F32, w, h, stride, pinned);
    const int fidx = next_fidx();
    f.fill(fidx);
    Expect& e = g_expect;
    e.fmt = LR_PIX_F32;
    e.w = w;
    e.h = h;
    e.fidx = fidx;
    e.follow = true;
    e.reset(1);
    model_hip_reset_counters();
    const int rc = lr_stage_filter_host(c, static_cast<const float*>(f.arg()), w, h, stride);
    CHECK(rc == 0, "%s: lr_stage_filter_host failed: %s", name, lr_last_error());
    const std::string trace = trace_string();
    if (rc == 0) after_call(f);
    std::vector<float> dx((size_t)w * h);
    CHECK(lr_download(c, LR_BUF_DX, dx.data(), dx.size() * 4) == 0, "%s: lr_download failed: %s", name, lr_last_error());
    // what lr_download does not wait for (under the lazy schedule: whatever nothing has forced yet) must be nothing at all
    const int left = model_hip_pending_work();
    if (left) model_hip_error("pending-after-download", "%s: %d copies, memsets or launches are still pending when lr_download returns", name, left);
    model_hip_drain();
    e.mode.store(0);
    CHECK(e.launches.load() == 1 && e.rows.load() == h, "%s: %d filter launches over %d rows of %d", name, e.launches.load(), e.rows.load(), h);
    std::printf("case %s fmt=f32 w=%d h=%d stride=%d pinned=%d threads=-1 follow=0 bands=%d launches=%d rows=%d trace=%s\n", name, w, h, stride, (int)pinned,
                (int)(((size_t)h * w * 4 + ((size_t)4 << 20) - 1) >> 22), e.launches.load(), e.rows.load(), trace.c_str());
    f.release();
}

// Two uploads into one slot with nothing between them (ctx_upload_frame, what lr_stage_filter_host is made of): the second
// staging fill meets the first frame's transfers.  Then the stage call itself, pageable and page-locked.
void group_consecutive() {
    lr_context* c = nullptr;
    if (lr_context_create(0, &c)) std::abort();
    for (int threads : {-1, 4})
        for (int slot = 0; slot < 2; ++slot) {
            HostFrame a = make_frame(LR_PIX_F32, 256, 129, 256, false), b = make_frame(LR_PIX_F32, 256, 129, 269, false);
            const int fa = next_fidx(), fb = next_fidx();
            a.fill(fa);
            b.fill(fb);
            g_expect.reset(0);
            model_hip_reset_counters();
            CHECK(ctx_upload_frame(c, slot, static_cast<const float*>(a.arg()), 256, 129, 256, threads) == 0, "ctx_upload_frame failed: %s", lr_last_error());
            model_hip_check_quiescent();
            a.poison();
            CHECK(ctx_upload_frame(c, slot, static_cast<const float*>(b.arg()), 256, 129, 269, threads) == 0, "ctx_upload_frame failed: %s", lr_last_error());
            const std::string trace = trace_string();
            after_call(b);
            model_hip_drain();
            const int bad = first_bad_row(reinterpret_cast<const uint8_t*>(c->frames.slot[slot].get()), LR_PIX_F32, 256, fb, 0, 129);
            CHECK(bad < 0, "consecutive uploads: row %d of slot %d does not hold the second frame", bad, slot);
            std::printf("case consecutive slot=%d threads=%d trace=%s\n", slot, threads, trace.c_str());
            a.release();
            b.release();
        }
    for (int pinned = 0; pinned < 2; ++pinned)
        for (int s = 0; s < 3; ++s) stage_filter_case(c, "stage", 256, 129, s == 0 ? 256 : s == 1 ? 269 : -256, pinned != 0);
    // frames of different sizes behind each other: the slot, the staging buffer and the workspace grow between two stage calls
    for (int pinned = 0; pinned < 2; ++pinned) {
        stage_filter_case(c, "stage", 512, 300, 512, pinned != 0);
        stage_filter_case(c, "stage", 256, 65, 256, pinned != 0);
        stage_filter_case(c, "stage", 1000, 563, 1000, pinned != 0);
    }
    lr_context_destroy(c);
}

// without the band knob: a frame above 8 MB, which upload_rows sends in 4 MB bands
void group_big() {
    lr_context* c = nullptr;
    if (lr_context_create(0, &c)) std::abort();
    stage_filter_case(c, "big", 2048, 1025, 2048, false);
    lr_context_destroy(c);
}

// ---- the staging crew on its own -------------------------------------------------------------------------------------------

struct CrewJob {
    HostFrame src;
    void* dst = nullptr;
    void* stage = nullptr;
    int fidx = 0;
};
void group_crew() {
    lr_context* c = nullptr;
    if (lr_context_create(0, &c)) std::abort();
    hipStream_t up = nullptr;
    if (hipStreamCreateWithFlags(&up, hipStreamNonBlocking) != hipSuccess) std::abort();
    const struct {
        const char* name;
        int helpers, w, h, stride, band_rows, pieces;
        bool own_hands;
    } cases[] = {
        {"one-band", 3, 64, 7, 64, 7, 0, false},           {"ragged-last-band", 3, 64, 23, 77, 5, 0, false},
        {"more-pieces-than-rows", 3, 64, 10, 64, 3, 8, false}, {"negative-stride", 2, 64, 23, -64, 4, 2, false},
        {"no-helper", 0, 64, 23, 64, 5, 0, false},         {"own-hands", 2, 64, 40, 64, 4, 0, true},
    };
    for (const auto& k : cases) {
        StagingCrew crew;
        crew.start(c, k.helpers);
        // two jobs right behind each other (the generation parity), each with buffers of its own
        CrewJob job[2];
        std::vector<Event> ev(64);
        for (auto& e : ev)
            if (e.ensure(hipEventDisableTiming)) std::abort();
        for (int j = 0; j < 2; ++j) {
            const int h = k.h + j * 3;
            job[j].src = make_frame(LR_PIX_F32, k.w, h, k.stride, false);
            job[j].fidx = next_fidx();
            job[j].src.fill(job[j].fidx);
            if (hipMalloc(&job[j].dst, (size_t)k.w * h * 4) != hipSuccess || hipHostMalloc(&job[j].stage, (size_t)k.w * h * 4) != hipSuccess) std::abort();
        }
        model_hip_reset_counters();
        for (int j = 0; j < 2; ++j) {
            const int h = k.h + j * 3;
            std::vector<std::atomic<int>> ready(64);
            for (auto& a : ready) a.store(0);
            const uint32_t g = crew.begin(job[j].dst, job[j].stage, job[j].src.arg(), k.w, h, k.stride, 4, up, ev.data(), ready.data(), (size_t)k.band_rows * k.w * 4, k.pieces);
            if (k.own_hands)
                while (crew.work_one(g)) {
                }
            CHECK(crew.finish() == 0, "crew %s: finish failed", k.name);
            const int n_bands = (h + k.band_rows - 1) / k.band_rows;
            for (int b = 0; b < n_bands; ++b) CHECK(ready[(size_t)b].load() == 1, "crew %s: band %d of job %d is not ready after finish()", k.name, b, j);
            job[j].src.poison();  // (every band has been staged)
        }
        const std::string trace = trace_string();
        model_hip_check_quiescent();
        CHECK(hipStreamSynchronize(up) == hipSuccess, "hipStreamSynchronize failed");
        for (int j = 0; j < 2; ++j) {
            const int bad = first_bad_row(static_cast<const uint8_t*>(job[j].dst), LR_PIX_F32, k.w, job[j].fidx, 0, k.h + j * 3);
            CHECK(bad < 0, "crew %s: row %d of job %d did not arrive", k.name, bad, j);
            (void)hipFree(job[j].dst);
            (void)hipHostFree(job[j].stage);
            job[j].src.release();
        }
        std::printf("case crew %s helpers=%d trace=%s\n", k.name, k.helpers, trace.c_str());
    }
    (void)hipStreamDestroy(up);
    lr_context_destroy(c);
}

// ---- batches of host frames -------------------------------------------------------------------------------------------------

enum Layout { kOneBlockOdd, kStrideAbove, kMixedPinned, kOneTwice };
const char* layout_name(int l) { return l == kOneBlockOdd ? "one-block-odd-offset" : l == kStrideAbove ? "stride-above-w" : l == kMixedPinned ? "mixed-pinned" : "one-twice"; }

struct Batch {
    std::vector<HostFrame> frames;  // views into `block` or page-locked allocations of their own
    std::vector<const float*> ptrs;
    std::vector<int> fidx, want;    // want[i]: launches that must find frame i
    void* block = nullptr;
    int w = 0, h = 0, stride = 0;
    void fill() {
        for (size_t i = 0; i < frames.size(); ++i) frames[i].fill(fidx[i]);
    }
    void poison() {
        for (auto& f : frames) f.poison();
    }
    void release() {
        for (auto& f : frames) f.release();
        std::free(block);
    }
};
Batch make_batch(int layout, int n, int w, int h) {
    Batch b;
    b.w = w;
    b.h = h;
    b.stride = layout == kStrideAbove ? w + 13 : w;
    const size_t frame_bytes = (size_t)h * b.stride * 4;
    const size_t off = 4097;  // an odd byte offset; the frames follow each other and share pages
    b.block = std::malloc(off + frame_bytes * n + 64);
    b.want.assign(16, 0);
    for (int i = 0; i < n; ++i) {
        HostFrame f;
        if (layout == kMixedPinned && (i % 2) == 0) {
            f = make_frame(LR_PIX_F32, w, h, b.stride, true);
        } else {
            f.fmt = LR_PIX_F32;
            f.w = w;
            f.h = h;
            f.stride = b.stride;
            f.mem = static_cast<uint8_t*>(b.block) + off + frame_bytes * i;
        }
        b.frames.push_back(f);
        b.fidx.push_back(i);
    }
    for (int i = 0; i < n; ++i) {
        const int src = (layout == kOneTwice && i == n - 3) ? 2 : i;  // one frame given twice
        b.ptrs.push_back(static_cast<const float*>(b.frames[(size_t)src].arg()));
        b.want[(size_t)b.fidx[(size_t)src]] += 1;
    }
    return b;
}

// one call; fail_memcpy / fail_register: the model's switches (0: none).  Returns the call's status.
int run_batch(lr_context* c, const char* name, int layout, int n, int w, int h, int lanes, int refuse_every, int fail_memcpy, int fail_register) {
    Batch b = make_batch(layout, n, w, h);
    b.fill();
    Expect& e = g_expect;
    e.fmt = LR_PIX_F32;
    e.w = w;
    e.h = h;
    e.reset(2);
    lr_set_batch_streams(c, lanes);
    model_hip_reset_counters();
    model_hip_refuse_register_every(refuse_every);
    model_hip_fail_memcpy_async_at(fail_memcpy);
    model_hip_fail_host_register_at(fail_register);
    std::vector<int> n_lines((size_t)n, -1);
    std::vector<LineSegment> lines((size_t)n * 4);
    const int rc = lr_find_line_segment_groups_batch_host_ptrs(c, b.ptrs.data(), n, w, h, b.stride, 10.f, 0, 4, lines.data(), 4, n_lines.data(), nullptr, nullptr);
    model_hip_fail_memcpy_async_at(0);
    model_hip_fail_host_register_at(0);
    model_hip_refuse_register_every(0);
    const std::string trace = trace_string();
    const int registered = model_hip_registered_total();
    // (after a call that failed as well: it must leave nothing pending on the caller's memory, and nothing registered)
    model_hip_check_quiescent();
    CHECK(model_hip_registered_ranges() == 0, "%s: %d ranges are still registered after the call", name, model_hip_registered_ranges());
    b.poison();
    model_hip_drain();
    e.mode.store(0);
    int checked = 0;
    for (int i = 0; i < 16; ++i) {
        checked += e.frame_hits[i].load();
        if (rc == 0) CHECK(e.frame_hits[i].load() == b.want[(size_t)i], "%s: frame %d was filtered %d times, not %d", name, i, e.frame_hits[i].load(), b.want[(size_t)i]);
    }
    if (fail_memcpy) CHECK(rc != 0, "%s: the call succeeded although a transfer failed", name);
    else CHECK(rc == 0, "%s: the call failed: %s", name, lr_last_error());
    std::printf("case %s layout=%s batch=%d w=%d h=%d lanes=%d refuse=%d fail_memcpy=%d fail_register=%d rc=%d checked=%d rows=%d registered=%d trace=%s\n", name, layout_name(layout), n,
                w, h, lanes, refuse_every, fail_memcpy, fail_register, rc, checked, e.rows.load(), registered, trace.c_str());
    b.release();
    return rc;
}

void group_batch() {
    for (int layout = 0; layout < 4; ++layout) {
        lr_context* c = nullptr;
        if (lr_context_create(0, &c)) std::abort();
        for (int lanes : {1, 2, 4}) {
            run_batch(c, "batch", layout, 12, 250, 120, lanes, 0, 0, 0);
            run_batch(c, "batch", layout, 12, 1000, 300, lanes, lanes == 2 ? 3 : 0, 0, 0);
        }
        lr_context_destroy(c);
    }
}

// failure paths: the n-th hipMemcpyAsync or hipHostRegister of a call fails; the next call on the same context is correct
void group_batchfail() {
    for (int layout : {(int)kOneBlockOdd, (int)kMixedPinned}) {
        lr_context* c = nullptr;
        if (lr_context_create(0, &c)) std::abort();
        run_batch(c, "batchfail-warm", layout, 12, 1000, 300, 1, 0, 0, 0);  // (the lane's workspace exists: its first frame is quick)
        for (int nth : {1, 4, 9}) {
            run_batch(c, "batchfail", layout, 12, 1000, 300, nth == 9 ? 2 : 1, 0, nth, 0);
            run_batch(c, "batchfail-next", layout, 12, 1000, 300, 2, 0, 0, 0);
        }
        run_batch(c, "batchfail-register", layout, 12, 1000, 300, 2, 0, 0, 2);
        run_batch(c, "batchfail-next", layout, 12, 1000, 300, 2, 0, 0, 0);
        lr_context_destroy(c);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: upload_order <eager|lazy|threaded> <seed> <group>[,<group>...]\n");
        return 2;
    }
    const std::string sched = argv[1];
    const int schedule = sched == "eager" ? MODEL_HIP_EAGER : sched == "lazy" ? MODEL_HIP_LAZY : MODEL_HIP_THREADED;
    // The flood's just-in-time rounds poll a page-locked word that a kernel writes: a host loop that no synchronising call
    // ends, so the lazy schedule has nothing that would ever run it.  Blind rounds instead (the library's own knob).
    setenv("LIBRECTIFY_FLOOD_JIT", "0", 1);
    model_hip_init(schedule, std::strtoull(argv[2], nullptr, 0), 40);
    std::vector<size_t> sizes(kFilterArgs, sizeof(void*));
    sizes[1] = sizes[2] = sizes[3] = sizes[11] = sizes[12] = sizes[13] = sizeof(int);
    sizes[4] = (4 + 2 * (size_t)kBins) * sizeof(float);  // FilterTaps: d1, d2, g1, g2, st[kBins], ct[kBins]
    model_hip_hook("filter_lanes_kernel", kFilterArgs, sizes.data(), filter_run, filter_writes, nullptr);
    std::string groups = argv[3];
    for (size_t pos = 0; pos <= groups.size();) {
        const size_t end = std::min(groups.find(',', pos), groups.size());
        const std::string g = groups.substr(pos, end - pos);
        pos = end + 1;
        if (g == "single") group_single(false);
        else if (g == "slow") group_single(true);
        else if (g == "seq") group_sequence();
        else if (g == "consecutive") group_consecutive();
        else if (g == "big") group_big();
        else if (g == "crew") group_crew();
        else if (g == "batch") group_batch();
        else if (g == "batchfail") group_batchfail();
        else {
            std::fprintf(stderr, "unknown group %s\n", g.c_str());
            return 2;
        }
    }
    model_hip_check_leaks();
    const int n = model_hip_error_count();
    model_hip_print_errors();
    std::printf(n ? "FAILED %d errors\n" : "ok\n", n);
    return n ? 1 : 0;
}
