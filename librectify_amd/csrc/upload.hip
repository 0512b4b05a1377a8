// Host frames on their way to the device: the copy stream, the page-lock test, the staging threads (bound to the device's
// NUMA node) and their crew, the two frame slots of single calls and the ring of batch calls.
#include "host.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <pthread.h>
#include <sched.h>
#if defined(__SSE2__)
#include <immintrin.h>
#endif

// Copy into a page-locked staging buffer with non-temporal stores (SSE2, part of every x86-64): a plain memcpy reads the
// destination's lines before it overwrites them, and the staging buffers are read next by the DMA engine, not by a core.
// Less host-memory traffic beside the transfers, which read the same memory.
static inline void stage_copy(void* dst, const void* src, size_t n) {
#if defined(__SSE2__)
    char* d = static_cast<char*>(dst);
    const char* s_ = static_cast<const char*>(src);
    if (n < 4096) {
        std::memcpy(d, s_, n);
        return;
    }
    const size_t head = (16u - (reinterpret_cast<uintptr_t>(d) & 15u)) & 15u;
    if (head) {
        std::memcpy(d, s_, head);
        d += head;
        s_ += head;
        n -= head;
    }
    size_t blocks = n / 64;
    while (blocks--) {
        const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s_));
        const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s_ + 16));
        const __m128i c2 = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s_ + 32));
        const __m128i e = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s_ + 48));
        _mm_stream_si128(reinterpret_cast<__m128i*>(d), a);
        _mm_stream_si128(reinterpret_cast<__m128i*>(d + 16), b);
        _mm_stream_si128(reinterpret_cast<__m128i*>(d + 32), c2);
        _mm_stream_si128(reinterpret_cast<__m128i*>(d + 48), e);
        s_ += 64;
        d += 64;
    }
    n &= 63;
    if (n) std::memcpy(d, s_, n);
    _mm_sfence();
#else
    std::memcpy(dst, src, n);
#endif
}

namespace lramd {

bool is_page_locked(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // an ordinary malloc'ed pointer: not an error of ours
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

int staging_threads(int num_threads, size_t frame_bytes) {
    // reference threading.h:24-27: t < 0 is the serial mode, otherwise min(t, available) threads (t = 0 is
    // ill-defined there: one thread here).  Eight threads saturate the copy into the staging buffer of a 4K frame; a frame
    // of more than 64 MB (8192^2: 268 MB) is one long copy in front of one long transfer, and sixteen get its first bands
    // onto the link sooner (round 4).
    if (num_threads <= 1) return 1;
    const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
    return std::min(std::min(num_threads, hw), frame_bytes > ((size_t)64 << 20) ? 16 : 8);
}

// The host cores next to a device: those of the NUMA node its PCI function sits on (sysfs), as far as this process may use
// them; empty if unknown.  Staging helpers bind themselves there: copies by cores of the other socket reach 41 GB/s where
// the same copies by cores of the device's own node keep the link at 54 (tools/ubench/h2d_placement.hip,
// profiles/r04_h2d_paths.txt).
// (Returned by value, copied under the lock: a reference into the cache dangled when another thread asked for a device with
// a higher index and the outer vector grew -- the start-up pattern of the multi-device batch call.)
static std::vector<int> device_node_cpus(int device) {
    static std::mutex mu;
    static std::map<int, std::vector<int>> cache;
    std::lock_guard<std::mutex> lk(mu);
    const auto found = cache.find(device);
    if (found != cache.end()) return found->second;
    std::vector<int>& out = cache[device];
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) return out;
    for (char* p = bus; *p; ++p) *p = (char)std::tolower((unsigned char)*p);
    int node = -1;
    if (FILE* f = std::fopen((std::string("/sys/bus/pci/devices/") + bus + "/numa_node").c_str(), "r")) {
        if (std::fscanf(f, "%d", &node) != 1) node = -1;
        std::fclose(f);
    }
    if (node < 0) return out;
    char line[4096] = {0};
    if (FILE* f = std::fopen(("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist").c_str(), "r")) {
        if (!std::fgets(line, (int)sizeof(line), f)) line[0] = 0;
        std::fclose(f);
    }
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return out;
    for (const char* p = line; *p;) {  // "0-63,128-191"
        char* e = nullptr;
        const long a = std::strtol(p, &e, 10);
        if (e == p) break;
        long b = a;
        if (*e == '-') b = std::strtol(e + 1, &e, 10);
        for (long cpu = a; cpu <= b && cpu < CPU_SETSIZE; ++cpu)
            if (CPU_ISSET((int)cpu, &allowed)) out.push_back((int)cpu);
        p = (*e == ',') ? e + 1 : e;
        if (*e != ',') break;
    }
    return out;
}

void bind_this_thread_near(int device) {
    const std::vector<int> cpus = device_node_cpus(device);
    if (cpus.empty()) return;
    cpu_set_t set;
    CPU_ZERO(&set);
    for (int c : cpus) CPU_SET(c, &set);
    (void)pthread_setaffinity_np(pthread_self(), sizeof(set), &set);  // (best effort)
}

// The copy stream of a context is made when it first uploads a frame: HIP maps streams onto a few hardware queues
// (GPU_MAX_HW_QUEUES), commands of streams that share one run in order, and a batch's lanes never upload -- their
// copy streams would only take queues away from the one that does (transfers were seen waiting 4-6 ms behind another
// lane's kernels).
int ensure_copy_stream(lr_context* c) {
    if (c->copy_stream) return 0;
    LR_HIP(hipSetDevice(c->device));
    // ... and at a higher priority than the lanes' streams: streams of different priorities do not share a queue
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
    if (hi == lo) LR_HIP(hipStreamCreateWithFlags(c->copy_stream.put(), hipStreamNonBlocking));
    else LR_HIP(hipStreamCreateWithPriority(c->copy_stream.put(), hipStreamNonBlocking, hi));
    return 0;
}

// Rows of a host frame (|stride| >= w; a negative stride addresses the same rows from the other end, reference
// image.cpp:11-19) into a device buffer of w x h pixels of `bpp` bytes, packed, on stream `up`.  Page-locked memory goes as it lies; pageable
// memory goes through the page-locked buffer `stage` in 4 MB bands, copied by up to `num_threads` threads, each band's
// transfer enqueued as soon as it is staged.  Nothing here waits for the transfers.
int upload_rows(lr_context* c, void* dst_, void* stage_, const void* buffer_, int w, int h, int stride, int bpp, int num_threads,
                       hipStream_t up) {
    uint8_t* dst = static_cast<uint8_t*>(dst_);
    uint8_t* stage = static_cast<uint8_t*>(stage_);
    const uint8_t* buffer = static_cast<const uint8_t*>(buffer_);
    if (stride < 0) {
        buffer = buffer + (std::ptrdiff_t)(h - 1) * stride * bpp;
        stride = -stride;
    }
    const size_t row_bytes = (size_t)w * bpp, pitch = (size_t)stride * bpp;
    if (stage == nullptr) {
        if (stride == w)  // one linear transfer: a pitched copy of the same bytes goes row by row
            LR_HIP(hipMemcpyAsync(dst, buffer, row_bytes * h, hipMemcpyHostToDevice, up));
        else
            LR_HIP(hipMemcpy2DAsync(dst, row_bytes, buffer, pitch, row_bytes, (size_t)h, hipMemcpyHostToDevice, up));
        return 0;
    }
    const int rows_per_band = (int)std::max<size_t>(1, ((size_t)4 << 20) / row_bytes);
    const int n_bands = (h + rows_per_band - 1) / rows_per_band;
    const int T = std::min(staging_threads(num_threads), n_bands);
    std::vector<int> rc(T, 0);
    auto run = [&](int t) {
        if (t > 0 && hipSetDevice(c->device) != hipSuccess) {
            rc[t] = 1;
            return;
        }
        for (int k = t; k < n_bands; k += T) {
            const int r0 = k * rows_per_band, r1 = std::min(h, r0 + rows_per_band);
            if (stride == w) {
                std::memcpy(stage + (size_t)r0 * row_bytes, buffer + (size_t)r0 * pitch, (size_t)(r1 - r0) * row_bytes);
            } else {
                for (int r = r0; r < r1; ++r) std::memcpy(stage + (size_t)r * row_bytes, buffer + (size_t)r * pitch, row_bytes);
            }
            if (hipMemcpyAsync(dst + (size_t)r0 * row_bytes, stage + (size_t)r0 * row_bytes, (size_t)(r1 - r0) * row_bytes,
                               hipMemcpyHostToDevice, up) != hipSuccess)
                rc[t] = 1;
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(run, t);
    run(0);
    for (auto& x : th) x.join();
    for (int t = 0; t < T; ++t)
        if (rc[t]) {
            (void)hipGetLastError();
            set_error("upload: staging copy failed");
            return 1;
        }
    return 0;
}

// One piece of job `gen`, if there is one left: true if a piece was claimed (and copied).  The descriptor is read only
// AFTER the claim: a claimed piece keeps bands_left above zero, the uploader is then still inside finish() of this very
// job, and nobody writes either descriptor (begin() of the next job comes after that finish(); the job after it, which
// reuses this slot, after the next one's).  A helper that is late for a job finds another job's number in `next` /
// `total` and leaves without having looked at anything else.
bool StagingCrew::work_one(uint32_t gen) {
    for (;;) {
        uint64_t x = next.load(std::memory_order_acquire);
        const uint64_t t = total.load(std::memory_order_acquire);
        if ((uint32_t)(x >> 32) != gen || (uint32_t)(t >> 32) != gen || (uint32_t)x >= (uint32_t)t) return false;
        if (!next.compare_exchange_weak(x, x + 1, std::memory_order_acq_rel)) continue;
        const Job& j = jobs[gen & 1u];
        const size_t row_bytes = j.row_bytes;
        const int kP = j.pieces;
        const int rows_per_piece = (j.rows_per_band + kP - 1) / kP;
        const int k = (int)(uint32_t)x / kP, piece = (int)(uint32_t)x % kP;
        const int b0 = k * j.rows_per_band, b1 = std::min(j.h, b0 + j.rows_per_band);
        const int r0 = std::min(b1, b0 + piece * rows_per_piece), r1 = std::min(b1, r0 + rows_per_piece);
        if (r1 > r0) {
            if (j.src_pitch == row_bytes) {
                stage_copy(j.stage + (size_t)r0 * row_bytes, j.src + (size_t)r0 * j.src_pitch, (size_t)(r1 - r0) * row_bytes);
            } else {
                for (int r = r0; r < r1; ++r) stage_copy(j.stage + (size_t)r * row_bytes, j.src + (size_t)r * j.src_pitch, row_bytes);
            }
        }
        if (pieces_left[gen & 1u][k].fetch_sub(1, std::memory_order_acq_rel) != 1) return true;  // not the band's last piece
        bool ok = hipMemcpyAsync(j.dst + (size_t)b0 * row_bytes, j.stage + (size_t)b0 * row_bytes, (size_t)(b1 - b0) * row_bytes,
                                 hipMemcpyHostToDevice, j.up) == hipSuccess;
        if (ok && j.band_ev) ok = hipEventRecord(j.band_ev[k], j.up) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            failed.store(1);
        }
        if (j.ready) j.ready[k].store(ok ? 1 : -1, std::memory_order_release);
        bands_left.fetch_sub(1, std::memory_order_acq_rel);  // (last: the descriptor is not touched after this)
        return true;
    }
}

void StagingCrew::start(lr_context* ctx, int helpers) {
    c = ctx;
    live.store(helpers, std::memory_order_relaxed);
    for (int t = 0; t < helpers; ++t)
        th.emplace_back([this]() {
            if (hipSetDevice(c->device) != hipSuccess) {  // a helper less; whoever waits for bands works on them itself
                (void)hipGetLastError();
                live.fetch_sub(1, std::memory_order_acq_rel);
                return;
            }
            bind_this_thread_near(c->device);
            uint32_t last = 0;
            int spins = 0;
            while (!quit.load(std::memory_order_acquire)) {
                const uint32_t g = job.load(std::memory_order_seq_cst);
                if (g == last) {
                    if (++spins < 512) {
                        std::this_thread::yield();
                        continue;
                    }
                    std::unique_lock<std::mutex> lk(mu);
                    sleepers.fetch_add(1, std::memory_order_seq_cst);
                    cv.wait(lk, [&]() { return quit.load(std::memory_order_acquire) || job.load(std::memory_order_seq_cst) != last; });
                    sleepers.fetch_sub(1, std::memory_order_seq_cst);
                    spins = 0;
                    continue;
                }
                spins = 0;
                last = g;
                work(g);
            }
        });
}

// the two halves of run(): publish the job (the helpers start on it), and wait for its last band
uint32_t StagingCrew::begin(void* dst_, void* stage_, const void* buffer_, int w_, int h_, int stride_, int bpp_, hipStream_t up_,
                            const Event* band_ev_, std::atomic<int>* ready_, size_t band_bytes, int pieces_) {
    const uint8_t* buffer = static_cast<const uint8_t*>(buffer_);
    if (stride_ < 0) {
        buffer = buffer + (std::ptrdiff_t)(h_ - 1) * stride_ * bpp_;
        stride_ = -stride_;
    }
    const uint32_t g = job.load(std::memory_order_relaxed) + 1u;
    Job& j = jobs[g & 1u];
    j.dst = static_cast<uint8_t*>(dst_);
    j.stage = static_cast<uint8_t*>(stage_);
    j.src = buffer;
    j.row_bytes = (size_t)w_ * bpp_;
    j.src_pitch = (size_t)stride_ * bpp_;
    j.h = h_;
    j.up = up_;
    j.band_ev = band_ev_;
    j.ready = ready_;
    j.rows_per_band = (int)std::max<size_t>(1, band_bytes / j.row_bytes);
    j.n_bands = (h_ + j.rows_per_band - 1) / j.rows_per_band;
    if (j.n_bands > kMaxBands) {  // (a frame of more than 1 GiB: fewer, larger bands)
        j.rows_per_band = (h_ + kMaxBands - 1) / kMaxBands;
        j.n_bands = (h_ + j.rows_per_band - 1) / j.rows_per_band;
    }
    j.pieces = pieces_ > 0 ? std::min(pieces_, kPieces) : (band_ev_ ? kPieces : 1);  // (band events = the single-frame path)
    for (int k = 0; k < j.n_bands; ++k) pieces_left[g & 1u][k].store(j.pieces, std::memory_order_relaxed);
    failed.store(0, std::memory_order_relaxed);  // (per frame: every band of the previous one has been accounted for)
    bands_left.store(j.n_bands, std::memory_order_relaxed);
    total.store(((uint64_t)g << 32) | (uint32_t)(j.n_bands * j.pieces), std::memory_order_release);
    next.store((uint64_t)g << 32, std::memory_order_release);
    job.store(g, std::memory_order_seq_cst);
    if (sleepers.load(std::memory_order_seq_cst) > 0) {  // (the helpers are woken only if somebody sleeps)
        { std::lock_guard<std::mutex> lk(mu); }
        cv.notify_all();
    }
    return g;
}

int StagingCrew::finish() {
    int spins = 0;
    while (bands_left.load(std::memory_order_acquire) > 0) {
        if (live.load(std::memory_order_acquire) == 0 && work_one(job.load(std::memory_order_relaxed))) continue;
        if (++spins < 256) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(10));
    }
    return failed.load() ? 1 : 0;
}

StagingCrew::~StagingCrew() {
    quit.store(true, std::memory_order_seq_cst);
    { std::lock_guard<std::mutex> lk(mu); }
    cv.notify_all();
    for (auto& t : th) t.join();
}

// Device slot `slot` of at least npix floats (a frame of any format fits) and, for a pageable source, its page-locked
// staging buffer (*stage; nullptr for a source that is page-locked already).  Growing either waits for whatever still uses the old one.
int ensure_frame_slot(lr_context* c, int slot, size_t npix, bool pageable, float** stage) {
    hipStream_t up = c->copy_stream;
    if (c->frames.slot[slot].cap() < npix) {
        LR_HIP(hipStreamSynchronize(c->stream));
        LR_HIP(hipStreamSynchronize(up));
        if (c->frames.slot[slot].grow(npix)) return 1;
    }
    *stage = nullptr;
    if (!pageable) return 0;
    if (c->frames.stage[slot].cap() < npix) {
        LR_HIP(hipStreamSynchronize(up));
        if (c->frames.stage[slot].grow(npix)) return 1;
    }
    // the DMA that last read this staging buffer has long finished (its frame has been processed), but make sure
    LR_HIP(hipEventSynchronize(c->ev_up[slot]));
    *stage = c->frames.stage[slot];
    return 0;
}

int ctx_upload_frame(lr_context* c, int slot, const float* buffer, int w, int h, int stride, int num_threads) {
    LR_HIP(hipSetDevice(c->device));
    if (w < 1 || h < 1 || buffer == nullptr) {
        set_error("upload: bad frame");
        return 1;
    }
    if ((stride < 0 ? -stride : stride) < w) {
        set_error("upload: |stride| smaller than the width");
        return 1;
    }
    if (ensure_copy_stream(c)) return 1;
    float* stage = nullptr;
    if (ensure_frame_slot(c, slot, (size_t)w * h, !is_page_locked(buffer), &stage)) return 1;
    if (upload_rows(c, c->frames.slot[slot], stage, buffer, w, h, stride, (int)sizeof(float), num_threads, c->copy_stream)) return 1;
    LR_HIP(hipEventRecord(c->ev_up[slot], c->copy_stream));
    return 0;
}

// The ring of a batch call on host frames (UploadRing): R device frames, an event each, and -- if any frame is pageable --
// R page-locked staging buffers.
int ensure_upload_ring(lr_context* c, int R, size_t npix, bool staging) {
    if (ensure_copy_stream(c)) return 1;
    UploadRing& r = c->ring;
    if ((int)r.img.size() < R || r.cap_pix < npix) {
        LR_HIP(hipStreamSynchronize(c->copy_stream));
        r.cap_pix = 0;
        if ((int)r.img.size() < R) r.img.resize((size_t)R);
        // (uncached or fine-grained memory for these buffers -- so that the incoming frames bypass the caches -- was measured
        // and not kept: profiles/r05_dma_interference.txt)
        for (auto& b : r.img)
            if (b.grow(npix)) return 1;
        r.cap_pix = npix;
    }
    static const bool lane_debug = std::getenv("LIBRECTIFY_LANE_DEBUG") != nullptr || std::getenv("LIBRECTIFY_BATCH_STATS") != nullptr;  // (they time the uploads)
    while (c->ring_ev.size() < r.img.size()) {
        Event e;
        if (e.ensure(lane_debug ? hipEventDefault : hipEventDisableTiming)) return 1;
        c->ring_ev.push_back(std::move(e));
    }
    if (staging && (r.stage.size() < r.img.size() || r.stage_cap_pix < npix)) {
        LR_HIP(hipStreamSynchronize(c->copy_stream));
        r.stage_cap_pix = 0;
        r.stage.resize(r.img.size());
        for (auto& b : r.stage)
            if (b.grow(npix)) return 1;
        r.stage_cap_pix = npix;
    }
    return 0;
}

static bool batch_stats_on() {
    static const bool on = std::getenv("LIBRECTIFY_BATCH_STATS") != nullptr;
    return on;
}
static bool lane_debug_on() {
    static const bool on = std::getenv("LIBRECTIFY_LANE_DEBUG") != nullptr;
    return on;
}
static void nap(int& spins) {  // a wait that is usually short: yield first, then sleep
    if (++spins < 64) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(30));
}

BatchUploader::BatchUploader(lr_context* ctx, const void* const* frames_, int batch_, int w_, int h_, int stride_, int bpp_, int lanes_,
                             int num_threads_)
    : c(ctx), frames(reinterpret_cast<const uint8_t* const*>(frames_)), batch(batch_), w(w_), h(h_), stride(stride_), bpp((size_t)bpp_),
      row_bytes((size_t)w_ * (size_t)bpp_), pitch((size_t)(stride_ < 0 ? -stride_ : stride_) * (size_t)bpp_), lanes(lanes_),
      num_threads(num_threads_) {}

int BatchUploader::check() const {
    if (w < 1 || h < 1) {
        set_error("upload: bad frame");
        return 1;
    }
    if ((stride < 0 ? -stride : stride) < w) {
        set_error("upload: |stride| smaller than the width");
        return 1;
    }
    for (int i = 0; i < batch; ++i) {
        if (frames[i] == nullptr) {
            set_error("upload: bad frame");
            return 1;
        }
    }
    return 0;
}

int BatchUploader::start() {
    // (asked once, before this call page-locks anything: a frame that overlaps one the call has registered is still
    // the caller's pageable memory)
    locked.assign((size_t)batch, 0);
    for (int i = 0; i < batch; ++i) {
        locked[(size_t)i] = is_page_locked(frames[i]);
        any_pageable = any_pageable || !locked[(size_t)i];
    }
    // slots beyond one per lane: what the link may be ahead.  Six absorb the moments when several lanes finish
    // together (pageable 4K frames: 7.8 Gpix/s with three, 8.0 with six or ten); at most 2 GiB of frames, though.
    static const int extra_env = std::getenv("LIBRECTIFY_RING_EXTRA") ? std::max(1, std::atoi(std::getenv("LIBRECTIFY_RING_EXTRA"))) : 0;
    const size_t npix = (size_t)w * h;
    const int by_bytes = (int)std::min<size_t>(64, ((size_t)2 << 30) / (npix * bpp));
    R = extra_env ? lanes + extra_env : std::max(lanes + 1, std::min(lanes + 6, by_bytes));
    R = std::min(batch, R);
    if (ensure_upload_ring(c, R, npix, any_pageable)) return 1;
    enq = std::vector<std::atomic<int>>((size_t)batch);
    slot_busy = std::vector<std::atomic<int>>((size_t)R);
    slot_edges.assign((size_t)R, SlotEdges());
    for (auto& a : enq) a.store(0, std::memory_order_relaxed);
    for (auto& a : slot_busy) a.store(0, std::memory_order_relaxed);
    // Pageable caller frames are page-locked WHERE THEY LIE (hipHostRegister) by a few helper threads running ahead of the
    // uploader, sent by DMA from there, and released when the call is over -- no staging copy, i.e. one pass through host DRAM
    // instead of three.
    // No page is ever registered twice: a frame's range is rounded INWARDS to whole pages, and the rows that reach into the
    // pages it shares with its neighbours -- at most 4 KB and a row at each end -- go through the slot's staging buffer
    // instead (reg_plan.h: RegPlan, with the reasons): the uploader copies them there and sends the rows in between in ONE
    // transfer, as ever; the frame's LANE fetches the few staged rows on its own stream before its filter, so the link's
    // queue carries one command a frame (three -- head, middle, tail on the copy stream -- cost the fp32 headline 3 %).
    // What registration costs instead of the copy is the pinning itself (page-table work, ~1.3 ms a 4K frame on one thread).
    // Round 5: 10.93 -> 11.38 Gpix/s on the headline leg with four helpers, the 1080p batch unchanged;
    // the default since.  A frame whose registration is refused (memory somebody else has registered, a mapping that cannot be
    // pinned) goes through the staging copy as before; LIBRECTIFY_REGISTER_FRAMES=0 sends every frame that way,
    // =<n> sets the helpers (profiles/r05_h2d_register.txt).
    static const int register_threads = std::getenv("LIBRECTIFY_REGISTER_FRAMES") ? std::max(0, std::atoi(std::getenv("LIBRECTIFY_REGISTER_FRAMES"))) : 4;
    // (a host on which pinning is slow -- measured on this box: 1.3 ms a 4K frame on one thread, 25 GB/s; the guard trips below
    // 6 GB/s -- gets the staging copy back: for the rest of the call, and for the context's next 32 batch calls before it tries again)
    if (c->register_slow_calls > 0) --c->register_slow_calls;
    reg_frames = register_threads > 0 && any_pageable && stride >= w && c->register_slow_calls == 0;
    if (reg_frames) {
        std::vector<char> may((size_t)batch);
        for (int i = 0; i < batch; ++i) may[(size_t)i] = !locked[(size_t)i] && !c->batch_no_register;
        plan = plan_registrations(reinterpret_cast<const void* const*>(frames), batch, h, pitch, row_bytes, 4096, may.data());
        reg_ready = std::vector<std::atomic<int>>((size_t)batch);
        for (auto& a : reg_ready) a.store(0, std::memory_order_relaxed);
    }
    started = true;
    if (reg_frames)
        for (int t = 0; t < register_threads; ++t) helpers.th.emplace_back([this]() { register_frames(); });
    t_call0 = now_ms();
    uploader.th.emplace_back([this]() { upload_frames(); });
    return 0;
}

// a registration helper: the frames in order, each by whoever gets there first
void BatchUploader::register_frames() {
    (void)hipSetDevice(c->device);
    bind_this_thread_near(c->device);
    for (int i = reg_next.fetch_add(1, std::memory_order_relaxed); i < batch && !stop.load(std::memory_order_relaxed);
         i = reg_next.fetch_add(1, std::memory_order_relaxed)) {
        if (reg_slow.load(std::memory_order_relaxed) >= 2) break;  // (pinning is slow here: the uploader stages the rest)
        int expect = 0;
        if (!reg_ready[(size_t)i].compare_exchange_strong(expect, 3, std::memory_order_acq_rel)) continue;  // (the uploader has it)
        int ok = 2;
        const double t_r0 = now_ms();
        // (only the frames with a plan: whole pages of their own, apart from every earlier frame's)
        const RegPlan& p = plan[(size_t)i];
        if (p.hi > p.lo)
            ok = hipHostRegister(reinterpret_cast<void*>(p.lo), p.hi - p.lo, hipHostRegisterDefault) == hipSuccess ? 1 : 2;
        if (ok == 2) (void)hipGetLastError();
        if (ok == 1 && (now_ms() - t_r0) * 6.0e6 > (double)(p.hi - p.lo)) reg_slow.fetch_add(1, std::memory_order_relaxed);
        reg_ready[(size_t)i].store(ok, std::memory_order_release);
    }
}

// the uploader thread: every frame, in order, into a free slot
void BatchUploader::upload_frames() {
    if (hipSetDevice(c->device) != hipSuccess) {
        up_err = "hipSetDevice failed";
        stop.store(1);
        return;
    }
    if (any_pageable) bind_this_thread_near(c->device);  // (this thread stages too; it is the library's own)
    StagingCrew crew;
    if (any_pageable) crew.start(c, staging_threads(num_threads, (size_t)w * h * bpp) - 1);
    for (int i = 0; i < batch; ++i) {
        int slot = -1, spins = 0;
        const double t_w0 = batch_stats_on() ? now_ms() : 0.0;
        // a slot whose frame is done (its transfer and its staging buffer are then free as well)
        while (slot < 0 && !stop.load(std::memory_order_relaxed)) {
            for (int k = 0; k < R && slot < 0; ++k)
                if (!slot_busy[(size_t)k].load(std::memory_order_acquire)) slot = k;
            if (slot < 0) nap(spins);
        }
        if (batch_stats_on()) up_wait_us.fetch_add((long long)((now_ms() - t_w0) * 1e3));
        if (stop.load(std::memory_order_relaxed)) return;
        slot_busy[(size_t)slot].store(1, std::memory_order_relaxed);
        if (reg_frames) {  // (the frame is being pinned by a helper: wait for it)
            int sp2 = 0;
            int expect = 0;
            if (!reg_ready[(size_t)i].compare_exchange_strong(expect, 2, std::memory_order_acq_rel))  // (else: nobody has it -- staged)
                while (reg_ready[(size_t)i].load(std::memory_order_acquire) == 3 && !stop.load(std::memory_order_relaxed)) nap(sp2);
        }
        const double t_u0 = now_ms();
        Event e_dbg;
        if (lane_debug_on() && e_dbg.create() == hipSuccess) (void)hipEventRecord(e_dbg, c->copy_stream);
        if (send_frame(crew, i, slot) || hipEventRecord(c->ring_ev[(size_t)slot], c->copy_stream) != hipSuccess) {
            up_err = get_error().empty() ? "upload failed" : get_error();
            stop.store(1);
            return;
        }
        enq[(size_t)i].store(slot + 1, std::memory_order_release);
        if (lane_debug_on()) {
            const double t_u1 = now_ms();
            float dma = 0.f;  // from the moment the link was free for this frame to the end of its last transfer
            if (e_dbg) {
                (void)hipEventSynchronize(c->ring_ev[(size_t)slot]);
                if (hipEventElapsedTime(&dma, e_dbg, c->ring_ev[(size_t)slot]) != hipSuccess) (void)hipGetLastError();
            }
            std::fprintf(stderr, "uploader frame %d: slot %d, waited %d naps for it, staged and enqueued in %.2f ms, on the link %.2f ms\n", i, slot, spins, t_u1 - t_u0, dma);
        }
    }
}

// frame i's transfer into `slot` on the copy stream: from where it lies if it is registered (its first and last rows into the
// slot's staging buffer, for the lane), else as it is (page-locked by the caller) or through the staging buffer
int BatchUploader::send_frame(StagingCrew& crew, int i, int slot) {
    constexpr size_t kBatchBand = (size_t)4 << 20;  // staging bands of the batch's pageable frames
    const bool registered = reg_frames && reg_ready[(size_t)i].load(std::memory_order_acquire) == 1;
    uint8_t* stage = locked[(size_t)i] ? nullptr : reinterpret_cast<uint8_t*>(c->ring.stage[(size_t)slot].get());
    uint8_t* dimg = reinterpret_cast<uint8_t*>(c->ring.img[(size_t)slot].get());
    if (!registered) {
        slot_edges[(size_t)slot].r_hi = 0;
        return stage ? crew.run(dimg, stage, frames[i], w, h, stride, (int)bpp, c->copy_stream, kBatchBand, 1)
                     : upload_rows(c, dimg, nullptr, frames[i], w, h, stride, (int)bpp, 1, c->copy_stream);
    }
    const RegPlan& p = plan[(size_t)i];
    const uint8_t* f = frames[i];
    // the rows that reach into a page shared with a neighbour: staged here, fetched by the lane
    for (int r = 0; r < p.r_lo; ++r) std::memcpy(stage + (size_t)r * row_bytes, f + (size_t)r * pitch, row_bytes);
    for (int r = p.r_hi; r < h; ++r) std::memcpy(stage + (size_t)r * row_bytes, f + (size_t)r * pitch, row_bytes);
    slot_edges[(size_t)slot].r_lo = p.r_lo;
    slot_edges[(size_t)slot].r_hi = p.r_hi;
    const hipError_t e = pitch == row_bytes
        ? hipMemcpyAsync(dimg + (size_t)p.r_lo * row_bytes, f + (size_t)p.r_lo * pitch, (size_t)(p.r_hi - p.r_lo) * row_bytes, hipMemcpyHostToDevice, c->copy_stream)
        : hipMemcpy2DAsync(dimg + (size_t)p.r_lo * row_bytes, row_bytes, f + (size_t)p.r_lo * pitch, pitch, row_bytes, (size_t)(p.r_hi - p.r_lo), hipMemcpyHostToDevice, c->copy_stream);
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    set_error("upload: transfer of a registered frame failed");
    return 1;
}

int BatchUploader::ready(int b, hipStream_t lane_stream, const void** img, int* slot_out) {
    *img = nullptr;
    int slot = -1, spins = 0;
    const double t_w0 = batch_stats_on() ? now_ms() : 0.0;
    while ((slot = enq[(size_t)b].load(std::memory_order_acquire) - 1) < 0 && !stop.load(std::memory_order_relaxed)) nap(spins);
    if (batch_stats_on()) lane_wait_us.fetch_add((long long)((now_ms() - t_w0) * 1e3));
    if (slot < 0) return 0;  // (whoever stopped the batch has the message)
    if (hipStreamWaitEvent(lane_stream, c->ring_ev[(size_t)slot], 0) != hipSuccess) {
        set_error("hipStreamWaitEvent failed");
        return 1;
    }
    uint8_t* dimg = reinterpret_cast<uint8_t*>(c->ring.img[(size_t)slot].get());
    const SlotEdges ed = slot_edges[(size_t)slot];
    if (ed.r_hi > 0) {  // (page-locked staging memory: two small transfers on the lane's own stream)
        const uint8_t* st = reinterpret_cast<const uint8_t*>(c->ring.stage[(size_t)slot].get());
        hipError_t e = hipSuccess;
        if (ed.r_lo > 0) e = hipMemcpyAsync(dimg, st, (size_t)ed.r_lo * row_bytes, hipMemcpyHostToDevice, lane_stream);
        if (e == hipSuccess && ed.r_hi < h)
            e = hipMemcpyAsync(dimg + (size_t)ed.r_hi * row_bytes, st + (size_t)ed.r_hi * row_bytes, (size_t)(h - ed.r_hi) * row_bytes, hipMemcpyHostToDevice, lane_stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("upload: transfer of a registered frame's first or last rows failed");
            return 1;
        }
    }
    *img = dimg;
    *slot_out = slot;
    return 0;
}

void BatchUploader::release(int slot, int b, const lr_context* l, int lane_index, double t_frame0) {
    if (batch_stats_on() && l->opt.timing_on) {  // (with the stage timers on: ev[0] is the frame's first kernel)
        float lead = 0.f;
        if (hipEventElapsedTime(&lead, c->ring_ev[(size_t)slot], l->ev[0]) == hipSuccess) {
            lead_sum_us.fetch_add((long long)(lead * 1e3));
            if (lead < 0.05f) late_frames.fetch_add(1);
        } else {
            (void)hipGetLastError();
        }
    }
    if (lane_debug_on()) {
        float lead = 0.f;  // how long the frame's upload had been finished when its first kernel started
        if (hipEventElapsedTime(&lead, c->ring_ev[(size_t)slot], l->ev[0]) != hipSuccess) (void)hipGetLastError();
        std::fprintf(stderr, "lane %d frame %d: enqueue %.2f ms, wait %.2f, whole call %.2f; device total %.2f; upload done %.2f ms before the first kernel\n",
                     lane_index, b, l->host_ms[0], l->host_ms[2], now_ms() - t_frame0, l->stage_ms[LR_T_TOTAL], lead);
    }
    slot_busy[(size_t)slot].store(0, std::memory_order_release);
}

void BatchUploader::close() {
    if (closed || !started) return;
    closed = true;
    uploader.join();
    if (batch_stats_on())
        std::fprintf(stderr, "batch of %d frames: %.2f ms; the uploader waited %.2f ms for free device frames; the %d lanes waited %.2f ms in all for their frame's transfer to be enqueued\n",
                     batch, now_ms() - t_call0, up_wait_us.load() * 1e-3, lanes, lane_wait_us.load() * 1e-3);
    if (batch_stats_on() && c->opt.timing_on)
        std::fprintf(stderr, "   a frame's transfer was finished %.3f ms (mean) before its first kernel started; %d of %d frames started within 0.05 ms of it (they waited for the link)\n",
                     lead_sum_us.load() * 1e-3 / batch, late_frames.load(), batch);
    (void)hipStreamSynchronize(c->copy_stream);  // (after an error: nothing may still read the caller's frames)
    helpers.join();
    if (reg_slow.load() >= 2) c->register_slow_calls = 32;
    if (reg_frames)  // the caller's frames go back to being pageable
        for (int i = 0; i < batch; ++i)
            if (reg_ready[(size_t)i].load(std::memory_order_acquire) == 1 && hipHostUnregister(reinterpret_cast<void*>(plan[(size_t)i].lo)) != hipSuccess)
                (void)hipGetLastError();  // (nothing to be done about it, and the caller's thread must not find it in its next call)
}

const std::string& BatchUploader::end() {
    close();
    return up_err;
}

BatchUploader::~BatchUploader() {
    stop.store(1);  // (no-one is left to take the frames if end() was not reached)
    close();
}

}  // namespace lramd
