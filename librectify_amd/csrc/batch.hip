// Many frames per call: the lanes of a batch call with their uploader, and the same over several devices.
#include "host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace lramd {

// The lanes of a batch call: the caller's context and S - 1 workers of its own (kept from call to call), set up for the
// length of the call; lanes_done gives the caller's context its own settings back.
static int lanes_begin(lr_context* c, int S, bool host_frames, std::vector<lr_context*>& lanes) {
    while ((int)c->workers.size() < S - 1) {
        lr_context* wc = nullptr;
        if (ctx_create(c->device, &wc)) return 1;
        c->workers.push_back(wc);
    }
    lanes.push_back(c);
    for (int i = 0; i < S - 1; ++i) lanes.push_back(c->workers[i]);
    for (lr_context* l : lanes) {
        l->opt = c->opt;  // (flood_staged: off unless lr_set_flood_staged: +6 % in round 1, -3 % now)
        // What only the lanes of a call run with (lane 0 is the caller's own context: it gets its own back below).
        // Re-walks from the logs: in the lanes only for walks of 32 tiles and more, behind a walk of 24 tiles.  With the
        // thresholds of a single call (16 / 12) round two's work on thousands of small logs is work on top, and S frames in
        // flight gain nothing from shorter rounds: 10.34 -> 10.2 Gpix/s; with these the long re-walks go and little is added:
        // 10.34 -> 10.55 (profiles/r04_flood_logs.txt section 14).
        l->flood_log_min = S == 1 ? 0 : 32;
        l->flood_log_walk = S == 1 ? 0 : 24;
        // ... and without the logs of second-tier walks: their kernel is a launch of 1 024 threads and 142 KB of LDS a
        // workgroup that has to find whole CUs beside the other lanes' kernels (2.7 launches a frame x 52 us in
        // profiles/r04_kernel_stats.csv): 10.67 -> 10.76 Gpix/s without (three repetitions each).
        l->flood_logbig_off = S > 1;
        // (a lane's thread has nothing else to do while its frame is in flight, but the call's staging threads need the cores:
        // a lane looks at the words every 20 microseconds instead of spinning -- the other lanes keep the GPU busy)
        // Measured (profiles/r04_flood_logs.txt, section 9): 9.93 -> 10.29 Gpix/s from pageable frames, 11.7 -> 12.1 from
        // resident ones -- a frame of a lane no longer drags 3-4 rounds of empty launches through its stream.
        l->flood_jit_sleep_us = S == 1 ? 0 : 20;
        // LIBRECTIFY_LANES_SLEEP: the lanes sleep on an event instead of spinning in hipStreamSynchronize, for hosts
        // short of cores (on the 16-core share of a one-GPU box: pageable frames equal, page-locked ones 5 % slower)
        static const bool sleep_env = std::getenv("LIBRECTIFY_LANES_SLEEP") != nullptr;
        l->sleep_in_wait = sleep_env && host_frames;
    }
    return 0;
}

static void lanes_done(lr_context* c, const std::vector<lr_context*>& lanes) {
    for (lr_context* l : lanes) l->sleep_in_wait = false;
    c->flood_logbig_off = false;
    c->flood_log_min = c->flood_log_walk = 0;
    c->flood_jit_sleep_us = 0;
}

// Batch of independent frames: the stages of one frame are latency-bound (flood rounds,
// host round trips), so several frames are kept in flight, one host thread + context + HIP stream each ("lanes");
// frames are handed out dynamically (they differ in cost, and with a fixed assignment the batch ends on one lane).
//
// Host-resident frames (h_frames != nullptr) are uploaded by ONE uploader thread, in frame order, on the caller's
// copy stream, into a pool of lanes + 6 device frames: frame i goes to whichever slot is free (frames finish out of
// order: a heavy frame runs as long as three light ones, and slot i mod R would make the link wait for it), so the link
// works up to six frames ahead of the lanes instead of starting a lane's next transfer only when the lane starts a
// frame.  (With one slot ahead per lane -- the first design -- a quarter to a third of the frames of a 4K
// batch still waited for their own upload, although the link was busy only two thirds of the time: 7.5 Gpix/s where
// the same batch without the transfers ran at 9.0; LIBRECTIFY_LANE_DEBUG prints each frame's lead.)  A lane makes its
// stream wait for the frame's transfer and never touches host memory itself.
// Frames are of one lr_pixel_format (`format`; strides and image_stride in pixels of it) and travel as bytes.
static int find_groups_batch(lr_context* c, const void* d_images_, int format, size_t image_stride, const void* const* h_frames_,
                             int batch, int w, int h, int stride, float min_length, bool refine, int num_threads,
                             LineSegment* out, int capacity, int* n_lines, const RectificationConfig* cfg,
                             ImageTransform* transforms) {
    if (batch <= 0) return 0;
    const uint8_t* d_images = static_cast<const uint8_t*>(d_images_);
    const uint8_t* const* h_frames = reinterpret_cast<const uint8_t* const*>(h_frames_);
    const size_t bpp = (size_t)pix_bytes(format);
    if (bpp == 0) {
        set_error("unknown pixel format of the frames");
        return 1;
    }
    const int S = std::max(1, std::min(c->opt.batch_streams, batch));
    std::vector<lr_context*> lanes;
    if (lanes_begin(c, S, h_frames != nullptr, lanes)) return 1;
    // ---- the upload ring
    const size_t npix = (size_t)w * h;
    int R = 0;
    bool any_pageable = false;
    std::vector<char> locked(h_frames ? (size_t)batch : 0, 0);  // frames in memory the CALLER has page-locked
    if (h_frames) {
        if (w < 1 || h < 1) {
            set_error("upload: bad frame");
            return 1;
        }
        if ((stride < 0 ? -stride : stride) < w) {
            set_error("upload: |stride| smaller than the width");
            return 1;
        }
        for (int i = 0; i < batch; ++i) {
            if (h_frames[i] == nullptr) {
                set_error("upload: bad frame");
                return 1;
            }
        }
        // (asked once, before this call page-locks anything: a frame that overlaps one the call has registered is still
        // the caller's pageable memory)
        for (int i = 0; i < batch; ++i) {
            locked[(size_t)i] = is_page_locked(h_frames[i]);
            any_pageable = any_pageable || !locked[(size_t)i];
        }
        // slots beyond one per lane: what the link may be ahead.  Six absorb the moments when several lanes finish
        // together (pageable 4K frames: 7.8 Gpix/s with three, 8.0 with six or ten); at most 2 GiB of frames, though.
        static const int extra_env = std::getenv("LIBRECTIFY_RING_EXTRA") ? std::max(1, std::atoi(std::getenv("LIBRECTIFY_RING_EXTRA"))) : 0;
        const int by_bytes = (int)std::min<size_t>(64, ((size_t)2 << 30) / (npix * bpp));
        R = extra_env ? S + extra_env : std::max(S + 1, std::min(S + 6, by_bytes));
        R = std::min(batch, R);
        if (ensure_upload_ring(c, R, npix, any_pageable)) return 1;
    }
    std::vector<std::atomic<int>> enq(h_frames ? (size_t)batch : 0);  // frame's slot + 1 once its transfer is enqueued
    std::vector<std::atomic<int>> slot_busy((size_t)R);
    struct SlotEdges {
        int r_lo = 0, r_hi = 0;  // rows [0, r_lo) and [r_hi, h) of the slot's frame wait in its staging buffer (r_hi = 0: none)
    };
    std::vector<SlotEdges> slot_edges((size_t)R);  // (written by the uploader before enq[], read by the frame's lane after it)
    for (auto& a : enq) a.store(0, std::memory_order_relaxed);
    for (auto& a : slot_busy) a.store(0, std::memory_order_relaxed);
    static const bool lane_debug = std::getenv("LIBRECTIFY_LANE_DEBUG") != nullptr;
    constexpr size_t kBatchBand = (size_t)4 << 20;  // staging bands of the batch's pageable frames
    std::atomic<int> abort_all{0};
    std::string up_err;
    auto nap = [](int& spins) {  // a wait that is usually short: yield first, then sleep
        if (++spins < 64) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(30));
    };
    // LIBRECTIFY_BATCH_STATS: who waited for whom in this call (host clocks only, nothing is synchronised for it)
    static const bool batch_stats = std::getenv("LIBRECTIFY_BATCH_STATS") != nullptr;
    std::atomic<long long> up_wait_us{0}, lane_wait_us{0}, lead_sum_us{0};
    std::atomic<int> late_frames{0};
    // Pageable caller frames are page-locked WHERE THEY LIE (hipHostRegister) by a few helper threads running ahead of the
    // uploader, sent by DMA from there, and released when the call is over -- no staging copy, i.e. one pass through host DRAM
    // instead of three.
    // No page is ever registered twice.  Frames of one array share the page at each end with their neighbours (an 8-bit
    // 1080p frame is 506.25 pages; an fp32 frame too, where the array does not start on a page), and the helpers register
    // and release frame by frame, concurrently.  So a frame's range is rounded INWARDS to whole pages: the pages two
    // frames share belong to neither, and the rows that reach into them -- at most 4 KB and a row at each end -- go through
    // the slot's staging buffer instead (RegPlan below): the uploader copies them there and sends the rows in between in ONE
    // transfer, as ever; the frame's LANE fetches the few staged rows on its own stream before its filter, so the link's
    // queue carries one command a frame (three -- head, middle, tail on the copy stream -- cost the fp32 headline 3 %).  A frame
    // whose pages overlap an earlier frame's (a frame listed twice, sliding windows over one array) is not registered at
    // all: it takes the staging copy, which only reads the caller's memory.
    // What registration costs instead of the copy is the pinning itself (page-table work, ~1.3 ms a 4K frame on one thread).
    // Round 5: 10.93 -> 11.38 Gpix/s on the headline leg with four helpers, the 1080p batch unchanged;
    // the default since.  A frame whose registration is refused (memory somebody else has registered, a mapping that cannot be
    // pinned) goes through the staging copy as before; LIBRECTIFY_REGISTER_FRAMES=0 sends every frame that way,
    // =<n> sets the helpers (profiles/r05_h2d_register.txt).
    static const int register_threads = std::getenv("LIBRECTIFY_REGISTER_FRAMES") ? std::max(0, std::atoi(std::getenv("LIBRECTIFY_REGISTER_FRAMES"))) : 4;
    // (a host on which pinning is slow -- measured on this box: 1.3 ms a 4K frame on one thread, 25 GB/s; the guard trips below
    // 6 GB/s -- gets the staging copy back: for the rest of the call, and for the context's next 32 batch calls before it tries again)
    if (c->register_slow_calls > 0) --c->register_slow_calls;
    const bool reg_frames = register_threads > 0 && h_frames != nullptr && any_pageable && stride >= w && c->register_slow_calls == 0;
    const size_t row_bytes = (size_t)w * bpp, pitch = (size_t)(stride < 0 ? -stride : stride) * bpp;
    struct RegPlan {
        uintptr_t lo = 0, hi = 0;  // the whole pages inside the frame (hi <= lo: none worth registering)
        int r_lo = 0, r_hi = 0;    // rows [r_lo, r_hi) lie in them; the rows before and after are staged
    };
    std::vector<RegPlan> plan(reg_frames ? (size_t)batch : 0);
    if (reg_frames) {
        constexpr uintptr_t kPage = 4096;
        for (int i = 0; i < batch; ++i) {
            RegPlan& p = plan[(size_t)i];
            const uintptr_t a = reinterpret_cast<uintptr_t>(h_frames[i]), e = a + (size_t)(h - 1) * pitch + row_bytes;
            const uintptr_t lo = (a + kPage - 1) / kPage * kPage, hi = e / kPage * kPage;
            if (hi <= lo) continue;
            const int r_lo = (int)((lo - a + pitch - 1) / pitch);                                // first row that starts at or behind lo
            const int r_hi = hi - a >= row_bytes ? (int)std::min<size_t>((size_t)h, (hi - a - row_bytes) / pitch + 1) : 0;  // rows that end at or before hi
            if (r_hi - r_lo < h / 2) continue;  // (a frame of a few pages: the staging copy)
            bool apart = !locked[(size_t)i] && !c->batch_no_register;  // ... from every earlier frame's pages
            for (int j = 0; j < i && apart; ++j) {
                const RegPlan& q = plan[(size_t)j];
                apart = q.hi <= q.lo || q.hi <= lo || hi <= q.lo;
            }
            if (!apart) continue;
            p.lo = lo;
            p.hi = hi;
            p.r_lo = r_lo;
            p.r_hi = r_hi;
        }
    }
    std::atomic<int> reg_slow{0};
    std::vector<std::atomic<int>> reg_ready(reg_frames ? (size_t)batch : 0);
    for (auto& a : reg_ready) a.store(0, std::memory_order_relaxed);
    // reg_ready[i]: 0 nobody has touched the frame, 3 a helper is registering it, 1 registered, 2 the staging copy takes it
    // (page-locked already, registration refused, or the uploader got there first).  The helpers take the frames in order; a
    // frame the uploader reaches before any helper has is staged.  (Helpers that begin at the fourth frame, the uploader staging
    // the call's first three rather than waiting 1.3 ms for the first registration: 11.30 against 11.41 Gpix/s -- the staging
    // copies cost the helpers more than the wait costs the call.)
    std::atomic<int> reg_next{0};
    std::vector<std::thread> reg_pool;
    if (reg_frames)
        for (int t = 0; t < register_threads; ++t)
            reg_pool.emplace_back([&]() {
                (void)hipSetDevice(c->device);
                bind_this_thread_near(c->device);
                for (int i = reg_next.fetch_add(1, std::memory_order_relaxed); i < batch && !abort_all.load(std::memory_order_relaxed);
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
            });
    const double t_call0 = now_ms();
    auto uploader = [&]() {
        if (hipSetDevice(c->device) != hipSuccess) {
            up_err = "hipSetDevice failed";
            abort_all.store(1);
            return;
        }
        if (any_pageable) bind_this_thread_near(c->device);  // (this thread stages too; it is the library's own)
        StagingCrew crew;
        if (any_pageable) crew.start(c, staging_threads(num_threads, npix * bpp) - 1);
        for (int i = 0; i < batch; ++i) {
            int slot = -1, spins = 0;
            const double t_w0 = batch_stats ? now_ms() : 0.0;
            // a slot whose frame is done (its transfer and its staging buffer are then free as well)
            while (slot < 0 && !abort_all.load(std::memory_order_relaxed)) {
                for (int k = 0; k < R && slot < 0; ++k)
                    if (!slot_busy[(size_t)k].load(std::memory_order_acquire)) slot = k;
                if (slot < 0) nap(spins);
            }
            if (batch_stats) up_wait_us.fetch_add((long long)((now_ms() - t_w0) * 1e3));
            if (abort_all.load(std::memory_order_relaxed)) return;
            slot_busy[(size_t)slot].store(1, std::memory_order_relaxed);
            if (reg_frames) {  // (the frame is being pinned by a helper: wait for it)
                int sp2 = 0;
                int expect = 0;
                if (!reg_ready[(size_t)i].compare_exchange_strong(expect, 2, std::memory_order_acq_rel))  // (else: nobody has it -- staged)
                    while (reg_ready[(size_t)i].load(std::memory_order_acquire) == 3 && !abort_all.load(std::memory_order_relaxed)) nap(sp2);
            }
            const bool registered = reg_frames && reg_ready[(size_t)i].load(std::memory_order_acquire) == 1;
            uint8_t* stage = locked[(size_t)i] ? nullptr : reinterpret_cast<uint8_t*>(c->ring.stage[(size_t)slot].get());
            uint8_t* dimg = reinterpret_cast<uint8_t*>(c->ring.img[(size_t)slot].get());
            const double t_u0 = now_ms();
            Event e_dbg;
            if (lane_debug && e_dbg.create() == hipSuccess) (void)hipEventRecord(e_dbg, c->copy_stream);
            int up_rc = 0;
            if (registered) {
                const RegPlan& p = plan[(size_t)i];
                const uint8_t* f = h_frames[i];
                // the rows that reach into a page shared with a neighbour: staged here, fetched by the lane
                for (int r = 0; r < p.r_lo; ++r) std::memcpy(stage + (size_t)r * row_bytes, f + (size_t)r * pitch, row_bytes);
                for (int r = p.r_hi; r < h; ++r) std::memcpy(stage + (size_t)r * row_bytes, f + (size_t)r * pitch, row_bytes);
                slot_edges[(size_t)slot].r_lo = p.r_lo;
                slot_edges[(size_t)slot].r_hi = p.r_hi;
                {
                    const hipError_t e = pitch == row_bytes
                        ? hipMemcpyAsync(dimg + (size_t)p.r_lo * row_bytes, f + (size_t)p.r_lo * pitch, (size_t)(p.r_hi - p.r_lo) * row_bytes, hipMemcpyHostToDevice, c->copy_stream)
                        : hipMemcpy2DAsync(dimg + (size_t)p.r_lo * row_bytes, row_bytes, f + (size_t)p.r_lo * pitch, pitch, row_bytes, (size_t)(p.r_hi - p.r_lo), hipMemcpyHostToDevice, c->copy_stream);
                    if (e != hipSuccess) up_rc = 1;
                }
                if (up_rc) {
                    (void)hipGetLastError();
                    set_error("upload: transfer of a registered frame failed");
                }
            } else {
                slot_edges[(size_t)slot].r_hi = 0;
                up_rc = stage ? crew.run(dimg, stage, h_frames[i], w, h, stride, (int)bpp, c->copy_stream, kBatchBand, 1)
                              : upload_rows(c, dimg, nullptr, h_frames[i], w, h, stride, (int)bpp, 1, c->copy_stream);
            }
            if (up_rc || hipEventRecord(c->ring_ev[(size_t)slot], c->copy_stream) != hipSuccess) {
                up_err = get_error().empty() ? "upload failed" : get_error();
                abort_all.store(1);
                return;
            }
            enq[(size_t)i].store(slot + 1, std::memory_order_release);
            if (lane_debug) {
                const double t_u1 = now_ms();
                float dma = 0.f;  // from the moment the link was free for this frame to the end of its last transfer
                if (e_dbg) {
                    (void)hipEventSynchronize(c->ring_ev[(size_t)slot]);
                    if (hipEventElapsedTime(&dma, e_dbg, c->ring_ev[(size_t)slot]) != hipSuccess) (void)hipGetLastError();
                }
                std::fprintf(stderr, "uploader frame %d: slot %d, waited %d naps for it, staged and enqueued in %.2f ms, on the link %.2f ms\n", i, slot, spins, t_u1 - t_u0, dma);
            }
        }
    };
    std::atomic<int> next_frame{0};
    std::vector<int> rc(S, 0);
    std::vector<std::string> err(S);
    auto work = [&](int si) {
        lr_context* l = lanes[si];
        auto fail = [&]() {
            rc[si] = 1;
            err[si] = get_error();
            abort_all.store(1);
        };
        if (si > 0 && hipSetDevice(c->device) != hipSuccess) {
            set_error("hipSetDevice failed");
            return fail();
        }
        for (int b = next_frame.fetch_add(1, std::memory_order_relaxed); b < batch; b = next_frame.fetch_add(1, std::memory_order_relaxed)) {
            const void* img = nullptr;
            int img_stride = stride, slot = -1;
            if (h_frames) {
                int spins = 0;
                const double t_w0 = batch_stats ? now_ms() : 0.0;
                while ((slot = enq[(size_t)b].load(std::memory_order_acquire) - 1) < 0 && !abort_all.load(std::memory_order_relaxed)) nap(spins);
                if (batch_stats) lane_wait_us.fetch_add((long long)((now_ms() - t_w0) * 1e3));
                if (slot < 0) return;  // (whoever stopped the batch has the message)
                if (hipStreamWaitEvent(l->stream, c->ring_ev[(size_t)slot], 0) != hipSuccess) {
                    set_error("hipStreamWaitEvent failed");
                    return fail();
                }
                img = c->ring.img[(size_t)slot].get();
                img_stride = w;
                const SlotEdges ed = slot_edges[(size_t)slot];
                if (ed.r_hi > 0) {  // (page-locked staging memory: two small transfers on the lane's own stream)
                    uint8_t* dimg = reinterpret_cast<uint8_t*>(c->ring.img[(size_t)slot].get());
                    const uint8_t* st = reinterpret_cast<const uint8_t*>(c->ring.stage[(size_t)slot].get());
                    hipError_t e = hipSuccess;
                    if (ed.r_lo > 0) e = hipMemcpyAsync(dimg, st, (size_t)ed.r_lo * row_bytes, hipMemcpyHostToDevice, l->stream);
                    if (e == hipSuccess && ed.r_hi < h)
                        e = hipMemcpyAsync(dimg + (size_t)ed.r_hi * row_bytes, st + (size_t)ed.r_hi * row_bytes, (size_t)(h - ed.r_hi) * row_bytes, hipMemcpyHostToDevice, l->stream);
                    if (e != hipSuccess) {
                        (void)hipGetLastError();
                        set_error("upload: transfer of a registered frame's first or last rows failed");
                        return fail();
                    }
                }
            } else {
                img = d_images + (size_t)b * image_stride * bpp;
            }
            std::vector<LineSegment> res;
            const double t_f0 = now_ms();
            if (ctx_find_groups_device(l, img, format, w, h, img_stride, min_length, refine, res)) return fail();
            if (batch_stats && h_frames && l->opt.timing_on) {  // (with the stage timers on: ev[0] is the frame's first kernel)
                float lead = 0.f;
                if (hipEventElapsedTime(&lead, c->ring_ev[(size_t)slot], l->ev[0]) == hipSuccess) {
                    lead_sum_us.fetch_add((long long)(lead * 1e3));
                    if (lead < 0.05f) late_frames.fetch_add(1);
                } else {
                    (void)hipGetLastError();
                }
            }
            if (lane_debug) {
                float lead = 0.f;  // how long the frame's upload had been finished when its first kernel started
                if (h_frames && hipEventElapsedTime(&lead, c->ring_ev[(size_t)slot], l->ev[0]) != hipSuccess) (void)hipGetLastError();
                std::fprintf(stderr, "lane %d frame %d: enqueue %.2f ms, wait %.2f, whole call %.2f; device total %.2f; upload done %.2f ms before the first kernel\n",
                             si, b, l->host_ms[0], l->host_ms[2], now_ms() - t_f0, l->stage_ms[LR_T_TOTAL], lead);
            }
            if (h_frames) slot_busy[(size_t)slot].store(0, std::memory_order_release);
            const int n = (int)res.size();
            if (n_lines) n_lines[b] = n;
            if (out && capacity > 0)
                std::memcpy(out + (size_t)b * capacity, res.data(), sizeof(LineSegment) * (size_t)std::min(n, capacity));
            if (transforms) {
                const RectificationConfig def;
                transforms[b] = rectification_transform(res.data(), std::min(n, capacity > 0 ? capacity : n), w, h,
                                                        cfg ? *cfg : def);
            }
        }
    };
    std::vector<std::thread> th;
    if (h_frames) th.emplace_back(uploader);
    for (int si = 1; si < S; ++si) th.emplace_back(work, si);
    work(0);
    for (auto& t : th) t.join();
    if (batch_stats && h_frames)
        std::fprintf(stderr, "batch of %d frames: %.2f ms; the uploader waited %.2f ms for free device frames; the %d lanes waited %.2f ms in all for their frame's transfer to be enqueued\n",
                     batch, now_ms() - t_call0, up_wait_us.load() * 1e-3, S, lane_wait_us.load() * 1e-3);
    if (batch_stats && h_frames && c->opt.timing_on)
        std::fprintf(stderr, "   a frame's transfer was finished %.3f ms (mean) before its first kernel started; %d of %d frames started within 0.05 ms of it (they waited for the link)\n",
                     lead_sum_us.load() * 1e-3 / batch, late_frames.load(), batch);
    if (h_frames) (void)hipStreamSynchronize(c->copy_stream);  // (after an error: nothing may still read the caller's frames)
    for (auto& t : reg_pool) t.join();
    if (reg_slow.load() >= 2) c->register_slow_calls = 32;
    if (reg_frames)  // the caller's frames go back to being pageable
        for (int i = 0; i < batch; ++i)
            if (reg_ready[(size_t)i].load(std::memory_order_acquire) == 1 && hipHostUnregister(reinterpret_cast<void*>(plan[(size_t)i].lo)) != hipSuccess)
                (void)hipGetLastError();  // (nothing to be done about it, and the caller's thread must not find it in its next call)
    lanes_done(c, lanes);
    for (int si = 0; si < S; ++si)
        if (rc[si]) {
            set_error(err[si]);
            return 1;
        }
    if (abort_all.load()) {
        set_error(up_err.empty() ? "batch: upload failed" : up_err);
        return 1;
    }
    return 0;
}

int ctx_find_groups_batch_device(lr_context* c, const void* d_images, int format, size_t image_stride, int batch, int w, int h,
                                 int stride, float min_length, bool refine, LineSegment* out, int capacity, int* n_lines,
                                 const RectificationConfig* cfg, ImageTransform* transforms) {
    return find_groups_batch(c, d_images, format, image_stride, nullptr, batch, w, h, stride, min_length, refine, -1, out,
                             capacity, n_lines, cfg, transforms);
}

// The device batch with a frame table (lr_find_line_segment_groups_batch_device with width == 0 && height == 0): every frame
// has its own address, size, stride and min_length.  The lanes take the frames dynamically, as above, and run the
// single-frame path on each; what is the call's own is the workspace: every lane grows ONCE, before the first frame, to the
// largest pixel count and the largest tile count among the frames (not necessarily one frame's), and for the length of the
// call no lane counts small frames towards giving its workspace back (ctx_ensure_image_capacity) -- nothing is freed or
// reallocated while another lane's kernels run.
int ctx_find_groups_frames_device(lr_context* c, const lr_frame* frames, int format, bool tagged, int batch, float min_length,
                                  bool refine, LineSegment* out, int capacity, int* n_lines, const RectificationConfig* cfg,
                                  ImageTransform* transforms) {
    auto bad = [](int b, const char* what) {
        set_error("lr_find_line_segment_groups_batch_device: frame " + std::to_string(b) + " of the table: " + what);
        return 1;
    };
    const size_t bpp = (size_t)pix_bytes(format);
    if (bpp == 0) {
        set_error("unknown pixel format of the frames");
        return 1;
    }
    if (frames == nullptr) {
        set_error("lr_find_line_segment_groups_batch_device: no frame table");
        return 1;
    }
    // the whole table, before anything is launched
    size_t max_pix = 0;
    int max_tiles = 0;
    for (int b = 0; b < batch; ++b) {
        const lr_frame& f = frames[b];
        if (f.data == nullptr) return bad(b, "null data");
        if (f.width < 1 || f.height < 1) return bad(b, "size below 1");
        if (f.stride < f.width) return bad(b, "stride smaller than the width");
        if (format == LR_PIX_F32 && (reinterpret_cast<uintptr_t>(f.data) & 3u)) return bad(b, "f32 address not 4-byte aligned");
        if (f.width < 5 || f.height < 5) {
            if (!tagged) return bad(b, "image smaller than the 5x5 filter");
            continue;  // (answered below without a launch)
        }
        max_pix = std::max(max_pix, (size_t)f.width * (size_t)f.height);
        max_tiles = std::max(max_tiles, filter_geometry(f.width, f.height).n_tiles);
    }
    const RectificationConfig def;
    const int S = std::max(1, std::min(c->opt.batch_streams, batch));
    std::vector<lr_context*> lanes;
    if (lanes_begin(c, S, false, lanes)) return 1;
    LR_HIP(hipSetDevice(c->device));
    int grow_rc = 0;
    for (lr_context* l : lanes) {
        l->keep_workspace = true;
        if (!grow_rc && max_pix) grow_rc = ctx_reserve_workspace(l, max_pix, max_tiles);
    }
    std::atomic<int> next_frame{0}, abort_all{0};
    std::vector<int> rc(S, 0);
    std::vector<std::string> err(S);
    auto work = [&](int si) {
        lr_context* l = lanes[si];
        auto fail = [&]() {
            rc[si] = 1;
            err[si] = get_error();
            abort_all.store(1);
        };
        if (si > 0 && hipSetDevice(c->device) != hipSuccess) {
            set_error("hipSetDevice failed");
            return fail();
        }
        for (int b = next_frame.fetch_add(1, std::memory_order_relaxed); b < batch && !abort_all.load(std::memory_order_relaxed);
             b = next_frame.fetch_add(1, std::memory_order_relaxed)) {
            const lr_frame& f = frames[b];
            std::vector<LineSegment> res;
            if (f.width >= 5 && f.height >= 5 &&
                ctx_find_groups_device(l, f.data, format, f.width, f.height, f.stride, f.min_length < 0.f ? min_length : f.min_length,
                                       refine, res))
                return fail();
            const int n = (int)res.size();
            if (n_lines) n_lines[b] = n;
            if (out && capacity > 0)
                std::memcpy(out + (size_t)b * capacity, res.data(), sizeof(LineSegment) * (size_t)std::min(n, capacity));
            if (transforms)
                transforms[b] = rectification_transform(res.data(), std::min(n, capacity > 0 ? capacity : n), f.width, f.height,
                                                        cfg ? *cfg : def);
        }
    };
    if (!grow_rc) {
        std::vector<std::thread> th;
        for (int si = 1; si < S; ++si) th.emplace_back(work, si);
        work(0);
        for (auto& t : th) t.join();
    }
    for (lr_context* l : lanes) l->keep_workspace = false;
    lanes_done(c, lanes);
    if (grow_rc) return 1;
    for (int si = 0; si < S; ++si)
        if (rc[si]) {
            set_error(err[si]);
            return 1;
        }
    return 0;
}

int ctx_find_groups_batch_host(lr_context* c, const void* const* frames, int format, int batch, int w, int h, int stride,
                               float min_length, bool refine, int num_threads, LineSegment* out, int capacity,
                               int* n_lines, const RectificationConfig* cfg, ImageTransform* transforms) {
    return find_groups_batch(c, nullptr, format, 0, frames, batch, w, h, stride, min_length, refine, num_threads, out, capacity,
                             n_lines, cfg, transforms);
}

// One batch call over several devices of this process.  Every entry of the device list has a context of its own (kept
// with `c` from call to call), configured like `c`, with its own uploader, copy stream, lanes and pool; a host thread per
// entry runs the single-device batch call on its contiguous block of the frames.
int ctx_find_groups_batch_host_multi(lr_context* c, const int* devices, int n_devices, const void* const* frames, int format, int batch,
                                     int w, int h, int stride, float min_length, bool refine, int num_threads,
                                     LineSegment* out, int capacity, int* n_lines, const RectificationConfig* cfg,
                                     ImageTransform* transforms) {
    if (batch <= 0) return 0;
    if (n_devices <= 0 || devices == nullptr) {
        set_error("multi-device batch: empty device list");
        return 1;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
    for (int i = 0; i < n_devices; ++i)
        if (devices[i] < 0 || devices[i] >= ndev) {
            set_error("multi-device batch: device index out of range");
            return 1;
        }
    // the contexts of the list (re-made where the list changed)
    if ((int)c->peers.size() > n_devices) {
        for (size_t i = (size_t)n_devices; i < c->peers.size(); ++i) ctx_destroy(c->peers[i]);
        c->peers.resize((size_t)n_devices);
    }
    c->peers.resize((size_t)n_devices, nullptr);
    for (int i = 0; i < n_devices; ++i) {
        if (c->peers[(size_t)i] && c->peers[(size_t)i]->device != devices[i]) {
            ctx_destroy(c->peers[(size_t)i]);
            c->peers[(size_t)i] = nullptr;
        }
        if (!c->peers[(size_t)i] && ctx_create(devices[i], &c->peers[(size_t)i])) {
            (void)hipSetDevice(c->device);
            return 1;
        }
        c->peers[(size_t)i]->opt = c->opt;
    }
    const int per = (batch + n_devices - 1) / n_devices;  // contiguous blocks of ceil(B / G) frames
    // The blocks register and release their frames independently of each other (find_groups_batch).  Frames of different
    // blocks that overlap (a frame listed in two blocks, sliding windows across a block's end) would have their pages
    // registered by two entries at once: such a call stages all its frames instead.
    bool blocks_apart = true;
    if (const size_t fbpp = (size_t)pix_bytes(format)) {
        const size_t span = (size_t)(h - 1) * (size_t)(stride < 0 ? -stride : stride) * fbpp + (size_t)w * fbpp;
        for (int i = 0; i < batch && blocks_apart && w > 0 && h > 0; ++i)
            for (int j = (i / per + 1) * per; j < batch && blocks_apart; ++j) {
                if (!frames[i] || !frames[j]) continue;
                const uintptr_t a = reinterpret_cast<uintptr_t>(frames[i]) - (stride < 0 ? (size_t)(h - 1) * (size_t)(-stride) * fbpp : 0);
                const uintptr_t b = reinterpret_cast<uintptr_t>(frames[j]) - (stride < 0 ? (size_t)(h - 1) * (size_t)(-stride) * fbpp : 0);
                blocks_apart = a + span <= b || b + span <= a;
            }
    }
    for (lr_context* p : c->peers) p->batch_no_register = !blocks_apart;
    std::vector<int> rc((size_t)n_devices, 0);
    std::vector<std::string> err((size_t)n_devices);
    auto run = [&](int i) {
        const int b0 = std::min(batch, i * per), b1 = std::min(batch, b0 + per);
        if (b1 <= b0) return;
        lr_context* p = c->peers[(size_t)i];
        if (hipSetDevice(p->device) != hipSuccess) {
            rc[(size_t)i] = 1;
            err[(size_t)i] = "hipSetDevice failed";
            return;
        }
        // (a share of the staging threads each: they all copy out of the same host memory)
        const int nt = num_threads > 1 ? std::max(2, num_threads / std::min(n_devices, (batch + per - 1) / per)) : num_threads;
        if (ctx_find_groups_batch_host(p, frames + b0, format, b1 - b0, w, h, stride, min_length, refine, nt,
                                       out ? out + (size_t)b0 * capacity : nullptr, capacity, n_lines ? n_lines + b0 : nullptr, cfg,
                                       transforms ? transforms + b0 : nullptr)) {
            rc[(size_t)i] = 1;
            err[(size_t)i] = get_error();  // (thread-local: carried back to the caller below)
        }
    };
    std::vector<std::thread> th;
    for (int i = 1; i < n_devices; ++i) th.emplace_back(run, i);
    run(0);
    for (auto& t : th) t.join();
    (void)hipSetDevice(c->device);
    for (int i = 0; i < n_devices; ++i)
        if (rc[(size_t)i]) {
            set_error("device list entry " + std::to_string(i) + " (device " + std::to_string(devices[i]) + "): " + err[(size_t)i]);
            return 1;
        }
    return 0;
}

}  // namespace lramd
