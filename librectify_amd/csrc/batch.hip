// Many frames per call: the lanes of a batch call and their work loop, the three batch entries, and the same over several devices.
#include "host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace lramd {

// Batch of independent frames: the stages of one frame are latency-bound (flood rounds,
// host round trips), so several frames are kept in flight, one host thread + context + HIP stream each ("lanes");
// frames are handed out dynamically (they differ in cost, and with a fixed assignment the batch ends on one lane).

// The lanes of a batch call: the caller's context and S - 1 workers of its own (kept from call to call), set up for the
// length of the call; the destructor gives the caller's context its own settings back, on every way out of the call.
class LaneSet {
public:
    LaneSet() = default;
    LaneSet(const LaneSet&) = delete;
    LaneSet& operator=(const LaneSet&) = delete;
    // keep_workspace: a call with a frame table, whose lanes are sized once for the call (lr_context::keep_workspace)
    int setup(lr_context* caller, int S, bool host_frames, bool keep_workspace) {
        c = caller;
        c->workers.reserve((size_t)std::max(0, S - 1));
        while ((int)c->workers.size() < S - 1) {
            lr_context* wc = nullptr;
            if (ctx_create(c->device, &wc)) return 1;
            c->workers.push_back(wc);
        }
        lanes.reserve((size_t)S);
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
            l->flood_sched_off = true;  // (the schedule hook is for single calls and stage calls: the caller's own is lane 0)
            // LIBRECTIFY_LANES_SLEEP: the lanes sleep on an event instead of spinning in hipStreamSynchronize, for hosts
            // short of cores (on the 16-core share of a one-GPU box: pageable frames equal, page-locked ones 5 % slower)
            static const bool sleep_env = std::getenv("LIBRECTIFY_LANES_SLEEP") != nullptr;
            l->sleep_in_wait = sleep_env && host_frames;
            l->keep_workspace = keep_workspace;
        }
        return 0;
    }
    ~LaneSet() {
        if (!c) return;
        for (lr_context* l : lanes) {
            l->sleep_in_wait = false;
            l->keep_workspace = false;
            l->flood_sched_off = false;
        }
        c->flood_logbig_off = false;
        c->flood_log_min = c->flood_log_walk = 0;
        c->flood_jit_sleep_us = 0;
    }
    int size() const { return (int)lanes.size(); }
    lr_context* operator[](int i) const { return lanes[(size_t)i]; }

private:
    lr_context* c = nullptr;
    std::vector<lr_context*> lanes;
};

// Where the results of a batch call go: the caller's arrays.
struct BatchOut {
    LineSegment* out;
    int capacity;
    int* n_lines;
    const RectificationConfig* cfg;
    ImageTransform* transforms;
    // the result of frame b (w x h): its count, its first `capacity` records and its transform
    void write(int b, const std::vector<LineSegment>& res, int w, int h) const {
        const int n = (int)res.size();
        if (n_lines) n_lines[b] = n;
        if (out && capacity > 0 && n > 0) std::memcpy(out + (size_t)b * capacity, res.data(), sizeof(LineSegment) * (size_t)std::min(n, capacity));
        if (transforms) {
            const RectificationConfig def;
            transforms[b] = rectification_transform(res.data(), std::min(n, capacity > 0 ? capacity : n), w, h, cfg ? *cfg : def);
        }
    }
};

// The work loop of a batch call: S - 1 threads and the calling one, a lane each, take the frames from one counter and run
// `frame(lane, lane_index, b)` (0, or 1 with the message set) on each.  A lane takes no further frame once `stop` is set --
// by a lane that failed, here, or by the call's uploader.  The message of the lowest-numbered failed lane is the call's.
template <class Frame>
static int run_lanes(const LaneSet& lanes, int batch, std::atomic<int>& stop, const Frame& frame) {
    const int S = lanes.size();
    std::atomic<int> next_frame{0};
    std::vector<int> rc((size_t)S, 0);
    std::vector<std::string> err((size_t)S);
    auto work = [&](int si) {
        bool failed = false;
        if (si > 0 && hipSetDevice(lanes[0]->device) != hipSuccess) {
            set_error("hipSetDevice failed");
            failed = true;
        }
        while (!failed && !stop.load(std::memory_order_relaxed)) {
            const int b = next_frame.fetch_add(1, std::memory_order_relaxed);
            if (b >= batch) break;
            failed = frame(lanes[si], si, b) != 0;
        }
        if (failed) {
            rc[(size_t)si] = 1;
            err[(size_t)si] = get_error();
            stop.store(1);
        }
    };
    {
        JoinedThreads workers;  // (joined here, and where starting one of them throws)
        for (int si = 1; si < S; ++si) workers.th.emplace_back(work, si);
        work(0);
    }
    for (int si = 0; si < S; ++si)
        if (rc[(size_t)si]) {
            set_error(err[(size_t)si]);
            return 1;
        }
    return 0;
}

// Frames resident on the device, of one size: frame b lies image_stride pixels behind frame b - 1.
// Frames are of one lr_pixel_format (`format`; strides and image_stride in pixels of it).
int ctx_find_groups_batch_device(lr_context* c, const void* d_images, int format, size_t image_stride, int batch, int w, int h,
                                 int stride, float min_length, bool refine, LineSegment* out, int capacity, int* n_lines,
                                 const RectificationConfig* cfg, ImageTransform* transforms) {
    if (batch <= 0) return 0;
    const size_t bpp = (size_t)pix_bytes(format);
    if (bpp == 0) {
        set_error("unknown pixel format of the frames");
        return 1;
    }
    LaneSet lanes;
    if (lanes.setup(c, std::max(1, std::min(c->opt.batch_streams, batch)), false, false)) return 1;
    const BatchOut results{out, capacity, n_lines, cfg, transforms};
    std::atomic<int> stop{0};
    return run_lanes(lanes, batch, stop, [&](lr_context* l, int, int b) {
        std::vector<LineSegment> res;
        if (ctx_find_groups_device(l, static_cast<const uint8_t*>(d_images) + (size_t)b * image_stride * bpp, format, w, h, stride, min_length,
                                   refine, res))
            return 1;
        results.write(b, res, w, h);
        return 0;
    });
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
    if (pix_bytes(format) == 0) {
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
    LaneSet lanes;
    if (lanes.setup(c, std::max(1, std::min(c->opt.batch_streams, batch)), false, true)) return 1;
    LR_HIP(hipSetDevice(c->device));
    for (int si = 0; si < lanes.size() && max_pix; ++si)
        if (ctx_reserve_workspace(lanes[si], max_pix, max_tiles)) return 1;
    const BatchOut results{out, capacity, n_lines, cfg, transforms};
    std::atomic<int> stop{0};
    return run_lanes(lanes, batch, stop, [&](lr_context* l, int, int b) {
        const lr_frame& f = frames[b];
        std::vector<LineSegment> res;
        if (f.width >= 5 && f.height >= 5 &&
            ctx_find_groups_device(l, f.data, format, f.width, f.height, f.stride, f.min_length < 0.f ? min_length : f.min_length, refine, res))
            return 1;
        results.write(b, res, f.width, f.height);
        return 0;
    });
}

// Host-resident frames (pageable or page-locked, any stride sign): the call's BatchUploader (host.h) brings them to device
// frames on the copy stream, ahead of the lanes; a lane makes its stream wait for its frame's transfer.
int ctx_find_groups_batch_host(lr_context* c, const void* const* frames, int format, int batch, int w, int h, int stride,
                               float min_length, bool refine, int num_threads, LineSegment* out, int capacity,
                               int* n_lines, const RectificationConfig* cfg, ImageTransform* transforms) {
    if (batch <= 0) return 0;
    const int bpp = pix_bytes(format);
    if (bpp == 0) {
        set_error("unknown pixel format of the frames");
        return 1;
    }
    const int S = std::max(1, std::min(c->opt.batch_streams, batch));
    BatchUploader up(c, frames, batch, w, h, stride, bpp, S, num_threads);
    if (up.check()) return 1;  // (before a lane is touched)
    LaneSet lanes;
    if (lanes.setup(c, S, true, false) || up.start()) return 1;
    const BatchOut results{out, capacity, n_lines, cfg, transforms};
    const int lanes_rc = run_lanes(lanes, batch, up.stop, [&](lr_context* l, int si, int b) {
        const void* img = nullptr;
        int slot = -1;
        if (up.ready(b, l->stream, &img, &slot)) return 1;
        if (img == nullptr) return 0;  // (the call has been stopped)
        std::vector<LineSegment> res;
        const double t_f0 = now_ms();
        if (ctx_find_groups_device(l, img, format, w, h, w, min_length, refine, res)) return 1;
        up.release(slot, b, l, si, t_f0);
        results.write(b, res, w, h);
        return 0;
    });
    const std::string& up_err = up.end();  // (leaves the lanes' message alone)
    if (lanes_rc) return 1;
    if (!up_err.empty()) {
        set_error(up_err);
        return 1;
    }
    return 0;
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
    // The blocks register and release their frames independently of each other (upload.hip: BatchUploader).  Frames of different
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
