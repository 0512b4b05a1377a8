// Internals shared by the host units: context.hip (workspace), upload.hip (host frames -> device: single frames and the
// uploader of batch calls, its page-registration plan from reg_plan.h), frame.hip (one frame), estimators.hip (vanishing
// points), batch.hip (the lanes of a call: many frames, many devices).
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "context.h"
#include "reg_plan.h"

namespace lramd {

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Threads that are joined on every way out of their scope (an exception included: a std::thread destroyed while joinable
// ends the process).
struct JoinedThreads {
    std::vector<std::thread> th;
    void join() {
        for (auto& t : th)
            if (t.joinable()) t.join();
    }
    ~JoinedThreads() { join(); }
};

// d_counts words (kCntLarge: seven words of the component lists, kernels_fit.hip; kCntFitComp, kCntFitPx: the components and
// pixels that the fit stage worked on -- kCntComp and kCntPx again unless the frame's fit was pruned)
enum { kCntSeeds = 0, kCntComp = 1, kCntPx = 2, kCntLarge = 4, kCntFitComp = 12, kCntFitPx = 13 };

// context.hip
int ensure_flood_buffers(lr_context* c);
int ensure_group_capacity(lr_context* c, size_t n_lines);

// frame.hip
int enqueue_groups(lr_context* c, uint32_t line_cap, int max_models, float inlier_deg, float garbage_deg, int n_iter,
                   uint64_t seed, bool model_done = false, bool gather = false);
int run_frame(lr_context* c, const void* d_image, int format, int w, int h, int stride, float min_length, bool refine,
              std::vector<LineSegment>& out, bool filter_enqueued = false);

// upload.hip
int ensure_copy_stream(lr_context* c);
bool is_page_locked(const void* p);
int staging_threads(int num_threads, size_t frame_bytes = 0);
void bind_this_thread_near(int device);
// (host frames travel as bytes: `bpp` bytes a pixel, strides in pixels, device and staging buffers packed at w * bpp a row)
int upload_rows(lr_context* c, void* dst, void* stage, const void* buffer, int w, int h, int stride, int bpp, int num_threads,
                hipStream_t up);
int ensure_frame_slot(lr_context* c, int slot, size_t npix, bool pageable, float** stage);
int ensure_upload_ring(lr_context* c, int R, size_t npix, bool staging);

// The threads that stage pageable frames for a batch call: started once per call, not once per frame (seven thread
// starts a frame were a tenth of a millisecond of the uploader's time and the larger part of its jitter).  A job is one
// frame; its 4 MB bands are claimed through a counter that carries the job's number, so that a thread that is late for
// one job cannot take a band of the next with the old job's pointers.
struct StagingCrew {
    lr_context* c = nullptr;
    std::vector<std::thread> th;
    std::atomic<uint32_t> job{0};
    std::atomic<uint64_t> next{0};   // job number << 32 | next piece
    std::atomic<uint64_t> total{0};  // job number << 32 | pieces of that job
    std::atomic<int> bands_left{0}, failed{0};
    std::atomic<bool> quit{false};
    // Two job descriptors, used alternately (job number & 1): the one a late helper may still be reading is not the one
    // the uploader fills for the next frame, and the one after that is only filled when every band of this one is done.
    struct Job {
        uint8_t* dst = nullptr;
        uint8_t* stage = nullptr;
        const uint8_t* src = nullptr;
        size_t row_bytes = 0, src_pitch = 0;  // bytes of a row, and from one source row to the next
        int h = 0, rows_per_band = 1, n_bands = 0;
        hipStream_t up = nullptr;
        int pieces = 1;                       // row runs a band is copied in (by different threads)
        const Event* band_ev = nullptr;       // optional: recorded after each band's transfer is enqueued ...
        std::atomic<int>* ready = nullptr;    // ... and then ready[k] = 1 (-1 if the band failed)
    } jobs[2];

    // A single frame's bands are staged by ALL the threads together, piece by piece (`pieces` row runs per band, claimed in
    // order through `next`), and sent by whichever thread finishes a band's last piece: the first transfer starts after one
    // band's worth of copying spread over the crew instead of after every thread has copied a whole band of its own (which
    // is when all of them are ready at once).  A batch's uploader keeps whole bands per thread (pieces = 1): there the
    // link is busy with the previous frame anyway, and fewer hand-overs are worth more than an early start.
    static constexpr int kPieces = 8;
    static constexpr int kMaxBands = 256;
    std::atomic<int> pieces_left[2][kMaxBands];

    // Helpers between jobs: a short spin (frames of a batch follow each other within microseconds), then they BLOCK on a
    // condition variable -- a library behind librectify.h must not keep eight threads polling in a process that is doing
    // nothing (round 3 did: 20 us naps for ever).  begin() wakes them only if somebody sleeps.
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<int> sleepers{0};
    std::atomic<int> live{0};  // helpers that have a device and are taking jobs (the caller stages alone if none is)

    bool work_one(uint32_t gen);  // one piece of job `gen`, if there is one left: true if a piece was claimed (and copied)
    void work(uint32_t gen) {
        while (work_one(gen)) {
        }
    }
    void start(lr_context* ctx, int helpers);
    // stages one frame (rows as in upload_rows) and enqueues its transfers; returns when every band is enqueued
    int run(void* dst_, void* stage_, const void* buffer, int w_, int h_, int stride_, int bpp_, hipStream_t up_,
            size_t band_bytes = (size_t)4 << 20, int pieces_ = 1) {
        const uint32_t g = begin(dst_, stage_, buffer, w_, h_, stride_, bpp_, up_, nullptr, nullptr, band_bytes, pieces_);
        work(g);
        return finish();
    }
    // the two halves of run(): publish the job (the helpers start on it), and wait for its last band
    uint32_t begin(void* dst_, void* stage_, const void* buffer, int w_, int h_, int stride_, int bpp_, hipStream_t up_,
                   const Event* band_ev_, std::atomic<int>* ready_, size_t band_bytes = (size_t)4 << 20, int pieces_ = 0);
    int finish();
    ~StagingCrew();
};

// Host frames of a batch call on their way to device frames (the lanes of the call never touch host memory).  The frames
// are uploaded by ONE uploader thread, in frame order, on the caller's copy stream, into a pool of lanes + 6 device frames:
// frame i goes to whichever slot is free (frames finish out of order: a heavy frame runs as long as three light ones, and
// slot i mod R would make the link wait for it), so the link works up to six frames ahead of the lanes instead of
// starting a lane's next transfer only when the lane starts a frame.  (With one slot ahead per lane -- the first design --
// a quarter to a third of the frames of a 4K batch still waited for their own upload, although the link was busy only two
// thirds of the time: 7.5 Gpix/s where the same batch without the transfers ran at 9.0; LIBRECTIFY_LANE_DEBUG prints each
// frame's lead.)  A lane makes its stream wait for the frame's transfer and never touches host memory itself.
// Frames are of one pixel format (`bpp` bytes a pixel; the stride in pixels of it) and travel as bytes.
// check() refuses what is wrong with the arguments (it needs no lane and touches nothing); start() sizes the ring and
// starts the threads; a lane asks for frame b with ready() and gives its slot back with release();
// end() -- or the destructor, where end() was not reached -- joins the threads, waits for the link and gives the caller's
// pages back.
class BatchUploader {
public:
    BatchUploader(lr_context* ctx, const void* const* frames, int batch, int w, int h, int stride, int bpp, int lanes, int num_threads);
    ~BatchUploader();
    BatchUploader(const BatchUploader&) = delete;
    BatchUploader& operator=(const BatchUploader&) = delete;
    int check() const;
    int start();
    // Frame b on the lane's stream: waits until its transfer is enqueued, makes `lane_stream` wait for it and fetch the rows
    // that were staged.  0 with *img the device frame (packed rows) and *slot its slot; 0 with *img == nullptr if the call
    // has been stopped (whoever stopped it has the message); 1 if this failed (the message is set).
    int ready(int b, hipStream_t lane_stream, const void** img, int* slot);
    // The frame of `slot` is done (its device frame and its staging buffer are free): frame b, by `lane` (number
    // lane_index), whose call began at t_frame0 -- for LIBRECTIFY_BATCH_STATS and LIBRECTIFY_LANE_DEBUG.
    void release(int slot, int b, const lr_context* lane, int lane_index, double t_frame0);
    const std::string& end();  // the uploader's message; empty if it did not fail
    std::atomic<int> stop{0};  // set by whoever fails, a lane or the uploader: everybody ends

private:
    void close();
    void register_frames();
    void upload_frames();
    int send_frame(StagingCrew& crew, int i, int slot);

    lr_context* c;
    const uint8_t* const* frames;
    const int batch, w, h, stride;
    const size_t bpp, row_bytes, pitch;
    const int lanes, num_threads;
    int R = 0;
    bool any_pageable = false, reg_frames = false, started = false, closed = false;
    std::vector<char> locked;  // frames in memory the CALLER has page-locked
    std::vector<RegPlan> plan;
    std::vector<std::atomic<int>> enq;  // frame's slot + 1 once its transfer is enqueued
    std::vector<std::atomic<int>> slot_busy;
    struct SlotEdges {
        int r_lo = 0, r_hi = 0;  // rows [0, r_lo) and [r_hi, h) of the slot's frame wait in its staging buffer (r_hi = 0: none)
    };
    std::vector<SlotEdges> slot_edges;  // (written by the uploader before enq[], read by the frame's lane after it)
    // reg_ready[i]: 0 nobody has touched the frame, 3 a helper is registering it, 1 registered, 2 the staging copy takes it
    // (page-locked already, registration refused, or the uploader got there first).  The helpers take the frames in order; a
    // frame the uploader reaches before any helper has is staged.  (Helpers that begin at the fourth frame, the uploader staging
    // the call's first three rather than waiting 1.3 ms for the first registration: 11.30 against 11.41 Gpix/s -- the staging
    // copies cost the helpers more than the wait costs the call.)
    std::vector<std::atomic<int>> reg_ready;
    std::atomic<int> reg_next{0}, reg_slow{0};
    std::string up_err;
    // LIBRECTIFY_BATCH_STATS: who waited for whom in this call (host clocks only, nothing is synchronised for it)
    std::atomic<long long> up_wait_us{0}, lane_wait_us{0}, lead_sum_us{0};
    std::atomic<int> late_frames{0};
    double t_call0 = 0.0;
    JoinedThreads helpers, uploader;
};

}  // namespace lramd
