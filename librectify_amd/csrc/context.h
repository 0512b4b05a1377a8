// lr_context: one device, one stream, one reusable workspace (see include/librectify_amd.h).
#pragma once
#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

#include "buffers.h"
#include "common.h"
#include "vp_host.h"

namespace lramd {
struct StagingCrew;  // host.h

// What a caller sets through lr_set_* (and the environment at creation): copied as a whole to the lanes of a batch call
// and to the peers of a multi-device call.
struct Settings {
    uint64_t ransac_seed = 0;
    int ransac_iters = kRansacMaxIter;
    int estimator = 0;            // 0 = RANSAC (reference default), 1 = PROSAC, 2 = DirectEstimator, 3 = diamond space (CHT)
    int prosac_T_N = -1;
    int cht_d = 128;              // accumulator size of estimator 3
    int batch_streams = 5;
    int flood_mode = 1;
    bool flood_giant_step = true;  // the lowest active seed's flood by the whole device when it outgrows the LDS tiers (kernels_flood.hip: kCtrlGiantStep); lr_set_flood_giant_step, LIBRECTIFY_FLOOD_GIANT_STEP=0
    bool flood_jit = true;       // single calls enqueue the flood's later rounds just in time (kernels_flood.hip: flood_enqueue); LIBRECTIFY_FLOOD_JIT=0
    bool flood_partial = true;  // partial commits of blocked seeds (kernels_flood.hip); lr_set_flood_partial_commits
    bool flood_log_sweep = false;  // test hook (lr_set_flood_logs(ctx, 2)): every footprint worked out from a log goes the fall-back way (sweeps)
    bool flood_logs = true;     // blocked seeds work their next footprint out from the records of their last walk (kernels_flood.hip: flood_rewalk_kernel); lr_set_flood_logs, LIBRECTIFY_FLOOD_LOGS=0
    bool flood_staged = false;  // lr_set_flood_staged: the rounds start on the strongest eighth of the seeds (test / experiment hook)
    bool fit_prune = true;      // fused frames leave out the fit of floods too small to pass the frame's length test (kernels_fit.hip: component_offsets_kernel); lr_set_estimator(ctx, 0, 0) fits them all
    // Stage timers (HIP events between the stages of a frame): off in the frame calls unless lr_set_stage_timing or
    // LIBRECTIFY_STAGE_TIMES asks -- every event record is a barrier packet in the stream, some 6 us of idle GPU each,
    // seven of them per frame.  The staged API (lr_stage_*) always times its stages.
    bool timing_on = false;
};

// The groups below are what lr_context_trim gives back: each is reset as a whole (ctx_trim).

// per-pixel workspace, sized by the largest frame seen (ctx_ensure_image_capacity)
struct Workspace {
    size_t cap_pix = 0;
    int cap_tiles = 0;
    // stage 1
    DeviceBuffer<float> dx, dy;
    DeviceBuffer<uint8_t> dmask;
    DeviceBuffer<uint64_t> cand;
    DeviceBuffer<uint32_t> cand_count, tile_max;
    // stage 2
    DeviceBuffer<uint32_t> tile_pass;
    DeviceBuffer<uint32_t> tile_off;  // (the fused seed selection keeps its workgroups' status words here: zeroed when allocated)
    DeviceBuffer<uint64_t> keys_a, keys_b;
    DeviceBuffer<int32_t> seed_idx, seed_bin;
    DeviceBuffer<float> seed_thr;
    DeviceBuffer<uint4> seed_rec;  // the three arrays above, a record per seed (FloodFrame::seed_rec)
    DeviceBuffer<int32_t> seed_size;
    // stage 3
    DeviceBuffer<uint32_t> label;
    DeviceBuffer<int32_t> queue;
    // stage 4
    DeviceBuffer<uint32_t> comp_rank, comp_seed, comp_off, cursor, px_a, px_b;
    DeviceBuffer<float> scratch_w;
    DeviceBuffer<LineSegment> d_lines;
    DeviceBuffer<unsigned char> temp;     // (cap() = its bytes)
    DeviceBuffer<uint32_t> comp_large;    // components of more than 64 pixels (sorted by a workgroup each)
    DeviceBuffer<uint32_t> huge_tab, huge_list, huge_jobs;
    HugeSort huge;                        // ... of more than 2^14: buckets (kernels_fit.hip: huge_count_kernel), pointing into the three above
};

// the parallel flood's per-seed buffers, logs and slabs; `fb` is what the kernels get (by value), pointing into the owners
struct FloodStore {
    DeviceBuffer<uint32_t> blocked, count, flags, blk, act_a, act_b, ctrl, big_list, handover, rewalk_list, log_off, log_len, log_buf;
    DeviceBuffer<uint8_t> state, tier, dirty;
    DeviceBuffer<uint64_t> giant_mask;
    DeviceBuffer<uint4> slab_ring, slab_hash;
    FloodBuffers fb;
    size_t cap_seeds = 0;
};

// Host-buffer entry points (the reference's only kind, image.cpp:11-19): frames go through one of two device
// slots on a copy stream of their own, so the upload of a lane's next frame overlaps the kernels of its current
// one.  Pageable sources are first copied (in row bands, by `upload_threads` host threads) into a pinned staging
// buffer per slot; sources that are already page-locked (lr_host_alloc, hipHostMalloc, hipHostRegister) are
// DMA-copied where they lie.
struct FrameSlots {
    DeviceBuffer<float> slot[2];
    PinnedBuffer<float> stage[2];
    // Device frames whose rows span 4 GiB or more (the filter kernel addresses a frame with 32-bit byte offsets) are
    // first copied here, packed, on the context's stream (enqueue_filter).
    // (of the frame's own format: an 8-bit frame is packed as bytes)
    DeviceBuffer<float> packed;
    // An interleaved 8-bit frame (LR_PIX_U8X3) becomes luma / 256 here, by one launch of the prepare kernel at the
    // frame's own size on the context's stream, and the fp32 filter reads this (enqueue_filter).
    DeviceBuffer<float> luma;
};

// Batch calls on host frames: a ring of device frames (and, for pageable frames, of page-locked staging buffers)
// that ONE uploader fills in frame order on the copy stream, as far ahead of the lanes as the ring allows
// (upload.hip: BatchUploader).
struct UploadRing {
    std::vector<DeviceBuffer<float>> img;
    std::vector<PinnedBuffer<float>> stage;
    size_t cap_pix = 0, stage_cap_pix = 0;
    void drop() {  // the memory goes, the ring keeps its length
        for (auto& b : img) b.reset();
        for (auto& b : stage) b.reset();
        cap_pix = stage_cap_pix = 0;
    }
};

// LR_WARP_PREPARE (kernels_prepare.hip): the span table of the last (source size, output size), made on the
// host in page-locked memory and kept on the device while the sizes repeat
struct PrepareSpans {
    MirroredBuffer<unsigned char> spans;  // (cap() = bytes: output width + output height entries)
    int key[4] = {0, 0, 0, 0};            // width, output width, height, output height of the table ([0] = 0: none)
    float w_in[2] = {0.f, 0.f};           // (float)(1 / scale) of the table's two axes
    // LR_WARP_RAGGED | LR_WARP_PREPARE: a call's frame records, tile prefix table and span tables (made per call, sized by
    // the call: cap() = bytes)
    MirroredBuffer<unsigned char> ragged;
};

// lr_draw_lines_device (kernels_overlay.hip): a call's frame records, tile prefix table, bins, index lists and segment
// records (made per call, sized by the call: cap() = bytes)
struct OverlayStore {
    MirroredBuffer<unsigned char> block;
};

// lr_encode_jpeg_device (kernels_jpeg.hip): a call's frame records, prefix tables and code tables going up and the streams'
// lengths coming back (block), the quantised coefficients (2 bytes per sample of the padded components), the restart
// intervals' lengths and places in their streams, and for the frames with LR_JPEG_OPTIMIZE the counters of their symbols (544
// a frame, zeroed on the stream by every call that counts); all sized by the call
struct JpegStore {
    MirroredBuffer<unsigned char> block;
    DeviceBuffer<int16_t> coef;
    DeviceBuffer<uint32_t> len;
    DeviceBuffer<unsigned long long> place;
    DeviceBuffer<unsigned long long> counts;
};

// lr_decode_jpeg_device (kernels_jpeg_decode.hip): a call's frame records (code tables and divisors in them), prefix tables
// and flags going up and the frames' results coming back (block), the coefficients (2 bytes per sample of the padded
// components; the transform leaves the samples in their place), and per 128-byte part of a scan its entry and exit states,
// counts, number of decodes and first block; all sized by the call
struct JpegDecodeStore {
    MirroredBuffer<unsigned char> block;
    DeviceBuffer<int16_t> coef;
    DeviceBuffer<unsigned long long> state;  // entry | exit | carry (two of them)
    DeviceBuffer<uint32_t> part;             // counts | tries | first block
};

// lr_pack_tensor_device (kernels_tensor.hip): a call's frame records, tile prefix table and the 256 x C elements (made per
// call, sized by the call: cap() = bytes)
struct TensorStore {
    MirroredBuffer<unsigned char> block;
};
}  // namespace lramd

struct lr_context {
    lr_context();
    ~lr_context();
    int device = 0;
    lramd::Stream stream, copy_stream;  // (first: everything below is gone before they are)
    lramd::Settings opt;

    int w = 0, h = 0;  // the last frame
    lramd::Workspace ws;
    lramd::FloodStore flood;
    lramd::FrameSlots frames;
    lramd::UploadRing ring;
    lramd::PrepareSpans prep;
    lramd::Event ev_prep_spans;  // the last upload from prep.spans.h
    lramd::Event ev_prep_ragged;  // the last upload from prep.ragged.h
    lramd::OverlayStore overlay;
    lramd::Event ev_overlay;  // the last upload from overlay.block.h (rewritten only once that has been read)
    lramd::JpegStore jpeg;

    lramd::Event ev_up[2];
    lramd::Event ev_wait;  // (blocking-sync flag) what a batch lane sleeps on
    std::vector<lramd::Event> band_ev;  // single host frames: one event per 4 MB upload band (the filter follows the bands)
    std::vector<lramd::Event> ring_ev;
    std::unique_ptr<lramd::StagingCrew> crew;  // single host frames: threads kept from call to call
    int crew_helpers = 0;
    bool sleep_in_wait = false;
    uint32_t fit_tag = 0;              // tag of the last component scan (kernels_fit.hip: component_offsets_kernel)
    bool batch_no_register = false;    // a multi-device call whose blocks overlap: its frames are staged, none is page-locked in place
    int register_slow_calls = 0;       // batch calls still to go with the staging copy after pinning frames in place turned out slow (upload.hip: BatchUploader)
    uint32_t select_tag = 0;           // tag of the last seed selection on this context (kernels_seeds.hip: seed_select_kernel)
    lramd::DeviceBuffer<float> maxmag;
    lramd::DeviceBuffer<uint32_t> d_counts;  // [0] n_seeds, [1] n_comp, [2] n_px, [3..] flood scratch
    uint32_t seed_cap = 0;           // capacity the seed sort runs with (the seed count is not known when it is enqueued)
    uint32_t seed_cap_once = 0;      // test hook: capacity of the next frame's seed sort
    int frame_laps = 0;              // laps the last frame took (1; 2 if the seed sort overflowed or the flood needed more rounds)
    lramd::FloodProgress flood_prog;
    bool keep_workspace = false;  // a batch call with a frame table: its lanes are sized once for the call's largest frame and the count below rests
    int small_frames = 0;  // frames in a row of at most a quarter of the workspace's capacity (ctx_ensure_image_capacity gives it back after eight)
    // filter_lines + peeling on the device (kernels_groups.hip)
    size_t cap_glines = 0;
    lramd::DeviceBuffer<float> d_tables;      // 3 pencil tables (all lines, two ping-pong round tables) x 8 arrays x cap_glines
    lramd::DeviceBuffer<uint32_t> d_orig;     // 3 x cap_glines
    lramd::DeviceBuffer<float> d_inl;         // 4 x cap_glines: (h, length) of a round's inliers beyond those staged in LDS
    lramd::DeviceBuffer<LineSegment> d_flines;  // filtered (then grouped) lines
    lramd::DeviceBuffer<uint32_t> d_gctl;     // peeling control block (kGc*)
    lramd::DeviceBuffer<float> d_gnorm;       // bounding-box centre and scale
    lramd::DeviceBuffer<float> d_models;      // refit model of each round
    lramd::PinnedBuffer<uint8_t> h_res;       // header (counts, control block, models) + the first res_lines_cap lines
    size_t res_lines_cap = 0;
    // grow-on-demand workspaces of the opt-in paths
    lramd::DeviceBuffer<float> d_refine_table;
    lramd::DeviceBuffer<uint2> d_refine_edges;
    lramd::DeviceBuffer<unsigned long long> d_cht_acc;
    lramd::MirroredBuffer<uint32_t> cht_idx;   // lines a peeling round of the diamond-space estimator takes out of the accumulator
    lramd::MirroredBuffer<uint32_t> cht_peak;  // {cell, value lo, value hi, -, votes lo, votes hi}
    // lr_warp_perspective_device: the frames' maps (9 doubles each) go up from page-locked memory on the context's stream;
    // with LR_WARP_PACKED or LR_WARP_RAGGED a record of 18 doubles per frame and the tiles' prefix table (sized by the
    // batch: ctx_trim)
    lramd::MirroredBuffer<double> warp_m;
    lramd::Event ev_warp_m;    // the last upload from warp_m.h (rewritten only once that has been read)
    // RANSAC
    lramd::MirroredBuffer<float> model;  // 8 arrays of lines
    lramd::DeviceBuffer<unsigned long long> d_best_slots;  // kRansacBestSlots words: a scoring launch's best (score, iteration), cleared by its reader
    // PROSAC / Hough weights (opt-in estimator)
    lramd::MirroredBuffer<int32_t> pairs;   // 2 x ht_pairs
    lramd::DeviceBuffer<float> d_peak;      // 3 floats
    lramd::MirroredBuffer<float> weights;   // one per line
    lramd::MirroredBuffer<uint32_t> samples;  // 2 buffers x 2 x chunk
    lramd::MirroredBuffer<uint32_t> hcounts;  // 2 x chunk
    lramd::MirroredBuffer<uint32_t> rec;      // PROSAC: new-best iterations of a chunk ([0] = how many) ...
    lramd::MirroredBuffer<uint8_t> recflags;  // ... and a row of inlier flags for each (two chunk buffers of each)
    lramd::Event prosac_ev[2];  // end of a chunk's work on the stream
    std::vector<int> prosac_imin;    // prosac.h's Imin(2, n) by n (constants of prosac.h:62-66 only)
    std::vector<lr_context*> workers;  // extra contexts (own stream + workspace) for frames in flight in batch calls
    std::vector<lr_context*> peers;    // one context per entry of the device list of the last multi-device batch call (each with its own lanes)
    // pinned host scalars
    lramd::PinnedBuffer<uint32_t> h_counts;  // 8 words of counts; + 16: the flood's control block; + 72: the words the flood's rounds report in
    lramd::PinnedBuffer<float> h_best;       // [0] score, [1] iter (as int bits)

    // constants
    lramd::FilterConsts fconsts;
    lramd::BinTrig trig;
    float seed_keep_ratio = 0.f;

    // state of the last run
    uint32_t n_seeds = 0, n_comp = 0, n_px = 0;
    int flood_rounds = 0;
    int flood_rounds_hint = 10;  // rounds the next flood enqueues blindly
    int flood_rounds_last = 0;   // rounds the last flood needed (0: none yet)
    // what a batch call gives its lanes for the length of the call (batch.hip: LaneSet; 0 / false otherwise)
    int flood_jit_sleep_us = 0;  // (when they enqueue just in time at all: pause between looks)
    bool flood_logbig_off = false;  // no logs of second-tier walks
    int flood_log_min = 0, flood_log_walk = 0;  // thresholds of the logs (0: the defaults; the lanes get 32 and 24)
    bool flood_logbig_hint = true;  // did the last frame have walks in the second tier? (their logs need a launch of their own per round: kernels_flood.hip, flood_rewalk_kernel)
    bool flood_big_hint = true;  // did the last frame's walks outgrow the first storage tier? (none yet: assume so)
    bool flood_hold_hint = false;  // did the last frame hold its weakest seeds back?
    int flood_staged_streak = 0;     // frames in a row that started staged (every sixteenth starts without the hint)
    bool flood_staged_hint = false;  // was the last frame one of overlapping giants (kernels_flood.hip: kCtrlStaged)?  Then this one starts on its strongest quarter
    bool flood_calm_hint = false;      // the last frame's walks all stayed in the first storage tier (FloodBuffers::calm_hint)
    uint32_t flood_tiers[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // last flood: seeds in the second tier, slabs used, seeds of the ordered tail, hold-back, walked px (lo, hi), steps (lo, hi), walks beyond the first tier's table, rounds enqueued under the schedule hook, re-walks from logs, logs given up, giants held back
    lramd::Event ev[16];  // stage timers (Settings::timing_on)
    float stage_ms[LR_T_COUNT] = {};
    double host_ms[3] = {0, 0, 0};  // last frame: enqueue, next-frame staging + upload, wait (LIBRECTIFY_LANE_DEBUG)
    bool stage_valid[4] = {false, false, false, false};
    bool dmask_consumed = false;  // the parallel flood clears the mask of labelled pixels: LR_BUF_DMASK is then stale
    // (last: the members above keep the places they had before it came)
    lramd::JpegDecodeStore jpeg_decode;
    // test hook (lr_set_flood_schedule; FloodBuffers::sched_order): the caller's single calls and stage calls only -- not part
    // of Settings, so no lane or peer gets it, and a batch call switches its caller's off while it runs (batch.hip: LaneSet)
    int flood_sched_order = 0;
    uint32_t flood_sched_seed = 0, flood_sched_width = 0;
    bool flood_sched_off = false;
    lramd::TensorStore tensor;
};

namespace lramd {
constexpr size_t kResHeaderBytes = 256;
int ctx_create(int device, lr_context** out);
void ctx_destroy(lr_context* c);
const std::string& get_error();
int ctx_ensure_image_capacity(lr_context* c, int w, int h);
int ctx_reserve_workspace(lr_context* c, size_t npix, int ntiles);
int ctx_trim(lr_context* c, bool frames_too);
int ctx_ensure_ransac_capacity(lr_context* c, size_t n_lines);
int ctx_stage_filter(lr_context* c, const float* d_image, int w, int h, int stride);
int ctx_stage_seeds(lr_context* c);
int ctx_stage_flood(lr_context* c);
int ctx_stage_fit(lr_context* c, std::vector<LineSegment>& out);
int ctx_detect(lr_context* c, const float* d_image, int w, int h, int stride, std::vector<LineSegment>& raw);
int ctx_ransac_best(lr_context* c, const PencilModel& model, const std::vector<int>& indices, float tol, int n_iter,
                    uint64_t seed, uint32_t round, Vec3* best_h, float* best_score, int* best_iter);
struct ProsacTrace {
    int iterations = 0, n_star = 0, best_iter = -1, I_N_best = 0;
};
int ctx_ht_weights(lr_context* c, const PencilModel& model, const std::vector<int>& indices, std::vector<float>& weights);
int ctx_prosac_solve(lr_context* c, const PencilModel& model, const std::vector<int>& indices, float tol, int T_N,
                     uint64_t seed, uint32_t round, Vec3* h, ProsacTrace* trace);
int ctx_estimate_line_pencils_prosac(lr_context* c, std::vector<LineSegment>& lines, int max_models, float inlier_deg,
                                     float garbage_deg, int T_N, uint64_t seed);
int ctx_estimate_line_pencils(lr_context* c, std::vector<LineSegment>& lines, int max_models, float inlier_deg,
                              float garbage_deg, int n_iter, uint64_t seed);
int ctx_direct_solve(lr_context* c, const PencilModel& model, const std::vector<int>& indices, Vec3* h);
int ctx_estimate_line_pencils_direct(lr_context* c, std::vector<LineSegment>& lines, int max_models, float inlier_deg,
                                     float garbage_deg);
int ctx_cht_vanishing_point(lr_context* c, const std::vector<LineSegment>& lines, int d, Vec3* vp,
                            std::vector<uint64_t>* acc_out);
struct ChtTrace {
    std::vector<Vec3> models;          // refit of each round (normalised coordinates)
    std::vector<uint32_t> peak_cell;   // winning accumulator cell of each round
    uint64_t votes = 0;                // cells voted for (added or taken back) over the call
};
int ctx_estimate_line_pencils_cht(lr_context* c, std::vector<LineSegment>& lines, int max_models, float inlier_deg,
                                  float garbage_deg, int d, ChtTrace* trace);
int ctx_refine(lr_context* c, std::vector<LineSegment>& lines);
// (the frame entries below: `format` is the frames' lr_pixel_format, strides are in pixels of it)
int ctx_find_groups_device(lr_context* c, const void* d_image, int format, int w, int h, int stride, float min_length, bool refine,
                           std::vector<LineSegment>& out);
int ctx_find_groups_host(lr_context* c, const void* buffer, int format, int w, int h, int stride, float min_length, bool refine,
                         int num_threads, std::vector<LineSegment>& out);
int ctx_find_groups_batch_device(lr_context* c, const void* d_images, int format, size_t image_stride, int batch, int w, int h,
                                 int stride, float min_length, bool refine, LineSegment* out, int capacity, int* n_lines,
                                 const RectificationConfig* cfg, ImageTransform* transforms);
// the same call with width == 0 && height == 0: `frames` is a HOST table of lr_frame records, every frame its own size
int ctx_find_groups_frames_device(lr_context* c, const lr_frame* frames, int format, bool tagged, int batch, float min_length,
                                  bool refine, LineSegment* out, int capacity, int* n_lines, const RectificationConfig* cfg,
                                  ImageTransform* transforms);
// host-resident frames (any stride sign, pageable or page-locked): staged uploads overlap the kernels
int ctx_find_groups_batch_host(lr_context* c, const void* const* frames, int format, int batch, int w, int h, int stride,
                               float min_length, bool refine, int num_threads, LineSegment* out, int capacity,
                               int* n_lines, const RectificationConfig* cfg, ImageTransform* transforms);
// The same over several devices of this process ("one host thread + stream set per device"): frames are
// dealt in contiguous blocks of ceil(batch / n_devices), block i to devices[i] (a device may be listed more than once:
// every entry gets a lane set of its own), results land in the caller's arrays; no collective, it is one process.
int ctx_find_groups_batch_host_multi(lr_context* c, const int* devices, int n_devices, const void* const* frames, int format, int batch,
                                     int w, int h, int stride, float min_length, bool refine, int num_threads,
                                     LineSegment* out, int capacity, int* n_lines, const RectificationConfig* cfg,
                                     ImageTransform* transforms);
// Enqueues the upload of a host frame into device slot `slot` on the copy stream and records ev_up[slot];
// the caller makes its compute stream wait on that event.  num_threads: the reference's knob (threading.h:24-27),
// here the number of host threads that stage a pageable frame (< 0: serial, as there).
int ctx_upload_frame(lr_context* c, int slot, const float* buffer, int w, int h, int stride, int num_threads);
// kernels_warp.hip: lr_warp_perspective_device (validates its arguments, uploads the maps, enqueues one launch)
int ctx_warp_perspective(lr_context* c, const void* d_src, size_t src_image_bytes, int batch, int width, int height,
                         size_t src_row_bytes, int format, const double* M, void* d_dst, size_t dst_image_bytes,
                         int out_width, int out_height, size_t dst_row_bytes);
// kernels_prepare.hip: the same entry with LR_WARP_PREPARE in `format` (the low byte arrives here): luma / 256, area-averaged
// to the output size as f32 gray
int ctx_prepare_frames(lr_context* c, const void* d_src, size_t src_image_bytes, int batch, int width, int height,
                       size_t src_row_bytes, int format, void* d_dst, size_t dst_image_bytes, int out_width,
                       int out_height, size_t dst_row_bytes);
// LR_WARP_RAGGED (kernels_warp.hip): a row of the caller's table as integers, and the check of the whole table that the warp
// and the prepare step share (sets the error and returns 1 on the first fault; tile_w x tile_h: the caller's destination tiles)
struct RaggedEntry {
    uint64_t ow, oh, dst_off, dst_row, w, h, src_off, src_row;
};
int ragged_parse(const void* d_src, size_t src_bytes, int batch, int width, int height, size_t src_row_bytes, int format,
                 bool prepare, const double* T, const void* d_dst, size_t dst_bytes, int out_width, int out_height,
                 size_t dst_row_bytes, int tile_w, int tile_h, std::vector<RaggedEntry>& out, int64_t* n_tiles);
// kernels_prepare.hip: LR_WARP_RAGGED | LR_WARP_PREPARE (the low byte of `format` arrives here; T: 18 doubles per frame)
int ctx_prepare_ragged(lr_context* c, const void* d_src, size_t src_bytes, int batch, int width, int height, size_t src_row_bytes,
                       int format, const double* T, void* d_dst, size_t dst_bytes, int out_width, int out_height,
                       size_t dst_row_bytes);
// kernels_overlay.hip: lr_draw_lines_device (validates the whole table, turns the segments into integer records and bins them
// on the host, uploads them and enqueues one launch)
int ctx_draw_lines(lr_context* c, const void* d_src, size_t src_bytes, int format, const LineSegment* lines, size_t n_lines,
                   const double* frames, int batch, const double* H, void* d_dst, size_t dst_bytes);
// kernels_jpeg.hip: lr_encode_jpeg_device (validates the whole table, builds the headers and tables on the host, enqueues the
// transform, the two entropy passes and the scan between them, and waits for the streams' lengths)
int ctx_encode_jpeg(lr_context* c, const void* d_src, size_t src_bytes, int format, const double* frames, int batch, void* d_dst,
                    size_t dst_bytes, uint64_t* sizes);
// kernels_jpeg_decode.hip: lr_decode_jpeg_device (validates the whole table, reads the headers on the host, enqueues the
// entropy decoder's rounds, the placement, the coefficient pass, the DC scan, the inverse transform and the output pass, and
// waits for the statuses); d_dst == NULL: the headers only, and then c may be NULL
int ctx_decode_jpeg(lr_context* c, const void* d_src, const void* h_src, size_t src_bytes, int format, const double* frames,
                    int batch, void* d_dst, size_t dst_bytes, int32_t* info);
// kernels_tensor.hip: lr_pack_tensor_device (validates the whole call, computes the elements' table on the host, uploads it with
// the frame records, enqueues one launch and waits for the stream)
int ctx_pack_tensor(lr_context* c, const void* d_src, size_t src_bytes, int format, const lr_tensor_args* args, int batch,
                    void* d_dst, size_t dst_bytes);
// bytes one frame spans: (rows - 1) * row_bytes + last_row_bytes; false if that does not fit in 64 bits
inline bool frame_span(int rows, size_t row_bytes, size_t last_row_bytes, size_t* out) {
    size_t s;
    if (__builtin_mul_overflow((size_t)(rows - 1), row_bytes, &s) || __builtin_add_overflow(s, last_row_bytes, &s)) return false;
    *out = s;
    return true;
}
}  // namespace lramd
