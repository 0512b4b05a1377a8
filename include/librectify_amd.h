/*
 * librectify_amd.h — extensions of the MI355X build beyond the reference's six functions.
 *
 * Plain C ABI (pointers and sizes only).  Everything here is additive: the drop-in symbols
 * of include/librectify.h behave as the reference's (src/interface.cpp) and are thin
 * wrappers over a thread-local context of this API.
 *
 * Why these exist:
 *  - the reference API takes a host buffer and has no device/stream notion
 *    (src/librectify.h:111-116); a caller that already holds frames in HBM, or wants many
 *    frames in flight, needs device-pointer and batch entry points;
 *  - parity tests and bench.py need stage-level access (filter / seeds / flood / fit /
 *    RANSAC scoring) and per-stage HIP-event timings.
 *
 * All functions return 0 on success, non-zero on failure (lr_last_error() has the text).
 * No function falls back to a CPU path: if no GPU is present they fail.
 */
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "librectify.h"

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#ifdef __cplusplus
using librectify::ImageTransform;
using librectify::LineSegment;
using librectify::Point;
using librectify::RectificationConfig;
extern "C" {
#endif

typedef struct lr_context lr_context;
enum lr_pixel_format { LR_PIX_U8 = 0, LR_PIX_U8X3 = 1, LR_PIX_F32 = 2 };

/* ---- context ------------------------------------------------------------------------- */
/* One context = one device, one HIP stream, one reusable workspace.  Not thread-safe; use
 * one context per host thread (the drop-in functions do exactly that). */
int lr_context_create(int device, lr_context** out);
void lr_context_destroy(lr_context* ctx);
/* The drop-in functions keep one context per calling host thread (device workspace of about 130 bytes per pixel of the
 * largest frame seen, 36 MB of flood overflow slabs, 32 MB of hand-over records, page-locked staging, staging threads) until the thread exits;
 * a thread that is done with the library for a while can give it back at once.  The next call makes a new one. */
void lr_release_thread_context(void);
/* The reference is stateless; a context is not: its device workspace is sized by the LARGEST frame it has seen (an 8192 x 8192
 * call leaves 8.9 GB behind).  It shrinks by itself -- after eight frames in a row of at most a quarter of its capacity the
 * workspace is given back and allocated again at the size in use -- and on request: lr_context_trim frees everything that is
 * sized by frames (workspace, flood buffers and slabs, frame slots, page-locked staging, the batch ring; streams and events
 * stay), the next call allocates what it needs.  lr_trim_thread_context does that for the calling thread's drop-in context
 * and keeps the context, where lr_release_thread_context destroys it. */
int lr_context_trim(lr_context* ctx);
int lr_trim_thread_context(void);
const char* lr_last_error(void);
int lr_synchronize(lr_context* ctx);
/* RANSAC sample stream seed (the reference seeds from std::random_device, estimator.h:35;
 * this build is reproducible: default 0 or env LIBRECTIFY_SEED). */
void lr_set_ransac_seed(lr_context* ctx, uint64_t seed);
/* RANSAC iterations per model (reference config.h:36 RANSAC_MAX_ITER = 10000). */
void lr_set_ransac_iterations(lr_context* ctx, int n_iter);
/* Flood implementation: 0 = ordered single-wave (simple, slow), 1 = parallel rounds (default);
 * 2 / 3 / 4 = test hooks: parallel rounds without the second LDS storage tier and with no / two / all overflow
 * slabs (exhausted-storage and slab paths; lr_stage_counters tells which storage a frame used); 5 = second tier with
 * room for one seed per round and no slab (a stall while the weakest seeds are held back); 6 / 7 = the second tier's team of
 * wavefronts runs out of storage after 200 tiles and hands the walk to a slab / has no slab to hand it to.
 * All modes give identical results. */
void lr_set_flood_mode(lr_context* ctx, int mode);
int lr_device_count(void);

/* ---- full path ------------------------------------------------------------------------ */
/* 8-bit frames.  The six lr_find_line_segment_groups_* entries below take the frames' pixel format in their `refine`
 * argument, which is a word: if it is non-negative, its bits 16 and up are zero and its bits 8-15 are 1, 2 or 3, the
 * frames are of lr_pixel_format (bits 8-15) - 1 and the reference's flag is (refine & 0xFF) != 0.  EVERY OTHER VALUE MEANS
 * WHAT IT ALWAYS MEANT: refine != 0 on fp32 frames -- 0, 1, -1, `true` are untouched; only the values 256 .. 1023 changed
 * their meaning (they were "refine on").  With a format word
 *  - the `const float*` frame parameters take the frames' address whatever the format: cast it
 *    ((const float*)bytes; nothing is read through it as float).  8-bit frames need no alignment, of pointer or of stride;
 *  - `stride` and `image_stride` stay in PIXELS of the frames' format: rows are stride * bpp bytes apart, bpp = 1 (u8),
 *    3 (u8x3, interleaved) or 4 (f32); any sign for host frames, as image.cpp:11-19;
 *  - the detector runs on p = float(luma) * (1/256.f), which is exact: luma is the byte (u8) or
 *    (4899 c0 + 9617 c1 + 1868 c2 + 8192) >> 14 (u8x3, the prepare step's); the result is, bit for bit, that of the fp32
 *    frame p.  A u8 frame is read by the filter kernel itself, byte by byte: no fp32 copy of it exists anywhere and a
 *    quarter of the bytes crosses the link and the host's memory.  A u8x3 frame (3 B/px on the link) becomes p in a
 *    buffer of the context by one launch on the frame's stream, and the fp32 filter reads that;
 *  - a frame smaller than 5 x 5 is answered as the drop-in symbol answers it: success, *n_lines = 0 (the plain flag keeps
 *    its error return).
 * The drop-in find_line_segment_groups (bool refine, float buffer) and the stage API (lr_stage_filter*) stay fp32. */
enum lr_frames_option { LR_FRAMES_U8 = 0x100, LR_FRAMES_U8X3 = 0x200, LR_FRAMES_F32 = 0x300 }; /* or-ed into `refine`: (lr_pixel_format + 1) << 8 */
/* find_line_segment_groups on an image already resident in HBM (row-major float, `stride`
 * elements between rows, stride >= width).  Writes at most `capacity` segments to the HOST
 * array `out`; *n_lines is the number found (0 on the reference's NULL paths,
 * interface.cpp:50-54,65-69). */
int lr_find_line_segment_groups_device(lr_context* ctx, const float* d_image, int width, int height, int stride,
                                       float min_length, int refine, int num_threads, LineSegment* out, int capacity,
                                       int* n_lines);
/* Same, host buffer (any stride sign, as the reference: image.cpp:11-19).  An 8-bit frame travels as it is: staged and
 * sent in bands of 4 MB (four times as many rows as of an fp32 frame), the filter following the bands (u8). */
int lr_find_line_segment_groups_host(lr_context* ctx, const float* buffer, int width, int height, int stride,
                                     float min_length, int refine, int num_threads, LineSegment* out, int capacity,
                                     int* n_lines);
/* Batch of `batch` device-resident frames of one size, frame b at d_images + b*image_stride.
 * Output b goes to out + b*capacity; n_lines[b]; transforms[b] (may be NULL) is
 * compute_rectification_transform(lines_b, cfg). */
int lr_find_line_segment_groups_batch_device(lr_context* ctx, const float* d_images, size_t image_stride, int batch,
                                             int width, int height, int stride, float min_length, int refine,
                                             int num_threads, LineSegment* out, int capacity, int* n_lines,
                                             const RectificationConfig* cfg, ImageTransform* transforms);
/* The same entry with width == 0 && height == 0 (and batch >= 1): every frame has its OWN size.  d_images is then a HOST
 * array of `batch` lr_frame records (cast to const float*), image_stride must be sizeof(lr_frame) (the layout check) and
 * stride must be 0.  data: the frame's DEVICE address; stride: in pixels of the frames' format (the `refine` word's, fp32
 * for a plain flag), >= width; min_length < 0: the call's min_length.  Output b goes to out + b*capacity, n_lines[b] is the
 * number found (even above capacity), transforms[b] is compute_rectification_transform for width_b x height_b.  The whole
 * table is checked before anything is launched (a null data, a size below 1, a stride below the width, a misaligned f32
 * address fail the call); a frame below 5 x 5 is answered as elsewhere (format word: n_lines[b] = 0 and the no-lines
 * transform; plain flag: the call fails).  Every frame's result is, bit for bit, lr_find_line_segment_groups_device's on
 * that frame alone, whatever its position, the number of lanes and the lane that took it.  The lanes' workspaces are
 * sized once, before the first frame, for the call's largest frame, and none is given back while the call runs.  The
 * other five lr_find_line_segment_groups_* entries keep refusing 0 x 0. */
typedef struct lr_frame { const void* data; int32_t width, height, stride; float min_length; } lr_frame; /* 24 bytes */

/* Batch of `batch` HOST-resident frames of one size, frame b at frames + b*image_stride (elements), rows `stride`
 * elements apart (any sign, as image.cpp:11-19).  This is the reference's own kind of input, many frames at once.
 * ONE uploader thread sends the frames, in frame order, on the context's (high-priority) copy stream into a pool of
 * lanes + 6 device frames (LIBRECTIFY_RING_EXTRA overrides the 6; never more than 2 GiB or `batch` frames: 0.5 GiB
 * of device memory for 4K frames with six lanes), so the link runs ahead of the lanes; a lane only makes its stream
 * wait for its frame's transfer.  Page-locked memory (lr_host_alloc, hipHostMalloc, hipHostRegister) is DMA-copied
 * where it lies.  Pageable memory goes through page-locked staging buffers -- as many as there are pool slots, i.e.
 * the same amount again in pinned host memory, allocated when a call first meets a pageable frame -- filled in 4 MB
 * row bands by `num_threads` host threads shared by the whole call (the reference's knob, threading.h:24-27: < 0 or
 * 1 = the uploader alone; capped at 8 and at the host's cores), started once per call.  By default pageable frames are
 * instead page-locked where they lie for the length of the call (LIBRECTIFY_REGISTER_FRAMES): only the whole pages INSIDE a
 * frame -- frames of one array share the page at each end, and no page is registered twice; the few rows that reach into
 * those pages take the staging buffer (and the frame's lane fetches them), and so does every frame that overlaps an earlier one of the call.  Outputs as for
 * the device batch. */
int lr_find_line_segment_groups_batch_host(lr_context* ctx, const float* frames, size_t image_stride, int batch,
                                           int width, int height, int stride, float min_length, int refine,
                                           int num_threads, LineSegment* out, int capacity, int* n_lines,
                                           const RectificationConfig* cfg, ImageTransform* transforms);
/* Same with one pointer per frame. */
int lr_find_line_segment_groups_batch_host_ptrs(lr_context* ctx, const float* const* frames, int batch, int width,
                                                int height, int stride, float min_length, int refine, int num_threads,
                                                LineSegment* out, int capacity, int* n_lines,
                                                const RectificationConfig* cfg, ImageTransform* transforms);
/* The same batch over SEVERAL devices of this process -- what a C / C++ caller of the reference's kind (one process, no
 * launcher: src/autorectify.cpp:136,350) needs to use the eight GPUs of a node.  Frames are dealt in contiguous blocks of
 * ceil(batch / n_devices), block i to devices[i]; every entry of the list gets a context of its own (kept with `ctx` from
 * call to call, configured like `ctx`: seed, iterations, estimator, lr_set_batch_streams lanes per device) with its own
 * uploader, copy stream, lanes and pool, driven by a host thread of its own; results land in the caller's arrays as for
 * the single-device call.  A device may be listed more than once (two independent lane sets on one GPU: how the call is
 * tested on a one-GPU box).  No collective: it is one process.  `ctx` itself only carries the settings. */
int lr_find_line_segment_groups_batch_host_multi(lr_context* ctx, const int* devices, int n_devices,
                                                 const float* const* frames, int batch, int width, int height, int stride,
                                                 float min_length, int refine, int num_threads, LineSegment* out,
                                                 int capacity, int* n_lines, const RectificationConfig* cfg,
                                                 ImageTransform* transforms);
/* Page-locked host memory for frames (hipHostMalloc / hipHostFree): uploads from it skip the staging copy. */
int lr_host_alloc(lr_context* ctx, size_t bytes, void** out);
int lr_host_free(lr_context* ctx, void* p);

/* Minimal device-memory helpers (hipMalloc / hipFree / synchronous hipMemcpy H2D on the context's device). */
int lr_device_malloc(lr_context* ctx, size_t bytes, void** out);
int lr_device_free(lr_context* ctx, void* p);
int lr_memcpy_h2d(lr_context* ctx, void* dst, const void* src, size_t bytes);
/* The twin of lr_memcpy_h2d: waits for the context's stream first (it is a non-blocking stream, which a plain hipMemcpy
 * would not wait for), then copies `bytes` from device to host. */
int lr_memcpy_d2h(lr_context* ctx, void* dst, const void* src, size_t bytes);
/* Frames kept in flight by the batch call (one host thread + HIP stream + workspace each; default 5). */
void lr_set_batch_streams(lr_context* ctx, int n);
/* Test hooks for the two situations in which a frame takes a second lap (lr_stage_counters [7] tells): the capacity
 * the NEXT frame's seed sort starts with (normally 1.5 x the previous frame's seed count; a frame with more seeds is
 * repeated with room), and the number of flood rounds the next frame enqueues before it looks at the flood's control
 * block (normally the previous frame's rounds + 2; a flood that needs more is completed after the frame's wait, and
 * the stages after it run again). */
void lr_set_seed_capacity(lr_context* ctx, uint32_t cap);
/* Test / experiment hook: start the flood's rounds on the strongest eighth of the seeds and widen the window round by
 * round (same result; it was the batch lanes' setting in round 1). */
void lr_set_flood_staged(lr_context* ctx, int on);
void lr_set_flood_blind_rounds(lr_context* ctx, int rounds);
/* Comparison hook: the flood's partial commits (a blocked seed commits at once the part of its footprint that no lower
 * seed can reach; on by default, LIBRECTIFY_FLOOD_PARTIAL=0 also switches them off).  Same labels either way. */
void lr_set_flood_partial_commits(lr_context* ctx, int on);
/* The flood's later rounds from the logs (kernels_flood.hip: flood_rewalk_kernel): a walk of twelve tiles or more leaves
 * its footprint as (tile, pixels) records, and since a footprint only ever shrinks (filter.cpp:101-153 accepts a pixel on
 * static data and on "not claimed yet"), the seed's next footprint is the connected part around it of those records minus
 * what has been committed since -- labelled in LDS instead of walked tile after tile.  Same labels.  On by default
 * (single 4K frames: flood 1.31 -> 0.92 ms); the lanes of a batch call keep logs only of walks of 32 tiles and more.
 * 0 = off, 1 = on, 2 = on, every log through the fall-back path (test hook).
 * LIBRECTIFY_FLOOD_LOGS=0 turns it off for every new context; lr_stage_counters [11], [12] count the logs worked on and
 * those that took the fall-back path. */
void lr_set_flood_logs(lr_context* ctx, int on);
/* Single calls enqueue the flood's first rounds blindly (what the context's last frame needed, less one; four at most) and every further
 * round only when the host has seen -- in page-locked words the last workgroup of a round writes -- that seeds are left: no
 * launch behind the last round with work (the blind rounds of a 4K frame were 60-120 us of empty launches); the calling
 * thread polls while the flood runs (a single call spins; a lane of a batch call looks every 20 us).  On by default.
 * 0 = blind rounds (the previous frame's count plus two: what lr_set_flood_blind_rounds steers), and a frame whose flood
 * needs more takes a second lap (lr_stage_counters [7]).  LIBRECTIFY_FLOOD_JIT=0 likewise. */
void lr_set_flood_just_in_time(lr_context* ctx, int on);
/* The giant step (kernels_flood.hip: kCtrlGiantStep).  The lowest active seed's flood is what the reference's loop
 * (line_detector.cpp:98-119 over filter.cpp:110-153) does next and nothing about it is speculative: when its walk outgrows
 * the LDS tiers (a smooth region of 100 000 pixels, a ring of a noiseless gradient) the whole device labels it between two
 * rounds -- the seed's acceptance test as a 64-bit mask per 8x8 tile, a union-find over the tiles' components, labels --
 * instead of one team of wavefronts walking it tile after tile through a global slab.  Same labels.  On by default;
 * 0 = the slab walk (comparison), LIBRECTIFY_FLOOD_GIANT_STEP=0 likewise; lr_stage_counters [14] counts the steps. */
void lr_set_flood_giant_step(lr_context* ctx, int on);
/* Test hook: the schedule of the flood's rounds.  The parallel flood is exact because a round's result depends neither on the
 * order nor on the concurrency in which its walks run (DESIGN.md section 7 has the argument, and the table of everything that
 * reads a list by position); this hook makes both a variable, so that a test can choose them instead of taking what the
 * hardware gives.
 *   order: the round's active list as its exploration reads it -- 0 as is, 1 reversed (the exploration reads from the end,
 *          so this walks the strongest seed first), 2 a permutation that depends only on (seed, the round's index, the list's
 *          length): position i takes the entry at (a i + b) mod n, a coprime to n (csrc/common.h: flood_schedule_perm;
 *          librectify_amd.flood_schedule_perm in Python).  A small kernel pair of its own in front of the exploration
 *          rewrites the list; behind a pending giant step it does nothing, like the round.
 *   width: workgroups of every launch of a round that walks a list -- the exploration (`width` workgroups for the last
 *          `width` entries, `width` more that stride over the rest), the second tier's teams, both re-walk launches and the
 *          partial commits.  0 = each launch's own grid; 1 = a serial round, its walks one after the other in list order.
 *          The commit pass and the survivors pass keep their grids (they walk no list of seeds in an order that matters).
 * With the hook set every round brings its `rest` launch, never takes the list's known length for its grid and sets no
 * barrier for entries "the next round will not reach": that path walks the FIRST entries of a list and counts on the order
 * the survivors pass left.  (0, 0, 0) -- the default -- enqueues the rounds as ever; the kernels of the rounds are the same
 * either way.  It applies to single calls and stage calls; the lanes of a batch call ignore it.  lr_stage_counters [10] counts
 * the rounds enqueued under it.  Same labels whatever the schedule. */
void lr_set_flood_schedule(lr_context* ctx, int order, uint32_t seed, int width);

/* ---- rectified images ------------------------------------------------------------------ */
/* The reference demo's last step (autorectify.cpp: homography_from_corners with clip 3.0, then warpPerspective).
 * In float, as the demo: bounding box of the four corners, centre (max + min) / 2, size min(max - min, t->width * clip)
 * (likewise the height), output size = its truncation, origin = centre - 0.5f * size.  In double: H (row-major, H[8] = 1)
 * maps the source corners (0,0), (w,0), (0,h), (w,h) to the corners minus the origin (exact 4-point solve, 8x8 system with
 * partial pivoting); M = H^-1 (adjugate / determinant) is the destination-to-source map lr_warp_perspective_device takes.
 * H or M may be NULL.  Fails (non-zero, lr_last_error) on a non-finite corner, clip <= 0, a size below 1 and a singular
 * system (three collinear corners).  Host only: needs no context and no GPU. */
int lr_rectification_homography(const ImageTransform* t, float clip, double* H, double* M, int* out_width,
                                int* out_height);
/* Bilinear perspective warp of `batch` device frames in ONE launch on the context's stream: frame b at
 * d_src + b*src_image_bytes (rows src_row_bytes apart), its output at d_dst + b*dst_image_bytes (rows dst_row_bytes
 * apart); M: 9 doubles per frame (HOST), the destination-to-source map of that frame; one output size for all.
 * Arithmetic: OpenCV's 8-bit bilinear warp, 5 fractional bits per axis, pixel centres on integer
 * coordinates, a constant zero border (LR_WARP_BORDER below: a border rule per frame).  Formats: u8 gray, u8 interleaved 3-channel, f32 gray (4-byte aligned pointers
 * and strides).  Byte offsets are 64-bit.  Fails cleanly on null pointers, batch < 1, sizes below 1, strides shorter
 * than a row (or, for batch > 1, than a frame), misaligned f32 pointers or strides, an unknown format, a non-finite M. */
int lr_warp_perspective_device(lr_context* ctx, const void* d_src, size_t src_image_bytes, int batch, int width,
                               int height, size_t src_row_bytes, int format, const double* M, void* d_dst,
                               size_t dst_image_bytes, int out_width, int out_height, size_t dst_row_bytes);
/* `format` is a word: its low byte is the source's lr_pixel_format, the bits above it are options (0: the warp above).
 * LR_WARP_PREPARE makes the call the detector's front end, the reference demo's first step (gray, / 256, INTER_AREA
 * prescale) on frames that stay in HBM: the destination is F32 GRAY whatever the source format, its value luma / 256
 * area-averaged from width x height down to out_width x out_height (scale n_src / n_dst per axis, as cv::resize with a
 * dsize; out == src is a pure conversion, exactly v / 256).  Luma: u8 the value; u8x3 (4899 c0 + 9617 c1 + 1868 c2 +
 * 8192) >> 14; f32 the value itself and no / 256 (the caller has scaled it).  M is ignored and may be NULL.  Batched
 * like the warp: one launch on the context's stream, 64-bit byte offsets, the caller's strides (dst_row_bytes >=
 * 4 * out_width).  Arithmetic: per axis destination sample i covers [i s, min(n_src,
 * (i + 1) s)), a tap's weight is its overlap / s computed in double and rounded once to float; h = h + w_x * p over a
 * source row's taps in order, then v = v + w_y * h over the rows in order, every product and sum rounded on its own.
 * Fails cleanly on what the warp rejects and on any other option bit, out_width > width or out_height > height (no
 * upscaling), a destination pointer or stride that is not 4-byte aligned. */
enum lr_warp_option { LR_WARP_PREPARE = 0x100 }; /* or-ed into `format` */
/* LR_WARP_PACKED is the warp for a batch whose frames have their OWN output sizes (lr_rectification_homography gives every
 * frame its own), still in one launch and into one destination region without padding to the largest.  The source is
 * as ever: `batch` frames of width x height, frame b at d_src + b*src_image_bytes.  M is a HOST table of 13 doubles per
 * frame: [0..8] the destination-to-source map, [9] and [10] that frame's out_width_b and out_height_b, [11] the byte
 * offset of its output from d_dst, [12] its row stride in bytes.  Entries 9..12 are integers (at most 2^53): sizes >= 1,
 * offset >= 0, stride >= out_width_b * bytes per pixel; for f32 offset and stride are multiples of 4 and d_dst is 4-byte
 * aligned.  out_width and out_height are upper bounds of the frames' sizes, dst_image_bytes is the size of the whole
 * region (every frame's offset + (out_height_b - 1) * stride + out_width_b * bpp lies within it) and dst_row_bytes is 0.
 * Frame b's pixels are exactly those of the single-frame warp with its map and size; no other byte of the region is
 * written, row padding and the gaps between frames included.  Fails cleanly (nothing launched, nothing written) on what
 * the warp rejects, a table entry that is not an integer in its range, a frame outside the region, two frames whose
 * extents [offset, end) overlap, more than 2^31 tiles of 64 x 16 pixels in total, LR_WARP_PACKED | LR_WARP_PREPARE and
 * any other option bit.  (An enum of its own: enumerators are ints, and lr_warp_option's one line stays as it was.) */
enum lr_warp_layout { LR_WARP_PACKED = 0x200 }; /* or-ed into `format` like lr_warp_option */
/* LR_WARP_RAGGED gives every frame its own SOURCE size and place as well: a folder of photographs (portrait and landscape,
 * several cameras) in one source region, one launch.  M is a HOST table of 18 doubles per frame: [0..8] the
 * destination-to-source map, [9] [10] out_width_b and out_height_b, [11] [12] byte offset of the output from d_dst and its
 * row stride in bytes (all as LR_WARP_PACKED), [13] [14] the source's width_b and height_b, [15] [16] byte offset of the
 * source from d_src and its row stride in bytes, [17] reserved, 0.  width x height and out_width x out_height are upper
 * bounds of the frames' sizes, src_image_bytes and dst_image_bytes the sizes of the two regions, src_row_bytes and
 * dst_row_bytes are 0.  Entries 9..16 are integers (at most 2^53) under LR_WARP_PACKED's rules for 9..12.  Outputs are laid
 * out as with LR_WARP_PACKED (no two extents overlap; any order, gaps and padded rows); sources are only read, may share or
 * overlap, and lie within [0, src_image_bytes).  Two spellings:
 *   fmt | LR_WARP_RAGGED                     the bilinear warp: frame b is exactly the single-frame call with its source,
 *                                            map and size; no other byte of the destination region is written;
 *   fmt | LR_WARP_RAGGED | LR_WARP_PREPARE   the prepare step: entries 0..8 are ignored (they may be NaN), the destination
 *                                            is f32 gray, frame b exactly the single-frame LR_WARP_PREPARE call for
 *                                            width_b x height_b -> out_width_b x out_height_b (equal sizes: the pure
 *                                            conversion); out sizes <= source sizes, destination offsets and strides
 *                                            multiples of 4, d_dst 4-byte aligned; f32 sources likewise.
 * Fails cleanly (nothing launched, nothing written) on LR_WARP_RAGGED | LR_WARP_PACKED, any other option bit, a non-zero
 * [17], an entry that is not an integer in its range, a source or output outside its region, overlapping outputs, a
 * non-finite map (the warp only), a non-zero src_row_bytes or dst_row_bytes, more than 2^31 tiles, the alignment rules. */
enum lr_warp_sources { LR_WARP_RAGGED = 0x800 }; /* or-ed into `format` like lr_warp_option */
/* LR_WARP_CUBIC is the warp's second sampling rule, cv::warpPerspective's INTER_CUBIC: a 4 x 4 bicubic (the Keys kernel with
 * a = -0.75, the constant OpenCV uses) in place of the 2 x 2 bilinear, for the rectified picture's magnified far side, where
 * the bilinear rule softens edges.  It is an option of the three warps and of nothing else:
 *   fmt | LR_WARP_CUBIC                     the warp above (one output size for all frames);
 *   fmt | LR_WARP_PACKED | LR_WARP_CUBIC    LR_WARP_PACKED's call;
 *   fmt | LR_WARP_RAGGED | LR_WARP_CUBIC    LR_WARP_RAGGED's call;
 * and holds for every frame of the call.  Arguments, tables, checks, failure behaviour and the promise that no other byte of
 * the destination is written are those of the same call without the bit; without the bit every call gives what it gave.
 * Arithmetic (tests/numpy_warp_cubic_ref.py restates it): the source coordinates X, Y are the
 * bilinear warp's, 5 fractional bits per axis; ix = X >> 5, ax = X & 31 (iy, ay likewise); the taps are columns ix - 1 ..
 * ix + 2 of rows iy - 1 .. iy + 2, a tap outside the source is 0; the four weights of an axis are row ax (ay) of a table of
 * 32 x 4 integers at scale 2048, whose rows sum to 2048.  u8 and u8x3, per channel, exact and in integers: h_j = sum_i
 * C[ax][i] v(i, j), s = sum_j C[ay][j] h_j, result (s + 2^21) >> 22 clamped to 0 .. 255 (a bicubic overshoots at edges).  f32:
 * weights C / 2048.f, each row's four products summed from the first tap to the last, then the rows' likewise, every product
 * and sum rounded to float on its own; no clamp.  The identity map gives back a u8 source byte for byte (an f32 source of
 * finite values bit for bit, -0 aside).  Fails cleanly (nothing launched, nothing written, lr_last_error names the
 * combination) together with LR_WARP_PREPARE (an area average by definition), LR_WARP_LINES, LR_WARP_JPEG or
 * LR_WARP_JPEG_DECODE. */
enum lr_warp_sampling { LR_WARP_CUBIC = 0x8000 }; /* or-ed into `format` like lr_warp_option */
/* LR_WARP_BORDER gives every frame a border rule, cv::warpPerspective's borderMode and borderValue, in place of the constant
 * zero border: what a tap OUTSIDE the source contributes.  It is an option of the three warps and of nothing else, alone or
 * with LR_WARP_CUBIC.  With the bit every frame's row of the host table M carries one border word:
 *   fmt | LR_WARP_BORDER                    10 doubles per frame instead of 9, the word is entry [9];
 *   fmt | LR_WARP_PACKED | LR_WARP_BORDER   14 doubles per frame instead of 13, the word is entry [13];
 *   fmt | LR_WARP_RAGGED | LR_WARP_BORDER   18 doubles per frame as ever, the word is entry [17].
 * The word is the integer mode + 8 * value.  mode, in OpenCV's numbers: 0 constant, 1 replicate (aaaa|abcd|dddd), 2 reflect
 * (cba|abc|cba), 4 reflect-101 (dcb|abcd|cba); 3 (wrap), 5 (transparent), 6 and 7 are refused.  value belongs to mode 0 and
 * is 0 with the others: u8 0 .. 255; u8x3 c0 | c1 << 8 | c2 << 16; f32 the IEEE bit pattern of a finite float.
 * Coordinates, the taps' positions, the weights, the u8 rounding and clamping and the f32 order of summation are exactly those
 * of the same call without the bit (tests/numpy_warp_border_ref.py restates it).  A
 * tap at (cx, cy) outside the source has, mode 0, the value `value` (per channel) or, modes 1, 2 and 4, the value of source
 * pixel (b(cx, width), b(cy, height)), b being OpenCV's borderInterpolate: replicate clamp(p, 0, n - 1); reflect q = p mod 2n
 * (non-negative), q < n ? q : 2n - 1 - q; reflect-101 0 for n == 1, else q = p mod (2n - 2), q < n ? q : 2n - 2 - q.  Zero
 * weights multiply their taps like any other.  A frame whose word is 0 is byte for byte the frame of the call without the bit.
 * Fails cleanly (nothing launched, nothing written, lr_last_error names the frame and the reason) on what the call without
 * the bit rejects, on a word that is not an integer from 0 to 2^35 - 1, a refused mode, a value out of the format's range, a
 * non-zero value with modes 1, 2 or 4, f32 bits that are no finite float, and together with LR_WARP_PREPARE, LR_WARP_LINES,
 * LR_WARP_JPEG or LR_WARP_JPEG_DECODE.  Without the bit nothing changes: rows keep their lengths, a non-zero [17] fails. */
enum lr_warp_border { LR_WARP_BORDER = 0x40000 }; /* or-ed into `format` like lr_warp_option */
enum lr_border_mode { LR_BORDER_CONSTANT = 0, LR_BORDER_REPLICATE = 1, LR_BORDER_REFLECT = 2, LR_BORDER_REFLECT_101 = 4 };
/* LR_WARP_LENS gives every frame a lens model, OpenCV's camera matrix and five distortion coefficients, so that the warp reads
 * a photograph that is no pinhole picture: it undistorts and warps in ONE resampling.  It is an option of the three warps and
 * of nothing else, with or without LR_WARP_CUBIC and LR_WARP_BORDER, for u8, u8x3 and f32.  With the bit every frame's row of
 * the host table M carries nine more doubles at its end, behind the border word where there is one:
 *   fmt | LR_WARP_LENS                    18 doubles per frame, 19 with LR_WARP_BORDER;
 *   fmt | LR_WARP_PACKED | LR_WARP_LENS   22 doubles per frame, 23 with LR_WARP_BORDER;
 *   fmt | LR_WARP_RAGGED | LR_WARP_LENS   27 doubles per frame (the border word stays entry [17]).
 * The nine are fx, fy, cx, cy, k1, k2, p1, p2, k3 in the source frame's pixel units.  M keeps its meaning, destination pixel
 * to source; with the bit "source" is the IDEAL (undistorted) picture, which has the source's size and camera matrix, and the
 * lens model takes that point to the pixel of the stored frame that is sampled.  Arithmetic (DESIGN.md section 3, item 17;
 * tests/numpy_warp_lens_ref.py restates it), in double, every operation rounded on its own; N0, N1, W0 are the three dot
 * products of the warp's rule:
 *   Wq = W0 != 0 ? 32 / W0 : 0;   U = N0 * Wq;   V = N1 * Wq
 *   a  = (U * 0.03125 - cx) / fx;                b = (V * 0.03125 - cy) / fy
 *   r2 = a*a + b*b;    rad = r2 * (k1 + r2 * (k2 + r2 * k3))
 *   ta = (2*p1) * (a*b) + p2 * (r2 + 2*(a*a));   tb = p1 * (r2 + 2*(b*b)) + (2*p2) * (a*b)
 *   du = fx * (a*rad + ta);                      dv = fy * (b*rad + tb)
 *   X  = fixed(U + 32*du);                       Y  = fixed(V + 32*dv)
 * fixed being the warp's clamp to [INT_MIN, INT_MAX] (a NaN becomes INT_MIN) and rounding half to even.  Taps, weights, both
 * sampling rules and every border mode behind X, Y are what they are without the bit.  A frame whose five coefficients are all
 * zero (of either sign) is by definition warped by the plain rule: byte for byte the frame of the call without the bit.
 * Infinities and NaN go the way they go in the plain rule; there is no guard against a model that folds over at a large radius
 * (the caller's model, as with cv::undistort).  Fails cleanly (nothing launched, nothing written, lr_last_error names the frame)
 * on what the call without the bit rejects, a non-finite entry among the nine, fx <= 0 or fy <= 0, and together with
 * LR_WARP_PREPARE, LR_WARP_LINES, LR_WARP_JPEG or LR_WARP_JPEG_DECODE.  Without the bit nothing changes. */
enum lr_warp_lens { LR_WARP_LENS = 0x100000 }; /* or-ed into `format` like lr_warp_option */
/* LR_WARP_LENS_MODEL, or-ed in TOGETHER with LR_WARP_LENS, widens every frame's lens from nine entries to seventeen, for the
 * calibrations the five coefficients cannot hold: cv::calibrateCamera's with CALIB_RATIONAL_MODEL (8 coefficients) and
 * CALIB_THIN_PRISM_MODEL (12), and cv::fisheye::calibrate's.  It works with everything LR_WARP_LENS works with: the three
 * layouts, LR_WARP_CUBIC, LR_WARP_BORDER and LR_WARP_AREA, u8, u8x3 and f32.  The seventeen sit where the nine sat, behind the
 * border word where there is one and in front of LR_WARP_AREA's S:
 *   fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, model
 *   fmt | LR_WARP_LENS | LR_WARP_LENS_MODEL                    26 doubles per frame, 27 with LR_WARP_BORDER;
 *   fmt | LR_WARP_PACKED | LR_WARP_LENS | LR_WARP_LENS_MODEL   30 doubles per frame, 31 with LR_WARP_BORDER;
 *   fmt | LR_WARP_RAGGED | LR_WARP_LENS | LR_WARP_LENS_MODEL   35 doubles per frame (the border word stays entry [17]);
 * each one more with LR_WARP_AREA.  model = 0 (LR_LENS_RATIONAL): entries [4..15] are OpenCV's twelve distCoeffs in OpenCV's
 * order, so the first nine entries mean what they mean without the bit.  model = 1 (LR_LENS_FISHEYE): entries [4..7] are
 * cv::fisheye's k1..k4 and entries [8..15] must be zero.  Frames of both models and frames without a lens mix in one launch.
 * Arithmetic (tests/numpy_warp_lens_model_ref.py restates it), in double, every operation rounded
 * on its own; U, V, a, b, r2 and fixed are LR_WARP_LENS's.  Model 0, a displacement like LR_WARP_LENS's:
 *   radn = r2 * (k1 + r2 * (k2 + r2 * k3));      radd = r2 * (k4 + r2 * (k5 + r2 * k6))
 *   rad  = (radn - radd) / (1 + radd)
 *   ta   = ((2*p1) * (a*b) + p2 * (r2 + 2*(a*a))) + r2 * (s1 + r2 * s2)
 *   tb   = (p1 * (r2 + 2*(b*b)) + (2*p2) * (a*b)) + r2 * (s3 + r2 * s4)
 *   du = fx * (a*rad + ta);   dv = fy * (b*rad + tb);   X = fixed(U + 32*du);   Y = fixed(V + 32*dv)
 * (OpenCV's x'' = x' (1 + k1 r2 + ..) / (1 + k4 r2 + ..) + tangential + prism terms, with x' subtracted).  A model-0 frame
 * whose entries [4..15] are all zero (of either sign) is by definition warped by the plain rule; one whose [9..15] are zero has,
 * for a finite r2, the coordinates of LR_WARP_LENS's rule.  Model 1, which has no displacement form and no "no lens" case (zero
 * coefficients are the pure equidistant lens):
 *   r = sqrt(r2);   th = ATAN(r);   t2 = th * th
 *   thd = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))));   sc = r != 0 ? thd / r : 1
 *   X = fixed(32 * (fx * (a*sc) + cx));   Y = fixed(32 * (fy * (b*sc) + cy))
 * sqrt is the correctly rounded one and ATAN is lr_lens_atan below, an arctangent made of + - * /, comparisons and one rint,
 * so that the device, this header and the NumPy reference compute the same bits.  Infinities and NaN go the way they go in the
 * plain rule; there is no guard against a model that folds over.  A call whose frames all fit the nine entries (model 0,
 * [9..15] zero) launches what the same call with LR_WARP_LENS alone launches, and gives its bytes.  Fails cleanly (nothing
 * launched, nothing written, lr_last_error names the frame and the reason) on what the call without the bit rejects, the bit
 * without LR_WARP_LENS, a non-finite entry among the seventeen, fx <= 0 or fy <= 0, a model other than 0 or 1, a fisheye row
 * with a non-zero entry in [8..15], and together with LR_WARP_PREPARE, LR_WARP_LINES, LR_WARP_JPEG or LR_WARP_JPEG_DECODE.
 * Without the bit nothing changes. */
enum lr_warp_lens_model { LR_WARP_LENS_MODEL = 0x800000 }; /* or-ed into `format` like lr_warp_option, with LR_WARP_LENS */
enum lr_lens_model { LR_LENS_RATIONAL = 0, LR_LENS_FISHEYE = 1 }; /* entry [16] of a frame's seventeen lens entries */
/* LR_WARP_AREA makes the warp an area-sampled one: every destination pixel is the mean of S x S samples spread over its own
 * footprint, so that a warp which SHRINKS (a bounded-size rectified picture: lr_shrink_homography below) does not alias.  One
 * resampling: the stored frame is read once and only the small picture is written.  It is an option of the three warps and of
 * nothing else, with or without LR_WARP_CUBIC, LR_WARP_BORDER and LR_WARP_LENS, for u8, u8x3 and f32.  With the bit every
 * frame's row of the host table M carries ONE more double at its very end, behind the border word and the nine lens entries
 * where they exist: the frame's sampling factor S, an integer from 1 to 8.  Rows are then
 *   fmt | LR_WARP_AREA                    10 / 11 / 19 / 20 doubles per frame (alone / BORDER / LENS / both);
 *   fmt | LR_WARP_PACKED | LR_WARP_AREA   14 / 15 / 23 / 24;
 *   fmt | LR_WARP_RAGGED | LR_WARP_AREA   19 / 28 (without / with LENS; the border word stays entry [17]).
 * Frames with different S mix in one launch.  Arithmetic (tests/numpy_warp_area_ref.py restates it):
 *   1. the fine map F = lr_area_fine_map(M, S), on the host in double: the destination-to-source map of a picture S times as
 *      large, whose pixel (S x + i, S y + j) is sub-sample (i, j) of destination pixel (x, y), at ((i + 0.5) / S - 0.5,
 *      (j + 0.5) / S - 0.5) from the pixel's centre;
 *   2. sub-sample v(i, j), i, j = 0 .. S - 1, is exactly what the call without the bit gives for pixel (S x + i, S y + j)
 *      under the map F: the frame's lens, the 5-bit coordinates, the bilinear or bicubic taps and weights, the frame's border
 *      rule and the per-sample rounding to a byte (u8, u8x3) or a float (f32);
 *   3. u8 and u8x3, per channel: s = the sum of the S^2 bytes, out = (2 s + S^2) / (2 S^2) in integers (round half up);
 *      f32: acc = 0.0f; for j from 0, for i from 0: acc = acc + v(i, j), every sum rounded to float; out = acc / (float)(S * S);
 *   4. a frame with S = 1 is by definition warped by the plain rule: byte for byte (f32: bit for bit) the frame of the call
 *      without the bit.
 * So a frame's picture is the S x S box mean of the warp without the bit, map F, into S out_width x S out_height; for the pure
 * shrink M = [[S, 0, (S - 1) / 2], [0, S, (S - 1) / 2], [0, 0, 1]] F is the identity and the picture the rounded S x S box mean
 * of the source (cv::resize's INTER_AREA for an integer factor).  Fails cleanly (nothing launched, nothing written,
 * lr_last_error names the frame and the reason) on what the call without the bit rejects, an S that is not an integer from 1 to
 * 8, S * out_width_b or S * out_height_b above 2^31 - 1, and together with LR_WARP_PREPARE, LR_WARP_LINES, LR_WARP_JPEG or
 * LR_WARP_JPEG_DECODE.  Without the bit nothing changes: rows keep their lengths and every call gives what it gave. */
enum lr_warp_area { LR_WARP_AREA = 0x400000 }; /* or-ed into `format` like lr_warp_option */

/* LR_WARP_AREA's fine map F (9 doubles; F may be M) of the map M and the sampling factor S, for k = 0, 1, 2:
 *   F[k][0] = M[k][0] / S;   F[k][1] = M[k][1] / S;   F[k][2] = M[k][2] - ((M[k][0] + M[k][1]) * (double)(S - 1)) / (double)(2 S)
 * Host arithmetic only, every operation rounded on its own (-ffp-contract=off); operation for operation the Python package's
 * area_fine_map and what the library computes per frame. */
static inline void lr_area_fine_map(const double* M, int S, double* F) {
    int k;
    for (k = 0; k < 3; ++k) {
        const double m0 = M[3 * k], m1 = M[3 * k + 1], m2 = M[3 * k + 2];
        F[3 * k] = m0 / (double)S;
        F[3 * k + 1] = m1 / (double)S;
        F[3 * k + 2] = m2 - ((m0 + m1) * (double)(S - 1)) / (double)(2 * S);
    }
}

/* A rectified picture of bounded size: the map, the size and the sampling factor with which LR_WARP_AREA writes the picture of
 * (H, M, out_width x out_height) -- what lr_rectification_homography or lr_crop_homography returned -- at no more than
 * max_size pixels on its longer side.  Host arithmetic only, in double; a static inline because the export table is full.
 * With L = max(out_width, out_height): if L <= max_size nothing changes and S = 1.  Otherwise
 *   w' = max(1, (out_width * max_size) / L) in 64-bit integers, h' likewise;  sx = out_width / (double)w', sy likewise;
 *   tx = (sx - 1) / 2, ty = (sy - 1) / 2;
 *   M_out[k][0] = M[k][0] * sx;  M_out[k][1] = M[k][1] * sy;  M_out[k][2] = M[k][2] + (M[k][0] * tx + M[k][1] * ty);
 *   H_out = diag(1 / sx, 1 / sy, 1) T(-tx, -ty) H:  H_out[0][i] = (H[0][i] - tx * H[2][i]) / sx,  H_out[1][i] = (H[1][i] - ty *
 *   H[2][i]) / sy,  H_out[2][i] = H[2][i] (H_out[8] stays 1);   S = min(8, ceil(max(sx, sy))).
 * Destination pixel (x, y) of the small picture covers the pixels [sx x, sx (x + 1)) x [sy y, sy (y + 1)) of the large one.
 * H or M may be NULL (not both), and so may any output pointer; H_out may be H and M_out may be M.  Compiled without
 * floating-point contraction it is, operation for operation, the Python package's shrink_homography.  Returns 0, or 1 with
 * nothing written: a non-finite entry of H or M, H and M both NULL, or a size or max_size below 1. */
static inline int lr_shrink_homography(const double* H, const double* M, int out_width, int out_height, int max_size, double* H_out,
                                       double* M_out, int* new_width, int* new_height, int* S) {
    int i, k, longer, nw = out_width, nh = out_height, s = 1;
    double sx = 1.0, sy = 1.0, tx, ty, top, h[9], m[9];
    if ((!H && !M) || out_width < 1 || out_height < 1 || max_size < 1) return 1;
    for (i = 0; i < 9; ++i)
        if ((H && !(H[i] - H[i] == 0.0)) || (M && !(M[i] - M[i] == 0.0))) return 1; /* (x - x is 0 for finite x alone) */
    for (i = 0; i < 9; ++i) {
        h[i] = H ? H[i] : 0.0;
        m[i] = M ? M[i] : 0.0;
    }
    longer = out_width > out_height ? out_width : out_height;
    if (longer > max_size) {
        nw = (int)(((long long)out_width * (long long)max_size) / (long long)longer);
        nh = (int)(((long long)out_height * (long long)max_size) / (long long)longer);
        if (nw < 1) nw = 1;
        if (nh < 1) nh = 1;
        sx = (double)out_width / (double)nw;
        sy = (double)out_height / (double)nh;
        tx = (sx - 1.0) / 2.0;
        ty = (sy - 1.0) / 2.0;
        for (i = 0; i < 3; ++i) {
            h[i] = (h[i] - tx * h[6 + i]) / sx;
            h[3 + i] = (h[3 + i] - ty * h[6 + i]) / sy;
        }
        for (k = 0; k < 3; ++k) {
            const double m0 = m[3 * k], m1 = m[3 * k + 1];
            m[3 * k] = m0 * sx;
            m[3 * k + 1] = m1 * sy;
            m[3 * k + 2] = m[3 * k + 2] + (m0 * tx + m1 * ty);
        }
        top = ceil(sx > sy ? sx : sy);
        s = top < 8.0 ? (int)top : 8;
    }
    if (H && H_out)
        for (i = 0; i < 9; ++i) H_out[i] = h[i];
    if (M && M_out)
        for (i = 0; i < 9; ++i) M_out[i] = m[i];
    if (new_width) *new_width = nw;
    if (new_height) *new_height = nh;
    if (S) *S = s;
    return 0;
}

/* The lens model on the host: the pixel (*ud, *vd) of the stored photograph that shows the ideal point (u, v); lens: the nine
 * entries above.  The same operations in the same order as LR_WARP_LENS's rule with U = 32 u and V = 32 v, returning
 * (U + 32 du) / 32 and (V + 32 dv) / 32: it takes detected lines, which are in ideal coordinates, back onto the photograph.
 * Host arithmetic only; a static inline because the export table is full.  Compiled without floating-point contraction
 * (-ffp-contract=off) it is, operation for operation, the Python package's lens_distort. */
static inline void lr_lens_distort(const double lens[9], double u, double v, double* ud, double* vd) {
    const double fx = lens[0], fy = lens[1], cx = lens[2], cy = lens[3];
    const double k1 = lens[4], k2 = lens[5], p1 = lens[6], p2 = lens[7], k3 = lens[8];
    const double U = 32.0 * u, V = 32.0 * v;
    const double a = (U * 0.03125 - cx) / fx, b = (V * 0.03125 - cy) / fy;
    const double r2 = a * a + b * b;
    const double rad = r2 * (k1 + r2 * (k2 + r2 * k3));
    const double ta = (2.0 * p1) * (a * b) + p2 * (r2 + 2.0 * (a * a));
    const double tb = p1 * (r2 + 2.0 * (b * b)) + (2.0 * p2) * (a * b);
    const double du = fx * (a * rad + ta), dv = fy * (b * rad + tb);
    if (ud) *ud = (U + 32.0 * du) / 32.0;
    if (vd) *vd = (V + 32.0 * dv) / 32.0;
}

/* LR_WARP_LENS_MODEL's arctangent of r >= 0: out of + - * /, comparisons and one rint (round to nearest, ties to even, the
 * default rounding mode), so that every side computes the same bits; within 2^-52 of atan.  r > 1 is reflected, pi/2 - ATAN(1 /
 * r); t in [0, 1] is reduced by the nearest of the nine points c = i / 8, z = (t - c) / (1 + t c) with |z| <= 1/16, and ATAN(t) =
 * atan(c) + (z + z (z^2 p)), p = -1/3 + z^2 (1/5 + z^2 (-1/7 + ... + z^2 (-1/15))) in Horner's form.  A NaN stays a NaN.  Host
 * arithmetic only; compiled without floating-point contraction it is, operation for operation, the Python package's lens_atan. */
static inline double lr_lens_atan(double r) {
    /* atan(i / 8), i = 0 .. 8, as the shortest decimals that give these doubles (the header is also compiled as C++14, which has
     * no hexadecimal floating literals); pi/2 below likewise, 0x1.921fb54442d18p+0 */
    static const double table[9] = {0.0,                  /* 0x0.0p+0 */
                                    0.12435499454676144,  /* 0x1.fd5ba9aac2f6ep-4 */
                                    0.24497866312686414,  /* 0x1.f5b75f92c80ddp-3 */
                                    0.35877067027057225,  /* 0x1.6f61941e4def1p-2 */
                                    0.4636476090008061,   /* 0x1.dac670561bb4fp-2 */
                                    0.5585993153435624,   /* 0x1.1e00babdefeb4p-1 */
                                    0.6435011087932844,   /* 0x1.4978fa3269ee1p-1 */
                                    0.7188299996216245,   /* 0x1.700a7c5784634p-1 */
                                    0.7853981633974483};  /* 0x1.921fb54442d18p-1 */
    const int big = r > 1.0;
    const double t = big ? 1.0 / r : r;
    const double n = rint(8.0 * t);
    const int i = n >= 0.0 && n <= 8.0 ? (int)n : 0; /* (a NaN takes entry 0 and stays a NaN through z) */
    const double c = (double)i / 8.0;
    const double z = (t - c) / (1.0 + t * c);
    const double z2 = z * z;
    const double p = -1.0 / 3.0 + z2 * (1.0 / 5.0 + z2 * (-1.0 / 7.0 + z2 * (1.0 / 9.0 + z2 * (-1.0 / 11.0 + z2 * (1.0 / 13.0 + z2 * (-1.0 / 15.0))))));
    const double at = table[i] + (z + z * (z2 * p));
    return big ? 1.5707963267948966 - at : at;
}

/* lr_lens_distort for LR_WARP_LENS_MODEL's seventeen entries (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4,
 * model): the pixel (*ud, *vd) of the stored photograph that shows the ideal point (u, v).  The same operations in the same
 * order as the bit's rule with U = 32 u and V = 32 v, returning X / 32 and Y / 32 before `fixed`; a model-0 lens whose entries
 * [4..15] are all zero returns (U / 32, V / 32), the plain rule.  It does not check the entries: a model other than 1 is taken
 * for 0.  Host arithmetic only; compiled without floating-point contraction (-ffp-contract=off) it is, operation for
 * operation, the Python package's lens_distort for a LensModel. */
static inline void lr_lens_distort_model(const double lens[17], double u, double v, double* ud, double* vd) {
    const double fx = lens[0], fy = lens[1], cx = lens[2], cy = lens[3];
    const double U = 32.0 * u, V = 32.0 * v;
    const double a = (U * 0.03125 - cx) / fx, b = (V * 0.03125 - cy) / fy;
    const double r2 = a * a + b * b;
    double X = U, Y = V;
    int i, any = 0;
    if (lens[16] == 1.0) {
        const double k1 = lens[4], k2 = lens[5], k3 = lens[6], k4 = lens[7];
        const double r = sqrt(r2);
        const double th = lr_lens_atan(r);
        const double t2 = th * th;
        const double thd = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))));
        const double sc = r != 0.0 ? thd / r : 1.0;
        X = 32.0 * (fx * (a * sc) + cx);
        Y = 32.0 * (fy * (b * sc) + cy);
    } else {
        for (i = 4; i < 16; ++i) any = any || lens[i] != 0.0;
        if (any) {
            const double k1 = lens[4], k2 = lens[5], p1 = lens[6], p2 = lens[7], k3 = lens[8], k4 = lens[9], k5 = lens[10], k6 = lens[11];
            const double s1 = lens[12], s2 = lens[13], s3 = lens[14], s4 = lens[15];
            const double radn = r2 * (k1 + r2 * (k2 + r2 * k3));
            const double radd = r2 * (k4 + r2 * (k5 + r2 * k6));
            const double rad = (radn - radd) / (1.0 + radd);
            const double ta = ((2.0 * p1) * (a * b) + p2 * (r2 + 2.0 * (a * a))) + r2 * (s1 + r2 * s2);
            const double tb = (p1 * (r2 + 2.0 * (b * b)) + (2.0 * p2) * (a * b)) + r2 * (s3 + r2 * s4);
            const double du = fx * (a * rad + ta), dv = fy * (b * rad + tb);
            X = U + 32.0 * du;
            Y = V + 32.0 * dv;
        }
    }
    if (ud) *ud = X / 32.0;
    if (vd) *vd = Y / 32.0;
}

/* The constrained crop: the largest upright rectangle of the rectified picture, of the given aspect and centred on the image
 * of the source's centre, that contains no border at all.  Host arithmetic only, in double; a static inline because the export
 * table is full.  H, M, out_width, out_height: what lr_rectification_homography returned for a source of width x height.
 * margin: source pixels kept clear at each side so that every tap of non-zero weight is inside: 0 for the bilinear rule, 1
 * for LR_WARP_CUBIC.  aspect: the rectangle's width / height; <= 0 means the source's width / height.
 * Rule: Q is the image under H of (m, m), (w-1-m, m), (w-1-m, h-1-m), (m, h-1-m) and c that of ((w-1)/2, (h-1)/2); the
 * rectangle is centred on c with half-extents (s a, s), s the minimum of eight bounds: the window's c.x / a, (out_width - 1 -
 * c.x) / a, c.y, out_height - 1 - c.y, and for each edge P -> R of Q with inward normal n, n.(c - P) / (|n.x| a + |n.y|).
 * x0 = ceil(c.x - s a), x1 = floor(c.x + s a), y0 and y1 likewise; crop_width = x1 - x0 + 1, crop_height = y1 - y0 + 1;
 * H_out = T(-x0, -y0) H (H_out[8] stays 1), M_out = M T(x0, y0): the warp with M_out into crop_width x crop_height gives the
 * crop.  Any output pointer may be NULL; H_out may be H and M_out may be M.  Compiled without floating-point contraction
 * (-ffp-contract=off) it is, operation for operation, the Python package's crop_homography.  Returns 0, or with nothing written:
 *   1  a non-finite input (H, M, aspect), a null H or M, or a size, output size or margin below its minimum (1, 1, 0);
 *   2  width - 1 - 2 margin < 1 or height - 1 - 2 margin < 1;
 *   3  a zero denominator, or denominators of mixed sign, at the five points;
 *   4  a quadrilateral Q that is not strictly convex;
 *   5  a crop below 1 x 1. */
static inline int lr_crop_homography(const double* H, const double* M, int width, int height, int out_width, int out_height,
                                     int margin, double aspect, double* H_out, double* M_out, int* x0, int* y0,
                                     int* crop_width, int* crop_height) {
    double px[5], py[5], qx[5], qy[5], a, s, area2, cx, cy, lo_x, hi_x, lo_y, hi_y;
    int i, pos = 0, neg = 0, w1, h1;
    if (!H || !M || width < 1 || height < 1 || out_width < 1 || out_height < 1 || margin < 0) return 1;
    for (i = 0; i < 9; ++i)
        if (!(H[i] - H[i] == 0.0) || !(M[i] - M[i] == 0.0)) return 1; /* (x - x is 0 for finite x alone) */
    if (!(aspect - aspect == 0.0)) return 1;
    if (width > 1073741824 || height > 1073741824 || margin > 1073741824) return 1;
    w1 = width - 1 - 2 * margin;
    h1 = height - 1 - 2 * margin;
    if (w1 < 1 || h1 < 1) return 2;
    a = aspect > 0.0 ? aspect : (double)width / (double)height;
    px[0] = margin;              py[0] = margin;
    px[1] = width - 1 - margin;  py[1] = margin;
    px[2] = width - 1 - margin;  py[2] = height - 1 - margin;
    px[3] = margin;              py[3] = height - 1 - margin;
    px[4] = (width - 1) / 2.0;   py[4] = (height - 1) / 2.0;
    for (i = 0; i < 5; ++i) {
        const double d = (H[6] * px[i] + H[7] * py[i]) + H[8];
        if (d > 0.0) ++pos;
        else if (d < 0.0) ++neg;
        else return 3;
        qx[i] = ((H[0] * px[i] + H[1] * py[i]) + H[2]) / d;
        qy[i] = ((H[3] * px[i] + H[4] * py[i]) + H[5]) / d;
    }
    if (pos && neg) return 3;
    cx = qx[4];
    cy = qy[4];
    /* twice the signed area gives the orientation; every corner must turn the same way, strictly */
    area2 = 0.0;
    for (i = 0; i < 4; ++i) area2 += qx[i] * qy[(i + 1) & 3] - qx[(i + 1) & 3] * qy[i];
    if (!(area2 - area2 == 0.0) || area2 == 0.0) return 4;
    for (i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3, k = (i + 2) & 3;
        const double turn = (qx[j] - qx[i]) * (qy[k] - qy[j]) - (qy[j] - qy[i]) * (qx[k] - qx[j]);
        if (!(area2 > 0.0 ? turn > 0.0 : turn < 0.0)) return 4;
    }
    s = cx / a;
    if ((out_width - 1 - cx) / a < s) s = (out_width - 1 - cx) / a;
    if (cy < s) s = cy;
    if (out_height - 1 - cy < s) s = out_height - 1 - cy;
    for (i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3;
        const double ex = qx[j] - qx[i], ey = qy[j] - qy[i];
        /* the inward normal of edge P -> R: the edge turned a quarter towards the inside */
        const double nx = area2 > 0.0 ? -ey : ey, ny = area2 > 0.0 ? ex : -ex;
        const double den = (nx < 0.0 ? -nx : nx) * a + (ny < 0.0 ? -ny : ny);
        const double bound = (nx * (cx - qx[i]) + ny * (cy - qy[i])) / den; /* (den > 0: the edge has a length) */
        if (!(bound >= s)) s = bound; /* (a NaN bound ends below as a crop below 1 x 1) */
    }
    if (!(s >= 0.0)) return 5;
    lo_x = ceil(cx - s * a);
    hi_x = floor(cx + s * a);
    lo_y = ceil(cy - s);
    hi_y = floor(cy + s);
    if (!(hi_x >= lo_x && hi_y >= lo_y) || lo_x < 0.0 || lo_y < 0.0 || hi_x > (double)(out_width - 1) || hi_y > (double)(out_height - 1))
        return 5;
    if (H_out) {
        for (i = 0; i < 3; ++i) {
            H_out[i] = H[i] - lo_x * H[6 + i];
            H_out[3 + i] = H[3 + i] - lo_y * H[6 + i];
            H_out[6 + i] = H[6 + i];
        }
    }
    if (M_out) {
        for (i = 0; i < 3; ++i) {
            M_out[3 * i] = M[3 * i];
            M_out[3 * i + 1] = M[3 * i + 1];
            M_out[3 * i + 2] = (M[3 * i] * lo_x + M[3 * i + 1] * lo_y) + M[3 * i + 2];
        }
    }
    if (x0) *x0 = (int)lo_x;
    if (y0) *y0 = (int)lo_y;
    if (crop_width) *crop_width = (int)(hi_x - lo_x) + 1;
    if (crop_height) *crop_height = (int)(hi_y - lo_y) + 1;
    return 0;
}

/* The demo's lines picture (autorectify.cpp:72-110, draw_lines; <name>_warp_lines.jpg) on frames that stay in HBM: every
 * segment of a frame as a 3-pixel stroke with a disc of radius 5 at each end, in its group's colour, later segments over
 * earlier ones, on the frame as u8x3.  One launch on the context's stream for a batch of frames of different sizes.
 * `frames` is a HOST table of
 * 8 doubles per frame: [0] [1] width_b, height_b, [2] [3] byte offset of the source from d_src and its row stride in bytes,
 * [4] [5] byte offset of the output from d_dst and its row stride, [6] [7] first segment of the frame in `lines` and count
 * `lines` is a HOST array of n_lines segments; [6] and [7] let the batch detector's output (out + b*capacity, n_lines[b])
 * be passed as it is.  H is on the host: 9 doubles per frame (what lr_rectification_homography returns as H: the lines are
 * then drawn on the rectified picture), or NULL for identity.  format is LR_PIX_U8 (pixel v becomes (v, v, v)) or
 * LR_PIX_U8X3 (copied); the destination is always u8x3.  d_src == NULL draws in place on what d_dst holds: src_bytes and
 * [2] [3] are 0, format is LR_PIX_U8X3, and only covered pixels are written.
 * The shapes are exact and in integers (a restatement of the demo's line(..., 3) and circle(..., 5,
 * -1), not OpenCV's bit pattern): endpoints are truncated toward zero, after H in double if there is one; a pixel takes
 * the colour of the highest-index segment of its frame whose shape contains it; colours are white for group_id < 0 and
 * otherwise entry group_id % 12 of the demo's palette with c0 red.  A segment with a non-finite coordinate, one beyond
 * 2^24, or (with H) denominators that are zero or differ in sign is not drawn.
 * The table follows LR_WARP_RAGGED's rules: integers (at most 2^53), sizes from 1 (to 2^30), strides at least a row, every
 * extent within its region of src_bytes or dst_bytes, output extents that do not overlap each other, [6] + [7] <= n_lines
 * (a count of 0 gives the background only); except in place the destination region does not overlap the source region.
 * The whole table is checked before anything is enqueued: on failure (also a null `lines` with n_lines != 0, a format
 * other than the two, batch < 1, a non-finite H) nothing is launched or written and lr_last_error names the frame and the
 * entry.  No byte of the destination region outside the frames' pixels is written, row padding and gaps included.
 * The library's table of exported symbols is full (tests/test_boundary_cpu.py holds it at 60), so the call travels through
 * lr_warp_perspective_device: LR_WARP_LINES or-ed into `format`, `M` pointing to an lr_draw_lines_args, src_image_bytes
 * and dst_image_bytes the two regions' sizes, and width, height, out_width, out_height and both row strides 0 (any other
 * option bit or a non-zero one of these fails cleanly).  lr_draw_lines_device below is that call, spelled out. */
typedef struct lr_draw_lines_args {
    const LineSegment* lines; /* HOST, n_lines records */
    size_t n_lines;
    const double* frames; /* HOST, 8 doubles per frame */
    const double* H;      /* HOST, 9 doubles per frame, or NULL */
} lr_draw_lines_args;
enum lr_warp_lines { LR_WARP_LINES = 0x1000 }; /* or-ed into `format` like lr_warp_option */
static inline int lr_draw_lines_device(lr_context* ctx, const void* d_src, size_t src_bytes, int format, const LineSegment* lines,
                                       size_t n_lines, const double* frames, int batch, const double* H, void* d_dst,
                                       size_t dst_bytes) {
    lr_draw_lines_args a;
    a.lines = lines;
    a.n_lines = n_lines;
    a.frames = frames;
    a.H = H;
    return lr_warp_perspective_device(ctx, d_src, src_bytes, batch, 0, 0, 0, format | LR_WARP_LINES, (const double*)(const void*)&a,
                                      d_dst, dst_bytes, 0, 0, 0);
}

/* The demo's products are JPEG files (autorectify.cpp:368-369, imwrite): lr_encode_jpeg_device compresses 8-bit frames that
 * lie in HBM into baseline JPEG streams in HBM, so that only the streams (about a tenth of the pixels' bytes at quality 95)
 * cross the link.  One chain of launches for a batch of frames of different sizes; the call is SYNCHRONOUS like the
 * detector's entries: it waits for the context's stream, and on return sizes[b] (HOST) is the length of frame b's stream.
 * `frames` is a HOST table of 8 doubles per frame: [0] [1] width_b, height_b (1 .. 65535), [2] [3] byte offset of the
 * source from d_src and its row stride in bytes, [4] [5] byte offset of the stream from d_dst and its CAPACITY in bytes,
 * [6] the quality, 1 .. 100, [7] the chroma layout: 0 = 4:2:0, 1 = 4:4:4 (0 for LR_PIX_U8).  format is LR_PIX_U8 (a
 * one-component stream) or LR_PIX_U8X3 (c0 red: a YCbCr stream).  The table follows LR_WARP_RAGGED's rules: integers (at most
 * 2^53), strides at least a row, every source inside src_bytes, every extent [offset, offset + capacity) inside dst_bytes,
 * no two extents overlapping, the destination region apart from the source region.  The whole table is checked before
 * anything is enqueued: on failure (also a null pointer, batch < 1, another format) nothing is launched or written, `sizes`
 * is untouched and lr_last_error names the frame and the entry.
 * sizes[b] is the stream's length EVEN WHEN IT EXCEEDS THE CAPACITY (the n_lines convention): a stream that fits is complete
 * at its offset; of one that does not fit the extent's content is unspecified, and the call still returns 0.  No byte
 * outside the frames' extents is ever written.  lr_jpeg_bound gives a capacity that always suffices.
 * The stream (tests/numpy_jpeg_ref.py produces the same bytes): SOI, JFIF 1.01 APP0, DQT (the
 * Annex K tables scaled by the IJG quality rule), SOF0 (8 bits), DHT (the Annex K tables), DRI, one interleaved scan with
 * RSTm after every restart interval but the last, EOI.  A restart interval is 96 blocks whatever the width: 16 MCUs of
 * 4:2:0, 32 of 4:4:4, 96 of one component.  A one-component stream carries table 0 only.  Colour conversion, the 2 x 2 mean,
 * the forward DCT and the quantisation are exact, in integers.  Frames are padded to whole MCUs by replicating the last
 * column and row; a 4:2:0 luminance block that holds no pixel of the frame is coded as libjpeg codes its dummy blocks (a DC
 * difference of 0 and an end of block).
 * LR_JPEG_OPTIMIZE added to a frame's [7] (0, 1, 16 or 17 for LR_PIX_U8X3; 0 or 16 for LR_PIX_U8; every frame of a batch its
 * own value): the frame's stream is coded with Huffman tables made from the frame's own symbols (DESIGN.md section 3, item
 * 13a; tests/numpy_jpeg_optimize_ref.py produces the same bytes), the two-pass mode of the CPU encoders (libjpeg's
 * optimize_coding).  The symbols the stream emits are counted per table over all restart intervals; the code lengths are
 * Annex K.2's as the IJG library finds them (a 257th pseudo-symbol of count 1 keeps the all-ones code free; of equal counts
 * the larger symbol is merged first), limited to 16 bits by the K.3 adjustment; the DHT segments list the symbols that occur
 * and nothing else.  Only the DHT payloads and the code bits differ from the stream without the option: a decoder gets
 * the same pixels from fewer bytes (about 15 % fewer for a photograph at quality 95).  Counting and table making run on the
 * device in front of the entropy coder, two more launches and the call's one synchronisation at its end; a call in
 * which no frame has the option launches exactly what it launched before the option existed.
 * The coefficients (2 bytes per sample of the padded components), the intervals' lengths and places and the symbol counters
 * belong to the context's workspace: lr_context_trim frees them.
 * The library's table of exported symbols is full, so the call travels through lr_warp_perspective_device like
 * lr_draw_lines_device: LR_WARP_JPEG or-ed into `format`, `M` pointing to an lr_jpeg_args, src_image_bytes and
 * dst_image_bytes the two regions' sizes, and width, height, out_width, out_height and both row strides 0 (any other option
 * bit or a non-zero one of these fails cleanly).  lr_encode_jpeg_device below is that call, spelled out. */
typedef struct lr_jpeg_args {
    const double* frames; /* HOST, 8 doubles per frame */
    uint64_t* sizes;      /* HOST, one per frame: the streams' lengths */
} lr_jpeg_args;
enum lr_warp_jpeg { LR_WARP_JPEG = 0x2000 }; /* or-ed into `format` like lr_warp_option */
enum lr_jpeg_option { LR_JPEG_OPTIMIZE = 0x10 }; /* added to [7] of a frame's row, and to lr_jpeg_bound's layout */
static inline int lr_encode_jpeg_device(lr_context* ctx, const void* d_src, size_t src_bytes, int format, const double* frames,
                                        int batch, void* d_dst, size_t dst_bytes, uint64_t* sizes) {
    lr_jpeg_args a;
    a.frames = frames;
    a.sizes = sizes;
    return lr_warp_perspective_device(ctx, d_src, src_bytes, batch, 0, 0, 0, format | LR_WARP_JPEG, (const double*)(const void*)&a,
                                      d_dst, dst_bytes, 0, 0, 0);
}
/* The longest stream lr_encode_jpeg_device can produce for a frame (0 for a size outside 1 .. 65535 or another format).
 * A block's longest code: its DC difference, at most 11 bits of code (chrominance category 11) and 11 of magnitude, and 63
 * AC coefficients of at most 16 bits of code and 10 of magnitude each, 22 + 63 * 26 = 1660 bits = 207.5 bytes: 208, which
 * also covers an interval's padding to a whole byte (96 blocks leave 48 bytes over).  Every byte can be 0xFF and is then
 * followed by a stuffed zero: 416 per block.  Every interval but the last is followed by a 2-byte RSTm.  The markers and
 * headers in front of the scan are 629 bytes (334 for one component), the EOI 2: 640 covers both.
 * With LR_JPEG_OPTIMIZE added to `layout` (the frame's [7]): a DC code can then have 16 bits, not 11, so a block's longest
 * code is 27 + 63 * 26 = 1665 bits.  n blocks of an interval are at most ceil(1665 n / 8) <= 208.125 n + 0.875 bytes with
 * their padding, twice that with every byte stuffed: 416.25 n + 1.75 <= 418 n for every n >= 1 (96 blocks: 39 960 of
 * 40 128): 418 per block.  The headers are never longer than the standard ones, a table of the frame's own listing at most
 * the 12 DC and 162 AC symbols that Annex K's lists.  Without the bit the value is what it always was. */
static inline size_t lr_jpeg_bound(int width, int height, int format, int layout) {
    size_t mcu, bpm, ri, mcus;
    const size_t block = (layout & LR_JPEG_OPTIMIZE) ? 418 : 416;
    if (layout >= 0) layout &= ~LR_JPEG_OPTIMIZE;
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return 0;
    if (format == LR_PIX_U8 && layout == 0) {
        mcu = 8; bpm = 1; ri = 96;
    } else if (format == LR_PIX_U8X3 && layout == 0) {
        mcu = 16; bpm = 6; ri = 16;
    } else if (format == LR_PIX_U8X3 && layout == 1) {
        mcu = 8; bpm = 3; ri = 32;
    } else {
        return 0;
    }
    mcus = (((size_t)width + mcu - 1) / mcu) * (((size_t)height + mcu - 1) / mcu);
    return 640 + 2 * ((mcus + ri - 1) / ri) + block * mcus * bpm;
}

/* The demo's inputs are JPEG files as well (autorectify.cpp: imread): lr_decode_jpeg_device decodes baseline JPEG streams
 * that lie in HBM into 8-bit frames in HBM, so that a folder of photographs goes up as files (about a tenth of the pixels'
 * bytes).  One chain of launches for a batch of streams of different sizes and samplings; the call is SYNCHRONOUS like the
 * encoder's, because the host needs the statuses.
 * `frames` is a HOST table of 8 doubles per frame: [0] [1] byte offset and length of the stream in the source region (a
 * length below 2^31), [2] [3] byte offset of the picture from d_dst and its row stride in bytes, [4] [5] the width and
 * height the caller allocated for, [6] reserved, 0 (with LR_JPEG_SCALED, below: the scale denominator), [7] 1 to apply the file's EXIF orientation (below), else 0.  `h_src` is a HOST copy of the source region (same layout as d_src):
 * the host reads the headers up to SOS from it and nothing behind them.  `format` is the OUTPUT's format: LR_PIX_U8 gives the
 * luminance plane (of a colour stream Y alone: its chrominance is entropy-decoded but never transformed), LR_PIX_U8X3 gives
 * RGB with c0 red (a one-component stream replicated).  The table follows LR_WARP_RAGGED's rules: integers (at most 2^53),
 * every extent inside its region, strides at least a row, output extents that overlap neither each other nor the source
 * region; stream extents are only read and may overlap.  The whole table is checked before anything is enqueued: on a
 * table error (also a null pointer, batch < 1, another format) nothing is launched or written, `info` is untouched and
 * lr_last_error names the frame and the entry.
 * `info` (HOST, 8 int32 per frame, written by the call): [0] width, [1] height, [2] components (1 or 3), [3] layout (0 =
 * 4:2:0 or one component, 1 = 4:4:4, 2 = 4:2:2; with LR_JPEG_ANY_SAMPLING, below, any other accepted sampling: component 0's
 * sampling byte), [4] restart interval in MCUs (0: none), [5] status, [6] the most often
 * any part of the scan had to be entropy-decoded until the chain of parts was consistent (see below; 0 in probe mode), [7] 0,
 * or for a frame whose entry [7] is 1 the orientation that was read, 1..8.
 * Status: 0 decoded; 1 not a JPEG stream, or truncated before SOS; 2 unsupported (progressive, arithmetic, lossless or
 * hierarchical coding, 12-bit precision, 16-bit quantisation tables, component counts other than 1 or 3, another sampling,
 * a non-interleaved or multi-scan file, a missing table, a file that is RGB and not YCbCr by libjpeg's rule -- no JFIF segment,
 * and an Adobe APP14 segment with transform 0 or, without an Adobe segment, the component ids 'R', 'G', 'B': lr_last_error tells which, for
 * the last such frame); 3 the
 * table's [4] [5] differ from the stream's size; 4 the scan is damaged (an invalid code, a coefficient index beyond 63,
 * fewer or more MCUs than the frame has, a missing or misnumbered RSTm, padding in front of an RSTm that is not 1-bits
 * (T.81 F.1.2.3); in front of EOI any padding is taken).  Per-frame failures are statuses, not failures of
 * the call: a frame of status 1 to 3 is skipped on the host and no byte of its extent is written; of one of status 4 the
 * extent's content is unspecified; nothing outside the frames' extents is ever written, and the call returns 0.
 * Accepted: SOF0 or SOF1 with 8-bit samples, Huffman-coded, one interleaved scan, any DHT (table ids 0..3), any DRI or none,
 * APPn and COM of any size, fill bytes in front of markers; the stream ends at EOI or at its length.
 * EXIF orientation (the demo's imread applies it; nearly every upright phone photograph is stored sideways, as 6 or 8) is
 * applied to the frames whose entry [7] is 1, each frame of a batch by its own entry, inside the output pass of the same
 * chain of launches: the picture is written upright, with no second pass over it.  With S the stored w x h picture that
 * [7] = 0 gives, the picture O that is written is, bit for bit,
 *     1: O[y][x] = S[y][x]        2: S[y][w-1-x]      3: S[h-1-y][w-1-x]    4: S[h-1-y][x]        (O is w x h)
 *     5: O[y][x] = S[x][y]        6: S[h-1-x][y]      7: S[h-1-x][w-1-y]    8: S[x][w-1-y]        (O is h x w)
 * (what PIL's ImageOps.exif_transpose does).  For such a frame info [0] [1] are the size of O (swapped for 5..8), info [7] is
 * the orientation, the table's [4] [5] and the stride [3] are held against the size of O (status 3 and its message speak of
 * that size), and probe mode does the same: probe with [7] = 1, allocate info [0] x info [1], decode with [7] = 1.
 * With [7] = 0 the call does and reports what it did before entry [7] had a meaning, and info [7] is 0.
 * Any sampling: LR_JPEG_ANY_SAMPLING (0x20000) or-ed into `format` beside the pixel format applies to the whole call, probe
 * mode included (lr_jpeg_info passes LR_PIX_U8X3 alone; with the option call lr_decode_jpeg_device with d_dst == NULL).
 * Without it a three-component stream is 4:4:4, 4:2:2 (Y 2x1) or 4:2:0 (Y 2x2) with Cb = Cr = 1x1, or its status is 2.
 * With it a three-component stream that passes every other check is accepted if every h_i, v_i is 1, 2 or 4, component 0
 * has the largest factors (h_0 = Hmax, v_0 = Vmax, so Hmax / h_i and Vmax / v_i are 1, 2 or 4; Cb and Cr may differ) and
 * the sum of h_i * v_i is at most 10 (T.81 B.2.3): 4:4:0 (Y 1x2, what a lossless rotation makes of 4:2:2), 4:1:1 (Y 4x1),
 * equal non-unit factors, and the like.  Status 2 stays: luminance sampled below chrominance, a factor of 3, four
 * components, non-interleaved, multi-scan and progressive files.  A one-component stream is one block to the MCU whatever
 * its header's factors say, with the option and without.  An MCU is 8 Hmax x 8 Vmax pixels, its blocks component by
 * component, each as v_i rows of h_i blocks; component i's own grid is ceil(w h_i / Hmax) x ceil(h v_i / Vmax) samples, and
 * coordinates are clamped to it.  Upsampling, exact and in integers, per axis by the ratio r of the largest factor to the
 * component's: r = 1 the sample; r = 2 the centred triangle, (3 near + far + 2) >> 2 on one axis and (9, 3, 3, 1) + 8 >> 4 on
 * both, near = x >> 1, far its neighbour on the side of x's parity, clamped; r = 4 the sample x >> 2 (replication, as the
 * IJG library does where it has no triangle); r = 4 on one axis and 2 on the other: the triangle along the ratio-2 axis over
 * the replicated samples.  The IDCT and the colour rule are the same.  The three layouts are special cases: with the
 * option they come out byte for byte as without it, and info [3] keeps 0, 1, 2 for them; for every other accepted sampling
 * info [3] is component 0's sampling byte of SOF (h << 4 | v: 0x12 = 18 for 4:4:0, 0x41 = 65 for 4:1:1), which cannot
 * collide with 0..2.  Without the option every call does, reports and launches exactly what it did before there was one.
 * Reduced size: LR_JPEG_SCALED (0x80000) or-ed into `format` (beside LR_JPEG_ANY_SAMPLING or without it; probe mode
 * included) gives entry [6] of every frame's row a meaning: that frame's scale denominator N.  0 or 1: as stored; 2, 4 or
 * 8: the picture at 1/N of its size, ceil(w / N) x ceil(h / N) (lr_jpeg_scaled_size); anything else is a table error that
 * names the frame and [6].  Frames of different N mix in one call.  The reduced size takes the stored size's place
 * everywhere: info [0] [1] (with [7] = 1 swapped for 5..8 after the reduction), the table's [4] [5] and status 3 with its
 * message, the stride [3], probe mode.  So: probe with the bit and [6], allocate info [0] x info [1], decode with the same
 * row.  Without the bit a non-zero [6] is the table error it always was.  The rule, exact and in integers: for component i
 * and each axis on its own let rho be the ratio of the largest sampling factor to the component's (1, 2 or 4), d = min(N,
 * rho), r = N / d (the reduction of the component's blocks on that axis, 1..8) and rho' = rho / d (the upsampling that is
 * left).  The reduced samples are S'[Y][X] = (sum over j < ry, i < rx of S[Y ry + j][X rx + i] + rx ry / 2) >> log2(rx ry),
 * S being the component's samples as the inverse transform leaves them (clamped to 0..255, the blocks' padding beyond the
 * component's size included; r divides 8, so a cell lies in one block); the reduced grid is ceil(cw_i / rx) x ceil(ch_i /
 * ry); it is upsampled per axis by rho' with the rule above (the sample, the triangle, replication), clamped at the reduced
 * grid's size; the colour rule is the same.  LR_PIX_U8 reduces the luminance alone.  A 4:2:0 file at N = 2 thus has its
 * luminance averaged 2 x 2 and its chrominance taken as it is, with no upsampling at all.  N = 1 is byte for byte the
 * unscaled decode, and the orientation is applied to the reduced picture as to a full one.  The reduced picture is within
 * a few levels of the N x N box average of the full decode (DESIGN.md section 3, item 14 has the figures); coordinates
 * found in it are the file's divided by N.
 * The tag: of the segments before SOS the first APP1 whose payload starts with "Exif\0\0" counts and later ones do not
 * (other APP1 segments, XMP for one, are passed over).  Behind those six bytes lies a TIFF block: "II*\0" (little endian)
 * or "MM\0*" (big endian), a 32-bit offset of IFD0 from the block's start, there a 16-bit count and 12-byte entries (tag,
 * type, count, value).  The entry with tag 0x0112 tells the orientation if its type is 3 (SHORT), its count 1 and its
 * value -- the first two bytes of the value field, in the file's byte order -- 1..8.  Anything else is no orientation and
 * behaves as 1: no Exif segment, another byte-order mark, an offset or an IFD that reaches beyond the segment, another type
 * or count, a value of 0 or above 8.  None of it is a failure of the frame or of the call; every read stays inside the
 * segment; IFD1 and the Exif sub-IFD are not followed.
 * Probe mode: d_dst == NULL fills `info` from the headers alone and launches nothing; it needs no context (ctx may be NULL)
 * and no GPU; [2] .. [5] of the table may then be 0 (no picture, no expected size).  lr_jpeg_info below spells it out.
 * The arithmetic (tests/numpy_jpeg_decode_ref.py restates it) is exact, in integers.
 * The entropy-coded bytes are cut into parts of 128 bytes, one lane each; every lane but a chain's first starts
 * speculatively, and the chain is accepted at a verified fixed point (every part's entry state is its predecessor's exit
 * state), which makes the result that of a sequential decoder on any content.
 * The coefficients (2 bytes per sample of the padded components), the parts' records and the per-frame tables belong to
 * the context's workspace: lr_context_trim frees them.
 * The call travels through lr_warp_perspective_device like lr_encode_jpeg_device: LR_WARP_JPEG_DECODE or-ed into `format`,
 * `M` pointing to an lr_jpeg_decode_args, src_image_bytes and dst_image_bytes the two regions' sizes, and width, height,
 * out_width, out_height and both row strides 0 (any option bit but LR_JPEG_ANY_SAMPLING and LR_JPEG_SCALED, or a non-zero one of these,
 * fails cleanly). */
typedef struct lr_jpeg_decode_args {
    const void* h_src;    /* HOST copy of the stream region (same layout as d_src); only the headers are read from it */
    const double* frames; /* HOST, 8 doubles per frame */
    int32_t* info;        /* HOST, 8 int32 per frame, written by the call */
} lr_jpeg_decode_args;
enum lr_warp_jpeg_decode { LR_WARP_JPEG_DECODE = 0x4000 }; /* or-ed into `format` like lr_warp_option */
enum lr_jpeg_decode_option { LR_JPEG_ANY_SAMPLING = 0x20000, LR_JPEG_SCALED = 0x80000 }; /* or-ed into lr_decode_jpeg_device's `format` (see above) */
/* One side of the picture that a frame of n samples gives at scale denominator N (LR_JPEG_SCALED, entry [6]: 0 or 1 as
 * stored, 2, 4, 8): ceil(n / N).  0 for anything else. */
static inline int lr_jpeg_scaled_size(int n, int N) {
    if (N == 0) N = 1;
    if (n < 1 || (N != 1 && N != 2 && N != 4 && N != 8)) return 0;
    return (n + N - 1) / N;
}
static inline int lr_decode_jpeg_device(lr_context* ctx, const void* d_src, const void* h_src, size_t src_bytes, int format,
                                        const double* frames, int batch, void* d_dst, size_t dst_bytes, int32_t* info) {
    lr_jpeg_decode_args a;
    a.h_src = h_src;
    a.frames = frames;
    a.info = info;
    return lr_warp_perspective_device(ctx, d_src, src_bytes, batch, 0, 0, 0, format | LR_WARP_JPEG_DECODE,
                                      (const double*)(const void*)&a, d_dst, dst_bytes, 0, 0, 0);
}
/* Probe mode of lr_decode_jpeg_device: width, height, components, layout, restart interval and status of every stream, from
 * the headers in host memory; for a frame whose entry [7] is 1 the upright size and, in info [7], the EXIF orientation.
 * No context, no GPU. */
static inline int lr_jpeg_info(const void* h_src, size_t src_bytes, const double* frames, int batch, int32_t* info) {
    return lr_decode_jpeg_device((lr_context*)0, (const void*)0, h_src, src_bytes, LR_PIX_U8X3, frames, batch, (void*)0, 0, info);
}

/* The commonest reader of a rectified picture is a network: lr_pack_tensor_device letterboxes finished 8-bit pictures that
 * lie in HBM into the slots of one contiguous batch tensor in HBM, converted, normalised and transposed, so that a model
 * reads its input where it lies.  The pass stands BEHIND the warp as the encoder does (the same pictures can go to both);
 * one launch for the whole batch; the call is SYNCHRONOUS like the encoder's: it waits for the context's stream, and on
 * return the tensor may be read from any stream.
 * format is LR_PIX_U8 (C = 1 channel, or C = 3 with LR_TENSOR_GRAY3) or LR_PIX_U8X3 (C = 3).  The tensor lies at d_dst (4-byte
 * aligned), contiguous, n x C x height x width (LR_TENSOR_NCHW) or n x height x width x C (LR_TENSOR_NHWC) elements of
 * `dtype`; dst_bytes is at least its size, and the destination region lies apart from the source region.
 * `frames` is a HOST table of 8 doubles per frame: [0] [1] the picture's width_b, height_b (1 .. width, 1 .. height), [2] [3]
 * byte offset of the picture from d_src and its row stride in bytes (at least a row), [4] its slot, 0 .. n - 1 (no two
 * frames share one), [5] [6] left, top of the picture inside its slot (left + width_b <= width, top + height_b <= height),
 * [7] reserved, 0.  The table follows LR_WARP_RAGGED's rules: integers (at most 2^53), every picture inside src_bytes.
 * EVERY element of a slot that a frame names is written: the picture where it lies, the pad level elsewhere.  Slots that no
 * frame names, and bytes behind the tensor, are not touched.
 * The rule (tests/numpy_tensor_ref.py produces the same bytes): an element of channel c whose
 * level is v (an integer 0 .. 255; pad[c] outside the picture) is p = v * scale[c] in double, y = p + bias[c] in double, f =
 * (float)y rounded to nearest even, and for LR_TENSOR_F16 and LR_TENSOR_BF16 f rounded to nearest even once more (BF16 on
 * the bits of f).  The host computes the 256 x C elements once per call; the kernel looks them up.  With LR_TENSOR_SWAP
 * channel c reads source channel 2 - c (scale, bias and pad stay the TENSOR channel's).
 * The whole call is checked before anything is enqueued: on failure nothing is launched or written and lr_last_error names
 * the frame and the entry.  Refused: a null pointer, batch < 1 or > n, n, height or width below 1 (or a side above 2^30), a
 * tensor beyond 2^53 bytes or beyond dst_bytes, an unknown dtype, layout or flag bit, LR_TENSOR_GRAY3 with LR_PIX_U8X3,
 * LR_TENSOR_SWAP with one channel, another source format, a non-finite scale or bias, a level of a channel whose element is
 * not finite in the dtype, a pad that is no integer 0 .. 255, a table entry that is no integer in its range, a picture
 * outside its slot or outside src_bytes, two frames in one slot, overlapping regions, a misaligned d_dst.
 * The frame records and the element table belong to the context's workspace: lr_context_trim frees them.
 * The library's table of exported symbols is full, so the call travels through lr_warp_perspective_device like
 * lr_encode_jpeg_device: LR_WARP_TENSOR or-ed into `format`, `M` pointing to an lr_tensor_args, src_image_bytes and
 * dst_image_bytes the two regions' sizes, and width, height, out_width, out_height and both row strides 0 (any other option
 * bit or a non-zero one of these fails cleanly).  lr_pack_tensor_device below is that call, spelled out. */
enum lr_tensor_dtype { LR_TENSOR_F32 = 0, LR_TENSOR_F16 = 1, LR_TENSOR_BF16 = 2 };
enum lr_tensor_layout { LR_TENSOR_NCHW = 0, LR_TENSOR_NHWC = 1 };
enum lr_tensor_flags { LR_TENSOR_SWAP = 1,    /* channel c comes from source channel 2 - c (BGR nets) */
                       LR_TENSOR_GRAY3 = 2 }; /* LR_PIX_U8 source into THREE channels, each through its own scale/bias */
typedef struct lr_tensor_args {
    const double* frames;     /* HOST, 8 doubles per frame */
    int32_t n, height, width; /* slots N and the slot size H x W */
    int32_t dtype, layout, flags;
    double scale[3], bias[3]; /* per channel */
    double pad[3];            /* per channel: the LEVEL (integer 0..255) of elements outside the picture */
} lr_tensor_args;
enum lr_warp_tensor { LR_WARP_TENSOR = 0x10000 }; /* or-ed into `format` like lr_warp_option */
static inline int lr_pack_tensor_device(lr_context* ctx, const void* d_src, size_t src_bytes, int format, const lr_tensor_args* args,
                                        int batch, void* d_dst, size_t dst_bytes) {
    return lr_warp_perspective_device(ctx, d_src, src_bytes, batch, 0, 0, 0, format | LR_WARP_TENSOR, (const double*)(const void*)args,
                                      d_dst, dst_bytes, 0, 0, 0);
}

/* ---- stage API (tests, bench) --------------------------------------------------------- */
/* Stage 1: fused 5x5 derivative filter + magnitude + direction bin + dilated-bin mask +
 * 5x5 non-max candidates (reference line_detector.cpp:41-49,126-182, filter.cpp:29-98,161-168). */
int lr_stage_filter(lr_context* ctx, const float* d_image, int width, int height, int stride);
/* Same on a host buffer (uploaded to the context's staging image first; any stride sign). */
int lr_stage_filter_host(lr_context* ctx, const float* buffer, int width, int height, int stride);
/* Stage 2: global max, seed threshold, ordered seed list (line_detector.cpp:209-220, filter.cpp:168-194). */
int lr_stage_seeds(lr_context* ctx, int* n_seeds);
/* Stage 3: ordered flood (filter.cpp:101-153, line_detector.cpp:92-122).  The parallel flood (mode >= 1) CONSUMES the
 * filter output: it clears the direction mask of every pixel it labels, so LR_BUF_DMASK can no longer be downloaded
 * and a second flood of the same frame needs lr_stage_filter + lr_stage_seeds again (both fail with a message). */
int lr_stage_flood(lr_context* ctx, int* n_components);
/* Stage 4: weighted-PCA line fit per component (geometry.cpp:20-61); output in seed order. */
int lr_stage_fit(lr_context* ctx, LineSegment* out, int capacity, int* n_lines);

enum lr_buffer_id {
    LR_BUF_DX = 0,        /* float  w*h */
    LR_BUF_DY = 1,        /* float  w*h */
    LR_BUF_DMASK = 2,     /* uint8  w*h: bit b = pixel is inside the 3x3 dilation of grad_bin==b */
    LR_BUF_LABEL = 3,     /* int32  w*h: claiming seed index or -1 */
    LR_BUF_SEED_IDX = 4,  /* int32  n_seeds: row*w+col, canonical order */
    LR_BUF_SEED_BIN = 5,  /* int32  n_seeds */
    LR_BUF_SEED_THR = 6,  /* float  n_seeds: (1-TRACE_TOLERANCE)*value at the seed */
    LR_BUF_MAXMAG = 7,    /* float  1 */
    LR_BUF_SEED_SIZE = 8, /* int32  n_seeds: pixels claimed by each seed's flood (0 = skipped) */
    LR_BUF_SEED_REC = 9,  /* uint32 n_seeds x 4: {SEED_IDX, SEED_BIN, bits of SEED_THR, 0}, the record the flood's walks read */
    LR_BUF_COUNTS = 10,   /* uint32 16: the last frame's count words -- [0] seeds, [1] components, [2] their pixels, [12] components
                             that were fitted, [13] their pixels ([1] and [2] again unless the frame call left out the fit of components
                             too small for its min_length: lr_set_estimator); the other words are internal */
};
int lr_download(lr_context* ctx, int buffer_id, void* dst, size_t bytes);

enum lr_stage_id {
    LR_T_UPLOAD = 0,
    LR_T_FILTER = 1,
    LR_T_SEEDS = 2,
    LR_T_FLOOD = 3,
    LR_T_FIT = 4,
    LR_T_RANSAC = 5,
    LR_T_TOTAL = 6,
    LR_T_FILTER_KERNEL = 7, /* the fused filter kernel alone */
    LR_T_COUNT = 8,
};
/* HIP-event times (ms) of the stages of the last call on this context. */
int lr_stage_times(lr_context* ctx, float* ms, int count);
/* The frame calls (lr_find_line_segment_groups_*, the batch entries and the drop-in symbol) record their stage timers
 * only when asked: lr_set_stage_timing(ctx, 1) or LIBRECTIFY_STAGE_TIMES in the environment (seven event records per
 * frame cost some 40 us of idle GPU).  lr_stage_times then returns the last frame's stages; the staged API below always
 * times its stages. */
void lr_set_stage_timing(lr_context* ctx, int on);
/* Duration (ms) of the last fused filter kernel alone (HIP events around its launch); valid right after
 * lr_stage_filter*, without running the later stages. */
int lr_filter_kernel_ms(lr_context* ctx, float* ms);
/* Extra counters of the last call: [0] seeds, [1] components, [2] flood rounds, [3] labelled pixels, and how the
 * flood's walks were stored: [4] seeds that moved to the second LDS tier, [5] global slabs used, [6] seeds finished by
 * the ordered single-wave tail (storage exhausted); [7] laps of the frame through the pipeline (1 normally); [8] pixels
 * the flood's explorations walked in all rounds together (over [3]: the re-walk factor), [9] their 8x8-tile steps, [10] rounds enqueued under
 * the schedule hook (lr_set_flood_schedule; counted on the host, 0 without the hook; the slot counted re-walks from
 * way-points once), [11] footprints worked out from a log instead of
 * walked (lr_set_flood_logs), [12] those of them that took the fall-back path (sweeps), [13] walks that outgrew the second
 * tier's table and were held back until their seed was the lowest active one (instead of moving into a global slab),
 * [14] giant steps: floods of the lowest active seed labelled by the whole device (lr_set_flood_giant_step), [15] walks that
 * outgrew the first tier in a round enqueued without the second (the context's last frame never needed it: such a walk waits
 * a round; LIBRECTIFY_FLOOD_CALM_HINT=0 enqueues every round with the second tier). */
int lr_stage_counters(lr_context* ctx, int64_t* out, int count);

/* ---- RANSAC --------------------------------------------------------------------------- */
/* Scores n_iter two-line hypotheses of the line-pencil model (line_pencil.cpp:89-140,
 * estimator.h:37-71) over the lines listed in `indices`, on the GPU.  lines_norm are
 * bbox-normalised segments (HOST).  Outputs the raw best hypothesis (first strictly best),
 * its score and iteration (-1 if every sample was degenerate). */
int lr_ransac_best(lr_context* ctx, const LineSegment* lines_norm, int n, const int32_t* indices, int n_idx, float tol,
                   int n_iter, uint64_t seed, uint32_t round, float* best_h3, float* best_score, int* best_iter);
/* estimate_line_pencils (line_pencil.cpp:148-177): writes group_id in place (HOST array). */
int lr_estimate_line_pencils(lr_context* ctx, LineSegment* lines, int n, int max_models, float inlier_deg,
                             float garbage_deg, int n_iter, uint64_t seed);

/* Diamond-space ("cascaded Hough") accumulator, opt-in: what reference cht.h:13-24 describes (its cht.cpp is an
 * uncompiled sketch).  d x d accumulator (8 <= d <= 128) of length-weighted line polylines, kept in LDS with integer
 * atomics; returns the de-normalised vanishing point of the strongest pencil (z = 0: ideal point) and, if acc_out is
 * not NULL, the d*d 64-bit accumulator. */
int lr_cht_vanishing_point(lr_context* ctx, const LineSegment* lines, int n, int d, Point* vp, uint64_t* acc_out);
/* postprocess_lines_segments (line_detector.cpp:332-444), what refine=true runs: merges collinear neighbours.
 * `out` must hold n records; the O(n^2) pair test runs on the GPU for n >= 2048. */
int lr_refine_lines(lr_context* ctx, const LineSegment* in, int n, LineSegment* out, int* n_out);

/* ---- PROSAC / Hough weights (opt-in) --------------------------------------------------- */
/* The reference compiles prosac.h and DirectEstimator (estimator.h:82-96) but never instantiates them (ChangeLog.md:
 * "pure RANSAC is used"), so RANSAC is the default here too.  kind: 0 = RANSAC, 1 = PROSAC with T_N iterations
 * (<= 0: the reference's niter_RANSAC(0.9, 0.5, 2) = 9, prosac.h:116), 2 = DirectEstimator (refit on the lines whose
 * Hough weight exceeds 0.95; the parameter is ignored), 3 = the diamond-space accumulator (cht.h:13-24) with a
 * param x param accumulator (<= 0: 128; 8..128), see lr_estimate_line_pencils_cht.
 * kind 0 has one setting: by default a frame call does not fit components of at most floor(max(min_length, 5) / 1.4157)
 * pixels, whose segments cannot pass its length test (results and counts are the same; LR_BUF_COUNTS [12], [13] say what
 * was fitted); param == 0 fits every component, any other value (the Python default is -1) leaves them out. */
void lr_set_estimator(lr_context* ctx, int kind, int param);
/* estimate_multiple_structures (estimator.h:99-145) around the diamond-space accumulator as cht.h:13-24 describes
 * it: all lines vote once (length-weighted polylines, integer votes in LDS), every round takes the accumulator's
 * strongest cell as the hypothesis, the remaining lines within `inlier_deg` of it decide the refit (fit_optimal), the
 * refit's inliers get the round's id, near misses (< garbage_deg) are dropped, and the votes of both are taken back
 * out of the accumulator ("the weights can be negative (so lines can be removed!)", cht.h:18).  Writes group_id in
 * place (HOST array).  Optional outputs: models3 = refit of each round (3 floats, normalised coordinates),
 * n_models = rounds run, peak_cells = winning cell (row * d + column) of each round, votes = accumulator cells voted
 * for (added or taken back) during the call.  Parity unpinned: the reference's cht.cpp is an uncompilable sketch. */
int lr_estimate_line_pencils_cht(lr_context* ctx, LineSegment* lines, int n, int max_models, float inlier_deg,
                                 float garbage_deg, int d, float* models3, int* n_models, uint32_t* peak_cells,
                                 uint64_t* votes);
/* LinePencilModel::get_weights (line_pencil.cpp:47-86): 65x65 hemisphere accumulator (LDS, 64-bit integer
 * atomics), peak direction, inclination^4 per line listed in `indices`. */
int lr_ht_weights(lr_context* ctx, const LineSegment* lines_norm, int n, const int32_t* indices, int n_idx, float* weights);
/* PROSAC_Estimator::solve (prosac.h:104-299); trace4 = iterations run, n_star, iteration of the best sample, its inlier count. */
int lr_prosac_solve(lr_context* ctx, const LineSegment* lines_norm, int n, const int32_t* indices, int n_idx, float tol,
                    int T_N, uint64_t seed, uint32_t round, float* h3, int32_t* trace4);
int lr_estimate_line_pencils_prosac(lr_context* ctx, LineSegment* lines, int n, int max_models, float inlier_deg,
                                    float garbage_deg, int T_N, uint64_t seed);
/* DirectEstimator::solve (estimator.h:82-96) and estimate_multiple_structures around it. */
int lr_direct_solve(lr_context* ctx, const LineSegment* lines_norm, int n, const int32_t* indices, int n_idx, float* h3);
int lr_estimate_line_pencils_direct(lr_context* ctx, LineSegment* lines, int n, int max_models, float inlier_deg,
                                    float garbage_deg);

#ifdef __cplusplus
}
#endif

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
