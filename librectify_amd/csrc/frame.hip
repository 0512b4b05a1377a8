// One frame: the stages' enqueue functions, the frame driver (run_frame), the staged API and the single-frame entry points
// for device and host images.
#include "host.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace lramd {

// ---- stages ------------------------------------------------------------------------------
//
// Every stage is an "enqueue" function that launches its kernels on the context stream and never waits: seed,
// component, pixel and line counts stay in device memory (d_counts, d_gctl) and the kernels read them there;
// launches cover capacities (seed_cap, line_cap) chosen before the counts exist.  The frame driver (run_frame) enqueues
// all stages back to back and synchronises once; the staged API (lr_stage_*) wraps one enqueue function each and waits
// for it, because its callers want the counts.

namespace {

uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// capacity of the seed sort for a frame of this size when nothing better is known: one seed per 32 pixels (the
// synthetic 4K frame has one per 204, the reference's doc image one per 85)
uint32_t initial_seed_cap(size_t npix) {
    return (uint32_t)std::min<size_t>(npix, std::max<size_t>(round_up((uint32_t)(npix / 32), 1024), 4096));
}

uint32_t line_cap_for(const lr_context* c) {
    return (uint32_t)std::min<size_t>(c->seed_cap, c->ws.cap_pix / 6 + 16);
}


PencilTable table_of(lr_context* c, int which) {
    const size_t cl = c->cap_glines;
    float* b = c->d_tables + (size_t)which * 8 * cl;
    return PencilTable{b, b + cl, b + 2 * cl, b + 3 * cl, b + 4 * cl, b + 5 * cl, b + 6 * cl, b + 7 * cl,
                       c->d_orig + (size_t)which * cl};
}

int ensure_result_block(lr_context* c, size_t lines) {
    if (lines <= c->res_lines_cap && c->h_res) return 0;
    LR_HIP(hipStreamSynchronize(c->stream));
    if (c->h_res.grow(kResHeaderBytes + lines * sizeof(LineSegment))) return 1;
    c->res_lines_cap = lines;
    return 0;
}

FloodBuffers flood_buffers_for(lr_context* c) {
    FloodBuffers fbuf = c->flood.fb;
    // test hooks: 2 and 3 exercise the slab and exhausted-storage paths (no second LDS tier, no / two slabs),
    // 4 the slab path with the full pool, 5 a stall during the hold-back, 6 / 7 the second tier's team running out of storage
    if (c->opt.flood_mode >= 2 && c->opt.flood_mode <= 4) fbuf.second_tier = false;
    fbuf.second_tier_from_start = c->flood_big_hint;
    fbuf.hold_from_start = c->flood_hold_hint;
    fbuf.staged_from_start = c->flood_staged_hint;
    if (c->opt.flood_mode == 2) fbuf.n_slabs = 0;
    if (c->opt.flood_mode == 3) fbuf.n_slabs = 2;
    if (c->opt.flood_mode == 5) {  // second tier with room for one seed per round and no slab: the rounds stall while
        fbuf.n_slabs = 0;      // the weakest seeds are held back, and must still hand over to the ordered tail
        fbuf.big_cap_override = 1;
    }
    if (c->opt.flood_mode == 6) fbuf.team_tile_cap = 200;  // the second tier's team runs out early: the whole team moves into a
    if (c->opt.flood_mode == 7) {                           // global slab and goes on there (6), or there is none: incomplete
        fbuf.team_tile_cap = 200;                       // walk, barrier, ordered tail (7)
        fbuf.n_slabs = 0;
    }
    static const bool partial_off = std::getenv("LIBRECTIFY_FLOOD_PARTIAL") && std::atoi(std::getenv("LIBRECTIFY_FLOOD_PARTIAL")) == 0;
    fbuf.partial_commits = !partial_off && c->opt.flood_partial;
    fbuf.rewalk_logs = c->opt.flood_logs;
    fbuf.log_sweep = c->opt.flood_log_sweep;
    if (!c->flood_sched_off) {  // (test hook lr_set_flood_schedule: single calls and stage calls)
        fbuf.sched_order = c->flood_sched_order;
        fbuf.sched_seed = c->flood_sched_seed;
        fbuf.sched_width = c->flood_sched_width;
    }
    fbuf.log_min_tiles = c->flood_log_min;
    fbuf.log_walk_tiles = c->flood_log_walk;
    fbuf.giant_hold = c->opt.flood_mode == 1;  // (the storage test hooks -- modes 2-7 -- keep their slabs)
    static const bool giant_step_off = std::getenv("LIBRECTIFY_FLOOD_GIANT_STEP") && std::atoi(std::getenv("LIBRECTIFY_FLOOD_GIANT_STEP")) == 0;
    fbuf.giant_step = !giant_step_off && c->opt.flood_giant_step;
    fbuf.giant_parent = reinterpret_cast<uint32_t*>(c->ws.queue.get());
    fbuf.rewalk_big = c->flood_logbig_hint && !c->flood_logbig_off;  // (the context's last frame had walks beyond the first tier)
    if (c->opt.flood_staged) fbuf.win_first_shift = 3;
    fbuf.blind_rounds = c->flood_rounds_hint;
    // rounds just in time (FloodBuffers::host_progress): what the last frame needed less one at once (three on a new context)
    static const bool jit_off = std::getenv("LIBRECTIFY_FLOOD_JIT") && std::atoi(std::getenv("LIBRECTIFY_FLOOD_JIT")) == 0;
    static_assert(16 + kFloodCtrlWords <= 72, "the control block's copy ends where the report word begins");
    fbuf.host_progress = c->h_counts + 72;
    fbuf.host_ctrl = c->h_counts + 16;
    // (LIBRECTIFY_FLOOD_CALM_HINT=0: every blind round brings the second tier's launch, as until round 5)
    static const int calm_hint_env = std::getenv("LIBRECTIFY_FLOOD_CALM_HINT") ? std::atoi(std::getenv("LIBRECTIFY_FLOOD_CALM_HINT")) : 1;
    fbuf.calm_hint = calm_hint_env != 0 && c->flood_calm_hint;
    fbuf.jit_sleep_us = c->flood_jit_sleep_us;
    // (at most four rounds blindly -- the rounds that always bring their `rest` launch, kernels_flood.hip kRestRounds: a later
    // blind round whose list is longer than its grid walks only a part of it, and lists stay long while a window is closed in
    // front of waiting seeds (a frame of soft blobs went to the ordered tail that way now and then: 42 -> 200 ms); a round
    // enqueued just in time knows its list's length and brings the launch when it needs it.
    constexpr int kJitFirstMax = 4;
    fbuf.jit_first = (c->opt.flood_jit && !jit_off) ? std::min(c->flood_rounds_last > 0 ? std::max(c->flood_rounds_last - 1, 2) : 3, kJitFirstMax) : 0;
    return fbuf;
}

FloodFrame flood_frame_for(lr_context* c) {
    return FloodFrame{c->ws.dx, c->ws.dy, c->ws.dmask, c->w, c->h, c->ws.seed_idx, c->ws.seed_bin, c->ws.seed_thr,
                      c->d_counts + kCntSeeds, c->seed_cap, c->trig, c->ws.label, c->ws.seed_size, c->ws.queue, c->ws.seed_rec};
}

// everything of a frame's first stage but the launch: workspace, seed-sort capacity, state of the last run
int prepare_frame(lr_context* c, int w, int h) {
    LR_HIP(hipSetDevice(c->device));
    if (w < 5 || h < 5) {
        set_error("image smaller than the 5x5 filter");
        return 1;
    }
    if (ctx_ensure_image_capacity(c, w, h)) return 1;
    if (c->w != w || c->h != h || c->seed_cap == 0) c->seed_cap = initial_seed_cap((size_t)w * h);
    if (c->seed_cap_once) {  // test hook (lr_set_seed_capacity): this frame starts with the given capacity
        c->seed_cap = (uint32_t)std::min<size_t>((size_t)w * h, c->seed_cap_once);
        c->seed_cap_once = 0;
    }
    c->w = w;
    c->h = h;
    c->n_seeds = c->n_comp = c->n_px = 0;
    c->dmask_consumed = false;
    for (bool& v : c->stage_valid) v = false;
    return 0;
}

// `format`: the frame's lr_pixel_format, `stride` in pixels of it.  fp32 and 8-bit gray frames are read by the filter kernel
// itself (an instantiation each); an interleaved 8-bit frame first becomes luma / 256 in a buffer of the context.
int enqueue_filter(lr_context* c, const void* d_image, int format, int w, int h, int stride) {
    if (prepare_frame(c, w, h)) return 1;
    const size_t bpp = (size_t)pix_bytes(format);
    if (bpp == 0 || d_image == nullptr || stride < w) {
        set_error(bpp == 0 ? "unknown pixel format of the frames" : "launch_filter: bad geometry");
        return 1;
    }
    const size_t npix = (size_t)w * h;
    if (format == LR_PIX_U8X3) {
        // three byte loads a row would keep thirty registers of the filter's prefetch queue busy; one
        // launch of the prepare kernel at the frame's own size (weights exactly 1: the value is exactly luma / 256) instead
        if (npix >= ((size_t)1 << 29)) {
            set_error("launch_filter: image larger than 2^29 pixels is not supported (seed key packs index in 29 bits)");
            return 1;
        }
        if (c->frames.luma.cap() < npix) {
            LR_HIP(hipStreamSynchronize(c->stream));
            if (c->frames.luma.grow(npix)) return 1;
        }
        if (ctx_prepare_frames(c, d_image, 0, 1, w, h, (size_t)stride * bpp, LR_PIX_U8X3, c->frames.luma.get(), 0, w, h, (size_t)w * sizeof(float)))
            return 1;
        d_image = c->frames.luma.get();
        format = LR_PIX_F32;
        stride = w;
    }
    // The filter kernel addresses the frame with 32-bit byte offsets from its first row (buffer resource and row offsets,
    // kernels_filter.hip).  A caller's frame whose rows span 4 GiB or more -- a narrow crop of a large device mosaic -- is
    // packed into a buffer of the context first, so the kernel sees the same pixels at stride w.  The limit is one of BYTES:
    // an 8-bit frame reaches it at four times the pixel span of an fp32 one, and is packed as bytes.
    // (a frame of 2^29 pixels or more is refused by launch_filter without the copy)
    const size_t fbpp = (size_t)pix_bytes(format);
    if (stride > w && (uint64_t)w * (uint64_t)h < (1ull << 29) &&
        ((uint64_t)(h - 1) * (uint64_t)stride + (uint64_t)w) * fbpp >= (1ull << 32)) {
        if (c->frames.packed.cap() < npix) {  // (sized in floats: a frame of bytes fits)
            LR_HIP(hipStreamSynchronize(c->stream));
            if (c->frames.packed.grow(npix)) return 1;
        }
        LR_HIP(hipMemcpy2DAsync(c->frames.packed, (size_t)w * fbpp, d_image, (size_t)stride * fbpp,
                                (size_t)w * fbpp, (size_t)h, hipMemcpyDeviceToDevice, c->stream));
        d_image = c->frames.packed;
        stride = w;
    }
    if (c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[0], c->stream));
    if (launch_filter(d_image, format, w, h, stride, c->fconsts, c->ws.dx, c->ws.dy, c->ws.dmask, c->ws.cand, c->ws.cand_count, c->ws.tile_max,
                      c->stream))
        return 1;
    if (c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[1], c->stream));
    return 0;
}

int enqueue_seeds(lr_context* c) {
    const FilterGeom fg = filter_geometry(c->w, c->h);
    if (launch_seed_select(c->ws.cand, c->ws.cand_count, c->ws.tile_max, fg.n_tiles, fg.cand_cap, c->seed_keep_ratio, c->maxmag,
                           c->ws.tile_pass, c->ws.tile_off, c->ws.keys_a, c->seed_cap, c->d_counts + kCntSeeds, ++c->select_tag ? c->select_tag : ++c->select_tag,
                           c->stream))
        return 1;
    if (launch_seed_order(c->ws.keys_a, c->ws.keys_b, c->d_counts + kCntSeeds, c->seed_cap, c->ws.dx, c->ws.dy, c->trig, kTraceTolerance,
                          c->ws.seed_idx, c->ws.seed_bin, c->ws.seed_thr, c->ws.seed_rec, c->stream))
        return 1;
    if (c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[2], c->stream));
    return 0;
}

// the flood's rounds, blindly (parallel modes) or the single-wave ordered kernel (mode 0)
int enqueue_flood(lr_context* c) {
    const size_t npix = (size_t)c->w * c->h;
    c->flood_rounds = 1;
    if (c->opt.flood_mode == 0) {
        if (launch_label_init(c->ws.label, npix, c->stream)) return 1;  // (the parallel rounds' set-up kernel does it itself)
        if (launch_flood_ordered(c->ws.dx, c->ws.dy, c->ws.dmask, c->w, c->h, c->ws.seed_idx, c->ws.seed_bin, c->ws.seed_thr,
                                 c->d_counts + kCntSeeds, c->seed_cap, c->trig, c->ws.label, c->ws.seed_size, c->ws.queue, c->stream))
            return 1;
    } else {
        if (ensure_flood_buffers(c)) return 1;
        if (flood_enqueue(flood_buffers_for(c), flood_frame_for(c), &c->flood_prog, c->h_counts + 16, c->stream)) return 1;
        // the commit pass clears the direction mask of every labelled pixel (kernels_flood.hip): the filter
        // output is consumed, a second flood needs lr_stage_filter + lr_stage_seeds again
        c->stage_valid[0] = c->stage_valid[1] = false;
        c->dmask_consumed = true;
    }
    if (c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[3], c->stream));
    return 0;
}

// After a synchronisation: did the blind rounds finish the flood?  If not, finish it now (synchronises).
int finish_flood(lr_context* c, bool* extra) {
    *extra = false;
    if (c->opt.flood_mode == 0) return 0;
    if (flood_finish(flood_buffers_for(c), flood_frame_for(c), &c->flood_prog, c->h_counts + 16, &c->flood_rounds,
                     c->flood_tiers, extra, c->stream))
        return 1;
    static const bool call_debug = std::getenv("LIBRECTIFY_CALL_DEBUG") != nullptr;
    if (call_debug)
        std::fprintf(stderr, "flood: %d rounds, %u walks in the second tier, %u of them long, hold-back phase %u (started with it: %d)\n",
                     c->flood_rounds, c->flood_tiers[0], c->flood_tiers[8], c->flood_tiers[3], (int)c->flood_hold_hint);
    c->flood_logbig_hint = c->flood_tiers[0] > 0;
    c->flood_calm_hint = c->flood_tiers[0] == 0 && c->flood_tiers[1] == 0 && c->flood_tiers[15] == 0;
    // The second tier is always there: a frame of regions that follows a frame of lines on this context used to run its
    // first batch of rounds without it, every long walk in a global slab (6.4 instead of 1.5 ms of flood on the natural
    // 4K frame), and an empty launch of its kernel costs a round 5 us.  The hold-back starts with the frame only after a
    // frame of REGIONS (many walks beyond the first tier's table): engaged from the start on a frame of lines it costs
    // three rounds (1.55 instead of 1.10 ms), and the old rule -- "the last frame engaged it" -- kept itself alive from
    // frame to frame once a single frame had.
    c->flood_big_hint = true;
    c->flood_hold_hint = c->flood_tiers[3] != 0 && c->flood_tiers[8] >= 16;
    // A frame that went on staged (many walks held back in its first round) hands that on; a frame that STARTED staged
    // keeps handing it on while its floods still look like regions (walks in the second tier: the staged start itself
    // keeps the giants away, so their count says nothing any more).
    constexpr uint32_t kStagedKeep = 64;  // second-tier walks of a staged frame that keep the hint
    c->flood_staged_hint = c->flood_tiers[14] != 0 && (!c->flood_staged_hint || c->flood_tiers[0] >= kStagedKeep);
    // (a frame that started staged cannot tell whether it would have gone staged by itself: every sixteenth frame of such
    // a run starts without the hint and finds out -- a ramp under noise pays 1.6 ms for that frame, soft blobs that
    // inherited the hint from other content are rid of it)
    c->flood_staged_streak = c->flood_staged_hint ? c->flood_staged_streak + 1 : 0;
    if (c->flood_staged_streak >= 16) {
        c->flood_staged_hint = false;
        c->flood_staged_streak = 0;
    }
    if (c->flood_staged_hint) c->flood_hold_hint = false;
    // (The verdict "many long walks" -- early hand-over to the second tier, flood_advance -- is NOT carried over: started
    // with it, the natural 4K frame sends 735 walks to the second tier in round one and its flood takes 1.88 ms instead
    // of 1.5, and a frame of lines that follows pays 0.7 ms for the wrong guess.)

    // blind rounds of the next frame: what this one needed plus two, decaying slowly
    c->flood_rounds_hint = std::max(std::max(c->flood_rounds + 2, 6), c->flood_rounds_hint - 1);
    c->flood_rounds_last = c->flood_rounds;
    return 0;
}

// Floods of up to this many pixels cannot give a segment longer than ml = max(min_length, kLineMinLength), whatever their
// shape (the proof stands beside component_offsets_kernel, kernels_fit.hip): floor(ml / 1.4157), never below the size
// threshold itself.  The frame's own min_length: the frames of a table each have theirs.
int fit_min_for(float min_length) {
    const double ml = std::fmax((double)min_length, (double)kLineMinLength);  // (a NaN is the floor, as in filter_lines_kernel)
    const double n = std::floor(ml / 1.4157);
    return (int)std::min(std::max(n, (double)kComponentMinSize), 1073741824.0);
}

// fit_min: floods of up to that many pixels get no component (kComponentMinSize: every component is fitted -- the staged API,
// refine and the opt-in estimators, which need all raw segments)
int enqueue_fit(lr_context* c, int fit_min = kComponentMinSize) {
    const size_t npix = (size_t)c->w * c->h;
    const uint32_t comp_cap = line_cap_for(c);
    // Floods of more than 2^14 pixels have launches of their own (kernels_fit.hip: huge_count_kernel, huge_sort_kernel), left
    // out when the host KNOWS that the frame has none: the flood's rounds, enqueued just in time, report their largest commit.
    const bool with_huge = !(c->opt.flood_mode != 0 && c->flood_prog.sizes_known && c->flood_prog.max_flood <= (1u << 14));
    if (launch_component_offsets(c->ws.seed_size, c->d_counts + kCntSeeds, c->seed_cap, kComponentMinSize, fit_min, c->ws.comp_rank,
                                 c->ws.comp_seed, c->ws.comp_off, c->d_counts + kCntComp, c->d_counts + kCntFitComp, c->ws.comp_large,
                                 (uint32_t)(c->ws.cap_pix / 64 + 16), c->d_counts + kCntLarge, c->ws.temp, c->ws.temp.cap(), ++c->fit_tag ? c->fit_tag : ++c->fit_tag, c->ws.cursor,
                                 with_huge ? c->ws.huge : HugeSort{}, c->stream))
        return 1;
    if (launch_component_scatter(c->ws.label, npix, c->ws.comp_rank, c->ws.comp_off, c->ws.cursor, c->ws.px_a, c->ws.huge, c->d_counts + kCntLarge, with_huge,
                                 c->stream))
        return 1;
    // (the sorted seed keys are dead once the seeds are set up: their buffer is the large lists' sorting scratch)
    if (launch_component_sort(c->ws.px_a, c->ws.px_b, c->ws.comp_off, c->d_counts + kCntFitComp, comp_cap, c->ws.comp_large,
                              (uint32_t)(c->ws.cap_pix / 64 + 16), c->d_counts + kCntLarge, reinterpret_cast<uint32_t*>(c->ws.keys_b.get()),
                              c->ws.cursor, c->ws.huge, with_huge, c->stream))
        return 1;
    static const bool fit_debug = std::getenv("LIBRECTIFY_FIT_DEBUG") != nullptr;
    if (fit_debug) {
        uint32_t cnt[16];
        LR_HIP(hipStreamSynchronize(c->stream));
        LR_HIP(hipMemcpy(cnt, c->d_counts, sizeof(cnt), hipMemcpyDeviceToHost));
        std::fprintf(stderr, "fit: threshold %d, %u components of %u px fitted\n", fit_min, cnt[kCntFitComp], cnt[kCntFitPx]);
        std::fprintf(stderr, "fit: with_huge %d (sizes known %d, largest flood %u); seeds %u comps %u px %u; lists: %u of 65..1024 px, %u longer, %u huge in %u buckets; counter %u\n",
                     (int)with_huge, (int)c->flood_prog.sizes_known, c->flood_prog.max_flood, cnt[0], cnt[1], cnt[2], cnt[4], cnt[5], cnt[6], cnt[7], cnt[10]);
        const uint32_t nj = std::min<uint32_t>(cnt[7], 6);
        std::vector<uint32_t> jobs(4 * nj + 4);
        if (nj) LR_HIP(hipMemcpy(jobs.data(), c->ws.huge.jobs, nj * 16, hipMemcpyDeviceToHost));
        for (uint32_t j = 0; j < nj; ++j) std::fprintf(stderr, "   bucket job %u: start %u, %u px, table word %u\n", j, jobs[4 * j], jobs[4 * j + 1], jobs[4 * j + 2]);
    }
    if (launch_fit(c->ws.px_b, c->ws.px_a, c->ws.comp_off, c->ws.comp_seed, c->d_counts + kCntFitComp, comp_cap, c->ws.seed_bin, c->ws.dx, c->ws.dy, c->w,
                   c->trig, c->ws.scratch_w, c->ws.d_lines, c->ws.cursor, c->ws.huge, c->d_counts + kCntLarge, with_huge, c->stream))
        return 1;
    if (c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[4], c->stream));
    return 0;
}

// estimate_line_pencils (line_pencil.cpp:148-177) on the lines in d_flines, whose count, bounding box and control
// words a filter_lines / lines_bbox launch has left in d_gctl / d_gnorm.
}  // namespace

int enqueue_groups(lr_context* c, uint32_t line_cap, int max_models, float inlier_deg, float garbage_deg, int n_iter,
                   uint64_t seed, bool model_done, bool gather) {
    if (max_models > kMaxPeelModels) {  // the refit models and the diagnostics slots of a frame are sized for this many
        set_error("estimate_line_pencils: max_models above " + std::to_string(kMaxPeelModels) + " (the reference uses 4, config.h:25)");
        return 1;
    }
    const float tol = cos_threshold(inlier_deg), garbage_tol = cos_threshold(garbage_deg);
    const PencilTable all = table_of(c, 0);
    PencilTable tab[2] = {table_of(c, 1), table_of(c, 2)};
    // (model_done: the launch that filtered the lines has written both tables already -- launch_filter_lines)
    if (!model_done && launch_pencil_model(c->d_flines, c->d_gctl, c->d_gnorm, all, tab[0], line_cap, c->stream)) return 1;
    const float degeneracy_tol = 0.05f;  // line_pencil.h:25
    for (int k = 0; k < max_models; ++k) {
        if (n_iter > 0 &&
            launch_ransac_score_dev(tab[k & 1].soa(), c->d_gctl, max_models, tol, degeneracy_tol, (uint32_t)n_iter, seed,
                                    c->d_best_slots, c->stream))
            return 1;
        // (gather: the last round's launch copies the frame's results into the page-locked block as well)
        const bool last = gather && k == max_models - 1;
        if (launch_peel(tab[k & 1], tab[(k + 1) & 1], all, c->d_best_slots, seed, tol, garbage_tol,
                        max_models, c->d_gctl, c->d_inl, c->d_flines, c->d_models, c->d_counts,
                        (uint32_t)std::min<size_t>(c->res_lines_cap, c->d_flines.cap()), last ? c->h_res.get() : nullptr, c->stream))
            return 1;
    }
    return 0;
}

namespace {

void record_stage_times(lr_context* c, bool with_groups) {
    if (!c->opt.timing_on) return;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
    c->stage_ms[LR_T_FILTER] = ms;
    c->stage_ms[LR_T_FILTER_KERNEL] = ms;
    (void)hipEventElapsedTime(&ms, c->ev[1], c->ev[2]);
    c->stage_ms[LR_T_SEEDS] = ms;
    (void)hipEventElapsedTime(&ms, c->ev[2], c->ev[3]);
    c->stage_ms[LR_T_FLOOD] = ms;
    (void)hipEventElapsedTime(&ms, c->ev[3], c->ev[4]);
    c->stage_ms[LR_T_FIT] = ms;
    if (with_groups) {
        (void)hipEventElapsedTime(&ms, c->ev[5], c->ev[6]);
        c->stage_ms[LR_T_RANSAC] = ms;
        (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[6]);
        c->stage_ms[LR_T_TOTAL] = ms;
    }
    // (lr_stage_fit behind a frame call that ran untimed: the earlier stages' events were never recorded, and the refusal
    // must not stay behind as the thread's last error for the next launch to find)
    (void)hipGetLastError();
}

// The seed sort's capacity follows the frames: kept between 1.25 and 3 times the last frame's seed count (launches of
// the flood and the fit are sized by it, and empty workgroups are not free), grown at once when a frame overflows it
// (that frame is repeated).
void adapt_seed_cap(lr_context* c, uint32_t n_seeds) {
    const size_t npix = (size_t)c->w * c->h;
    if (n_seeds > c->seed_cap)
        c->seed_cap = (uint32_t)std::min<size_t>(npix, std::max<uint32_t>(4096, round_up(n_seeds * 2u, 1024)));
    else if (n_seeds < c->seed_cap / 3 || n_seeds > c->seed_cap / 5 * 4)
        c->seed_cap = (uint32_t)std::min<size_t>(npix, std::max<uint32_t>(4096, round_up(n_seeds + n_seeds / 2, 1024)));
}

}  // namespace

// (the staged API exists for tests and measurements: its stages are always timed)
struct TimingOn {
    lr_context* c;
    bool was;
    explicit TimingOn(lr_context* ctx) : c(ctx), was(ctx->opt.timing_on) { c->opt.timing_on = true; }
    ~TimingOn() { c->opt.timing_on = was; }
};

int ctx_stage_filter(lr_context* c, const float* d_image, int w, int h, int stride) {
    TimingOn t(c);
    if (enqueue_filter(c, d_image, LR_PIX_F32, w, h, stride)) return 1;
    c->stage_valid[0] = true;
    return 0;
}

int ctx_stage_seeds(lr_context* c) {
    if (!c->stage_valid[0]) {
        set_error("lr_stage_seeds: run lr_stage_filter first");
        return 1;
    }
    TimingOn t(c);
    for (int attempt = 0;; ++attempt) {
        if (enqueue_seeds(c)) return 1;
        LR_HIP(hipMemcpyAsync(c->h_counts, c->d_counts, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        LR_HIP(hipStreamSynchronize(c->stream));
        c->n_seeds = c->h_counts[0];
        if (c->n_seeds <= c->seed_cap) break;
        if (attempt > 0) {
            set_error("seed count exceeds the sort capacity twice");
            return 1;
        }
        adapt_seed_cap(c, c->n_seeds);  // more seeds than the sort was sized for: again with room
    }
    c->stage_valid[1] = true;
    return 0;
}

int ctx_stage_flood(lr_context* c) {
    if (!c->stage_valid[1]) {
        set_error(c->dmask_consumed ? "lr_stage_flood: the previous flood consumed the filter output; run lr_stage_filter and lr_stage_seeds again"
                                    : "lr_stage_flood: run lr_stage_seeds first");
        return 1;
    }
    TimingOn t(c);
    if (enqueue_flood(c)) return 1;
    LR_HIP(hipStreamSynchronize(c->stream));
    bool extra;
    if (finish_flood(c, &extra)) return 1;
    c->stage_valid[2] = true;
    return 0;
}

int ctx_stage_fit(lr_context* c, std::vector<LineSegment>& out) {
    if (!c->stage_valid[2]) {
        set_error("lr_stage_fit: run lr_stage_flood first");
        return 1;
    }
    out.clear();
    TimingOn t(c);
    if (enqueue_fit(c)) return 1;
    LR_HIP(hipMemcpyAsync(c->h_counts, c->d_counts, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    LR_HIP(hipStreamSynchronize(c->stream));
    c->n_comp = c->h_counts[kCntComp];
    c->n_px = c->h_counts[kCntPx];
    if (c->n_comp > 0) {
        out.resize(c->n_comp);
        LR_HIP(hipMemcpyAsync(out.data(), c->ws.d_lines, (size_t)c->n_comp * sizeof(LineSegment), hipMemcpyDeviceToHost,
                              c->stream));
        LR_HIP(hipStreamSynchronize(c->stream));
    }
    c->stage_valid[3] = true;
    record_stage_times(c, false);
    return 0;
}

int ctx_detect(lr_context* c, const float* d_image, int w, int h, int stride, std::vector<LineSegment>& raw) {
    if (ctx_stage_filter(c, d_image, w, h, stride)) return 1;
    if (ctx_stage_seeds(c)) return 1;
    if (ctx_stage_flood(c)) return 1;
    return ctx_stage_fit(c, raw);
}

// find_line_segment_groups (interface.cpp:35-80) on a device-resident image.
//
// Default path (RANSAC, refine off): every stage of the frame -- filter, seeds, flood rounds, line fit, filter_lines,
// the four peeling rounds -- is enqueued without a single host round trip, then the counts and the grouped lines come
// back in one copy and the host waits ONCE.  Two things can make a frame take a second lap, both rare and both
// detected from that copy: more seeds than the seed sort was sized for (the frame is repeated with room), and a flood
// that needs more rounds than were enqueued blindly (the rounds are completed, the stages after the flood repeated).
// With refine or PROSAC the raw segments go to the host after the fit, as before.
int run_frame(lr_context* c, const void* d_image, int format, int w, int h, int stride, float min_length, bool refine,
              std::vector<LineSegment>& out, bool filter_enqueued) {
    out.clear();
    const double t_begin = now_ms();
    const bool fused = !refine && c->opt.estimator == 0;
    // The fused path's next launch after the fit is the length test: components that cannot pass it are not fitted at all.
    // (Everything else reads ALL raw segments -- refine merges short ones before the length test -- and fits them all.)
    const int fit_min = fused && c->opt.fit_prune ? fit_min_for(min_length) : kComponentMinSize;
    const int n_iter = c->opt.ransac_iters;
    auto groups_after_fit = [&]() -> int {
        const uint32_t lc = line_cap_for(c);
        if (ensure_group_capacity(c, lc)) return 1;
        if (ensure_result_block(c, std::max<size_t>(c->res_lines_cap, 4096))) return 1;
        if (c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[5], c->stream));
        const PencilTable all = table_of(c, 0), round0 = table_of(c, 1);
        if (launch_filter_lines(c->ws.d_lines, c->d_counts + kCntFitComp, c->d_counts + kCntComp, lc, min_length, c->d_flines, c->d_gctl, c->d_gnorm, &all, &round0,
                                c->stream))
            return 1;
        static_assert(kMaxModels >= 1 && kGcWords == 8 && kResHeaderBytes == 256, "the last peeling round carries the result block (peel_kernel)");
        if (enqueue_groups(c, lc, kMaxModels, kInlierDeg, kGarbageDeg, n_iter, c->opt.ransac_seed, true, true)) return 1;
        if (c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[6], c->stream));
        return 0;
    };
    // what follows the fit: the groups on the device, or (refine, opt-in estimators) the counts for the host
    auto after_fit = [&]() -> int {
        if (fused) return groups_after_fit();
        LR_HIP(hipMemcpyAsync(c->h_counts, c->d_counts, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        return 0;
    };
    c->frame_laps = 0;
    for (int attempt = 0;; ++attempt) {
        c->frame_laps += 1;
        // (a frame that came from a host buffer has had its filter launched band by band as its rows arrived:
        // ctx_find_groups_host; a second lap takes the whole frame from the device slot)
        if (!(filter_enqueued && attempt == 0) && enqueue_filter(c, d_image, format, w, h, stride)) return 1;
        if (enqueue_seeds(c)) return 1;
        if (enqueue_flood(c)) return 1;
        if (enqueue_fit(c, fit_min)) return 1;
        if (after_fit()) return 1;
        const double t_enq = now_ms();
        const double t_pre = now_ms();
        if (c->sleep_in_wait) {  // a batch lane: leave the core to the threads that stage frames
            LR_HIP(hipEventRecord(c->ev_wait, c->stream));
            LR_HIP(hipEventSynchronize(c->ev_wait));
        } else {
            LR_HIP(hipStreamSynchronize(c->stream));
        }
        c->host_ms[0] = t_enq - t_begin;      // enqueue of the frame's kernels
        c->host_ms[1] = t_pre - t_enq;        // staging + upload of the lane's next frame
        c->host_ms[2] = now_ms() - t_pre;     // wait for the GPU
        const uint32_t* cnt = fused ? reinterpret_cast<const uint32_t*>(c->h_res.get()) : c->h_counts.get();
        c->n_seeds = cnt[kCntSeeds];
        if (c->n_seeds <= c->seed_cap) break;
        if (attempt > 0) {
            set_error("seed count exceeds the sort capacity twice");
            return 1;
        }
        adapt_seed_cap(c, c->n_seeds);
    }
    bool extra = false;
    if (finish_flood(c, &extra)) return 1;
    if (extra) {  // the label image changed after the fit ran: the stages after the flood again
        c->frame_laps += 1;
        if (enqueue_fit(c, fit_min)) return 1;
        if (after_fit()) return 1;
        LR_HIP(hipStreamSynchronize(c->stream));
    }
    const uint32_t* cnt = fused ? reinterpret_cast<const uint32_t*>(c->h_res.get()) : c->h_counts.get();
    c->n_comp = cnt[kCntComp];
    c->n_px = cnt[kCntPx];
    adapt_seed_cap(c, c->n_seeds);
    c->stage_valid[0] = c->stage_valid[1] = false;
    c->stage_valid[2] = true;
    // (after a pruned fit d_lines holds a part of the raw segments: whoever wants them all runs lr_stage_fit, which fits every
    // component of the label image that is still there)
    c->stage_valid[3] = fit_min == kComponentMinSize;
    if (fused) {
        const uint32_t* gctl = reinterpret_cast<const uint32_t*>(c->h_res + 32);
        const size_t n = gctl[kGcLines];
        out.resize(n);
        const size_t have = std::min<size_t>(n, c->res_lines_cap);
        if (have) std::memcpy(out.data(), c->h_res + kResHeaderBytes, have * sizeof(LineSegment));
        if (n > have) {  // more lines than the result block holds: fetch the rest, and size the block for the next frame
            LR_HIP(hipMemcpyAsync(out.data() + have, c->d_flines + have, (n - have) * sizeof(LineSegment),
                                  hipMemcpyDeviceToHost, c->stream));
            LR_HIP(hipStreamSynchronize(c->stream));
            if (ensure_result_block(c, round_up((uint32_t)(n + n / 2), 1024))) return 1;
        }
        record_stage_times(c, true);
#ifdef LR_PEEL_TIMING
        {
            const float* tm = reinterpret_cast<const float*>(c->h_res + 64) + 16;
            for (int r = 0; r < 4; ++r)
                std::fprintf(stderr, "peel round %d: best %.1f us, inliers %.1f, sums %.1f, jacobi %.1f, verdict %.1f\n", r,
                             tm[r * 5], tm[r * 5 + 1], tm[r * 5 + 2], tm[r * 5 + 3], tm[r * 5 + 4]);
        }
#endif
        return 0;
    }
    // ---- refine and / or PROSAC: raw segments to the host
    std::vector<LineSegment> raw(c->n_comp);
    if (c->n_comp) {
        LR_HIP(hipMemcpyAsync(raw.data(), c->ws.d_lines, (size_t)c->n_comp * sizeof(LineSegment), hipMemcpyDeviceToHost,
                              c->stream));
        LR_HIP(hipStreamSynchronize(c->stream));
    }
    record_stage_times(c, false);
    if (raw.size() < 2) return 0;  // interface.cpp:50-54
    if (refine && ctx_refine(c, raw)) return 1;
    std::vector<LineSegment> filtered = filter_lines(raw, min_length);
    if (filtered.empty()) return 0;
    if (c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[5], c->stream));
    if (c->opt.estimator == 1) {
        if (ctx_estimate_line_pencils_prosac(c, filtered, kMaxModels, kInlierDeg, kGarbageDeg, c->opt.prosac_T_N,
                                             c->opt.ransac_seed))
            return 1;
    } else if (c->opt.estimator == 2) {
        if (ctx_estimate_line_pencils_direct(c, filtered, kMaxModels, kInlierDeg, kGarbageDeg)) return 1;
    } else if (c->opt.estimator == 3) {
        if (ctx_estimate_line_pencils_cht(c, filtered, kMaxModels, kInlierDeg, kGarbageDeg, c->opt.cht_d, nullptr)) return 1;
    } else if (ctx_estimate_line_pencils(c, filtered, kMaxModels, kInlierDeg, kGarbageDeg, n_iter, c->opt.ransac_seed)) {
        return 1;
    }
    if (c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[6], c->stream));
    LR_HIP(hipStreamSynchronize(c->stream));
    record_stage_times(c, true);
    out.swap(filtered);
    return 0;
}

int ctx_find_groups_device(lr_context* c, const void* d_image, int format, int w, int h, int stride, float min_length, bool refine,
                           std::vector<LineSegment>& out) {
    return run_frame(c, d_image, format, w, h, stride, min_length, refine, out);
}

// find_line_segment_groups on a HOST buffer (the reference's only kind of input: interface.cpp:43-48, image.cpp:11-19),
// one frame.  The upload, the filter and the host's enqueueing of the rest of the frame overlap:
//  - the frame goes up in 4 MB row bands (pageable memory through the page-locked staging buffer, filled by the
//    context's staging threads; page-locked memory straight from where it lies), an event after every band;
//  - the filter is launched band by band: a band row of the filter reads the image rows 30 by - 4 .. 30 by + 33, so the
//    band rows whose last image row lies in upload band k are launched as soon as that band's transfer is enqueued,
//    behind a wait for its event -- when the last transfer ends, all but the last ninth of the filter has run;
//  - the calling thread only drives (waits for "band k enqueued", launches its filter rows) and then enqueues the rest
//    of the frame while the last transfers are still on the link.
// What cannot overlap: everything after the filter needs the frame's largest magnitude, i.e. the whole frame.
// Frames of any lr_pixel_format travel as bytes (bpp a pixel; upload bands of 4 MB are four times as many rows of an 8-bit
// frame).  An interleaved frame goes up whole before its luma launch: the filter does not follow its bands.
int ctx_find_groups_host(lr_context* c, const void* buffer_, int format, int w, int h, int stride, float min_length, bool refine,
                         int num_threads, std::vector<LineSegment>& out) {
    const uint8_t* buffer = static_cast<const uint8_t*>(buffer_);
    const int bpp = pix_bytes(format);
    if (bpp == 0) {
        set_error("unknown pixel format of the frames");
        return 1;
    }
    const double t_call = now_ms();
    LR_HIP(hipSetDevice(c->device));
    if (w < 5 || h < 5 || buffer == nullptr) {
        set_error("image smaller than the 5x5 filter");
        return 1;
    }
    if ((stride < 0 ? -stride : stride) < w) {
        set_error("upload: |stride| smaller than the width");
        return 1;
    }
    if (ensure_copy_stream(c)) return 1;
    hipStream_t up = c->copy_stream;
    const size_t npix = (size_t)w * h;
    const int slot = 0;
    uint8_t* stage = nullptr;
    {
        float* stage_f = nullptr;  // (slots and staging buffers are sized in floats: a frame of bytes fits)
        if (ensure_frame_slot(c, slot, npix, !is_page_locked(buffer), &stage_f)) return 1;
        stage = reinterpret_cast<uint8_t*>(stage_f);
    }
    if (prepare_frame(c, w, h)) return 1;
    // Whatever way this call ends, nothing of it may still be on the link or the GPU when it returns with an error: the
    // next call would fill the staging buffer under a transfer that still reads it (ev_up is only recorded on success).
    struct DrainOnError {
        lr_context* c;
        hipStream_t up;
        bool ok = false;
        ~DrainOnError() {
            if (ok) return;
            (void)hipStreamSynchronize(up);
            (void)hipStreamSynchronize(c->stream);
            (void)hipGetLastError();
        }
    } drain{c, up};
    const uint8_t* src = buffer;
    int sstride = stride;
    if (sstride < 0) {  // image.cpp:14-18: the same rows, addressed from the other end (no flip)
        src = buffer + (std::ptrdiff_t)(h - 1) * sstride * bpp;
        sstride = -sstride;
    }
    const size_t row_bytes = (size_t)w * bpp, pitch = (size_t)sstride * bpp;
    const bool follow = format != LR_PIX_U8X3;  // the filter reads the slot itself, band by band
    // Upload bands of 4 MB, the filter behind every band.  Smaller bands would start the link earlier (with eight staging
    // threads the first 4 MB bands are all ready at the same moment, 0.4 ms in), but every band costs about 18 us of its
    // own -- transfer submission, event, cross-stream wait -- on the stream that carries the frame: measured on 4K frames
    // 3.01 ms per call with 4 MB bands, 3.49 with 1 MB, 4.07 with 512 KB (profiles/r03_single_call_sweep.txt).
    static const size_t band_bytes = std::getenv("LIBRECTIFY_UPLOAD_BAND_KB") ? (size_t)std::max(64, std::atoi(std::getenv("LIBRECTIFY_UPLOAD_BAND_KB"))) << 10 : (size_t)4 << 20;
    // (a page-locked source goes up in ONE transfer unless the knob says otherwise: eight bands of 4 MB with an event each cost
    // the call more than the filter gains by starting under the transfer -- 2.07 -> 1.94 ms per 4K frame, round 5)
    static const bool band_env = std::getenv("LIBRECTIFY_UPLOAD_BAND_KB") != nullptr;
    int rpb = (int)std::max<size_t>(1, ((stage == nullptr && !band_env) ? (size_t)h * row_bytes : band_bytes) / row_bytes);
    if ((h + rpb - 1) / rpb > StagingCrew::kMaxBands) rpb = (h + StagingCrew::kMaxBands - 1) / StagingCrew::kMaxBands;  // (as StagingCrew::begin)
    const int n_bands = (h + rpb - 1) / rpb;
    while ((int)c->band_ev.size() < n_bands) {
        Event e;
        if (e.ensure(hipEventDisableTiming)) return 1;
        c->band_ev.push_back(std::move(e));
    }
    uint8_t* dst = reinterpret_cast<uint8_t*>(c->frames.slot[slot].get());
    const int fb = filter_band_rows(), band_rows = (h + fb - 1) / fb;
    int by_next = 0;
    // filter rows that upload band k completes, behind that band's event
    auto filter_after_band = [&](int k) -> int {
        // the compute stream waits for EVERY band's own event: the bands are enqueued by several threads in no particular
        // order, so a later band's event says nothing about an earlier band
        LR_HIP(hipStreamWaitEvent(c->stream, c->band_ev[(size_t)k], 0));
        if (!follow) return 0;
        const int last_row = std::min(h, (k + 1) * rpb) - 1;  // last image row on the device once bands 0..k are
        int by_end = by_next;
        while (by_end < band_rows && std::min(h - 1, filter_band_last_row(by_end)) <= last_row) ++by_end;
        if (k == n_bands - 1) by_end = band_rows;
        if (launch_filter_rows(dst, format, w, h, w, c->fconsts, c->ws.dx, c->ws.dy, c->ws.dmask, c->ws.cand, c->ws.cand_count, c->ws.tile_max, by_next,
                               by_end, c->stream))
            return 1;
        by_next = by_end;
        return 0;
    };
    if (follow && c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[0], c->stream));
    const int T = stage ? staging_threads(num_threads, npix * bpp) : 1;  // (the threads share every band: StagingCrew::work)
    if (T <= 1) {
        // the calling thread alone (the reference's serial mode, or a page-locked source that needs no staging)
        for (int k = 0; k < n_bands; ++k) {
            const int r0 = k * rpb, r1 = std::min(h, r0 + rpb);
            if (stage) {
                if (sstride == w) std::memcpy(stage + (size_t)r0 * row_bytes, src + (size_t)r0 * pitch, (size_t)(r1 - r0) * row_bytes);
                else
                    for (int r = r0; r < r1; ++r) std::memcpy(stage + (size_t)r * row_bytes, src + (size_t)r * pitch, row_bytes);
                LR_HIP(hipMemcpyAsync(dst + (size_t)r0 * row_bytes, stage + (size_t)r0 * row_bytes, (size_t)(r1 - r0) * row_bytes,
                                      hipMemcpyHostToDevice, up));
            } else if (sstride == w) {
                LR_HIP(hipMemcpyAsync(dst + (size_t)r0 * row_bytes, src + (size_t)r0 * row_bytes, (size_t)(r1 - r0) * row_bytes,
                                      hipMemcpyHostToDevice, up));
            } else {
                LR_HIP(hipMemcpy2DAsync(dst + (size_t)r0 * row_bytes, row_bytes, src + (size_t)r0 * pitch, pitch,
                                        row_bytes, (size_t)(r1 - r0), hipMemcpyHostToDevice, up));
            }
            LR_HIP(hipEventRecord(c->band_ev[(size_t)k], up));
            if (filter_after_band(k)) return 1;
        }
    } else {
        // the context's staging threads fill and send the bands; this thread follows them with the filter
        if (!c->crew || c->crew_helpers != T) {
            c->crew.reset();  // (the old helpers end first)
            c->crew.reset(new StagingCrew());
            c->crew->start(c, T);
            c->crew_helpers = T;
        }
        StagingCrew* cr = c->crew.get();
        std::vector<std::atomic<int>> ready((size_t)n_bands);
        for (auto& a : ready) a.store(0, std::memory_order_relaxed);
        const uint32_t g = cr->begin(dst, stage, src, w, h, sstride, bpp, up, c->band_ev.data(), ready.data(), band_bytes);
        int rc = 0;
        for (int k = 0; k < n_bands && rc == 0; ++k) {
            int spins = 0, r;
            while ((r = ready[(size_t)k].load(std::memory_order_acquire)) == 0) {
                // No helper alive (none got a device), or the helpers are starved of cores: this thread stages pieces itself
                // instead of waiting for ever for somebody else to.
                if ((cr->live.load(std::memory_order_acquire) == 0 || spins > 4096) && cr->work_one(g)) continue;
                if (++spins < 2048) std::this_thread::yield();
                else std::this_thread::sleep_for(std::chrono::microseconds(5));
            }
            if (r < 0 || filter_after_band(k)) rc = 1;
        }
        if (rc) cr->work(g);  // (the bands still unclaimed must be accounted for before finish() can return)
        if (cr->finish() || rc) {  // (every band accounted for before `ready` goes out of scope)
            if (get_error().empty()) set_error("upload: staging copy failed");
            return 1;
        }
    }
    if (follow && c->opt.timing_on) LR_HIP(hipEventRecord(c->ev[1], c->stream));
    LR_HIP(hipEventRecord(c->ev_up[slot], up));
    static const bool call_debug = std::getenv("LIBRECTIFY_CALL_DEBUG") != nullptr;
    const double t_up = now_ms();
    const int rc = run_frame(c, dst, format, w, h, w, min_length, refine, out, follow);
    drain.ok = rc == 0;
    if (call_debug)
        std::fprintf(stderr, "host frame: bands staged, sent and filter launched in %.3f ms; rest of the frame enqueued in %.3f ms; waited %.3f ms; "
                     "results out in %.3f ms; whole call %.3f ms\n", t_up - t_call, c->host_ms[0], c->host_ms[2],
                     now_ms() - t_up - c->host_ms[0] - c->host_ms[2], now_ms() - t_call);
    return rc;
}

}  // namespace lramd
