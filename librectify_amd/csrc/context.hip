// The context's memory: creation and destruction, the workspace that follows the frames' size (grow, trim), the flood's
// buffers and slabs, the line tables of the estimators.  The buffers own themselves (buffers.h): nothing here lists them.
#include "host.h"

#include <cmath>
#include <cstdlib>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

lr_context::lr_context() = default;
lr_context::~lr_context() = default;

namespace lramd {

namespace {

thread_local std::string g_error;

// 1-D factors of the reference's taps (filter.cpp:65-78: H = z / a * exp(-(x^2 + y^2) / 2s^2), a = 2 pi s^4):
// d(t) = t / a * exp(-t^2 / 2s^2), g(t) = exp(-t^2 / 2s^2), evaluated with the same float operations
void gauss_deriv_factors(int size, float sigma, float* d, float* g) {
    const int n = 2 * size + 1;
    for (int t = 0; t < n; ++t) {
        const float x = float(t - size);
        const float a = float(2 * M_PI * std::pow(sigma, 4.0f));
        const float e = std::exp(-std::pow(x, 2.0f) / (2 * std::pow(sigma, 2.0f)));
        d[t] = x / a * e;
        g[t] = e;
    }
}

void init_constants(lr_context* c) {
    gauss_deriv_factors(kEdgeKernelSize, kEdgeKernelSigma, c->fconsts.d, c->fconsts.g);
    for (int b = 0; b < kBins; ++b) {
        const float theta = float(b * M_PI) / kBins;  // line_detector.cpp:144
        c->trig.st[b] = std::sin(theta);
        c->trig.ct[b] = std::cos(theta);
        c->fconsts.st[b] = c->trig.st[b];
        c->fconsts.ct[b] = c->trig.ct[b];
    }
    c->seed_keep_ratio = 1 - std::max(std::min(kSeedRatio, 1.f), 0.f);  // line_detector.cpp:209
}

}  // namespace

void set_error(const std::string& msg) { g_error = msg; }
const std::string& get_error() { return g_error; }

// Gives the device and page-locked memory that is sized by the largest frame the context has seen back to the system: the
// per-pixel workspace (about 130 bytes a pixel), the flood's per-seed buffers, slabs and hand-over records, the frame slots
// and their staging buffers, the batch ring.  Streams, events and small tables stay; the next frame allocates what it needs.
int ctx_trim(lr_context* c, bool frames_too) {
    LR_HIP(hipSetDevice(c->device));
    LR_HIP(hipStreamSynchronize(c->stream));
    if (c->copy_stream) LR_HIP(hipStreamSynchronize(c->copy_stream));
    c->ws = Workspace{};
    c->flood = FloodStore{};
    // (the frame slots hold the frame that is being processed when the workspace shrinks by itself: only on request)
    if (frames_too) {
        c->frames = FrameSlots{};
        c->ring.drop();
        c->prep = PrepareSpans{};  // (sized by a frame's width + height)
        c->warp_m = MirroredBuffer<double>{};  // (sized by the largest batch warped)
        c->overlay = OverlayStore{};           // (sized by the most segments drawn in a call)
        c->jpeg = JpegStore{};                 // (coefficients and interval tables of the largest batch encoded)
        c->jpeg_decode = JpegDecodeStore{};    // (coefficients and part records of the largest batch decoded)
        c->tensor = TensorStore{};             // (frame records of the largest batch packed, and the elements' table)
    }
    c->small_frames = 0;
    c->w = c->h = 0;
    c->seed_cap = 0;
    c->flood_hold_hint = c->flood_staged_hint = c->flood_calm_hint = false;  // (what the frames before taught the context goes with the workspace)
    c->flood_staged_streak = 0;
    for (bool& v : c->stage_valid) v = false;
    // (the lanes of a batch call are contexts of their own that shrink by themselves; a lane that shrinks in the middle of a
    // call must not touch the others, which are in the middle of their frames -- only a trim on request goes through them)
    if (frames_too)
        for (lr_context* wc : c->workers)
            if (ctx_trim(wc, true)) return 1;
    return 0;
}

int ctx_ensure_image_capacity(lr_context* c, int w, int h) {
    const size_t npix = (size_t)w * h;
    // What a context hands from frame to frame describes the previous frame of the SAME stream: a frame of another size is the
    // start of another one (bench.py's content-latency frames: the 1080p soft blobs inherited "staged" from the 4K ones and
    // kept it -- 17 ms a frame instead of 13.7).
    if (c->w != 0 && (c->w != w || c->h != h)) {
        c->flood_hold_hint = false;
        c->flood_staged_hint = false;
        c->flood_calm_hint = false;
        c->flood_staged_streak = 0;
    }
    const FilterGeom fg = filter_geometry(w, h);
    const int ntiles = fg.n_tiles;
    // A context that has seen one large frame keeps serving small ones out of the large workspace (an 8192 x 8192 call leaves
    // 8.9 GB behind): after eight frames in a row of at most a quarter of the capacity it is given back, and this frame
    // allocates its own size (lr_context_trim does the same at once).
    // (keep_workspace: a batch call with a frame table has sized its lanes for the call and the count rests until it is over)
    if (!c->keep_workspace) {
        if (c->ws.cap_pix != 0 && npix * 4 <= c->ws.cap_pix) {
            if (++c->small_frames >= 8 && ctx_trim(c, false)) return 1;
        } else {
            c->small_frames = 0;
        }
    }
    return ctx_reserve_workspace(c, npix, ntiles);
}

// Grows the per-pixel workspace to npix pixels and ntiles candidate lists (which need not be one frame's); never shrinks it.
int ctx_reserve_workspace(lr_context* c, size_t npix, int ntiles) {
    const FilterGeom fg = filter_geometry(5, 5);  // (cand_cap: the same for every size)
    if (npix <= c->ws.cap_pix && ntiles <= c->ws.cap_tiles) return 0;
    LR_HIP(hipStreamSynchronize(c->stream));
    const size_t cp = std::max(npix, c->ws.cap_pix);
    const int ct = std::max(ntiles, c->ws.cap_tiles);
    // (seed_select_kernel keeps one 64-bit status word a workgroup in tile_off: 2 words for a one-tile frame)
    const size_t tile_off_words = std::max(ct, 2);
    Workspace& s = c->ws;
    s.cap_pix = 0;  // (until every buffer below is there: a growth that fails half-way leaves no capacity behind)
    s.cap_tiles = 0;
    if (s.dx.grow(cp) || s.dy.grow(cp) || s.dmask.grow(cp + 16) || s.cand.grow((size_t)ct * fg.cand_cap) || s.cand_count.grow(ct) ||
        s.tile_max.grow(ct) || s.tile_pass.grow(ct) || s.tile_off.grow(tile_off_words) || s.keys_a.grow(cp) || s.keys_b.grow(cp) ||
        s.seed_idx.grow(cp) || s.seed_bin.grow(cp) || s.seed_thr.grow(cp) || s.seed_rec.grow(cp) || s.seed_size.grow(cp) || s.label.grow(cp) ||
        s.queue.grow(cp) || s.comp_rank.grow(cp) || s.comp_seed.grow(cp) || s.comp_off.grow(cp + 1) || s.cursor.grow(cp) ||
        s.px_a.grow(cp) || s.px_b.grow(cp) || s.scratch_w.grow(cp) || s.d_lines.grow(cp / 6 + 16) || s.comp_large.grow(cp / 64 + 16))
        return 1;
    LR_HIP(hipMemsetAsync(s.tile_off, 0, tile_off_words * sizeof(uint32_t), c->stream));  // (seed_select_kernel's status words)
    {   // huge components: a row of buckets (2^14 pixel indices each) for up to 256 of them; the table is zero between frames
        const size_t nb = (cp + 16383) >> 14;
        const uint32_t max = 256;
        if (s.huge_tab.grow(max * nb) || s.huge_jobs.grow(4 * max * nb) || s.huge_list.grow(max)) return 1;
        s.huge = HugeSort{s.huge_tab, s.huge_list, s.huge_jobs, max};
        LR_HIP(hipMemsetAsync(s.huge.tab, 0, max * nb * sizeof(uint32_t), c->stream));
    }
    const size_t tb = std::max(seeds_temp_bytes(ct, cp), fit_temp_bytes(cp, (uint32_t)std::min<size_t>(cp / 6 + 16, 0xFFFFFFFFu)));
    if (s.temp.grow(tb)) return 1;
    LR_HIP(hipMemsetAsync(s.temp, 0, tb, c->stream));  // (component_offsets_kernel's status words)
    s.cap_pix = cp;
    s.cap_tiles = ct;
    return 0;
}

// The overflow slabs (2.25 MB each).  With the giant step the default mode needs them for nothing but the walks of the
// lowest active seed when the step is switched off: 16 of them (36 MB; the default pool was 128 = 288 MB).  The storage
// test hooks (modes 2-7: no second tier, every long walk in a slab) and LIBRECTIFY_FLOOD_GIANT_STEP=0 get the full pool.
// a flood buffer and the pointer the kernels get to it
template <class T, class P>
static int grow_into(DeviceBuffer<T>& own, P*& raw, size_t count) {
    raw = nullptr;
    if (own.grow(count)) return 1;
    raw = own.get();
    return 0;
}

static int ensure_flood_slabs(lr_context* c) {
    FloodBuffers& f = c->flood.fb;
    static const bool giant_step_off = std::getenv("LIBRECTIFY_FLOOD_GIANT_STEP") && std::atoi(std::getenv("LIBRECTIFY_FLOOD_GIANT_STEP")) == 0;
    uint32_t want = (c->opt.flood_mode == 1 && c->opt.flood_giant_step && !giant_step_off) ? 16u : 128u;
    if (const char* e = std::getenv("LIBRECTIFY_FLOOD_SLABS")) want = (uint32_t)std::max(1, std::atoi(e));
    if (f.slab_ring && f.n_slabs >= want) return 0;
    LR_HIP(hipStreamSynchronize(c->stream));
    f.n_slabs = want;
    f.slab_ring_cap = 1u << 14;  // (tile, entry mask) records, 16 B each
    f.slab_hash_cap = 1u << 16;  // tile -> (walked, acceptable) records, 32 B each (48 Ki tiles = 3 M pixels)
    if (grow_into(c->flood.slab_ring, f.slab_ring, (size_t)f.n_slabs * f.slab_ring_cap) ||
        grow_into(c->flood.slab_hash, f.slab_hash, (size_t)f.n_slabs * f.slab_hash_cap * 2))
        return 1;
    LR_HIP(hipMemsetAsync(f.slab_hash, 0, (size_t)f.n_slabs * f.slab_hash_cap * 32, c->stream));
    if (f.ctrl) LR_HIP(hipMemsetAsync(f.ctrl, 0, kFloodCtrlWords * sizeof(uint32_t), c->stream));  // (the generation counter starts again with the cleared tables)
    return 0;
}

int ensure_flood_buffers(lr_context* c) {
    FloodStore& o = c->flood;
    FloodBuffers& f = o.fb;
    if (c->flood.cap_seeds >= c->ws.cap_pix && f.ctrl) return ensure_flood_slabs(c);
    LR_HIP(hipStreamSynchronize(c->stream));
    const size_t cs = c->ws.cap_pix;
    if (grow_into(o.blocked, f.blocked, cs) || grow_into(o.count, f.count, cs) || grow_into(o.flags, f.flags, cs) ||
        grow_into(o.state, f.state, cs) || grow_into(o.tier, f.tier, cs + 4) /* (read a word at a time) */ || grow_into(o.blk, f.blk, cs) ||
        grow_into(o.act_a, f.act_a, cs) || grow_into(o.act_b, f.act_b, cs) || grow_into(o.ctrl, f.ctrl, kFloodCtrlWords) ||
        grow_into(o.big_list, f.big_list, 8192) || grow_into(o.handover, f.handover, 8192 * kFloodHandWords) ||
        grow_into(o.dirty, f.dirty, cs / 256 + 16) ||
        // the giant step's tile masks: (w + 7) / 8 x (h + 7) / 8 tiles <= cs / 16 + 64 for frames of 5 x 5 and more
        grow_into(o.giant_mask, f.giant_mask, cs / 16 + 64))
        return 1;
    // footprint logs (FloodBuffers::rewalk_logs): per-seed words for one seed per 16 pixels (the 4K bench frame has one per
    // 200), a record per 8 pixels
    constexpr size_t kLogCapDiv = 8;
    f.log_seeds = (uint32_t)std::min<size_t>(std::max<size_t>(cs / 16, 4096), cs);
    f.log_cap = (uint32_t)std::min<size_t>(std::max<size_t>(cs / kLogCapDiv, 65536), 1u << 28);
    if (grow_into(o.rewalk_list, f.rewalk_list, 8192) || grow_into(o.log_off, f.log_off, f.log_seeds) ||
        grow_into(o.log_len, f.log_len, f.log_seeds) || grow_into(o.log_buf, f.log_buf, (size_t)f.log_cap * 3))
        return 1;
    LR_HIP(hipMemsetAsync(f.ctrl, 0, kFloodCtrlWords * sizeof(uint32_t), c->stream));
    o.cap_seeds = cs;
    return ensure_flood_slabs(c);
}


int ctx_ensure_ransac_capacity(lr_context* c, size_t n_lines) {
    if (8 * n_lines <= c->model.cap()) return 0;
    LR_HIP(hipStreamSynchronize(c->stream));
    return c->model.grow(8 * std::max<size_t>(n_lines, 4096));
}

int ensure_group_capacity(lr_context* c, size_t n_lines) {
    if (n_lines > c->cap_glines) {
        LR_HIP(hipStreamSynchronize(c->stream));
        const size_t cl = std::max<size_t>(n_lines, 4096);
        c->cap_glines = 0;
        if (c->d_tables.grow(3 * 8 * cl) || c->d_orig.grow(3 * cl) || c->d_inl.grow(4 * cl)) return 1;
        c->cap_glines = cl;
    }
    if (n_lines > c->d_flines.cap()) {
        LR_HIP(hipStreamSynchronize(c->stream));
        if (c->d_flines.grow(n_lines + 16)) return 1;
    }
    return 0;
}

int ctx_create(int device, lr_context** out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available: librectify_amd has no CPU fallback");
        return 1;
    }
    if (device < 0 || device >= ndev) {
        set_error("device index out of range");
        return 1;
    }
    LR_HIP(hipSetDevice(device));
    lr_context* c = new lr_context();
    c->device = device;
    if (hipStreamCreateWithFlags(c->stream.put(), hipStreamNonBlocking) != hipSuccess) {
        delete c;
        set_error("hipStreamCreate failed");
        return 1;
    }
    // Every allocation is checked: a create that ran out of memory must fail here, cleanly, and not hand out a context
    // whose first kernel faults on a null buffer (six lanes and their pools hold several GB -- exactly when it can happen).
    // LIBRECTIFY_TEST_CREATE_FAIL=n (test hook) makes the n-th allocation of a create report hipErrorOutOfMemory.
    {
        static const int fail_at = std::getenv("LIBRECTIFY_TEST_CREATE_FAIL") ? std::atoi(std::getenv("LIBRECTIFY_TEST_CREATE_FAIL")) : 0;
        int n_alloc = 0;
        hipError_t bad = hipSuccess;
        const char* what = "";
        auto check = [&](hipError_t e, const char* name) {
            if (++n_alloc == fail_at) e = hipErrorOutOfMemory;
            if (e != hipSuccess && bad == hipSuccess) {
                bad = e;
                what = name;
            }
        };
        for (auto& e : c->ev) check(e.create(), "hipEventCreate");
        check(c->ev_wait.create(hipEventBlockingSync | hipEventDisableTiming), "hipEventCreate");
        static const bool lane_debug = std::getenv("LIBRECTIFY_LANE_DEBUG") != nullptr;  // (its timeline times the uploads)
        for (auto& e : c->ev_up) check(e.create(lane_debug ? hipEventDefault : hipEventDisableTiming), "hipEventCreate");
        check(c->maxmag.alloc(1), "hipMalloc(maxmag)");
        check(c->d_counts.alloc(64), "hipMalloc(counts)");
        check(c->d_gctl.alloc(kGcWords), "hipMalloc(peeling control block)");
        check(c->d_gnorm.alloc(4), "hipMalloc(normalisation)");
        check(c->d_models.alloc(64), "hipMalloc(models)");
        check(c->d_best_slots.alloc(kRansacBestSlots), "hipMalloc(best slots)");
        check(c->h_counts.alloc(128), "hipHostMalloc(counts)");
        check(c->h_best.alloc(2), "hipHostMalloc(best)");
        if (bad == hipSuccess) check(hipMemset(c->d_models, 0, 64 * sizeof(float)), "hipMemset(models)");
        if (bad == hipSuccess) check(hipMemset(c->d_counts, 0, 64 * sizeof(uint32_t)), "hipMemset(counts)");
        if (bad == hipSuccess) check(hipMemset(c->d_best_slots, 0, kRansacBestSlots * sizeof(unsigned long long)), "hipMemset(best slots)");
        if (bad != hipSuccess) {
            (void)hipGetLastError();
            const std::string msg = std::string("lr_context_create: ") + what + " failed: " + hipGetErrorString(bad);
            ctx_destroy(c);  // (frees whatever was made)
            set_error(msg);
            return 1;
        }
    }
    init_constants(c);
    const char* env = std::getenv("LIBRECTIFY_SEED");
    c->opt.ransac_seed = env ? std::strtoull(env, nullptr, 0) : 0ull;
    c->opt.timing_on = std::getenv("LIBRECTIFY_STAGE_TIMES") != nullptr;
    if (const char* e = std::getenv("LIBRECTIFY_FLOOD_LOGS")) c->opt.flood_logs = std::atoi(e) != 0;
    *out = c;
    return 0;
}

void ctx_destroy(lr_context* c) {
    if (!c) return;
    for (lr_context* wc : c->workers) ctx_destroy(wc);
    for (lr_context* pc : c->peers) ctx_destroy(pc);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    c->crew.reset();  // (its threads end before the buffers they copy into go)
    delete c;
}

}  // namespace lramd
