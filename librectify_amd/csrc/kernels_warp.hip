// Rectified images: the perspective warp of lr_warp_perspective_device for gfx950, bilinear or (LR_WARP_CUBIC) bicubic.
//
// A gather: every destination pixel maps back into its source frame through the frame's 3x3 matrix M and reads four
// source pixels.  The source is read through L2, so what matters is that the pixels a workgroup reads lie close
// together, and that workgroups reading neighbouring source rows share an L2:
//
//   * a workgroup takes one 64 x 16 tile of the destination (a wavefront 64 x 4: 16 lanes across, 4 pixels a lane,
//     4 rows), so its source footprint is a compact patch rather than a long row;
//   * the tiles of all frames, in row-major order frame by frame, are cut into eight contiguous runs, one per XCD
//     (workgroups are dealt to the XCDs round-robin: the XCD band order of kernels_filter.hip), so each XCD's L2 holds
//     one band of destination rows and the source rows they read;
//   * a lane's four pixels are consecutive, so its u8 results go out as one dword (u8x3: three, f32: one dwordx4)
//     wherever the destination address allows; the two horizontal taps of a source row are one u16 (u8) or dwordx2 (f32)
//     load where they are both inside and aligned.
//
// The arithmetic is the canonical one of DESIGN.md section 3 (mirrored by tests/numpy_warp_ref.py): coordinates in
// double without contraction (-ffp-contract=off), 5 fractional bits per axis, integer taps and weights.
//
// LR_WARP_CUBIC is a second sampling rule, not a second kernel: warp_lane takes the rule as a template parameter and samples a
// pixel from 4 x 4 taps (cubic_pixel) instead of 2 x 2; tiles, records, the XCD bands and the stores are the same.  The four
// taps of a source row are consecutive bytes and come in with one load (row_taps), straight through L1 / L2 like the
// bilinear taps.
//
// LR_WARP_BORDER is a third template parameter of warp_lane: what a tap outside the source contributes is the frame's border
// rule (a constant, or the pixel that replicate, reflect or reflect-101 names) instead of 0.  Pixels and rows of taps that lie
// inside keep the loads above; only the others map their indices.  Its launches all go through warp_ragged_border_kernel, which
// is kernels_warp_border.hip's; the lane body is in warp_lane.h for the two files.
//
// LR_WARP_LENS is a fourth: between the perspective divide and the rounding to 5-bit coordinates the point goes through the
// frame's lens model (OpenCV's five coefficients; fixed_xy and lens_displace of warp_lane.h).  Its launches all go through
// warp_ragged_lens_kernel, which is kernels_warp_lens.hip's, with a second array of records, one LensRecord per frame.
// LR_WARP_LENS_MODEL widens the lens to seventeen entries (OpenCV's rational and thin-prism model, or cv::fisheye's); only a
// call with a frame that needs them (LensSet below) launches kernels_warp_lens_model.hip's kernels, with a LensModelRecord per
// frame; lenses that all fit the nine entries become LensRecords and take the kernels above.
//
// LR_WARP_AREA is no parameter of warp_lane but a loop around its per-pixel rules: S x S sub-samples per destination pixel under
// the frame's fine map, averaged.  Its launches all go through warp_ragged_area_kernel, which is
// kernels_warp_area.hip's, with a third array of records, one AreaRecord per frame; the fine maps are made here, on the host.
//
// One lane body, two kernels.  warp_lane is a lane's work inside a tile: its four pixels' taps, blends and stores.  The two
// kernels differ only in how a workgroup finds its frame and the frame's values, all of which depend on the tile index
// alone and are uniform across the workgroup:
//
//   * warp_perspective_kernel (one size for all frames): the frame is tile / tiles per frame, and sizes, strides and
//     pointers are kernel arguments.
//   * warp_ragged_kernel (LR_WARP_PACKED and LR_WARP_RAGGED): the tile list is ragged -- frame b adds ceil(ow_b / 64) *
//     ceil(oh_b / 16) tiles -- and is cut into the same eight runs.  A workgroup finds its frame by a binary search of the
//     tiles' prefix table (tiles.h) and reads the frame's record: its map, its output's size, place and stride, and its
//     source's size, place and stride.  LR_WARP_PACKED, whose frames share one source size and stride, is the same launch
//     with records that say so.
//
// LR_WARP_JPEG is no warp: lr_encode_jpeg_device's call goes on to kernels_jpeg.hip.
// LR_WARP_JPEG_DECODE neither: lr_decode_jpeg_device's call goes on to kernels_jpeg_decode.hip.
// LR_WARP_LINES is none either: the entry hands lr_draw_lines_device's call on to kernels_overlay.hip (the export table is full).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "warp_lane.h"

namespace lramd {
namespace {

template <int kFormat, bool kCubic>
__global__ __launch_bounds__(kBlock) void warp_perspective_kernel(WarpArgs g) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const unsigned lx = (unsigned)lane & 15u, row_in_tile = (unsigned)(wave * 4 + (lane >> 4));
    XcdBand band(g.n_tiles);
    for (int tile; band.next(&tile);) {
        const int b = tile / g.tiles_per_frame;
        const int r = tile - b * g.tiles_per_frame;
        const int ty = r / g.tiles_x, tx = r - ty * g.tiles_x;
        const unsigned y = (unsigned)ty * kTileH + row_in_tile;
        const unsigned x0 = (unsigned)tx * kTileW + lx * 4u;
        if (y >= (unsigned)g.oh || x0 >= (unsigned)g.ow) continue;
        const uint8_t* src = g.src + (size_t)b * g.src_image_bytes;
        uint8_t* out = g.dst + (size_t)b * g.dst_image_bytes + (size_t)y * g.dst_row_bytes;
        warp_lane<kFormat, kCubic, false>(g.M + (size_t)b * 9, src, g.src_row_bytes, g.w, g.h, out, g.ow, x0, y);
    }
}

// The same tiles over a ragged list.  frames and start (batch + 1 entries: frame b owns the tiles [start[b], start[b + 1]))
// are arguments of their own, restrict-qualified: the stores to dst cannot change them, so their uniform reads stay scalar
// loads.
template <int kFormat, bool kCubic>
__global__ __launch_bounds__(kBlock) void warp_ragged_kernel(RaggedArgs g, const RaggedFrame* __restrict__ frames,
                                                             const int* __restrict__ start, uint8_t* __restrict__ dst) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const unsigned lx = (unsigned)lane & 15u, row_in_tile = (unsigned)(wave * 4 + (lane >> 4));
    XcdBand band(g.n_tiles);
    for (int tile; band.next(&tile);) {
        const int b = frame_of_tile(start, g.batch, tile);
        const RaggedFrame* f = frames + b;
        const int ow = f->ow, oh = f->oh, tiles_x = f->tiles_x;
        const int r = tile - start[b];
        const int ty = r / tiles_x, tx = r - ty * tiles_x;
        const unsigned y = (unsigned)ty * kTileH + row_in_tile;
        const unsigned x0 = (unsigned)tx * kTileW + lx * 4u;
        if (y >= (unsigned)oh || x0 >= (unsigned)ow) continue;
        const uint8_t* src = g.src + (size_t)f->src_offset;
        uint8_t* out = dst + (size_t)f->offset + (size_t)y * (size_t)f->row_bytes;
        warp_lane<kFormat, kCubic, false>(f->m, src, (size_t)f->src_row_bytes, f->w, f->h, out, ow, x0, y);
    }
}

// A frame's border word (LR_WARP_BORDER): mode + 8 * value, an integer.  Fills the record's two fields; on a fault returns
// the reason (NULL: none).
const char* parse_border_word(double word, int format, RaggedFrame* f) {
    uint64_t v;
    if (!table_integer(word, 0, 34359738367.0, &v)) return "is not an integer from 0 to 2^35 - 1";
    const int mode = (int)(v & 7u);
    const uint64_t value = v >> 3;
    if (mode != kBorderConstant && mode != kBorderReplicate && mode != kBorderReflect && mode != kBorderReflect101)
        return "names a mode that is not 0 (constant), 1 (replicate), 2 (reflect) or 4 (reflect-101)";
    if (mode != kBorderConstant && value != 0) return "carries a value with a mode other than 0 (constant)";
    if (format == LR_PIX_U8 && value > 0xFFu) return "carries a value above 255 for u8";
    if (format == LR_PIX_U8X3 && value > 0xFFFFFFu) return "carries a value above 2^24 - 1 for u8x3";
    if (format == LR_PIX_F32 && (value & 0x7F800000u) == 0x7F800000u) return "carries f32 bits that are not a finite float";
    f->border_mode = mode;
    f->border_value = (unsigned)value;
    return nullptr;
}

int fail_border(const char* layout, int b, const char* why) {
    set_error(std::string("lr_warp_perspective_device: ") + layout + "LR_WARP_BORDER: frame " + std::to_string(b) + ": the border word " + why);
    return 1;
}

// A frame's nine lens entries (LR_WARP_LENS): fx, fy, cx, cy, k1, k2, p1, p2, k3.  Fills the record; on a fault returns the
// reason (NULL: none).  A frame whose five coefficients are all zero, of either sign, has no lens: the plain rule.
const char* parse_lens(const double* t, LensRecord* l) {
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(t[i])) return "are not all finite";
    if (!(t[0] > 0.0)) return "have fx <= 0";
    if (!(t[1] > 0.0)) return "have fy <= 0";
    std::memset(l, 0, sizeof *l);
    l->fx = t[0];
    l->fy = t[1];
    l->cx = t[2];
    l->cy = t[3];
    l->k1 = t[4];
    l->k2 = t[5];
    l->p1 = t[6];
    l->p2 = t[7];
    l->k3 = t[8];
    l->has_lens = t[4] != 0.0 || t[5] != 0.0 || t[6] != 0.0 || t[7] != 0.0 || t[8] != 0.0;
    return nullptr;
}

int fail_lens(const char* layout, int b, const char* why, int entries = 9) {
    set_error(std::string("lr_warp_perspective_device: ") + layout + (entries == 17 ? "LR_WARP_LENS_MODEL: frame " : "LR_WARP_LENS: frame ") +
              std::to_string(b) + (entries == 17 ? ": the seventeen lens entries " : ": the nine lens entries ") + why);
    return 1;
}

bool any_lens(const std::vector<LensRecord>& lens) {
    return std::any_of(lens.begin(), lens.end(), [](const LensRecord& l) { return l.has_lens != 0; });
}

// A frame's seventeen lens entries (LR_WARP_LENS_MODEL): fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, model.
// Fills the record; on a fault returns the reason (NULL: none).  A frame of model 0 whose twelve coefficients are all zero, of
// either sign, has no lens: the plain rule.  A fisheye always has one: zero coefficients are the pure equidistant lens.
const char* parse_lens_model(const double* t, LensModelRecord* l) {
    for (int i = 0; i < 17; ++i)
        if (!std::isfinite(t[i])) return "are not all finite";
    if (!(t[0] > 0.0)) return "have fx <= 0";
    if (!(t[1] > 0.0)) return "have fy <= 0";
    if (t[16] != 0.0 && t[16] != 1.0) return "name a model that is not 0 (LR_LENS_RATIONAL) or 1 (LR_LENS_FISHEYE)";
    const bool fisheye = t[16] == 1.0;
    if (fisheye)
        for (int i = 8; i < 16; ++i)
            if (t[i] != 0.0) return "are a fisheye's (model 1) with a non-zero entry among [8..15]";
    std::memset(l, 0, sizeof *l);
    std::memcpy(&l->fx, t, 17 * sizeof(double));
    l->kind = fisheye ? kLensFisheye : kLensNone;
    for (int i = 4; i < 16 && !fisheye; ++i)
        if (t[i] != 0.0) l->kind = kLensRational;
    return nullptr;
}

// The lenses of a call, from rows of nine (LR_WARP_LENS) or seventeen (with LR_WARP_LENS_MODEL) entries.  After the last frame
// settle() says what is launched: where no frame has a lens, what the call launches without the bits; where every frame fits the
// nine entries (model 0, [9..15] zero), LR_WARP_LENS's records and kernels; the records of seventeen only where a frame needs them.
struct LensSet {
    int entries;  // per frame in the table: 0, 9 or 17
    std::vector<LensRecord> nine;
    std::vector<LensModelRecord> model;
    LensSet(int entries_, size_t batch) : entries(entries_), nine(entries_ == 9 ? batch : 0), model(entries_ == 17 ? batch : 0) {}
    const char* parse(size_t b, const double* t) { return entries == 17 ? parse_lens_model(t, &model[b]) : parse_lens(t, &nine[b]); }
    void settle() {
        if (entries != 17) return;
        const bool fits = std::all_of(model.begin(), model.end(), [](const LensModelRecord& l) {
            return l.kind != kLensFisheye && l.k4 == 0.0 && l.k5 == 0.0 && l.k6 == 0.0 && l.s1 == 0.0 && l.s2 == 0.0 && l.s3 == 0.0 && l.s4 == 0.0;
        });
        if (!fits) return;
        nine.resize(model.size());
        for (size_t b = 0; b < model.size(); ++b) parse_lens(&model[b].fx, &nine[b]);  // (checked already: the first nine entries are the nine)
        model.clear();
    }
    const std::vector<LensRecord>* nine_if_any() const { return model.empty() && any_lens(nine) ? &nine : nullptr; }
    const std::vector<LensModelRecord>* model_if_any() const { return model.empty() ? nullptr : &model; }
};

// A frame's sampling factor (LR_WARP_AREA): the last double of its row, an integer from 1 to 8.  Fills the record with S and
// the fine map of the frame's map m (S = 1: m itself, the plain rule); on a fault returns the reason (NULL: none).
const char* parse_area(double entry, const double* m, uint64_t ow, uint64_t oh, AreaRecord* a) {
    uint64_t v;
    if (!table_integer(entry, 1, 8, &v)) return "is not an integer from 1 to 8";
    if (v * ow > 2147483647ull) return "times the frame's output width is above 2^31 - 1";
    if (v * oh > 2147483647ull) return "times the frame's output height is above 2^31 - 1";
    std::memset(a, 0, sizeof *a);
    a->s = (int)v;
    if (v == 1) std::memcpy(a->f, m, sizeof a->f);
    else lr_area_fine_map(m, (int)v, a->f);
    return nullptr;
}

int fail_area(const char* layout, int b, const char* why) {
    set_error(std::string("lr_warp_perspective_device: ") + layout + "LR_WARP_AREA: frame " + std::to_string(b) + ": the sampling factor S " + why);
    return 1;
}

bool any_area(const std::vector<AreaRecord>& area) {
    return std::any_of(area.begin(), area.end(), [](const AreaRecord& a) { return a.s > 1; });
}

// The table kernel's launch: records, then (LR_WARP_LENS, `lens` not NULL) the lens records or (LR_WARP_LENS_MODEL, `model` not
// NULL; never both) the records of seventeen entries, then (LR_WARP_AREA, `area` not NULL) the area records, then the tiles'
// prefix table, go up in the mirror of the maps (in doubles: 18 a frame, 10 a lens or 18 a lens of seventeen entries,
// 10 an area record + the table's ints).  The area kernel cuts a frame with S > 1 into tiles of (64 / S) x (16 / S) destination
// pixels (kernels_warp_area.hip: a tile is 64 x 16 samples), so with `area` the frames' tiles are counted again by that size.
int launch_ragged(lr_context* c, const void* d_src, int format, bool cubic, bool border, const std::vector<RaggedFrame>& frame_rec,
                  const std::vector<int>& frame_start, void* d_dst, const std::vector<LensRecord>* lens = nullptr,
                  const std::vector<AreaRecord>* area = nullptr, const std::vector<LensModelRecord>* model = nullptr) {
    const size_t batch = frame_rec.size(), lens_doubles = model ? batch * 18 : (lens ? batch * 10 : 0), area_doubles = area ? batch * 10 : 0;
    const size_t rec_doubles = batch * 18 + lens_doubles + area_doubles;
    std::vector<RaggedFrame> area_rec;
    std::vector<int> area_start;
    if (area) {
        area_rec = frame_rec;
        area_start.resize(batch + 1);
        int64_t tiles = 0;
        for (size_t b = 0; b < batch; ++b) {
            RaggedFrame& f = area_rec[b];
            const int tile_w = kTileW / (*area)[b].s, tile_h = kTileH / (*area)[b].s;  // (S = 1: the plain tile)
            f.tiles_x = (int)(((int64_t)f.ow + tile_w - 1) / tile_w);
            area_start[b] = (int)tiles;
            tiles += (int64_t)f.tiles_x * (((int64_t)f.oh + tile_h - 1) / tile_h);
            if (tiles > 0x7FFFFFF0ll) {
                set_error("lr_warp_perspective_device: LR_WARP_AREA: frame " + std::to_string(b) + ": output larger than 2^31 tiles of 64 x 16 samples");
                return 1;
            }
        }
        area_start[batch] = (int)tiles;
    }
    const std::vector<RaggedFrame>& rec = area ? area_rec : frame_rec;
    const std::vector<int>& start = area ? area_start : frame_start;
    const int64_t n_tiles = start[batch];
    LR_HIP(hipSetDevice(c->device));
    if (upload_reserve(c, c->warp_m, c->ev_warp_m, rec_doubles + (batch + 2) / 2)) return 1;
    std::memcpy(c->warp_m.h, rec.data(), batch * 18 * sizeof(double));
    if (model) std::memcpy(c->warp_m.h + batch * 18, model->data(), lens_doubles * sizeof(double));
    else if (lens) std::memcpy(c->warp_m.h + batch * 18, lens->data(), lens_doubles * sizeof(double));
    if (area) std::memcpy(c->warp_m.h + batch * 18 + lens_doubles, area->data(), area_doubles * sizeof(double));
    std::memcpy(c->warp_m.h + rec_doubles, start.data(), start.size() * sizeof(int));
    if (upload_send(c, c->warp_m, c->ev_warp_m, rec_doubles * sizeof(double) + start.size() * sizeof(int))) return 1;

    RaggedArgs g;
    g.src = static_cast<const uint8_t*>(d_src);
    g.batch = (int)batch;
    g.n_tiles = (int)n_tiles;
    uint8_t* dst = static_cast<uint8_t*>(d_dst);
    const RaggedFrame* frames = reinterpret_cast<const RaggedFrame*>(c->warp_m.d.get());
    const int* tile_start = reinterpret_cast<const int*>(c->warp_m.d.get() + rec_doubles);
    const int grid = (int)std::min<int64_t>((n_tiles + 7) / 8 * 8, kMaxGrid);
    if (model) {  // (some frame's lens needs the seventeen entries: the kernels of kernels_warp_lens_model.hip)
        launch_warp_ragged_lens_model(format, cubic, border, grid, c->stream, g.src, g.batch, g.n_tiles, frames, c->warp_m.d.get() + batch * 18,
                                      area ? c->warp_m.d.get() + batch * 18 + lens_doubles : nullptr, tile_start, dst);
        LR_HIP(hipGetLastError());
        return 0;
    }
    if (area) {  // (some frame's S is above 1: the kernels of kernels_warp_area.hip, which take the border rules as they are)
        launch_warp_ragged_area(format, cubic, grid, c->stream, g.src, g.batch, g.n_tiles, frames, lens ? c->warp_m.d.get() + batch * 18 : nullptr,
                                c->warp_m.d.get() + batch * 18 + lens_doubles, tile_start, dst);
        LR_HIP(hipGetLastError());
        return 0;
    }
    if (lens) {  // (some frame has a lens: the kernels of kernels_warp_lens.hip)
        launch_warp_ragged_lens(format, cubic, border, grid, c->stream, g.src, g.batch, g.n_tiles, frames, c->warp_m.d.get() + batch * 18, tile_start, dst);
        LR_HIP(hipGetLastError());
        return 0;
    }
    if (border) {  // (some frame's word is not 0: the kernels of kernels_warp_border.hip)
        launch_warp_ragged_border(format, cubic, grid, c->stream, g.src, g.batch, g.n_tiles, frames, tile_start, dst);
        LR_HIP(hipGetLastError());
        return 0;
    }
    launch_by_format_and_rule(format, cubic, [&](auto fmt, auto rule) {
        hipLaunchKernelGGL((warp_ragged_kernel<decltype(fmt)::value, decltype(rule)::value>), dim3(grid), dim3(kBlock), 0, c->stream, g, frames, tile_start, dst);
    });
    LR_HIP(hipGetLastError());
    return 0;
}

// lr_warp_perspective_device with LR_WARP_PACKED: M is the table of 13 doubles per frame, out_width x out_height bound the
// frames' sizes and dst_image_bytes is the size of the whole destination region
int warp_packed(lr_context* c, const void* d_src, size_t src_image_bytes, int batch, int width, int height, size_t src_row_bytes,
                int format, bool cubic, bool border, int lens, bool area, const double* T, void* d_dst, size_t dst_bytes, int out_width,
                int out_height, size_t dst_row_bytes) {
    auto fail = [](const char* what) {
        set_error(std::string("lr_warp_perspective_device: LR_WARP_PACKED: ") + what);
        return 1;
    };
    if (!d_src || !d_dst || !T) return fail("null pointer (source, destination or table)");
    if (batch < 1) return fail("batch < 1");
    if (width < 1 || height < 1 || out_width < 1 || out_height < 1) return fail("source size or output bound below 1");
    if (format != LR_PIX_U8 && format != LR_PIX_U8X3 && format != LR_PIX_F32) return fail("unknown pixel format");
    if (dst_row_bytes != 0) return fail("dst_row_bytes must be 0 (every frame's stride is in the table)");
    const size_t bpp = format == LR_PIX_U8 ? 1 : (format == LR_PIX_U8X3 ? 3 : 4);
    if (src_row_bytes < (size_t)width * bpp) return fail("source row stride shorter than a row");
    size_t src_span;
    if (!frame_span(height, src_row_bytes, (size_t)width * bpp, &src_span)) return fail("frame larger than the address space");
    if (batch > 1 && src_image_bytes < src_span) return fail("image stride shorter than a frame");
    if (format == LR_PIX_F32) {
        const uintptr_t bits = reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst) | src_row_bytes |
                               (batch > 1 ? src_image_bytes : 0);
        if (bits & 3u) return fail("f32 pointer or stride not 4-byte aligned");
    }
    // the table: every frame's map, size and place, and the tiles before it
    std::vector<RaggedFrame> rec((size_t)batch);
    std::vector<int> start((size_t)batch + 1);
    std::vector<std::pair<uint64_t, uint64_t>> extent((size_t)batch);  // [first byte, end)
    int64_t n_tiles = 0;
    const size_t lens_at = border ? 14 : 13;                // (LR_WARP_BORDER: the border word behind the row)
    const size_t area_at = lens_at + (size_t)lens;          // (LR_WARP_LENS: the nine or seventeen lens entries behind that)
    const size_t row_doubles = area_at + (area ? 1 : 0);    // (LR_WARP_AREA: the sampling factor at the very end)
    bool bordered = false;                                  // some frame's word is not 0
    LensSet lenses(lens, (size_t)batch);
    std::vector<AreaRecord> areas(area ? (size_t)batch : 0);
    for (int b = 0; b < batch; ++b) {
        const double* t = T + (size_t)b * row_doubles;
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(t[i])) return fail("M is not finite");
        uint64_t ow, oh, off, row;
        if (!table_integer(t[9], 1, out_width, &ow) || !table_integer(t[10], 1, out_height, &oh))
            return fail("a frame's size is not an integer from 1 to out_width x out_height");
        if (!table_integer(t[11], 0, kExact, &off)) return fail("a frame's offset is not an integer from 0 to 2^53");
        if (!table_integer(t[12], (double)(ow * bpp), kExact, &row))
            return fail("a frame's row stride is not an integer from a row's bytes to 2^53");
        if (format == LR_PIX_F32 && ((off | row) & 3u)) return fail("f32 offset or stride not a multiple of 4");
        uint64_t end;
        if (__builtin_mul_overflow(oh - 1, row, &end) || __builtin_add_overflow(end, off, &end) ||
            __builtin_add_overflow(end, ow * bpp, &end) || end > dst_bytes)
            return fail("a frame reaches beyond dst_image_bytes");
        extent[(size_t)b] = {off, end};
        RaggedFrame& f = rec[(size_t)b];
        std::memset(&f, 0, sizeof f);
        std::memcpy(f.m, t, sizeof f.m);
        f.offset = off;
        f.row_bytes = row;
        f.src_offset = (uint64_t)b * src_image_bytes;  // (the frames share one source size and stride)
        f.src_row_bytes = src_row_bytes;
        f.ow = (int)ow;
        f.oh = (int)oh;
        f.tiles_x = (int)((ow + kTileW - 1) / kTileW);
        f.w = width;
        f.h = height;
        if (border) {
            if (const char* why = parse_border_word(t[13], format, &f)) return fail_border("LR_WARP_PACKED: ", b, why);
            bordered = bordered || t[13] != 0.0;
        }
        if (lens)
            if (const char* why = lenses.parse((size_t)b, t + lens_at)) return fail_lens("LR_WARP_PACKED: ", b, why, lens);
        if (area)
            if (const char* why = parse_area(t[area_at], f.m, ow, oh, &areas[(size_t)b])) return fail_area("LR_WARP_PACKED: ", b, why);
        start[(size_t)b] = (int)n_tiles;
        n_tiles += (int64_t)f.tiles_x * (int64_t)((oh + kTileH - 1) / kTileH);
        if (n_tiles > 0x7FFFFFF0ll) return fail("output larger than 2^31 tiles of 64 x 16 pixels");
    }
    start[(size_t)batch] = (int)n_tiles;
    if (extents_overlap(extent)) return fail("two frames' extents overlap");
    lenses.settle();
    return launch_ragged(c, d_src, format, cubic, bordered, rec, start, d_dst, lenses.nine_if_any(), any_area(areas) ? &areas : nullptr,
                         lenses.model_if_any());
}

// lr_warp_perspective_device with LR_WARP_RAGGED: M is the table of 18 doubles per frame, width x height and out_width x
// out_height bound the frames' sizes, src_image_bytes and dst_image_bytes are the sizes of the two regions
int warp_ragged(lr_context* c, const void* d_src, size_t src_bytes, int batch, int width, int height, size_t src_row_bytes,
                int format, bool cubic, bool border, int lens, bool area, const double* T, void* d_dst, size_t dst_bytes, int out_width,
                int out_height, size_t dst_row_bytes) {
    std::vector<RaggedEntry> e;
    int64_t n_tiles = 0;
    // LR_WARP_BORDER: entry [17] is the frame's border word; the table's other checks see it as the 0 they ask for
    // LR_WARP_LENS: rows of 27 (LR_WARP_LENS_MODEL: 35), the lens entries behind [17]; the table's checks see rows of 18
    // LR_WARP_AREA: one more, the sampling factor at the very end
    std::vector<double> plain;
    const double* words = T;
    const size_t area_at = 18 + (size_t)lens, row_doubles = area_at + (area ? 1 : 0);
    if ((border || lens || area) && T && batch >= 1) {
        plain.resize((size_t)batch * 18);
        for (int b = 0; b < batch; ++b) {
            std::memcpy(&plain[(size_t)b * 18], words + (size_t)b * row_doubles, 18 * sizeof(double));
            if (border) plain[(size_t)b * 18 + 17] = 0.0;
        }
        T = plain.data();
    }
    LensSet lenses(lens, batch >= 1 ? (size_t)batch : 0);
    std::vector<AreaRecord> areas(area && batch >= 1 ? (size_t)batch : 0);
    bool bordered = false;  // some frame's word is not 0
    if (ragged_parse(d_src, src_bytes, batch, width, height, src_row_bytes, format, false, T, d_dst, dst_bytes, out_width,
                     out_height, dst_row_bytes, kTileW, kTileH, e, &n_tiles))
        return 1;
    std::vector<RaggedFrame> rec((size_t)batch);
    std::vector<int> start((size_t)batch + 1);
    int tiles = 0;
    for (int b = 0; b < batch; ++b) {
        const RaggedEntry& s = e[(size_t)b];
        RaggedFrame& f = rec[(size_t)b];
        std::memset(&f, 0, sizeof f);
        std::memcpy(f.m, T + (size_t)b * 18, sizeof f.m);
        f.offset = s.dst_off;
        f.row_bytes = s.dst_row;
        f.src_offset = s.src_off;
        f.src_row_bytes = s.src_row;
        f.ow = (int)s.ow;
        f.oh = (int)s.oh;
        f.tiles_x = (int)((s.ow + kTileW - 1) / kTileW);
        f.w = (int)s.w;
        f.h = (int)s.h;
        if (border) {
            const double word = words[(size_t)b * row_doubles + 17];
            if (const char* why = parse_border_word(word, format, &f)) return fail_border("LR_WARP_RAGGED: ", b, why);
            bordered = bordered || word != 0.0;
        }
        if (lens)
            if (const char* why = lenses.parse((size_t)b, words + (size_t)b * row_doubles + 18)) return fail_lens("LR_WARP_RAGGED: ", b, why, lens);
        if (area)
            if (const char* why = parse_area(words[(size_t)b * row_doubles + area_at], f.m, s.ow, s.oh, &areas[(size_t)b])) return fail_area("LR_WARP_RAGGED: ", b, why);
        start[(size_t)b] = tiles;
        tiles += f.tiles_x * (int)((s.oh + kTileH - 1) / kTileH);
    }
    start[(size_t)batch] = tiles;
    lenses.settle();
    return launch_ragged(c, d_src, format, cubic, bordered, rec, start, d_dst, lenses.nine_if_any(), any_area(areas) ? &areas : nullptr,
                         lenses.model_if_any());
}

}  // namespace

// The table of LR_WARP_RAGGED, checked as a whole before anything is launched (the warp and the prepare step share it):
// fills `out` and the number of tile_w x tile_h destination tiles; sets the error and returns 1 on the first fault.
int ragged_parse(const void* d_src, size_t src_bytes, int batch, int width, int height, size_t src_row_bytes, int format,
                 bool prepare, const double* T, const void* d_dst, size_t dst_bytes, int out_width, int out_height,
                 size_t dst_row_bytes, int tile_w, int tile_h, std::vector<RaggedEntry>& out, int64_t* n_tiles_out) {
    auto fail = [](const char* what) {
        set_error(std::string("lr_warp_perspective_device: LR_WARP_RAGGED: ") + what);
        return 1;
    };
    if (!d_src || !d_dst || !T) return fail("null pointer (source, destination or table)");
    if (batch < 1) return fail("batch < 1");
    if (width < 1 || height < 1 || out_width < 1 || out_height < 1) return fail("source bound or output bound below 1");
    if (format != LR_PIX_U8 && format != LR_PIX_U8X3 && format != LR_PIX_F32) return fail("unknown pixel format");
    if (src_row_bytes != 0 || dst_row_bytes != 0) return fail("src_row_bytes and dst_row_bytes must be 0 (every frame's strides are in the table)");
    const uint64_t bpp = format == LR_PIX_U8 ? 1 : (format == LR_PIX_U8X3 ? 3 : 4);
    const uint64_t obpp = prepare ? 4 : bpp;  // (the prepare step writes f32 gray)
    const bool src_f32 = format == LR_PIX_F32, dst_f32 = prepare || format == LR_PIX_F32;
    if (src_f32 && (reinterpret_cast<uintptr_t>(d_src) & 3u)) return fail("f32 source pointer not 4-byte aligned");
    if (dst_f32 && (reinterpret_cast<uintptr_t>(d_dst) & 3u)) return fail("f32 destination pointer not 4-byte aligned");
    out.assign((size_t)batch, RaggedEntry{});
    std::vector<std::pair<uint64_t, uint64_t>> extent((size_t)batch);  // of the outputs: [first byte, end)
    int64_t n_tiles = 0;
    for (int b = 0; b < batch; ++b) {
        const double* t = T + (size_t)b * 18;
        RaggedEntry& s = out[(size_t)b];
        if (!(t[17] == 0.0)) return fail("a frame's entry [17] is reserved and must be 0");
        if (!prepare)
            for (int i = 0; i < 9; ++i)
                if (!std::isfinite(t[i])) return fail("M is not finite");
        if (!table_integer(t[9], 1, out_width, &s.ow) || !table_integer(t[10], 1, out_height, &s.oh))
            return fail("a frame's output size is not an integer from 1 to out_width x out_height");
        if (!table_integer(t[11], 0, kExact, &s.dst_off)) return fail("a frame's output offset is not an integer from 0 to 2^53");
        if (!table_integer(t[12], (double)(s.ow * obpp), kExact, &s.dst_row))
            return fail("a frame's output row stride is not an integer from a row's bytes to 2^53");
        if (!table_integer(t[13], 1, width, &s.w) || !table_integer(t[14], 1, height, &s.h))
            return fail("a frame's source size is not an integer from 1 to width x height");
        if (!table_integer(t[15], 0, kExact, &s.src_off)) return fail("a frame's source offset is not an integer from 0 to 2^53");
        if (!table_integer(t[16], (double)(s.w * bpp), kExact, &s.src_row))
            return fail("a frame's source row stride is not an integer from a row's bytes to 2^53");
        if (dst_f32 && ((s.dst_off | s.dst_row) & 3u)) return fail("f32 output offset or stride not a multiple of 4");
        if (src_f32 && ((s.src_off | s.src_row) & 3u)) return fail("f32 source offset or stride not a multiple of 4");
        if (prepare && (s.ow > s.w || s.oh > s.h)) return fail("LR_WARP_PREPARE: a frame's output larger than its source (no upscaling)");
        uint64_t end;
        if (__builtin_mul_overflow(s.oh - 1, s.dst_row, &end) || __builtin_add_overflow(end, s.dst_off, &end) ||
            __builtin_add_overflow(end, s.ow * obpp, &end) || end > dst_bytes)
            return fail("a frame's output reaches beyond dst_image_bytes");
        extent[(size_t)b] = {s.dst_off, end};
        if (__builtin_mul_overflow(s.h - 1, s.src_row, &end) || __builtin_add_overflow(end, s.src_off, &end) ||
            __builtin_add_overflow(end, s.w * bpp, &end) || end > src_bytes)
            return fail("a frame's source reaches beyond src_image_bytes");
        n_tiles += (int64_t)((s.ow + (uint64_t)tile_w - 1) / (uint64_t)tile_w) * (int64_t)((s.oh + (uint64_t)tile_h - 1) / (uint64_t)tile_h);
        if (n_tiles > 0x7FFFFFF0ll) return fail("output larger than 2^31 tiles");
    }
    if (extents_overlap(extent)) return fail("two frames' output extents overlap");
    *n_tiles_out = n_tiles;
    return 0;
}

int ctx_warp_perspective(lr_context* c, const void* d_src, size_t src_image_bytes, int batch, int width, int height,
                         size_t src_row_bytes, int format, const double* M, void* d_dst, size_t dst_image_bytes,
                         int out_width, int out_height, size_t dst_row_bytes) {
    auto fail = [](const char* what) {
        set_error(std::string("lr_warp_perspective_device: ") + what);
        return 1;
    };
    // LR_WARP_CUBIC: the sampling rule of the three warps (one size, LR_WARP_PACKED, LR_WARP_RAGGED) and of nothing else
    const bool cubic = (format & LR_WARP_CUBIC) != 0;
    if (cubic) {
        if (format & LR_WARP_PREPARE) return fail("LR_WARP_CUBIC together with LR_WARP_PREPARE (the prepare step is an area average)");
        if (format & LR_WARP_LINES) return fail("LR_WARP_CUBIC together with LR_WARP_LINES (the lines picture samples nothing)");
        if (format & LR_WARP_JPEG) return fail("LR_WARP_CUBIC together with LR_WARP_JPEG (the encoder samples nothing)");
        if (format & LR_WARP_JPEG_DECODE) return fail("LR_WARP_CUBIC together with LR_WARP_JPEG_DECODE (the decoder samples nothing)");
        if (format & LR_WARP_TENSOR) return fail("unknown option bits in format: LR_WARP_CUBIC together with LR_WARP_TENSOR (the pack samples nothing)");
        format &= ~LR_WARP_CUBIC;
    }
    // LR_WARP_BORDER: a border word per frame behind (LR_WARP_RAGGED: in) its row of M; likewise of the three warps alone
    const bool border = (format & LR_WARP_BORDER) != 0;
    if (border) {
        if (format & LR_WARP_PREPARE) return fail("LR_WARP_BORDER together with LR_WARP_PREPARE (the prepare step reads no pixel outside its source)");
        if (format & LR_WARP_LINES) return fail("LR_WARP_BORDER together with LR_WARP_LINES (the lines picture samples nothing)");
        if (format & LR_WARP_JPEG) return fail("LR_WARP_BORDER together with LR_WARP_JPEG (the encoder samples nothing)");
        if (format & LR_WARP_JPEG_DECODE) return fail("LR_WARP_BORDER together with LR_WARP_JPEG_DECODE (the decoder samples nothing)");
        if (format & LR_WARP_TENSOR) return fail("unknown option bits in format: LR_WARP_BORDER together with LR_WARP_TENSOR (the pack samples nothing)");
        format &= ~LR_WARP_BORDER;
    }
    // LR_WARP_LENS: nine lens entries per frame at the end of its row of M; likewise of the three warps alone
    // LR_WARP_LENS_MODEL: with it the lens entries are seventeen; an option of LR_WARP_LENS and of nothing else
    const bool lens_model = (format & LR_WARP_LENS_MODEL) != 0;
    if (lens_model) {
        if (format & LR_WARP_PREPARE) return fail("LR_WARP_LENS_MODEL together with LR_WARP_PREPARE (the prepare step is an area average of the stored frame)");
        if (format & LR_WARP_LINES) return fail("LR_WARP_LENS_MODEL together with LR_WARP_LINES (the lines picture samples nothing)");
        if (format & LR_WARP_JPEG) return fail("LR_WARP_LENS_MODEL together with LR_WARP_JPEG (the encoder samples nothing)");
        if (format & LR_WARP_JPEG_DECODE) return fail("LR_WARP_LENS_MODEL together with LR_WARP_JPEG_DECODE (the decoder samples nothing)");
        if (format & LR_WARP_TENSOR) return fail("unknown option bits in format: LR_WARP_LENS_MODEL together with LR_WARP_TENSOR (the pack samples nothing)");
        if (!(format & LR_WARP_LENS)) return fail("LR_WARP_LENS_MODEL without LR_WARP_LENS (it widens that bit's lens entries)");
        format &= ~LR_WARP_LENS_MODEL;
    }
    const int lens = (format & LR_WARP_LENS) != 0 ? (lens_model ? 17 : 9) : 0;
    if (lens) {
        if (format & LR_WARP_PREPARE) return fail("LR_WARP_LENS together with LR_WARP_PREPARE (the prepare step is an area average of the stored frame)");
        if (format & LR_WARP_LINES) return fail("LR_WARP_LENS together with LR_WARP_LINES (the lines picture samples nothing)");
        if (format & LR_WARP_JPEG) return fail("LR_WARP_LENS together with LR_WARP_JPEG (the encoder samples nothing)");
        if (format & LR_WARP_JPEG_DECODE) return fail("LR_WARP_LENS together with LR_WARP_JPEG_DECODE (the decoder samples nothing)");
        if (format & LR_WARP_TENSOR) return fail("unknown option bits in format: LR_WARP_LENS together with LR_WARP_TENSOR (the pack samples nothing)");
        format &= ~LR_WARP_LENS;
    }
    // LR_WARP_AREA: a sampling factor per frame at the very end of its row of M; likewise of the three warps alone
    const bool area = (format & LR_WARP_AREA) != 0;
    if (area) {
        if (format & LR_WARP_PREPARE) return fail("LR_WARP_AREA together with LR_WARP_PREPARE (the prepare step is an area average of its own)");
        if (format & LR_WARP_LINES) return fail("LR_WARP_AREA together with LR_WARP_LINES (the lines picture samples nothing)");
        if (format & LR_WARP_JPEG) return fail("LR_WARP_AREA together with LR_WARP_JPEG (the encoder samples nothing)");
        if (format & LR_WARP_JPEG_DECODE) return fail("LR_WARP_AREA together with LR_WARP_JPEG_DECODE (the decoder samples nothing)");
        if (format & LR_WARP_TENSOR) return fail("unknown option bits in format: LR_WARP_AREA together with LR_WARP_TENSOR (the pack samples nothing)");
        format &= ~LR_WARP_AREA;
    }
    if (format & LR_WARP_JPEG_DECODE) {  // lr_decode_jpeg_device (kernels_jpeg_decode.hip): its own arguments arrive behind M
        // (LR_JPEG_ANY_SAMPLING and LR_JPEG_SCALED are the decoder's own options and travel on with the format)
        constexpr int kDecoderOptions = LR_JPEG_ANY_SAMPLING | LR_JPEG_SCALED;
        if ((format & ~(0xFF | kDecoderOptions)) != LR_WARP_JPEG_DECODE) return fail("LR_WARP_JPEG_DECODE together with another option bit");
        if (width != 0 || height != 0 || src_row_bytes != 0 || out_width != 0 || out_height != 0 || dst_row_bytes != 0)
            return fail("LR_WARP_JPEG_DECODE: width, height, out_width, out_height and the row strides must be 0 (they are in the frame table)");
        if (!M) return fail("LR_WARP_JPEG_DECODE: null pointer (lr_jpeg_decode_args)");
        const lr_jpeg_decode_args* a = reinterpret_cast<const lr_jpeg_decode_args*>(M);
        // (probe mode, d_dst == NULL, needs no context)
        return ctx_decode_jpeg(c, d_src, a->h_src, src_image_bytes, format & (0xFF | kDecoderOptions), a->frames, batch, d_dst, dst_image_bytes, a->info);
    }
    if (!c) return fail("no context");
    if (format & LR_WARP_JPEG) {  // lr_encode_jpeg_device (kernels_jpeg.hip): its own arguments arrive behind M
        if ((format & ~0xFF) != LR_WARP_JPEG) return fail("LR_WARP_JPEG together with another option bit");
        if (width != 0 || height != 0 || src_row_bytes != 0 || out_width != 0 || out_height != 0 || dst_row_bytes != 0)
            return fail("LR_WARP_JPEG: width, height, out_width, out_height and the row strides must be 0 (they are in the frame table)");
        if (!M) return fail("LR_WARP_JPEG: null pointer (lr_jpeg_args)");
        const lr_jpeg_args* a = reinterpret_cast<const lr_jpeg_args*>(M);
        return ctx_encode_jpeg(c, d_src, src_image_bytes, format & 0xFF, a->frames, batch, d_dst, dst_image_bytes, a->sizes);
    }
    if (format & LR_WARP_LINES) {  // lr_draw_lines_device (kernels_overlay.hip): its own arguments arrive behind M
        if ((format & ~0xFF) != LR_WARP_LINES) return fail("LR_WARP_LINES together with another option bit");
        if (width != 0 || height != 0 || src_row_bytes != 0 || out_width != 0 || out_height != 0 || dst_row_bytes != 0)
            return fail("LR_WARP_LINES: width, height, out_width, out_height and the row strides must be 0 (they are in the frame table)");
        if (!M) return fail("LR_WARP_LINES: null pointer (lr_draw_lines_args)");
        const lr_draw_lines_args* a = reinterpret_cast<const lr_draw_lines_args*>(M);
        return ctx_draw_lines(c, d_src, src_image_bytes, format & 0xFF, a->lines, a->n_lines, a->frames, batch, a->H, d_dst,
                              dst_image_bytes);
    }
    if (format & LR_WARP_TENSOR) {  // lr_pack_tensor_device (kernels_tensor.hip): its own arguments arrive behind M
        if ((format & ~0xFF) != LR_WARP_TENSOR) return fail("unknown option bits in format: LR_WARP_TENSOR together with another option bit");
        if (width != 0 || height != 0 || src_row_bytes != 0 || out_width != 0 || out_height != 0 || dst_row_bytes != 0)
            return fail("unknown option bits in format for a warp; as LR_WARP_TENSOR: width, height, out_width, out_height and the row strides must be 0 (they are in the frame table)");
        if (!M) return fail("LR_WARP_TENSOR: null pointer (lr_tensor_args)");
        return ctx_pack_tensor(c, d_src, src_image_bytes, format & 0xFF, reinterpret_cast<const lr_tensor_args*>(M), batch, d_dst, dst_image_bytes);
    }
    if (format & LR_WARP_RAGGED) {  // every frame its own source and output: one table for the warp and the prepare step
        const int opts = format & ~0xFF;
        if (opts & LR_WARP_PACKED) return fail("LR_WARP_RAGGED together with LR_WARP_PACKED (ragged outputs are always packed)");
        if (opts == LR_WARP_RAGGED)
            return warp_ragged(c, d_src, src_image_bytes, batch, width, height, src_row_bytes, format & 0xFF, cubic, border, lens, area, M, d_dst,
                               dst_image_bytes, out_width, out_height, dst_row_bytes);
        if (opts == (LR_WARP_RAGGED | LR_WARP_PREPARE))
            return ctx_prepare_ragged(c, d_src, src_image_bytes, batch, width, height, src_row_bytes, format & 0xFF, M, d_dst,
                                      dst_image_bytes, out_width, out_height, dst_row_bytes);
        return fail("unknown option bits in format");
    }
    if (format & ~0xFF) {  // option bits above the pixel format
        if ((format & ~0xFF) == LR_WARP_PACKED)
            return warp_packed(c, d_src, src_image_bytes, batch, width, height, src_row_bytes, format & 0xFF, cubic, border, lens, area, M, d_dst,
                               dst_image_bytes, out_width, out_height, dst_row_bytes);
        if ((format & ~0xFF) == (LR_WARP_PACKED | LR_WARP_PREPARE)) return fail("LR_WARP_PACKED together with LR_WARP_PREPARE");
        if ((format & ~0xFF) != LR_WARP_PREPARE) return fail("unknown option bits in format");
        return ctx_prepare_frames(c, d_src, src_image_bytes, batch, width, height, src_row_bytes, format & 0xFF, d_dst,
                                  dst_image_bytes, out_width, out_height, dst_row_bytes);
    }
    if (!d_src || !d_dst || !M) return fail("null pointer (source, destination or M)");
    if (batch < 1) return fail("batch < 1");
    if (width < 1 || height < 1 || out_width < 1 || out_height < 1) return fail("source or output size below 1");
    if (format != LR_PIX_U8 && format != LR_PIX_U8X3 && format != LR_PIX_F32) return fail("unknown pixel format");
    const size_t bpp = format == LR_PIX_U8 ? 1 : (format == LR_PIX_U8X3 ? 3 : 4);
    if (src_row_bytes < (size_t)width * bpp) return fail("source row stride shorter than a row");
    if (dst_row_bytes < (size_t)out_width * bpp) return fail("destination row stride shorter than a row");
    size_t src_span, dst_span;
    if (!frame_span(height, src_row_bytes, (size_t)width * bpp, &src_span) ||
        !frame_span(out_height, dst_row_bytes, (size_t)out_width * bpp, &dst_span))
        return fail("frame larger than the address space");
    if (batch > 1 && (src_image_bytes < src_span || dst_image_bytes < dst_span))
        return fail("image stride shorter than a frame");
    if (format == LR_PIX_F32) {
        const uintptr_t bits = reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst) | src_row_bytes |
                               dst_row_bytes | (batch > 1 ? (src_image_bytes | dst_image_bytes) : 0);
        if (bits & 3u) return fail("f32 pointer or stride not 4-byte aligned");
    }
    const size_t lens_at = border ? 10 : 9;               // (LR_WARP_BORDER: the border word behind the map)
    const size_t area_at = lens_at + (size_t)lens;        // (LR_WARP_LENS: the nine or seventeen lens entries behind that)
    const size_t row_doubles = area_at + (area ? 1 : 0);  // (LR_WARP_AREA: the sampling factor at the very end)
    for (size_t b = 0; b < (size_t)batch; ++b)
        for (size_t i = 0; i < 9; ++i)
            if (!std::isfinite(M[b * row_doubles + i])) return fail("M is not finite");
    const int64_t tiles_x = ((int64_t)out_width + kTileW - 1) / kTileW, tiles_y = ((int64_t)out_height + kTileH - 1) / kTileH;
    const int64_t n_tiles = tiles_x * tiles_y * (int64_t)batch;
    if (n_tiles > 0x7FFFFFF0ll) return fail("output larger than 2^31 tiles of 64 x 16 pixels");
    if (border || lens || area) {  // the frames as records of the table kernel; where every word is 0, no frame has a lens and every S is 1, the launch below as without the bits
        std::vector<RaggedFrame> rec((size_t)batch);
        LensSet lenses(lens, (size_t)batch);
        std::vector<AreaRecord> areas(area ? (size_t)batch : 0);
        std::vector<int> start((size_t)batch + 1);
        bool bordered = false;
        for (int b = 0; b < batch; ++b) {
            const double* t = M + (size_t)b * row_doubles;
            RaggedFrame& f = rec[(size_t)b];
            std::memset(&f, 0, sizeof f);
            std::memcpy(f.m, t, sizeof f.m);
            f.offset = (uint64_t)b * dst_image_bytes;
            f.row_bytes = dst_row_bytes;
            f.src_offset = (uint64_t)b * src_image_bytes;
            f.src_row_bytes = src_row_bytes;
            f.ow = out_width;
            f.oh = out_height;
            f.tiles_x = (int)tiles_x;
            f.w = width;
            f.h = height;
            if (border) {
                if (const char* why = parse_border_word(t[9], format, &f)) return fail_border("", b, why);
                bordered = bordered || t[9] != 0.0;
            }
            if (lens)
                if (const char* why = lenses.parse((size_t)b, t + lens_at)) return fail_lens("", b, why, lens);
            if (area)
                if (const char* why = parse_area(t[area_at], f.m, (uint64_t)out_width, (uint64_t)out_height, &areas[(size_t)b])) return fail_area("", b, why);
            start[(size_t)b] = (int)(tiles_x * tiles_y * b);
        }
        start[(size_t)batch] = (int)n_tiles;
        lenses.settle();
        const bool lensed = lenses.nine_if_any() || lenses.model_if_any(), sampled = any_area(areas);
        if (bordered || lensed || sampled)
            return launch_ragged(c, d_src, format, cubic, bordered, rec, start, d_dst, lenses.nine_if_any(), sampled ? &areas : nullptr, lenses.model_if_any());
    }

    LR_HIP(hipSetDevice(c->device));
    if (upload_reserve(c, c->warp_m, c->ev_warp_m, (size_t)batch * 9)) return 1;
    for (size_t b = 0; b < (size_t)batch; ++b) std::memcpy(c->warp_m.h + b * 9, M + b * row_doubles, 9 * sizeof(double));
    if (upload_send(c, c->warp_m, c->ev_warp_m, (size_t)batch * 9 * sizeof(double))) return 1;

    WarpArgs g;
    g.src = static_cast<const uint8_t*>(d_src);
    g.src_image_bytes = src_image_bytes;
    g.src_row_bytes = src_row_bytes;
    g.w = width;
    g.h = height;
    g.dst = static_cast<uint8_t*>(d_dst);
    g.dst_image_bytes = dst_image_bytes;
    g.dst_row_bytes = dst_row_bytes;
    g.ow = out_width;
    g.oh = out_height;
    g.M = c->warp_m.d;
    g.tiles_x = (int)tiles_x;
    g.tiles_per_frame = (int)(tiles_x * tiles_y);
    g.n_tiles = (int)n_tiles;
    const int grid = (int)std::min<int64_t>((n_tiles + 7) / 8 * 8, kMaxGrid);
    launch_by_format_and_rule(format, cubic, [&](auto fmt, auto rule) {
        hipLaunchKernelGGL((warp_perspective_kernel<decltype(fmt)::value, decltype(rule)::value>), dim3(grid), dim3(kBlock), 0, c->stream, g);
    });
    LR_HIP(hipGetLastError());
    return 0;
}

}  // namespace lramd
