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

#include "tables.h"
#include "tiles.h"

namespace lramd {
namespace {

constexpr int kTileW = 64;  // destination pixels per tile row (16 lanes x 4 pixels)
constexpr int kTileH = 16;  // destination rows per tile (4 wavefronts x 4 rows)
constexpr int kBlock = 256;
constexpr int kMaxGrid = 8 * 8192;  // beyond that the workgroups of an XCD loop over its run of tiles

struct WarpArgs {
    const uint8_t* src;
    size_t src_image_bytes, src_row_bytes;
    int w, h;
    uint8_t* dst;
    size_t dst_image_bytes, dst_row_bytes;
    int ow, oh;
    const double* M;  // 9 doubles per frame
    int tiles_x, tiles_per_frame, n_tiles;
};

// a frame's record of the table kernel, 18 doubles long like the row of LR_WARP_RAGGED's table it is made from
struct RaggedFrame {
    double m[9];
    unsigned long long offset, row_bytes;          // of its output, from the destination pointer
    unsigned long long src_offset, src_row_bytes;  // of its source, from the source pointer
    int ow, oh, tiles_x, w, h, pad[5];
};
static_assert(sizeof(RaggedFrame) == 18 * sizeof(double), "a record per 18 doubles of the mirror");

struct RaggedArgs {
    const uint8_t* src;
    int batch, n_tiles;
};

// ((M0 x + M1 y) + M2) * Wq clamped to [INT_MIN, INT_MAX] and rounded half to even; a NaN fails both comparisons and
// becomes INT_MIN, whose taps lie outside every source
__device__ __forceinline__ int fixed_coord(double v) {
    const double c = v >= 2147483647.0 ? 2147483647.0 : (v >= -2147483648.0 ? v : -2147483648.0);
    return (int)rint(c);
}

struct Taps {
    int ix, iy;        // the top-left tap
    int w00, w01, w10, w11;  // weights of (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1); they sum to 1024
};

// the 5-bit fixed-point source coordinates of destination pixel (x, y): both sampling rules start from them
__device__ __forceinline__ void fixed_xy(const double* __restrict__ m, unsigned x, unsigned y, int& X, int& Y) {
    const double xd = (double)x, yd = (double)y;
    const double W0 = (m[6] * xd + m[7] * yd) + m[8];
    const double Wq = W0 != 0.0 ? 32.0 / W0 : 0.0;
    X = fixed_coord(((m[0] * xd + m[1] * yd) + m[2]) * Wq);
    Y = fixed_coord(((m[3] * xd + m[4] * yd) + m[5]) * Wq);
}

__device__ __forceinline__ Taps taps_of(const double* __restrict__ m, unsigned x, unsigned y) {
    int X, Y;
    fixed_xy(m, x, y, X, Y);
    Taps t;
    t.ix = X >> 5;
    t.iy = Y >> 5;
    const int ax = X & 31, ay = Y & 31;
    t.w00 = (32 - ax) * (32 - ay);
    t.w01 = ax * (32 - ay);
    t.w10 = (32 - ax) * ay;
    t.w11 = ax * ay;
    return t;
}

__device__ __forceinline__ bool inside(int i, int n) { return (unsigned)i < (unsigned)n; }

// the two horizontal taps (ix, ix+1) of one source row; 0 outside
__device__ __forceinline__ void pair_u8(const uint8_t* row, bool row_in, int ix, int w, uint32_t& a, uint32_t& b) {
    const bool in_a = row_in && inside(ix, w), in_b = row_in && inside(ix + 1, w);
    a = 0;
    b = 0;
    if (in_a && in_b && ((reinterpret_cast<uintptr_t>(row) + (unsigned)ix) & 1u) == 0) {
        const uint32_t v = *reinterpret_cast<const uint16_t*>(row + ix);
        a = v & 0xFFu;
        b = v >> 8;
    } else {
        if (in_a) a = row[ix];
        if (in_b) b = row[ix + 1];
    }
}

__device__ __forceinline__ void pair_f32(const uint8_t* row, bool row_in, int ix, int w, float& a, float& b) {
    const bool in_a = row_in && inside(ix, w), in_b = row_in && inside(ix + 1, w);
    a = 0.f;
    b = 0.f;
    const float* r = reinterpret_cast<const float*>(row);
    if (in_a && in_b && ((reinterpret_cast<uintptr_t>(r + ix)) & 7u) == 0) {
        const float2 v = *reinterpret_cast<const float2*>(r + ix);
        a = v.x;
        b = v.y;
    } else {
        if (in_a) a = r[ix];
        if (in_b) b = r[ix + 1];
    }
}

// one interleaved 3-byte tap at p: an aligned u16 and the byte beside it (two loads, no branch)
__device__ __forceinline__ uint32_t tap_u8x3(const uint8_t* p, bool in) {
    if (!in) return 0;
    const uint32_t odd = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 1u);
    const uint32_t v = *reinterpret_cast<const uint16_t*>(p + odd);
    const uint32_t s = p[odd ? 0 : 2];
    return odd ? (s | (v << 8)) : (v | (s << 16));  // bytes r | g << 8 | b << 16
}

__device__ __forceinline__ uint32_t blend_u8(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const Taps& t) {
    return (a * (uint32_t)t.w00 + b * (uint32_t)t.w01 + c * (uint32_t)t.w10 + d * (uint32_t)t.w11 + 512u) >> 10;
}

// ---- LR_WARP_CUBIC: the 4 x 4 bicubic rule (tests/numpy_warp_cubic_ref.py) ----

template <int kFormat>
struct PixelBytes {
    static constexpr int value = kFormat == LR_PIX_U8 ? 1 : (kFormat == LR_PIX_U8X3 ? 3 : 4);
};

// The four horizontal taps (ix - 1 .. ix + 2) of one source row as the 4, 12 or 16 consecutive bytes they are, in kBpp
// dwords; a tap outside the source is 0.  Where all four are inside, their bytes and no others come in with one load
// (dword, dwordx3, dwordx4: global memory asks for no alignment of an 8-bit row's taps and for 4 bytes of f32's);
// otherwise every tap that is inside is fetched on its own.  So no byte outside the row's own pixels [row, row + w * kBpp)
// is ever read: not a row's padding, not a neighbouring frame, nothing behind the last row.
template <int kFormat>
__device__ __forceinline__ void row_taps(const uint8_t* row, bool row_in, int ix, int w, uint32_t (&d)[PixelBytes<kFormat>::value]) {
    constexpr int kBpp = PixelBytes<kFormat>::value;
#pragma unroll
    for (int i = 0; i < kBpp; ++i) d[i] = 0;
    if (!row_in) return;
    const bool cols_in = ix >= 1 && ix + 2 < w;  // (|ix| <= 2^26: no overflow)
    if constexpr (kFormat == LR_PIX_F32) {
        const float* r = reinterpret_cast<const float*>(row);
        if (cols_in) {  // sixteen bytes at a 4-byte aligned address: one dwordx4, which asks for no more than that
            __builtin_memcpy(d, r + (ix - 1), 16);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (inside(ix - 1 + i, w)) d[i] = __float_as_uint(r[ix - 1 + i]);
        }
    } else {
        if (cols_in) {  // the taps' own 4 or 12 bytes, wherever they start: one load (global memory needs no alignment)
            __builtin_memcpy(d, row + (size_t)(ix - 1) * kBpp, 4 * kBpp);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = ix - 1 + i;
                const bool in = inside(c, w);
                if constexpr (kFormat == LR_PIX_U8) {
                    if (in) d[0] |= (uint32_t)row[c] << (8 * i);
                } else {
                    const uint32_t t = tap_u8x3(row + (size_t)(in ? c : 0) * 3, in);
                    const int bit = 24 * i;  // the tap's three bytes start at byte 3 i of the twelve
                    d[(bit >> 5)] |= t << (bit & 31);
                    if ((bit & 31) > 8) d[((bit >> 5) + 1)] |= t >> (32 - (bit & 31));
                }
            }
        }
    }
}

// One destination pixel by the bicubic rule: a u8 pixel's byte or a u8x3 pixel's bytes r | g << 8 | b << 16 in `px`, an
// f32 pixel in `pf`.  8-bit: h_j = sum_i C[ax][i] v(i, j), s = sum_j C[ay][j] h_j, (s + 2^21) >> 22 clamped to 0 .. 255.
// Everything fits int32: max sum |C[a]| is 2816 and 255 * 2816^2 + 2^21 = 2 024 210 432 < 2^31.  f32: weights C / 2048.f
// (exact), rows and then the column summed from the first tap to the last, every product and sum rounded on its own.
template <int kFormat>
__device__ __forceinline__ void cubic_pixel(const double* m, const uint8_t* src, size_t src_row_bytes, int w, int h, unsigned x,
                                            unsigned y, uint32_t& px, float& pf) {
    constexpr int kBpp = PixelBytes<kFormat>::value;
    constexpr int kChannels = kFormat == LR_PIX_U8X3 ? 3 : 1;
    int X, Y;
    fixed_xy(m, x, y, X, Y);
    const int ix = X >> 5, iy = Y >> 5;
    const int16_t* cx = kCubicWeights[X & 31];
    const int16_t* cy = kCubicWeights[Y & 31];
    const int wx[4] = {cx[0], cx[1], cx[2], cx[3]};
    const int wy[4] = {cy[0], cy[1], cy[2], cy[3]};
    int s[kChannels];
#pragma unroll
    for (int ch = 0; ch < kChannels; ++ch) s[ch] = 0;
    float hf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ry = iy - 1 + j;
        const bool row_in = inside(ry, h);
        const uint8_t* row = src + (size_t)(row_in ? ry : 0) * src_row_bytes;
        uint32_t d[kBpp];
        row_taps<kFormat>(row, row_in, ix, w, d);
        if constexpr (kFormat == LR_PIX_F32) {
            const float v0 = __uint_as_float(d[0]), v1 = __uint_as_float(d[1]);
            const float v2 = __uint_as_float(d[2]), v3 = __uint_as_float(d[3]);
            hf[j] = ((v0 * ((float)wx[0] / 2048.0f) + v1 * ((float)wx[1] / 2048.0f)) + v2 * ((float)wx[2] / 2048.0f)) +
                    v3 * ((float)wx[3] / 2048.0f);
        } else {
#pragma unroll
            for (int ch = 0; ch < kChannels; ++ch) {
                int hsum = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int byte = kChannels * i + ch;
                    hsum += wx[i] * (int)((d[(byte >> 2)] >> (8 * (byte & 3))) & 0xFFu);
                }
                s[ch] += wy[j] * hsum;
            }
        }
    }
    px = 0;
    pf = 0.f;
    if constexpr (kFormat == LR_PIX_F32) {
        pf = ((hf[0] * ((float)wy[0] / 2048.0f) + hf[1] * ((float)wy[1] / 2048.0f)) + hf[2] * ((float)wy[2] / 2048.0f)) +
             hf[3] * ((float)wy[3] / 2048.0f);
    } else {
#pragma unroll
        for (int ch = 0; ch < kChannels; ++ch) {
            // clamped BEFORE the shift ((s + 2^21) >> 22 within 0 .. 255 is s + 2^21 within 0 .. 2^30 - 1): the same value, but
            // written as shift-then-clamp two neighbouring pixels become one v_ashr_pk_u8_i32, whose result the compiler
            // takes to be zero above bit 15 while the instruction leaves other bits there, which then land in the lane's
            // third and fourth pixel
            const int t = min(max(s[ch] + (1 << 21), 0), (1 << 30) - 1);
            px |= ((uint32_t)t >> 22) << (8 * ch);
        }
    }
}

// One lane's four consecutive pixels (x0 .. x0 + 3, those below ow) of destination row y, whose first byte is `out`;
// kCubic: sampled by the bicubic rule above instead of the bilinear one
template <int kFormat, bool kCubic>
__device__ __forceinline__ void warp_lane(const double* m, const uint8_t* src, size_t src_row_bytes, int w, int h,
                                          uint8_t* out, int ow, unsigned x0, unsigned y) {
    const int n = min(4, ow - (int)x0);  // pixels of this lane inside the row

    uint32_t res_u8 = 0;          // LR_PIX_U8: four bytes
    uint32_t res_rgb[3] = {0, 0, 0};  // LR_PIX_U8X3: twelve bytes
    float res_f[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (kCubic) {
            uint32_t px;
            cubic_pixel<kFormat>(m, src, src_row_bytes, w, h, x0 + (unsigned)k, y, px, res_f[k]);
            if (kFormat == LR_PIX_U8) res_u8 |= px << (8 * k);
            if (kFormat == LR_PIX_U8X3) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int byte = 3 * k + ch;  // byte of the lane's twelve
                    res_rgb[byte >> 2] |= ((px >> (8 * ch)) & 0xFFu) << (8 * (byte & 3));
                }
            }
            continue;
        }
        const Taps t = taps_of(m, x0 + (unsigned)k, y);
        const bool in0 = inside(t.iy, h), in1 = inside(t.iy + 1, h);
        const uint8_t* row0 = src + (size_t)(in0 ? t.iy : 0) * src_row_bytes;
        const uint8_t* row1 = src + (size_t)(in1 ? t.iy + 1 : 0) * src_row_bytes;
        if (kFormat == LR_PIX_U8) {
            uint32_t a, bb, c, d;
            pair_u8(row0, in0, t.ix, w, a, bb);
            pair_u8(row1, in1, t.ix, w, c, d);
            res_u8 |= blend_u8(a, bb, c, d, t) << (8 * k);
        } else if (kFormat == LR_PIX_U8X3) {
            const bool ia = inside(t.ix, w), ib = inside(t.ix + 1, w);
            const size_t oa = (size_t)(ia ? t.ix : 0) * 3, ob = (size_t)(ib ? t.ix + 1 : 0) * 3;
            const uint32_t p00 = tap_u8x3(row0 + oa, in0 && ia), p01 = tap_u8x3(row0 + ob, in0 && ib);
            const uint32_t p10 = tap_u8x3(row1 + oa, in1 && ia), p11 = tap_u8x3(row1 + ob, in1 && ib);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int s = 8 * ch;
                const uint32_t v = blend_u8((p00 >> s) & 0xFFu, (p01 >> s) & 0xFFu, (p10 >> s) & 0xFFu, (p11 >> s) & 0xFFu, t);
                const int byte = 3 * k + ch;  // byte of the lane's twelve
                res_rgb[byte >> 2] |= v << (8 * (byte & 3));
            }
        } else {
            float a, bb, c, d;
            pair_f32(row0, in0, t.ix, w, a, bb);
            pair_f32(row1, in1, t.ix, w, c, d);
            const float f00 = (float)t.w00 / 1024.0f, f01 = (float)t.w01 / 1024.0f;
            const float f10 = (float)t.w10 / 1024.0f, f11 = (float)t.w11 / 1024.0f;
            res_f[k] = ((a * f00 + bb * f01) + c * f10) + d * f11;
        }
    }

    if (kFormat == LR_PIX_U8) {
        uint8_t* p = out + x0;
        if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(p) = res_u8;
        } else {
            for (int k = 0; k < n; ++k) p[k] = (uint8_t)(res_u8 >> (8 * k));
        }
    } else if (kFormat == LR_PIX_U8X3) {
        uint8_t* p = out + (size_t)x0 * 3;
        if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
            uint32_t* q = reinterpret_cast<uint32_t*>(p);
            q[0] = res_rgb[0];
            q[1] = res_rgb[1];
            q[2] = res_rgb[2];
        } else {
            for (int k = 0; k < 3 * n; ++k) p[k] = (uint8_t)(res_rgb[k >> 2] >> (8 * (k & 3)));
        }
    } else {
        float* p = reinterpret_cast<float*>(out) + x0;
        if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
            *reinterpret_cast<float4*>(p) = make_float4(res_f[0], res_f[1], res_f[2], res_f[3]);
        } else {
            for (int k = 0; k < n; ++k) p[k] = res_f[k];
        }
    }
}

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
        warp_lane<kFormat, kCubic>(g.M + (size_t)b * 9, src, g.src_row_bytes, g.w, g.h, out, g.ow, x0, y);
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
        warp_lane<kFormat, kCubic>(f->m, src, (size_t)f->src_row_bytes, f->w, f->h, out, ow, x0, y);
    }
}

// The table kernel's launch: records, then the tiles' prefix table, go up in the mirror of the maps (in doubles: 18 a
// frame + the table's ints)
int launch_ragged(lr_context* c, const void* d_src, int format, bool cubic, const std::vector<RaggedFrame>& rec,
                  const std::vector<int>& start, void* d_dst) {
    const size_t batch = rec.size(), rec_doubles = batch * 18;
    const int64_t n_tiles = start[batch];
    LR_HIP(hipSetDevice(c->device));
    if (upload_reserve(c, c->warp_m, c->ev_warp_m, rec_doubles + (batch + 2) / 2)) return 1;
    std::memcpy(c->warp_m.h, rec.data(), rec_doubles * sizeof(double));
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
    launch_by_format_and_rule(format, cubic, [&](auto fmt, auto rule) {
        hipLaunchKernelGGL((warp_ragged_kernel<decltype(fmt)::value, decltype(rule)::value>), dim3(grid), dim3(kBlock), 0, c->stream, g, frames, tile_start, dst);
    });
    LR_HIP(hipGetLastError());
    return 0;
}

// lr_warp_perspective_device with LR_WARP_PACKED: M is the table of 13 doubles per frame, out_width x out_height bound the
// frames' sizes and dst_image_bytes is the size of the whole destination region
int warp_packed(lr_context* c, const void* d_src, size_t src_image_bytes, int batch, int width, int height, size_t src_row_bytes,
                int format, bool cubic, const double* T, void* d_dst, size_t dst_bytes, int out_width, int out_height,
                size_t dst_row_bytes) {
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
    for (int b = 0; b < batch; ++b) {
        const double* t = T + (size_t)b * 13;
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
        start[(size_t)b] = (int)n_tiles;
        n_tiles += (int64_t)f.tiles_x * (int64_t)((oh + kTileH - 1) / kTileH);
        if (n_tiles > 0x7FFFFFF0ll) return fail("output larger than 2^31 tiles of 64 x 16 pixels");
    }
    start[(size_t)batch] = (int)n_tiles;
    if (extents_overlap(extent)) return fail("two frames' extents overlap");
    return launch_ragged(c, d_src, format, cubic, rec, start, d_dst);
}

// lr_warp_perspective_device with LR_WARP_RAGGED: M is the table of 18 doubles per frame, width x height and out_width x
// out_height bound the frames' sizes, src_image_bytes and dst_image_bytes are the sizes of the two regions
int warp_ragged(lr_context* c, const void* d_src, size_t src_bytes, int batch, int width, int height, size_t src_row_bytes,
                int format, bool cubic, const double* T, void* d_dst, size_t dst_bytes, int out_width, int out_height,
                size_t dst_row_bytes) {
    std::vector<RaggedEntry> e;
    int64_t n_tiles = 0;
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
        start[(size_t)b] = tiles;
        tiles += f.tiles_x * (int)((s.oh + kTileH - 1) / kTileH);
    }
    start[(size_t)batch] = tiles;
    return launch_ragged(c, d_src, format, cubic, rec, start, d_dst);
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
        format &= ~LR_WARP_CUBIC;
    }
    if (format & LR_WARP_JPEG_DECODE) {  // lr_decode_jpeg_device (kernels_jpeg_decode.hip): its own arguments arrive behind M
        // (LR_JPEG_ANY_SAMPLING is the decoder's own option and travels on with the format)
        if ((format & ~(0xFF | LR_JPEG_ANY_SAMPLING)) != LR_WARP_JPEG_DECODE) return fail("LR_WARP_JPEG_DECODE together with another option bit");
        if (width != 0 || height != 0 || src_row_bytes != 0 || out_width != 0 || out_height != 0 || dst_row_bytes != 0)
            return fail("LR_WARP_JPEG_DECODE: width, height, out_width, out_height and the row strides must be 0 (they are in the frame table)");
        if (!M) return fail("LR_WARP_JPEG_DECODE: null pointer (lr_jpeg_decode_args)");
        const lr_jpeg_decode_args* a = reinterpret_cast<const lr_jpeg_decode_args*>(M);
        // (probe mode, d_dst == NULL, needs no context)
        return ctx_decode_jpeg(c, d_src, a->h_src, src_image_bytes, format & (0xFF | LR_JPEG_ANY_SAMPLING), a->frames, batch, d_dst, dst_image_bytes, a->info);
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
    if (format & LR_WARP_RAGGED) {  // every frame its own source and output: one table for the warp and the prepare step
        const int opts = format & ~0xFF;
        if (opts & LR_WARP_PACKED) return fail("LR_WARP_RAGGED together with LR_WARP_PACKED (ragged outputs are always packed)");
        if (opts == LR_WARP_RAGGED)
            return warp_ragged(c, d_src, src_image_bytes, batch, width, height, src_row_bytes, format & 0xFF, cubic, M, d_dst,
                               dst_image_bytes, out_width, out_height, dst_row_bytes);
        if (opts == (LR_WARP_RAGGED | LR_WARP_PREPARE))
            return ctx_prepare_ragged(c, d_src, src_image_bytes, batch, width, height, src_row_bytes, format & 0xFF, M, d_dst,
                                      dst_image_bytes, out_width, out_height, dst_row_bytes);
        return fail("unknown option bits in format");
    }
    if (format & ~0xFF) {  // option bits above the pixel format
        if ((format & ~0xFF) == LR_WARP_PACKED)
            return warp_packed(c, d_src, src_image_bytes, batch, width, height, src_row_bytes, format & 0xFF, cubic, M, d_dst,
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
    for (size_t i = 0; i < (size_t)batch * 9; ++i)
        if (!std::isfinite(M[i])) return fail("M is not finite");
    const int64_t tiles_x = ((int64_t)out_width + kTileW - 1) / kTileW, tiles_y = ((int64_t)out_height + kTileH - 1) / kTileH;
    const int64_t n_tiles = tiles_x * tiles_y * (int64_t)batch;
    if (n_tiles > 0x7FFFFFF0ll) return fail("output larger than 2^31 tiles of 64 x 16 pixels");

    LR_HIP(hipSetDevice(c->device));
    if (upload_reserve(c, c->warp_m, c->ev_warp_m, (size_t)batch * 9)) return 1;
    std::memcpy(c->warp_m.h, M, (size_t)batch * 9 * sizeof(double));
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
