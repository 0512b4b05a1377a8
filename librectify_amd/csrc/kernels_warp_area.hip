// LR_WARP_AREA: the perspective warp's kernels that average S x S samples per destination pixel (kernels_warp.hip has the
// layout of tiles and records, warp_lane.h the per-pixel rules).  A translation unit and so a code object of their own: a
// process that never sets the bit loads the warp's code as it was.
//
// The rule: sub-sample (i, j) of destination pixel (x, y) is the pixel (S x + i, S y + j) of
// the warp without the bit under the frame's fine map F, rounded as that warp rounds it; the pixel is the rounded mean of the
// S^2 bytes (u8, u8x3) or their float sum in the order j outer, i inner, divided by S^2 (f32).
//
// A workgroup of a frame with S > 1 takes the plain warp's 64 x 16 tile of the FINE picture, a lane four consecutive fine
// pixels of a row, exactly as the plain kernel does: neighbouring lanes read neighbouring source pixels, so the taps come in as
// coalesced as they do there.  The samples go to LDS (a dword each), and after a barrier one lane per destination pixel sums its
// S x S block in the rule's order and stores the pixel.  The tile holds (64 / S) x (16 / S) whole destination pixels; the fine
// columns and rows beyond them (S = 3, 5, 6, 7) stay idle.  The host counts a frame's tiles by that size (area_tile below).
// Two LDS buffers alternate tile by tile, so one barrier a tile is enough: a wave that runs ahead fills the other buffer and
// waits at the next barrier before anybody overwrites this one.  S and with it the whole path are the frame's and so uniform
// across the workgroup.  A frame with S = 1 in the same launch is warp_lane's own tile, lane for lane, with the record's border
// rule: a zero word is the zero border.
#include "warp_lane.h"

namespace lramd {
namespace {

// warp_ragged_kernel with an area record per frame beside its RaggedFrame and (kLens) its LensRecord.  All three layouts come
// through here, the plain one with records the host makes.  (S x + i, S y + j) fits an unsigned: the host refuses a frame
// whose S * ow or S * oh is above 2^31 - 1.
template <int kFormat, bool kCubic, bool kLens>
__global__ __launch_bounds__(kBlock) void warp_ragged_area_kernel(RaggedArgs g, const RaggedFrame* __restrict__ frames,
                                                                  const LensRecord* __restrict__ lenses,
                                                                  const AreaRecord* __restrict__ areas,
                                                                  const int* __restrict__ start, uint8_t* __restrict__ dst) {
    constexpr int kChannels = kFormat == LR_PIX_U8X3 ? 3 : 1;
    __shared__ uint32_t fine[2][kTileH][kTileW];  // a sample each: a byte, bytes r | g << 8 | b << 16, or a float's bits
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const unsigned lx = (unsigned)lane & 15u, row_in_tile = (unsigned)(wave * 4 + (lane >> 4));
    unsigned turn = 0;
    XcdBand band(g.n_tiles);
    for (int tile; band.next(&tile);) {
        const int b = frame_of_tile(start, g.batch, tile);
        const RaggedFrame* f = frames + b;
        const AreaRecord* a = areas + b;
        const LensRecord* lens = kLens ? lenses + b : nullptr;
        const int ow = f->ow, oh = f->oh, tiles_x = f->tiles_x;
        const int r = tile - start[b];
        const int ty = r / tiles_x, tx = r - ty * tiles_x;
        const uint8_t* src = g.src + (size_t)f->src_offset;
        const size_t src_row_bytes = (size_t)f->src_row_bytes;
        const unsigned S = (unsigned)a->s;
        if (S == 1u) {  // the plain rule, warp_lane's tile (a->f is the frame's map itself)
            const unsigned y = (unsigned)ty * kTileH + row_in_tile;
            const unsigned x0 = (unsigned)tx * kTileW + lx * 4u;
            if (y >= (unsigned)oh || x0 >= (unsigned)ow) continue;
            uint8_t* out = dst + (size_t)f->offset + (size_t)y * (size_t)f->row_bytes;
            warp_lane<kFormat, kCubic, true, kLens>(a->f, src, src_row_bytes, f->w, f->h, out, ow, x0, y, f->border_mode, f->border_value, lens);
            continue;
        }
        const int w = f->w, h = f->h, mode = f->border_mode;
        const uint32_t value = f->border_value;
        const unsigned dw = (unsigned)kTileW / S, dh = (unsigned)kTileH / S;  // destination pixels of a tile
        const unsigned by_s = (65536u + S - 1u) / S;  // (n * by_s) >> 16 is n / S for n < 64 (the error n (by_s - 65536 / S) / 65536 stays below 1 / S)
        uint32_t (*buf)[kTileW] = fine[turn & 1u];
        ++turn;

        // a lane's four fine pixels: columns lx * 4 .. + 3 of row row_in_tile of the tile's fine picture
        const unsigned dy = (unsigned)ty * dh + ((row_in_tile * by_s) >> 16);
        const bool row_on = row_in_tile < dh * S && dy < (unsigned)oh;
        const unsigned sy = (unsigned)ty * dh * S + row_in_tile;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned fx = lx * 4u + (unsigned)k;
            const unsigned dx = (unsigned)tx * dw + ((fx * by_s) >> 16);
            if (row_on && fx < dw * S && dx < (unsigned)ow) {
                const unsigned sx = (unsigned)tx * dw * S + fx;
                uint32_t px;
                float pf;
                if constexpr (kCubic) cubic_pixel<kFormat, true, kLens>(a->f, src, src_row_bytes, w, h, sx, sy, mode, value, px, pf, lens);
                else border_linear_pixel<kFormat, kLens>(a->f, src, src_row_bytes, w, h, sx, sy, mode, value, px, pf, lens);
                buf[row_in_tile][fx] = kFormat == LR_PIX_F32 ? __float_as_uint(pf) : px;
            }
        }
        __syncthreads();

        // one lane per destination pixel of the tile: its S x S block, j outer and i inner
        const unsigned t = threadIdx.x;
        const unsigned by_dw = (65536u + dw - 1u) / dw;  // (t * by_dw) >> 16 is t / dw for t < 256 (dw <= 32)
        const unsigned qy = (t * by_dw) >> 16, qx = t - qy * dw;
        const unsigned x = (unsigned)tx * dw + qx, y = (unsigned)ty * dh + qy;
        if (qy < dh && x < (unsigned)ow && y < (unsigned)oh) {
            const unsigned s2 = S * S;
            uint8_t* out = dst + (size_t)f->offset + (size_t)y * (size_t)f->row_bytes;
            if constexpr (kFormat == LR_PIX_F32) {
                float acc = 0.0f;
                for (unsigned j = 0; j < S; ++j)
                    for (unsigned i = 0; i < S; ++i) acc = acc + __uint_as_float(buf[qy * S + j][qx * S + i]);
                reinterpret_cast<float*>(out)[x] = acc / (float)s2;
            } else {
                uint32_t sum[kChannels];  // at most 64 * 255
#pragma unroll
                for (int ch = 0; ch < kChannels; ++ch) sum[ch] = 0;
                for (unsigned j = 0; j < S; ++j) {
                    for (unsigned i = 0; i < S; ++i) {
                        const uint32_t v = buf[qy * S + j][qx * S + i];
#pragma unroll
                        for (int ch = 0; ch < kChannels; ++ch) sum[ch] += (v >> (8 * ch)) & 0xFFu;
                    }
                }
#pragma unroll
                for (int ch = 0; ch < kChannels; ++ch) out[(size_t)x * kChannels + ch] = (uint8_t)((2u * sum[ch] + s2) / (2u * s2));
            }
        }
    }
}

}  // namespace

void launch_warp_ragged_area(int format, bool cubic, int grid, hipStream_t stream, const uint8_t* src, int batch, int n_tiles,
                             const void* frames, const void* lenses, const void* areas, const int* start, uint8_t* dst) {
    RaggedArgs g;
    g.src = src;
    g.batch = batch;
    g.n_tiles = n_tiles;
    launch_by_format_and_rule(format, cubic, [&](auto fmt, auto rule) {
        constexpr int kFormat = decltype(fmt)::value;
        constexpr bool kCubic = decltype(rule)::value;
        if (lenses)
            hipLaunchKernelGGL((warp_ragged_area_kernel<kFormat, kCubic, true>), dim3(grid), dim3(kBlock), 0, stream, g,
                               static_cast<const RaggedFrame*>(frames), static_cast<const LensRecord*>(lenses),
                               static_cast<const AreaRecord*>(areas), start, dst);
        else
            hipLaunchKernelGGL((warp_ragged_area_kernel<kFormat, kCubic, false>), dim3(grid), dim3(kBlock), 0, stream, g,
                               static_cast<const RaggedFrame*>(frames), static_cast<const LensRecord*>(lenses),
                               static_cast<const AreaRecord*>(areas), start, dst);
    });
}

}  // namespace lramd
