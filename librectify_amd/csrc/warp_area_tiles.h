// The tile loop of LR_WARP_AREA's kernels, shared by its two translation units: kernels_warp_area.hip (frames without a lens or
// with LR_WARP_LENS's nine-entry record) and kernels_warp_lens_model.hip (frames with LR_WARP_LENS_MODEL's record).  What
// kernels_warp_area.hip says about tiles, LDS and the barrier holds for both.
#pragma once
#include "warp_lane.h"

namespace lramd {
namespace {

// warp_ragged_area_kernel's body: `fine` is the kernel's LDS, two buffers of a tile's samples (a byte, bytes r | g << 8 |
// b << 16, or a float's bits each); kLens: as warp_lane's.  (S x + i, S y + j) fits an unsigned: the host refuses a frame whose
// S * ow or S * oh is above 2^31 - 1.
template <int kFormat, bool kCubic, int kLens>
__device__ __forceinline__ void area_tiles(const RaggedArgs& g, const RaggedFrame* __restrict__ frames,
                                           const typename LensOf<kLens>::type* __restrict__ lenses,
                                           const AreaRecord* __restrict__ areas, const int* __restrict__ start,
                                           uint8_t* __restrict__ dst, uint32_t (*fine)[kTileH][kTileW]) {
    constexpr int kChannels = kFormat == LR_PIX_U8X3 ? 3 : 1;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const unsigned lx = (unsigned)lane & 15u, row_in_tile = (unsigned)(wave * 4 + (lane >> 4));
    unsigned turn = 0;
    XcdBand band(g.n_tiles);
    for (int tile; band.next(&tile);) {
        const int b = frame_of_tile(start, g.batch, tile);
        const RaggedFrame* f = frames + b;
        const AreaRecord* a = areas + b;
        const typename LensOf<kLens>::type* lens = kLens ? lenses + b : nullptr;
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
}  // namespace lramd
