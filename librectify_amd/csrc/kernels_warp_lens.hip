// LR_WARP_LENS: the perspective warp's kernels with a lens model per frame (kernels_warp.hip has the layout of tiles and
// records, warp_lane.h the lane body and the rule).  A translation unit and so a code object of their own: a process that never
// sets the bit loads the warp's code as it was.
//
// The lens costs a pixel about twenty fp64 operations and two fp64 divisions between the perspective divide and the rounding
// to 5-bit coordinates; nothing behind the coordinates changes.  The nine values and the flag are the frame's, so uniform
// across the workgroup: they come in by scalar loads, and the branch on the flag (a frame without a lens takes the plain rule)
// does not diverge.
#include "warp_lane.h"

namespace lramd {
namespace {

// warp_ragged_kernel with a lens record per frame beside its RaggedFrame; kBorder: with the record's border rule as
// warp_ragged_border_kernel.  All three layouts come through here, the plain one with records the host makes.
template <int kFormat, bool kCubic, bool kBorder>
__global__ __launch_bounds__(kBlock) void warp_ragged_lens_kernel(RaggedArgs g, const RaggedFrame* __restrict__ frames,
                                                                  const LensRecord* __restrict__ lenses,
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
        warp_lane<kFormat, kCubic, kBorder, true>(f->m, src, (size_t)f->src_row_bytes, f->w, f->h, out, ow, x0, y, f->border_mode,
                                                  f->border_value, lenses + b);
    }
}

}  // namespace

void launch_warp_ragged_lens(int format, bool cubic, bool border, int grid, hipStream_t stream, const uint8_t* src, int batch,
                             int n_tiles, const void* frames, const void* lenses, const int* start, uint8_t* dst) {
    RaggedArgs g;
    g.src = src;
    g.batch = batch;
    g.n_tiles = n_tiles;
    launch_by_format_and_rule(format, cubic, [&](auto fmt, auto rule) {
        constexpr int kFormat = decltype(fmt)::value;
        constexpr bool kCubic = decltype(rule)::value;
        if (border)
            hipLaunchKernelGGL((warp_ragged_lens_kernel<kFormat, kCubic, true>), dim3(grid), dim3(kBlock), 0, stream, g,
                               static_cast<const RaggedFrame*>(frames), static_cast<const LensRecord*>(lenses), start, dst);
        else
            hipLaunchKernelGGL((warp_ragged_lens_kernel<kFormat, kCubic, false>), dim3(grid), dim3(kBlock), 0, stream, g,
                               static_cast<const RaggedFrame*>(frames), static_cast<const LensRecord*>(lenses), start, dst);
    });
}

}  // namespace lramd
