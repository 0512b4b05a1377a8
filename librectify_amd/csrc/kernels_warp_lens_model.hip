// LR_WARP_LENS_MODEL: the perspective warp's kernels with a lens of seventeen entries per frame, OpenCV's rational and
// thin-prism model or cv::fisheye's equidistant one (kernels_warp.hip has the layout of tiles and records, warp_lane.h the lane
// body and the rule, warp_area_tiles.h LR_WARP_AREA's tile loop).  A translation unit and so a code object of their own: a
// process that never sets the bit, or whose lenses all fit LR_WARP_LENS's nine entries, loads the warp's code as it was.
//
// Model 0 costs a pixel about forty fp64 operations and three fp64 divisions between the perspective divide and the rounding to
// 5-bit coordinates; the fisheye five divisions (two in its arctangent), a square root and about forty operations.  The
// seventeen values and the frame's kind are the frame's, so uniform across the workgroup: they come in by scalar loads, and the
// branches on the kind (no lens: the plain rule; rational; fisheye) do not diverge.  The arctangent stays out of line
// (warp_lane.h, lens_atan): a call, not a copy per pixel of the lane's four; no instantiation uses scratch.
#include "warp_area_tiles.h"

namespace lramd {
namespace {

// warp_ragged_lens_kernel with a LensModelRecord per frame in place of the LensRecord: the same tiles, XCD bands and prefix
// search.  All three layouts come through here, the plain one with records the host makes.
template <int kFormat, bool kCubic, bool kBorder>
__global__ __launch_bounds__(kBlock) void warp_ragged_lens_model_kernel(RaggedArgs g, const RaggedFrame* __restrict__ frames,
                                                                        const LensModelRecord* __restrict__ lenses,
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
        warp_lane<kFormat, kCubic, kBorder, 2>(f->m, src, (size_t)f->src_row_bytes, f->w, f->h, out, ow, x0, y, f->border_mode,
                                               f->border_value, lenses + b);
    }
}

// warp_ragged_area_kernel likewise: LR_WARP_AREA over the lens of seventeen entries
template <int kFormat, bool kCubic>
__global__ __launch_bounds__(kBlock) void warp_ragged_area_lens_model_kernel(RaggedArgs g, const RaggedFrame* __restrict__ frames,
                                                                             const LensModelRecord* __restrict__ lenses,
                                                                             const AreaRecord* __restrict__ areas,
                                                                             const int* __restrict__ start, uint8_t* __restrict__ dst) {
    __shared__ uint32_t fine[2][kTileH][kTileW];  // a sample each: a byte, bytes r | g << 8 | b << 16, or a float's bits
    area_tiles<kFormat, kCubic, 2>(g, frames, lenses, areas, start, dst, fine);
}

}  // namespace

void launch_warp_ragged_lens_model(int format, bool cubic, bool border, int grid, hipStream_t stream, const uint8_t* src, int batch,
                                   int n_tiles, const void* frames, const void* lenses, const void* areas, const int* start,
                                   uint8_t* dst) {
    RaggedArgs g;
    g.src = src;
    g.batch = batch;
    g.n_tiles = n_tiles;
    launch_by_format_and_rule(format, cubic, [&](auto fmt, auto rule) {
        constexpr int kFormat = decltype(fmt)::value;
        constexpr bool kCubic = decltype(rule)::value;
        const LensModelRecord* l = static_cast<const LensModelRecord*>(lenses);
        if (areas)
            hipLaunchKernelGGL((warp_ragged_area_lens_model_kernel<kFormat, kCubic>), dim3(grid), dim3(kBlock), 0, stream, g,
                               static_cast<const RaggedFrame*>(frames), l, static_cast<const AreaRecord*>(areas), start, dst);
        else if (border)
            hipLaunchKernelGGL((warp_ragged_lens_model_kernel<kFormat, kCubic, true>), dim3(grid), dim3(kBlock), 0, stream, g,
                               static_cast<const RaggedFrame*>(frames), l, start, dst);
        else
            hipLaunchKernelGGL((warp_ragged_lens_model_kernel<kFormat, kCubic, false>), dim3(grid), dim3(kBlock), 0, stream, g,
                               static_cast<const RaggedFrame*>(frames), l, start, dst);
    });
}

}  // namespace lramd
