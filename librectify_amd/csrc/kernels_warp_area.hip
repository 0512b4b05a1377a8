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
#include "warp_area_tiles.h"

namespace lramd {
namespace {

// warp_ragged_kernel with an area record per frame beside its RaggedFrame and (kLens) its LensRecord.  All three layouts come
// through here, the plain one with records the host makes.
template <int kFormat, bool kCubic, bool kLens>
__global__ __launch_bounds__(kBlock) void warp_ragged_area_kernel(RaggedArgs g, const RaggedFrame* __restrict__ frames,
                                                                  const LensRecord* __restrict__ lenses,
                                                                  const AreaRecord* __restrict__ areas,
                                                                  const int* __restrict__ start, uint8_t* __restrict__ dst) {
    __shared__ uint32_t fine[2][kTileH][kTileW];  // a sample each: a byte, bytes r | g << 8 | b << 16, or a float's bits
    area_tiles<kFormat, kCubic, kLens ? 1 : 0>(g, frames, lenses, areas, start, dst, fine);  // (warp_area_tiles.h)
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
