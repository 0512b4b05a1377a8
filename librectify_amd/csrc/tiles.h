// What the image kernels (warp, prepare, overlay, JPEG transform) share on the device: which tiles a workgroup takes, and
// which frame of a batch a tile belongs to.  Both depend on the workgroup alone, so everything here is uniform across its
// lanes and compiles to scalar loads and compares.
#pragma once
#include <hip/hip_runtime.h>

namespace lramd {

// XCD band order.  Workgroups are dealt to the eight XCDs round-robin; the tiles, in their flat order, are cut into eight
// contiguous runs of per_xcd = ceil(n_tiles / 8), and the workgroups of XCD x take the tiles [x per_xcd, (x + 1) per_xcd)
// between them, so each XCD's L2 holds one band of the pictures.  The launcher makes the grid a multiple of eight; a grid
// smaller than the tile list makes every workgroup loop over its run.
//
//     XcdBand band(n_tiles);
//     for (int tile; band.next(&tile);) { ... }
struct XcdBand {
    int base, count, j, slots;  // the run's first tile and length; this workgroup's next tile in it and its stride
    __device__ __forceinline__ explicit XcdBand(int n_tiles) {
        const int per_xcd = (n_tiles + 7) / 8;
        base = (int)(blockIdx.x & 7u) * per_xcd;
        count = min(per_xcd, n_tiles - base);  // (the last runs may be short or empty)
        j = (int)(blockIdx.x >> 3);
        slots = (int)(gridDim.x >> 3);
    }
    __device__ __forceinline__ bool next(int* tile) {
        if (j >= count) return false;
        *tile = base + j;
        j += slots;
        return true;
    }
};

// The frame b whose tiles (or groups, or intervals) include `tile`: start[b] <= tile < start[b + 1], start holding batch + 1
// ascending entries.  `start` is restrict-qualified all the way from the kernel's argument: no store can change it, so
// its reads stay scalar loads.
__device__ __forceinline__ int frame_of_tile(const int* __restrict__ start, int batch, int tile) {
    int b = 0, hi = batch;
    while (hi - b > 1) {
        const int mid = (b + hi) >> 1;
        if (start[mid] <= tile) b = mid;
        else hi = mid;
    }
    return b;
}

}  // namespace lramd
