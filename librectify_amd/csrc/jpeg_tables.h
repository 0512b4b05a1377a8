// The device tables that the JPEG encoder (kernels_jpeg.hip) and decoder (kernels_jpeg_decode.hip) share: the 13-bit DCT
// matrix and the zig-zag order.  Every translation unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lramd {
namespace {

// T[u][x] = round(2^13 c(u) / 2 cos((2x + 1) u pi / 16)) for x < 4; T[u][7 - x] = (-1)^u T[u][x]
__device__ constexpr int kDctHalf[8][4] = {{2896, 2896, 2896, 2896},  {4017, 3406, 2276, 799},  {3784, 1567, -1567, -3784},
                                           {3406, -799, -4017, -2276}, {2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406},
                                           {1567, -3784, 3784, -1567}, {799, -2276, 3406, -4017}};
// zig-zag position -> natural index: one list, for the device and (kZigzagOrder) for the host's header parser
#define LR_JPEG_ZIGZAG                                                                                                  \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
__device__ const uint8_t kZigzag[64] = LR_JPEG_ZIGZAG;
constexpr uint8_t kZigzagOrder[64] = LR_JPEG_ZIGZAG;

}  // namespace
}  // namespace lramd
