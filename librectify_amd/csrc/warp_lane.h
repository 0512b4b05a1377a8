// The lane body of the perspective warp, shared by its two translation units: kernels_warp.hip (the kernels of a call without
// LR_WARP_BORDER and all host code) and kernels_warp_border.hip (the kernels with a border rule per frame).  The bordered
// kernels are a code object of their own, so that the one kernels_warp.hip makes holds exactly the kernels it held before them.
// kernels_warp_lens.hip (the kernels with a lens model per frame, LR_WARP_LENS) is a third of the same kind.
// kernels_warp_area.hip (the kernels that average S x S samples per destination pixel, LR_WARP_AREA) is a fourth.
// kernels_warp_lens_model.hip (the kernels with a lens of seventeen entries per frame, LR_WARP_LENS_MODEL) is a fifth.
// Everything here has internal linkage; what kernels_warp.hip says about tiles, records and loads holds for all of them.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "tables.h"
#include "tiles.h"

namespace lramd {

// warp_ragged_border_kernel's launch (kernels_warp_border.hip): the arguments of warp_ragged_kernel's, `frames` the device
// array of RaggedFrame records
void launch_warp_ragged_border(int format, bool cubic, int grid, hipStream_t stream, const uint8_t* src, int batch, int n_tiles,
                               const void* frames, const int* start, uint8_t* dst);

// warp_ragged_lens_kernel's launch (kernels_warp_lens.hip): the same arguments, `lenses` the device array of LensRecord
// records, one per frame; `border`: with the records' border rules
void launch_warp_ragged_lens(int format, bool cubic, bool border, int grid, hipStream_t stream, const uint8_t* src, int batch,
                             int n_tiles, const void* frames, const void* lenses, const int* start, uint8_t* dst);

// warp_ragged_area_kernel's launch (kernels_warp_area.hip): the same arguments, `areas` the device array of AreaRecord records,
// one per frame; `lenses` NULL: no frame has a lens; the records' border rules always hold (a zero word is the zero border)
void launch_warp_ragged_area(int format, bool cubic, int grid, hipStream_t stream, const uint8_t* src, int batch, int n_tiles,
                             const void* frames, const void* lenses, const void* areas, const int* start, uint8_t* dst);

// the launch of kernels_warp_lens_model.hip's kernels (LR_WARP_LENS_MODEL): `lenses` the device array of LensModelRecord
// records, one per frame; `areas` NULL: warp_ragged_lens_model_kernel (`border`: with the records' border rules), otherwise
// warp_ragged_area_lens_model_kernel with the AreaRecord records, for which the border rules always hold
void launch_warp_ragged_lens_model(int format, bool cubic, bool border, int grid, hipStream_t stream, const uint8_t* src, int batch,
                                   int n_tiles, const void* frames, const void* lenses, const void* areas, const int* start,
                                   uint8_t* dst);

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
    int ow, oh, tiles_x, w, h;
    int border_mode;        // LR_WARP_BORDER: the frame's mode and value (0, 0 without the bit)
    unsigned border_value;
    int pad[3];
};
static_assert(sizeof(RaggedFrame) == 18 * sizeof(double), "a record per 18 doubles of the mirror");

// LR_WARP_LENS: a frame's lens, the nine doubles of its table row (fx, fy, cx, cy, k1, k2, p1, p2, k3), and whether any of
// the five coefficients is not zero; a frame without one is warped by the plain rule
struct LensRecord {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
    int has_lens;
    int pad;
};
static_assert(sizeof(LensRecord) == 10 * sizeof(double), "a record per 10 doubles of the mirror");

// LR_WARP_LENS_MODEL: a frame's lens of seventeen entries, the doubles of its table row (OpenCV's order of distCoeffs behind the
// camera matrix, then the model), and what the host made of them: kLensNone (model 0 with [4..15] all zero: the plain rule),
// kLensRational or kLensFisheye
struct LensModelRecord {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, model;
    int kind;
    int pad;
};
static_assert(sizeof(LensModelRecord) == 18 * sizeof(double), "a record per 18 doubles of the mirror");
enum : int { kLensNone = 0, kLensRational = 1, kLensFisheye = 2 };

// the lens argument of the lane body: kLens 0: none (never looked at), 1: a LensRecord, 2: a LensModelRecord
template <int kLens>
struct LensOf {
    using type = LensRecord;
};
template <>
struct LensOf<2> {
    using type = LensModelRecord;
};

// LR_WARP_AREA: a frame's sampling factor S (1 .. 8) and its fine map F (lr_area_fine_map of the frame's M and S; S = 1: M)
struct AreaRecord {
    double f[9];
    int s;
    int pad;
};
static_assert(sizeof(AreaRecord) == 10 * sizeof(double), "a record per 10 doubles of the mirror");

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

// LR_WARP_LENS (tests/numpy_warp_lens_ref.py): the displacement, in 1/32 pixels, that the
// frame's lens adds to the ideal point (U, V) (1/32 pixels as well), every operation rounded on its own.  The two divisions
// stay divisions: the rule says so, and a reciprocal would round differently.
__device__ __forceinline__ void lens_displace(const LensRecord* __restrict__ l, double& U, double& V) {
    const double a = (U * 0.03125 - l->cx) / l->fx, b = (V * 0.03125 - l->cy) / l->fy;
    const double aa = a * a, bb = b * b, ab = a * b;
    const double r2 = aa + bb;
    const double rad = r2 * (l->k1 + r2 * (l->k2 + r2 * l->k3));
    const double ta = (2.0 * l->p1) * ab + l->p2 * (r2 + 2.0 * aa);
    const double tb = l->p1 * (r2 + 2.0 * bb) + (2.0 * l->p2) * ab;
    const double du = l->fx * (a * rad + ta), dv = l->fy * (b * rad + tb);
    U = U + 32.0 * du;
    V = V + 32.0 * dv;
}

// ---- LR_WARP_LENS_MODEL (tests/numpy_warp_lens_model_ref.py) ----

// The rule's arctangent of r >= 0, out of + - * /, comparisons and one rint, so that the device, the header's lr_lens_atan and
// the NumPy reference run it operation for operation: r > 1 is reflected (pi/2 - ATAN(1 / r)); t in [0, 1] is reduced by the
// nearest of the nine points c = i / 8 (z = (t - c) / (1 + t c), |z| <= 1/16), and ATAN(t) = atan(c) + (z + z (z^2 p(z^2))), p the
// series -1/3 + z^2 / 5 - ... - z^14 / 15.  A NaN takes entry 0 of the table and stays a NaN.  Out of line: one copy a kernel
// instead of one per pixel of a lane's unrolled four (the frame's model is uniform, so the call does not diverge).
__device__ __noinline__ double lens_atan(double r) {
    static constexpr double kAtan[9] = {0x0.0p+0,
                                        0x1.fd5ba9aac2f6ep-4,
                                        0x1.f5b75f92c80ddp-3,
                                        0x1.6f61941e4def1p-2,
                                        0x1.dac670561bb4fp-2,
                                        0x1.1e00babdefeb4p-1,
                                        0x1.4978fa3269ee1p-1,
                                        0x1.700a7c5784634p-1,
                                        0x1.921fb54442d18p-1};
    const bool big = r > 1.0;
    const double t = big ? 1.0 / r : r;
    const double n = rint(8.0 * t);
    const int i = n >= 0.0 && n <= 8.0 ? (int)n : 0;
    const double c = (double)i / 8.0;
    const double z = (t - c) / (1.0 + t * c);
    const double z2 = z * z;
    const double p = -1.0 / 3.0 + z2 * (1.0 / 5.0 + z2 * (-1.0 / 7.0 + z2 * (1.0 / 9.0 + z2 * (-1.0 / 11.0 + z2 * (1.0 / 13.0 + z2 * (-1.0 / 15.0))))));
    const double at = kAtan[i] + (z + z * (z2 * p));
    return big ? 0x1.921fb54442d18p+0 - at : at;
}

// the point (U, V) of the ideal picture (1/32 pixels) through the frame's lens of seventeen entries: model 0 as a displacement,
// like lens_displace; model 1 (the fisheye) has no displacement form.  Divisions and the square root stay what they are.
__device__ __forceinline__ void lens_model_apply(const LensModelRecord* __restrict__ l, double& U, double& V) {
    const double a = (U * 0.03125 - l->cx) / l->fx, b = (V * 0.03125 - l->cy) / l->fy;
    const double aa = a * a, bb = b * b;
    const double r2 = aa + bb;
    if (l->kind == kLensFisheye) {
        const double r = __dsqrt_rn(r2);
        const double th = lens_atan(r);
        const double t2 = th * th;
        const double thd = th * (1.0 + t2 * (l->k1 + t2 * (l->k2 + t2 * (l->p1 + t2 * l->p2))));  // (entries [4..7] are the fisheye's k1..k4)
        const double sc = r != 0.0 ? thd / r : 1.0;
        U = 32.0 * (l->fx * (a * sc) + l->cx);
        V = 32.0 * (l->fy * (b * sc) + l->cy);
        return;
    }
    const double ab = a * b;
    const double radn = r2 * (l->k1 + r2 * (l->k2 + r2 * l->k3));
    const double radd = r2 * (l->k4 + r2 * (l->k5 + r2 * l->k6));
    const double rad = (radn - radd) / (1.0 + radd);
    const double ta = ((2.0 * l->p1) * ab + l->p2 * (r2 + 2.0 * aa)) + r2 * (l->s1 + r2 * l->s2);
    const double tb = (l->p1 * (r2 + 2.0 * bb) + (2.0 * l->p2) * ab) + r2 * (l->s3 + r2 * l->s4);
    const double du = l->fx * (a * rad + ta), dv = l->fy * (b * rad + tb);
    U = U + 32.0 * du;
    V = V + 32.0 * dv;
}

// the 5-bit fixed-point source coordinates of destination pixel (x, y): both sampling rules start from them; kLens: through the
// frame's lens (`lens`, uniform across the workgroup like m) where it has one; kLens 2: the lens is a LensModelRecord
template <int kLens = 0>
__device__ __forceinline__ void fixed_xy(const double* __restrict__ m, unsigned x, unsigned y, int& X, int& Y,
                                         const typename LensOf<kLens>::type* __restrict__ lens = nullptr) {
    const double xd = (double)x, yd = (double)y;
    const double W0 = (m[6] * xd + m[7] * yd) + m[8];
    const double Wq = W0 != 0.0 ? 32.0 / W0 : 0.0;
    if constexpr (kLens != 0) {
        double U = ((m[0] * xd + m[1] * yd) + m[2]) * Wq, V = ((m[3] * xd + m[4] * yd) + m[5]) * Wq;
        if constexpr (kLens == 2) {
            if (lens->kind != kLensNone) lens_model_apply(lens, U, V);
        } else {
            if (lens->has_lens) lens_displace(lens, U, V);
        }
        X = fixed_coord(U);
        Y = fixed_coord(V);
    } else {
        X = fixed_coord(((m[0] * xd + m[1] * yd) + m[2]) * Wq);
        Y = fixed_coord(((m[3] * xd + m[4] * yd) + m[5]) * Wq);
    }
}

template <int kLens = 0>
__device__ __forceinline__ Taps taps_of(const double* __restrict__ m, unsigned x, unsigned y, const typename LensOf<kLens>::type* __restrict__ lens = nullptr) {
    int X, Y;
    fixed_xy<kLens>(m, x, y, X, Y, lens);
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

// ---- LR_WARP_BORDER: what a tap outside the source contributes (tests/numpy_warp_border_ref.py) ----

enum : int { kBorderConstant = 0, kBorderReplicate = 1, kBorderReflect = 2, kBorderReflect101 = 4 };

// OpenCV's borderInterpolate for replicate, reflect and reflect-101 in closed form: coordinate p (|p| <= 2^26 + 2, what the
// 5-bit coordinates can yield) of an axis of n >= 1 pixels becomes an index in [0, n).  One fold serves the period around the
// source; only beyond it is the remainder taken (then n <= |p|, so the period 2 n fits an int with room to spare).  The last
// clamp changes nothing and makes the promise unconditional: whatever comes out is inside [0, n).
__device__ __forceinline__ int border_index(int p, int n, int mode) {
    if (inside(p, n)) return p;
    if (mode == kBorderReplicate) return p < 0 ? 0 : n - 1;
    if (n == 1) return 0;
    const int d = mode == kBorderReflect ? 1 : 0;        // reflect repeats the edge pixel, reflect-101 does not
    int q = p < 0 ? -p - d : (n - 1) + (n - 1) + d - p;  // the fold about the edge that p is beyond
    if (!inside(q, n)) {
        const int period = 2 * n - 2 + 2 * d;
        q = p % period;
        if (q < 0) q += period;
        if (q >= n) q = period - d - q;
    }
    return min(max(q, 0), n - 1);
}

// Pixel cx (inside the row) of a source row: a u8 pixel's byte, a u8x3 pixel's bytes r | g << 8 | b << 16 or an f32 pixel's
// bits.  The constant border's `value` has the same form.
template <int kFormat>
__device__ __forceinline__ uint32_t load_tap(const uint8_t* row, int cx) {
    if constexpr (kFormat == LR_PIX_U8) return row[cx];
    else if constexpr (kFormat == LR_PIX_U8X3) return tap_u8x3(row + (size_t)cx * 3, true);
    else return __float_as_uint(reinterpret_cast<const float*>(row)[cx]);
}

// One destination pixel by the bilinear rule with a border: taps and weights are taps_of's; where all four taps are inside
// they come in as in the unbordered rule (paired loads); otherwise the constant border gives `value` for a tap outside and
// the other modes map the two columns and the two rows once (border_index) and read the four pixels they name.  `mode` is the
// frame's and uniform across the workgroup.  Result as cubic_pixel's.
template <int kFormat, int kLens = 0>
__device__ __forceinline__ void border_linear_pixel(const double* m, const uint8_t* src, size_t src_row_bytes, int w, int h,
                                                    unsigned x, unsigned y, int mode, uint32_t value, uint32_t& px, float& pf,
                                                    const typename LensOf<kLens>::type* lens = nullptr) {
    const Taps t = taps_of<kLens>(m, x, y, lens);
    uint32_t v[4];  // (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1), in border_tap's form
    if (t.ix >= 0 && t.ix + 1 < w && t.iy >= 0 && t.iy + 1 < h) {  // (|ix|, |iy| <= 2^26: no overflow)
        const uint8_t* row0 = src + (size_t)t.iy * src_row_bytes;
        const uint8_t* row1 = row0 + src_row_bytes;
        if constexpr (kFormat == LR_PIX_U8) {
            pair_u8(row0, true, t.ix, w, v[0], v[1]);
            pair_u8(row1, true, t.ix, w, v[2], v[3]);
        } else if constexpr (kFormat == LR_PIX_U8X3) {
            const size_t o = (size_t)t.ix * 3;
            v[0] = tap_u8x3(row0 + o, true);
            v[1] = tap_u8x3(row0 + o + 3, true);
            v[2] = tap_u8x3(row1 + o, true);
            v[3] = tap_u8x3(row1 + o + 3, true);
        } else {
            float a, b, c, d;
            pair_f32(row0, true, t.ix, w, a, b);
            pair_f32(row1, true, t.ix, w, c, d);
            v[0] = __float_as_uint(a);
            v[1] = __float_as_uint(b);
            v[2] = __float_as_uint(c);
            v[3] = __float_as_uint(d);
        }
    } else {
        int cx[2] = {t.ix, t.ix + 1}, cy[2] = {t.iy, t.iy + 1};
        bool in_x[2] = {true, true}, in_y[2] = {true, true};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (mode == kBorderConstant) {
                in_x[k] = inside(cx[k], w);
                in_y[k] = inside(cy[k], h);
                cy[k] = in_y[k] ? cy[k] : 0;
            } else {
                cx[k] = border_index(cx[k], w, mode);
                cy[k] = border_index(cy[k], h, mode);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint8_t* row = src + (size_t)cy[k >> 1] * src_row_bytes;
            v[k] = in_x[k & 1] && in_y[k >> 1] ? load_tap<kFormat>(row, cx[k & 1]) : value;
        }
    }
    px = 0;
    pf = 0.f;
    if constexpr (kFormat == LR_PIX_F32) {
        const float f00 = (float)t.w00 / 1024.0f, f01 = (float)t.w01 / 1024.0f;
        const float f10 = (float)t.w10 / 1024.0f, f11 = (float)t.w11 / 1024.0f;
        pf = ((__uint_as_float(v[0]) * f00 + __uint_as_float(v[1]) * f01) + __uint_as_float(v[2]) * f10) + __uint_as_float(v[3]) * f11;
    } else {
        constexpr int kChannels = kFormat == LR_PIX_U8X3 ? 3 : 1;
#pragma unroll
        for (int ch = 0; ch < kChannels; ++ch) {
            const int s = 8 * ch;
            px |= blend_u8((v[0] >> s) & 0xFFu, (v[1] >> s) & 0xFFu, (v[2] >> s) & 0xFFu, (v[3] >> s) & 0xFFu, t) << s;
        }
    }
}

// row_taps with a border: the four horizontal taps (ix - 1 .. ix + 2) of a source row.  Constant border: `row` is the taps'
// own row (row_in: it is inside the source), cx their columns as they are, and a tap outside is `value`.  Other modes: `row`
// is the row border_index names (row_in is true) and cx the columns it names, mapped once for the pixel's four rows.  Where the
// four columns are inside the source, the row's taps come in with row_taps' one load.
template <int kFormat>
__device__ __forceinline__ void border_row_taps(const uint8_t* row, bool row_in, int ix, int w, const int (&cx)[4], bool constant,
                                                uint32_t value, uint32_t (&d)[PixelBytes<kFormat>::value]) {
    constexpr int kBpp = PixelBytes<kFormat>::value;
    if (row_in && ix >= 1 && ix + 2 < w) {
        row_taps<kFormat>(row, true, ix, w, d);
        return;
    }
#pragma unroll
    for (int i = 0; i < kBpp; ++i) d[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t t = !constant || (row_in && inside(cx[i], w)) ? load_tap<kFormat>(row, cx[i]) : value;
        if constexpr (kFormat == LR_PIX_F32) {
            d[i] = t;
        } else if constexpr (kFormat == LR_PIX_U8) {
            d[0] |= t << (8 * i);
        } else {
            const int bit = 24 * i;  // the tap's three bytes start at byte 3 i of the twelve
            d[(bit >> 5)] |= t << (bit & 31);
            if ((bit & 31) > 8) d[((bit >> 5) + 1)] |= t >> (32 - (bit & 31));
        }
    }
}

// One destination pixel by the bicubic rule: a u8 pixel's byte or a u8x3 pixel's bytes r | g << 8 | b << 16 in `px`, an
// f32 pixel in `pf`.  8-bit: h_j = sum_i C[ax][i] v(i, j), s = sum_j C[ay][j] h_j, (s + 2^21) >> 22 clamped to 0 .. 255.
// Everything fits int32: max sum |C[a]| is 2816 and 255 * 2816^2 + 2^21 = 2 024 210 432 < 2^31.  f32: weights C / 2048.f
// (exact), rows and then the column summed from the first tap to the last, every product and sum rounded on its own.
// kBorder: a row's taps come through border_row_taps (the frame's `mode` and `value`); without it the two arguments are unused.
template <int kFormat, bool kBorder, int kLens = 0>
__device__ __forceinline__ void cubic_pixel(const double* m, const uint8_t* src, size_t src_row_bytes, int w, int h, unsigned x,
                                            unsigned y, int mode, uint32_t value, uint32_t& px, float& pf,
                                            const typename LensOf<kLens>::type* lens = nullptr) {
    constexpr int kBpp = PixelBytes<kFormat>::value;
    constexpr int kChannels = kFormat == LR_PIX_U8X3 ? 3 : 1;
    int X, Y;
    fixed_xy<kLens>(m, x, y, X, Y, lens);
    const int ix = X >> 5, iy = Y >> 5;
    const int16_t* cx = kCubicWeights[X & 31];
    const int16_t* cy = kCubicWeights[Y & 31];
    const int wx[4] = {cx[0], cx[1], cx[2], cx[3]};
    const int wy[4] = {cy[0], cy[1], cy[2], cy[3]};
    int s[kChannels];
#pragma unroll
    for (int ch = 0; ch < kChannels; ++ch) s[ch] = 0;
    float hf[4];
    int cols[4] = {ix - 1, ix, ix + 1, ix + 2};  // kBorder: the taps' columns, mapped into the source unless the border is constant
    if constexpr (kBorder) {
        if (mode != kBorderConstant && !(ix >= 1 && ix + 2 < w)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) cols[i] = border_index(cols[i], w, mode);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ry = iy - 1 + j;
        uint32_t d[kBpp];
        if constexpr (kBorder) {
            const bool constant = mode == kBorderConstant;
            const bool row_in = !constant || inside(ry, h);
            const int cy = constant ? (row_in ? ry : 0) : border_index(ry, h, mode);
            border_row_taps<kFormat>(src + (size_t)cy * src_row_bytes, row_in, ix, w, cols, constant, value, d);
        } else {
            const bool row_in = inside(ry, h);
            const uint8_t* row = src + (size_t)(row_in ? ry : 0) * src_row_bytes;
            row_taps<kFormat>(row, row_in, ix, w, d);
        }
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
// kCubic: sampled by the bicubic rule above instead of the bilinear one; kBorder: with the frame's border rule (`mode`,
// `value`: LR_WARP_BORDER) instead of the constant zero one, which with kBorder false is the parent's code and ignores both;
// kLens: the coordinates go through the frame's lens (`lens`: 1 LR_WARP_LENS's record, 2 LR_WARP_LENS_MODEL's), which with
// kLens 0 is never looked at
template <int kFormat, bool kCubic, bool kBorder, int kLens = 0>
__device__ __forceinline__ void warp_lane(const double* m, const uint8_t* src, size_t src_row_bytes, int w, int h,
                                          uint8_t* out, int ow, unsigned x0, unsigned y, int mode = 0, uint32_t value = 0,
                                          const typename LensOf<kLens>::type* lens = nullptr) {
    const int n = min(4, ow - (int)x0);  // pixels of this lane inside the row

    uint32_t res_u8 = 0;          // LR_PIX_U8: four bytes
    uint32_t res_rgb[3] = {0, 0, 0};  // LR_PIX_U8X3: twelve bytes
    float res_f[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (kCubic || kBorder) {
            uint32_t px;
            if constexpr (kCubic) cubic_pixel<kFormat, kBorder, kLens>(m, src, src_row_bytes, w, h, x0 + (unsigned)k, y, mode, value, px, res_f[k], lens);
            else border_linear_pixel<kFormat, kLens>(m, src, src_row_bytes, w, h, x0 + (unsigned)k, y, mode, value, px, res_f[k], lens);
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
        const Taps t = taps_of<kLens>(m, x0 + (unsigned)k, y, lens);
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

}  // namespace
}  // namespace lramd
