// Network input tensors from finished 8-bit pictures: lr_pack_tensor_device for gfx950.
//
// The pass stands behind the warp as the JPEG encoder does: it reads u8 / u8x3 pictures that lie in HBM and writes one
// contiguous batch tensor (N x C x H x W or N x H x W x C; f32, f16 or bf16), every picture letterboxed into its slot.  The
// rule is DESIGN.md section 3, item 20 (tests/numpy_tensor_ref.py gives the same bytes): an element of channel c whose level
// is v is (float)(v * scale[c] + bias[c]), the product and the sum in double, for f16 and bf16 rounded once more to nearest
// even.  There are 256 x C such elements, so the HOST computes them once per call as a table of bit patterns; the kernel
// only looks them up (a copy in LDS per workgroup) and no float arithmetic on a value runs on the device.
//
//   * A named slot is one contiguous run of C x H x W elements.  It is cut, by ABSOLUTE address, into chunks of 16 bytes (4
//     f32 or 8 half elements), and a tile is 2048 chunks (32 KB): a workgroup of 256 lanes takes a tile in 8 steps of 256
//     neighbouring chunks, so a wavefront stores 1 KB contiguous bytes a step whatever the layout.  A chunk that lies wholly
//     inside the slot is one 16-byte store; the first and the last chunk of a slot (d_dst is only 4-byte aligned, and with
//     half elements a slot of an odd element count starts 2-byte aligned) store their own elements one by one, so no
//     byte of a neighbouring slot is touched.
//   * Flat tile index, per-frame prefix table and XCD bands are the image kernels' (tiles.h).  A tile's first element is
//     taken apart into (c, y, x) once, in 64 bits and uniformly; a chunk's own first element is at most 2^14 + 8 elements
//     further, which two 32-bit divisions settle (divmod below: a float estimate corrected exactly).
//   * An element outside its picture takes the channel's pad level and reads no source byte.
//
// All bounds are settled on the host: the kernel's only tests are "inside the slot" and "inside the picture".
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "tables.h"
#include "tiles.h"

namespace lramd {
namespace {

constexpr int kBlock = 256;
constexpr int kSteps = 8;                    // chunks a lane takes of a tile
constexpr int kTileChunks = kBlock * kSteps; // 2048 chunks of 16 bytes
constexpr int kMaxGrid = 8 * 256;            // (8 workgroups a CU: what is resident at once) beyond that the workgroups of an XCD loop over its run of tiles
constexpr uint64_t kMaxSide = 1073741824;    // 2^30: x + a tile's elements stays below 2^32, also with three channels

struct TensorFrame {
    unsigned long long dst_off;           // the slot's first byte, from d_dst
    unsigned long long src_off, src_row;  // the picture's first byte from d_src and its row stride
    unsigned long long n_chunks;          // 16-byte chunks (by absolute address) that hold an element of the slot
    int w, h, left, top;                  // the picture and its place in the slot
};
static_assert(sizeof(TensorFrame) == 48, "six doubles");

struct TensorArgs {
    const uint8_t* src;
    uint8_t* dst;
    const TensorFrame* __restrict__ frames;
    const int* __restrict__ start;  // tile prefix table, batch + 1 entries
    const void* __restrict__ lut;   // C x 256 elements' bit patterns
    unsigned long long plane;       // H x W
    unsigned long long elems;       // C x H x W: a slot
    int batch, n_tiles;
    uint32_t H, W;
    float rcp_row, rcp_h;  // 1 / (elements of a row: W, or W x C for NHWC) and 1 / H, as estimates for divmod
    uint32_t pad[3];       // the pad level per channel
    int swap;              // LR_TENSOR_SWAP
};

// q = x / n and r = x % n for n <= 3 x 2^30 and x / n < 2^15: the float quotient is off by less than 2^-7 (three roundings
// of 2^-24 each on a quotient below 2^15), so its floor is the true floor or one beside it; the remainder says which.
__host__ __device__ __forceinline__ void divmod(uint32_t x, uint32_t n, float rcp, uint32_t* q, uint32_t* r) {
    uint32_t qq = (uint32_t)((float)x * rcp);
    long long rr = (long long)x - (long long)qq * (long long)n;
    if (rr < 0) {
        --qq;
        rr += n;
    } else if (rr >= (long long)n) {
        ++qq;
        rr -= n;
    }
    *q = qq;
    *r = (uint32_t)rr;
}

template <int ELEM>
struct ElemType;
template <>
struct ElemType<4> {
    using type = uint32_t;
};
template <>
struct ElemType<2> {
    using type = uint16_t;
};

enum { kNCHW = 0, kNHWC = 1 };

// ELEM: bytes of an element; LAYOUT: kNCHW or kNHWC (one channel: always kNCHW, the same bytes); BPP: bytes of a source pixel;
// C: channels of the tensor (BPP 1 with C 3 is LR_TENSOR_GRAY3)
template <int ELEM, int LAYOUT, int BPP, int C>
__global__ __launch_bounds__(kBlock) void tensor_pack_kernel(const TensorArgs g) {
    using T = typename ElemType<ELEM>::type;
    constexpr int kPer = 16 / ELEM;  // elements of a chunk
    __shared__ T lut[C * 256];
    for (int k = (int)threadIdx.x; k < C * 256; k += kBlock) lut[k] = static_cast<const T*>(g.lut)[k];
    __syncthreads();

    const uint32_t row_n = LAYOUT == kNHWC ? g.W * (uint32_t)C : g.W;
    XcdBand band(g.n_tiles);
    for (int tile; band.next(&tile);) {
        const int b = frame_of_tile(g.start, g.batch, tile);
        const long long t = tile - g.start[b];
        const TensorFrame* __restrict__ f = g.frames + b;
        const unsigned long long a0 = (unsigned long long)reinterpret_cast<uintptr_t>(g.dst) + f->dst_off;
        const int hd = (int)(a0 & 15ull) / ELEM;  // elements of the first chunk in front of the slot
        uint8_t* const base = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(a0 & ~15ull));
        const unsigned long long n_chunks = f->n_chunks, src_row = f->src_row;
        const uint8_t* const src = g.src + f->src_off;
        const uint32_t pw = (uint32_t)f->w, ph = (uint32_t)f->h, left = (uint32_t)f->left, top = (uint32_t)f->top;

        // the tile's first element that lies in the slot, taken apart (uniform)
        const long long e_t = t * (long long)(kTileChunks * kPer) - hd;
        const unsigned long long eb = e_t > 0 ? (unsigned long long)e_t : 0ull;
        uint32_t c0, y0, r0;  // NCHW: channel, row, column; NHWC: 0, row, element of the row
        if (LAYOUT == kNCHW) {
            c0 = (uint32_t)(eb / g.plane);
            const unsigned long long r = eb % g.plane;
            y0 = (uint32_t)(r / g.W);
            r0 = (uint32_t)(r % g.W);
        } else {
            c0 = 0;
            y0 = (uint32_t)(eb / row_n);
            r0 = (uint32_t)(eb % row_n);
        }

        // the level of element (c, y, x) of the slot, as an index into the table
        auto index_of = [&](uint32_t c, uint32_t y, uint32_t x) -> uint32_t {
            const uint32_t px = x - left, py = y - top;
            uint32_t v = g.pad[c];
            if (px < pw && py < ph) {
                const uint32_t sc = BPP == 1 ? 0u : (g.swap ? 2u - c : c);
                v = src[(unsigned long long)py * src_row + (unsigned long long)px * BPP + sc];
            }
            return c * 256u + v;
        };

#pragma unroll 1
        for (int k = 0; k < kSteps; ++k) {
            const long long j = t * kTileChunks + k * kBlock + (int)threadIdx.x;
            if ((unsigned long long)j >= n_chunks) break;
            const long long e_j = j * kPer - hd;  // the chunk's first element (below 0 in the slot's first chunk alone)
            const long long d0 = e_j - (long long)eb;
            const int skip = d0 < 0 ? (int)-d0 : 0;  // elements of the chunk in front of the slot ...
            const long long rest = (long long)g.elems - e_j;
            const int count = rest < kPer ? (int)rest : kPer;  // ... and where the slot ends in it
            // (c, y, x) of the chunk's first element in the slot
            uint32_t c, y, x, q;
            if (LAYOUT == kNCHW) {
                divmod(r0 + (uint32_t)(d0 + skip), g.W, g.rcp_row, &q, &x);
                divmod(y0 + q, g.H, g.rcp_h, &q, &y);
                c = c0 + q;
            } else {
                uint32_t r;
                divmod(r0 + (uint32_t)(d0 + skip), row_n, g.rcp_row, &q, &r);
                y = y0 + q;
                x = r / (uint32_t)C;
                c = r - x * (uint32_t)C;
            }
            auto step = [&]() {
                if (LAYOUT == kNCHW) {
                    if (++x == g.W) {
                        x = 0;
                        if (++y == g.H) {
                            y = 0;
                            ++c;
                        }
                    }
                } else {
                    if (++c == (uint32_t)C) {
                        c = 0;
                        if (++x == g.W) {
                            x = 0;
                            ++y;
                        }
                    }
                }
            };
            T* const out = reinterpret_cast<T*>(base + j * 16);
            if (skip == 0 && count == kPer) {
                uint32_t idx[kPer];
#pragma unroll
                for (int i = 0; i < kPer; ++i) {
                    idx[i] = index_of(c, y, x);
                    step();
                }
                uint32_t wd[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    wd[i] = ELEM == 4 ? (uint32_t)lut[idx[i]] : ((uint32_t)lut[idx[2 * i]] | (uint32_t)lut[idx[2 * i + 1]] << 16);
                *reinterpret_cast<uint4*>(out) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            } else {
                for (int i = skip; i < count; ++i) {
                    out[i] = lut[index_of(c, y, x)];
                    step();
                }
            }
        }
    }
}

// float to half, round to nearest even, on the bits
uint16_t half_bits(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return (uint16_t)(sign | 0x7C00u | (a > 0x7F800000u ? 0x200u : 0u));
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // 65520 and above round to infinity
    if (a < 0x38800000u) {                                   // below 2^-14: a multiple of 2^-24
        if (a <= 0x33000000u) return (uint16_t)sign;         // up to 2^-25 (the tie goes to the even 0)
        const uint32_t shift = 126u - (a >> 23), mant = (a & 0x7FFFFFu) | 0x800000u;
        uint32_t m = mant >> shift;
        const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        if (rem > half || (rem == half && (m & 1u))) ++m;
        return (uint16_t)(sign | m);
    }
    uint32_t h = (a - 0x38000000u) >> 13;
    const uint32_t rem = a & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
    return (uint16_t)(sign | h);
}

// ... and to bfloat16 (f is finite)
uint16_t bf16_bits(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16);
}

}  // namespace

int ctx_pack_tensor(lr_context* c, const void* d_src, size_t src_bytes, int format, const lr_tensor_args* a, int batch, void* d_dst,
                    size_t dst_bytes) {
    auto fail = [](const std::string& what) {
        set_error("lr_pack_tensor_device: " + what);
        return 1;
    };
    auto fail_at = [&](int b, int entry, const char* what) {
        return fail("frame " + std::to_string(b) + ": entry [" + std::to_string(entry) + "] " + what);
    };
    if (!c) return fail("no context");
    if (!d_src || !d_dst || !a || !a->frames) return fail("null pointer (source, destination, lr_tensor_args or frame table)");
    if (a->n < 1 || a->height < 1 || a->width < 1) return fail("n, height or width below 1");
    if ((uint64_t)a->height > kMaxSide || (uint64_t)a->width > kMaxSide) return fail("height or width above 2^30");
    if (batch < 1) return fail("batch < 1");
    if (batch > a->n) return fail("batch > n (more frames than slots)");
    if (format != LR_PIX_U8 && format != LR_PIX_U8X3) return fail("format is LR_PIX_U8 or LR_PIX_U8X3");
    if (a->dtype != LR_TENSOR_F32 && a->dtype != LR_TENSOR_F16 && a->dtype != LR_TENSOR_BF16) return fail("unknown dtype");
    if (a->layout != LR_TENSOR_NCHW && a->layout != LR_TENSOR_NHWC) return fail("unknown layout");
    if (a->flags & ~(LR_TENSOR_SWAP | LR_TENSOR_GRAY3)) return fail("unknown flag bit");
    if ((a->flags & LR_TENSOR_GRAY3) && format != LR_PIX_U8) return fail("LR_TENSOR_GRAY3 with LR_PIX_U8X3 (it spreads a gray source)");
    const int C = (format == LR_PIX_U8X3 || (a->flags & LR_TENSOR_GRAY3)) ? 3 : 1;
    if ((a->flags & LR_TENSOR_SWAP) && C == 1) return fail("LR_TENSOR_SWAP with one channel");
    if (reinterpret_cast<uintptr_t>(d_dst) & 3u) return fail("d_dst is not 4-byte aligned");
    const uint64_t bpp = format == LR_PIX_U8 ? 1 : 3, elem = a->dtype == LR_TENSOR_F32 ? 4 : 2;
    const uint64_t H = (uint64_t)a->height, W = (uint64_t)a->width, plane = H * W;
    uint64_t slot_elems, slot_bytes, total;
    if (__builtin_mul_overflow(plane, (uint64_t)C, &slot_elems) || __builtin_mul_overflow(slot_elems, elem, &slot_bytes) ||
        __builtin_mul_overflow(slot_bytes, (uint64_t)a->n, &total) || total > (uint64_t)kExact)
        return fail("the tensor (n x C x height x width elements) is larger than 2^53 bytes");
    if (total > dst_bytes) return fail("the tensor (n x C x height x width elements) reaches beyond dst_bytes");
    {
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
        if (s0 < d0 + dst_bytes && d0 < s0 + src_bytes) return fail("the destination region overlaps the source region");
    }

    // the elements, all 256 x C of them
    uint32_t pad[3] = {0, 0, 0};
    std::vector<uint32_t> lut((size_t)C * 256);
    for (int ch = 0; ch < C; ++ch) {
        const std::string at = "[" + std::to_string(ch) + "]";
        if (!std::isfinite(a->scale[ch]) || !std::isfinite(a->bias[ch])) return fail("scale" + at + " or bias" + at + " is not finite");
        uint64_t level;
        if (!table_integer(a->pad[ch], 0, 255, &level)) return fail("pad" + at + " is not an integer from 0 to 255");
        pad[ch] = (uint32_t)level;
        for (int v = 0; v < 256; ++v) {
            const double p = (double)v * a->scale[ch];
            const double y = p + a->bias[ch];
            const float f = (float)y;
            uint32_t bits;
            bool finite = std::isfinite(f);
            if (a->dtype == LR_TENSOR_F32) {
                std::memcpy(&bits, &f, 4);
            } else if (a->dtype == LR_TENSOR_F16) {
                bits = half_bits(f);
                finite = finite && (bits & 0x7C00u) != 0x7C00u;
            } else {
                bits = finite ? bf16_bits(f) : 0x7F80u;
                finite = finite && (bits & 0x7F80u) != 0x7F80u;
            }
            if (!finite) return fail("channel " + std::to_string(ch) + ": level " + std::to_string(v) + " gives a non-finite element in the chosen dtype");
            lut[(size_t)ch * 256 + v] = bits;
        }
    }

    // the table, as a whole
    std::vector<TensorFrame> fr((size_t)batch);
    std::vector<int> start((size_t)batch + 1);
    std::vector<std::pair<uint64_t, int>> named((size_t)batch);  // (slot, frame)
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(d_dst);
    int64_t n_tiles = 0;
    for (int b = 0; b < batch; ++b) {
        const double* t = a->frames + (size_t)b * 8;
        TensorFrame& f = fr[(size_t)b];
        std::memset(&f, 0, sizeof f);
        uint64_t w, h, src_off, src_row, slot, left, top;
        if (!table_integer(t[0], 1, (double)W, &w)) return fail_at(b, 0, "(width) is not an integer from 1 to the slot's width");
        if (!table_integer(t[1], 1, (double)H, &h)) return fail_at(b, 1, "(height) is not an integer from 1 to the slot's height");
        if (!table_integer(t[2], 0, kExact, &src_off)) return fail_at(b, 2, "(source offset) is not an integer from 0 to 2^53");
        if (!table_integer(t[3], (double)(w * bpp), kExact, &src_row))
            return fail_at(b, 3, "(source row stride) is not an integer from a row's bytes to 2^53");
        if (!table_integer(t[4], 0, (double)(a->n - 1), &slot)) return fail_at(b, 4, "(slot) is not an integer from 0 to n - 1");
        if (!table_integer(t[5], 0, (double)(W - w), &left)) return fail_at(b, 5, "(left) is not an integer from 0 to the slot's width less the picture's");
        if (!table_integer(t[6], 0, (double)(H - h), &top)) return fail_at(b, 6, "(top) is not an integer from 0 to the slot's height less the picture's");
        if (!(t[7] == 0.0)) return fail_at(b, 7, "(reserved) must be 0");
        uint64_t end;
        if (__builtin_mul_overflow(h - 1, src_row, &end) || __builtin_add_overflow(end, src_off, &end) ||
            __builtin_add_overflow(end, w * bpp, &end) || end > src_bytes)
            return fail_at(b, 2, "(source offset): the picture reaches beyond src_bytes");
        named[(size_t)b] = {slot, b};
        f.dst_off = slot * slot_bytes;
        f.src_off = src_off;
        f.src_row = src_row;
        f.n_chunks = (((uint64_t)(d0 + f.dst_off) & 15u) + slot_bytes + 15u) / 16u;
        f.w = (int)w;
        f.h = (int)h;
        f.left = (int)left;
        f.top = (int)top;
        start[(size_t)b] = (int)n_tiles;
        n_tiles += (int64_t)((f.n_chunks + kTileChunks - 1) / kTileChunks);
        if (n_tiles > 0x7FFFFFF0ll) return fail_at(b, 4, "(slot): the named slots are larger than 2^31 tiles of 32 KB");
    }
    start[(size_t)batch] = (int)n_tiles;
    std::sort(named.begin(), named.end());
    for (size_t k = 1; k < named.size(); ++k)
        if (named[k].first == named[k - 1].first)
            return fail_at(named[k].second, 4, ("(slot): frame " + std::to_string(named[k - 1].second) + " has the same slot").c_str());

    // one block of the mirror: frames | tile prefix | elements, each from a multiple of 8 bytes
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    const size_t o_frames = 0, o_start = o_frames + fr.size() * sizeof(TensorFrame);
    const size_t o_lut = up8(o_start + start.size() * sizeof(int)), need = o_lut + lut.size() * (size_t)elem;
    LR_HIP(hipSetDevice(c->device));
    MirroredBuffer<unsigned char>& m = c->tensor.block;
    if (need > m.cap()) {
        LR_HIP(hipStreamSynchronize(c->stream));
        if (m.grow(need + need / 2)) return 1;
    }
    // (the call before this one waited for the stream: the page-locked copy has been read)
    std::memcpy(m.h + o_frames, fr.data(), fr.size() * sizeof(TensorFrame));
    std::memcpy(m.h + o_start, start.data(), start.size() * sizeof(int));
    for (size_t k = 0; k < lut.size(); ++k) {
        if (elem == 4) reinterpret_cast<uint32_t*>(m.h + o_lut)[k] = lut[k];
        else reinterpret_cast<uint16_t*>(m.h + o_lut)[k] = (uint16_t)lut[k];
    }
    LR_HIP(hipMemcpyAsync(m.d, m.h, need, hipMemcpyHostToDevice, c->stream));

    const unsigned char* d = m.d.get();
    TensorArgs g;
    g.src = static_cast<const uint8_t*>(d_src);
    g.dst = static_cast<uint8_t*>(d_dst);
    g.frames = reinterpret_cast<const TensorFrame*>(d + o_frames);
    g.start = reinterpret_cast<const int*>(d + o_start);
    g.lut = d + o_lut;
    g.plane = plane;
    g.elems = slot_elems;
    g.batch = batch;
    g.n_tiles = (int)n_tiles;
    g.H = (uint32_t)H;
    g.W = (uint32_t)W;
    const bool nhwc = a->layout == LR_TENSOR_NHWC && C == 3;  // (one channel: the two layouts are the same bytes)
    g.rcp_row = 1.0f / (float)(nhwc ? W * 3 : W);
    g.rcp_h = 1.0f / (float)H;
    for (int ch = 0; ch < 3; ++ch) g.pad[ch] = pad[ch];
    g.swap = (a->flags & LR_TENSOR_SWAP) ? 1 : 0;
    const int grid = (int)std::min<int64_t>((n_tiles + 7) / 8 * 8, kMaxGrid);
    auto launch = [&](auto e) {
        constexpr int E = decltype(e)::value;
        if (C == 1) hipLaunchKernelGGL((tensor_pack_kernel<E, kNCHW, 1, 1>), dim3(grid), dim3(kBlock), 0, c->stream, g);
        else if (!nhwc && bpp == 1) hipLaunchKernelGGL((tensor_pack_kernel<E, kNCHW, 1, 3>), dim3(grid), dim3(kBlock), 0, c->stream, g);
        else if (!nhwc) hipLaunchKernelGGL((tensor_pack_kernel<E, kNCHW, 3, 3>), dim3(grid), dim3(kBlock), 0, c->stream, g);
        else if (bpp == 1) hipLaunchKernelGGL((tensor_pack_kernel<E, kNHWC, 1, 3>), dim3(grid), dim3(kBlock), 0, c->stream, g);
        else hipLaunchKernelGGL((tensor_pack_kernel<E, kNHWC, 3, 3>), dim3(grid), dim3(kBlock), 0, c->stream, g);
    };
    if (elem == 4) launch(std::integral_constant<int, 4>{});
    else launch(std::integral_constant<int, 2>{});
    LR_HIP(hipGetLastError());
    LR_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace lramd
