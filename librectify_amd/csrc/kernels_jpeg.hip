// Baseline JPEG streams from frames in HBM: lr_encode_jpeg_device for gfx950 (the demo's imwrite, autorectify.cpp:368-369).
//
// The arithmetic is the integer one of DESIGN.md section 3, item 13; tests/numpy_jpeg_ref.py restates it and produces the same
// bytes.  One chain of four launches covers a batch of frames of different sizes:
//
//   1. transform   A wavefront takes eight 8 x 8 blocks that follow each other in coding order, a lane a row of one block:
//                  colour conversion and the 2 x 2 mean from the source bytes (edges replicated), the row pass of the DCT in
//                  registers, the transpose through LDS, the column pass, and -- a lane now taking eight consecutive zig-zag
//                  positions -- the quantisation; a wavefront stores 1 KB of int16 coefficients in one piece.
//   2. lengths     A wavefront takes a restart interval (96 blocks: 16 MCUs of 4:2:0, 32 of 4:4:4, 96 of one component), a lane
//                  two neighbouring blocks.  It counts its blocks' bits, a wave prefix sum gives every lane its place, the lanes
//                  or their bits into the interval's bit string in LDS, the string is padded with ones to a whole byte, and a
//                  second prefix (ballots over the 0xFF bytes) gives the stuffed length.
//   3. places      A workgroup per frame scans its intervals' lengths into places, writes the host-built header and the EOI
//                  and the stream's length.
//   4. placement   Step 2 again, the stuffed bytes now stored at the interval's place with its RSTm behind it.  Intervals are
//                  byte-aligned by the standard, so nothing is concatenated at bit level across them.
//
// Entropy coding runs twice so that no staging buffer of worst-case size (416 bytes a block) is needed between 2 and 4: the
// workspace holds the coefficients (2 bytes a sample), 4 bytes and 8 bytes an interval.  Every store into the destination
// is guarded by the frame's capacity; all device writes are ordinary C++ stores (and LDS atomics).
//
// LR_JPEG_OPTIMIZE (tests/numpy_jpeg_optimize_ref.py): a frame that asks is coded with Huffman
// tables made from its own symbols.  A call with such a frame runs  transform, count, tables, lengths, places, placement:
//
//   count          Step 2's walk over the blocks in a third mode of the sink: every table look-up becomes an LDS atomic on
//                  a histogram laid out like the code table (2 x (256 AC + 16 DC)); a wavefront takes a run of
//                  neighbouring intervals and adds the non-zero bins to the frame's 64-bit counters when it leaves the frame.
//   tables         A workgroup per optimised frame, a wavefront per table (DC 0, AC 0, DC 1, AC 1): Annex K.2's merges with
//                  the 257 entries in registers (a lane holds five) and wave reductions for the two minima, the K.3 limit
//                  to 16 bits, the canonical codes into the frame's 544-word code table, and the four DHT segments and the
//                  header's new length into the frame's device record (the segments that follow them move up).
//
// Lengths and placement then run in their per-frame-table instantiation (the table is loaded into LDS again whenever the
// interval's frame changes; table 0 of the array is Annex K's, for frames of the call that did not ask).  A call without
// such a frame launches the four kernels above in the instantiations it always had.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "jpeg_tables.h"
#include "tables.h"
#include "tiles.h"

namespace lramd {
namespace {

constexpr int kWave = 64;
constexpr int kIntervalBlocks = 96;  // blocks of a restart interval (two per lane, 64 lanes: up to 128)
constexpr int kBlockWords = 52;      // a block's longest code, 22 + 63 * 26 = 1660 bits, in 32-bit words
constexpr int kBitWords = kIntervalBlocks * kBlockWords + 2;
constexpr int kBlockWordsOpt = 53;   // with a frame's own tables a DC code can have 16 bits: 27 + 63 * 26 = 1665 bits
constexpr int kBitWordsOpt = kIntervalBlocks * kBlockWordsOpt + 2;
constexpr int kDummyDC = 0x7FFF;     // in a block's DC: a 4:2:0 luminance block wholly outside the frame (coded as diff 0, EOB)
constexpr int kHeaderMax = 640;
constexpr int kHuffWords = 2 * 272;  // per table class: 256 AC symbols, then 16 DC categories; entry = code | length << 16
constexpr int kRowShift = 7;         // the row pass keeps 13 - 7 = 6 fractional bits
enum { kGray = 0, k444 = 1, k420 = 2 };

struct JpegFrame {
    unsigned long long src_off, src_row, dst_off, cap;  // bytes, from d_src and d_dst
    int w, h, mcus_x, n_mcus;
    int bpm, ri, n_intervals, hdr_len;  // blocks per MCU, MCUs per interval
    int layout;
    int opt;              // 0: Annex K's tables; else the frame's place in the array of code tables (and, less one, of counters)
    int dht_at, tail_at;  // in hdr: the first DHT segment, the first segment behind the last
    uint16_t q[2][64];  // divisors in zig-zag order: luminance, chrominance
    uint8_t hdr[kHeaderMax];
};
static_assert(sizeof(JpegFrame) % 8 == 0, "rows of the mirror block stay 8-byte aligned");

// one pass of the DCT over eight values: out[u] = sum_x T[u][x] s[x] (every |s| < 2^23 and every product < 2^31)
__device__ __forceinline__ void dct8(const int (&s)[8], int (&out)[8]) {
    int e[4], o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        e[i] = s[i] + s[7 - i];
        o[i] = s[i] - s[7 - i];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int acc = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc += __mul24(kDctHalf[u][i], (u & 1) ? o[i] : e[i]);
        out[u] = acc;
    }
}

struct Rgb {
    int r, g, b;
};
__device__ __forceinline__ Rgb load_rgb(const uint8_t* __restrict__ row, int x) {
    const uint8_t* p = row + (size_t)x * 3;
    return Rgb{(int)p[0], (int)p[1], (int)p[2]};
}
// IJG's fixed-point rule; comp 0 = Y, 1 = Cb, 2 = Cr
__device__ __forceinline__ int ycc(const Rgb& v, int comp) {
    if (comp == 0) return (19595 * v.r + 38470 * v.g + 7471 * v.b + 32768) >> 16;
    if (comp == 1) return (-11059 * v.r - 21709 * v.g + 32768 * v.b + (128 << 16) + 32767) >> 16;
    return (32768 * v.r - 27439 * v.g - 5329 * v.b + (128 << 16) + 32767) >> 16;
}

__global__ __launch_bounds__(kWave) void jpeg_transform_kernel(const uint8_t* __restrict__ src, int batch, int n_groups,
                                                               const JpegFrame* __restrict__ frames,
                                                               const int* __restrict__ grp_start, int16_t* __restrict__ coef) {
    __shared__ int s_t[8][65];
    const int lane = (int)threadIdx.x, k = lane >> 3, r = lane & 7;
    for (int grp = (int)blockIdx.x; grp < n_groups; grp += (int)gridDim.x) {
        const int b = frame_of_tile(grp_start, batch, grp);
        const JpegFrame* f = frames + b;
        const int w = f->w, h = f->h, bpm = f->bpm, layout = f->layout;
        const int blk = (grp - grp_start[b]) * 8 + k;
        const bool valid = blk < f->n_mcus * bpm;
        int s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        bool dummy = false;
        int comp = 0;
        if (valid) {
            const int mcu = blk / bpm, kb = blk - mcu * bpm;
            const int my = mcu / f->mcus_x, mx = mcu - my * f->mcus_x;
            const uint8_t* base = src + (size_t)f->src_off;
            const size_t src_row = (size_t)f->src_row;
            if (layout == kGray) {
                const uint8_t* row = base + (size_t)min(my * 8 + r, h - 1) * src_row;
#pragma unroll
                for (int i = 0; i < 8; ++i) s[i] = (int)row[min(mx * 8 + i, w - 1)] - 128;
            } else if (layout == k444 || kb < 4) {
                int x0 = mx * 8, y = my * 8 + r;
                comp = kb;
                if (layout == k420) {
                    x0 = mx * 16 + (kb & 1) * 8;
                    const int y_top = my * 16 + (kb >> 1) * 8;
                    y = y_top + r;
                    comp = 0;
                    dummy = x0 >= w || y_top >= h;
                }
                if (!dummy) {
                    const uint8_t* row = base + (size_t)min(y, h - 1) * src_row;
#pragma unroll
                    for (int i = 0; i < 8; ++i) s[i] = ycc(load_rgb(row, min(x0 + i, w - 1)), comp) - 128;
                }
            } else {  // a chrominance block of 4:2:0: the 2 x 2 mean over 16 x 2 pixels
                comp = kb - 3;
                const uint8_t* row0 = base + (size_t)min(my * 16 + 2 * r, h - 1) * src_row;
                const uint8_t* row1 = base + (size_t)min(my * 16 + 2 * r + 1, h - 1) * src_row;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int xa = min(mx * 16 + 2 * i, w - 1), xb = min(mx * 16 + 2 * i + 1, w - 1);
                    const int sum = ycc(load_rgb(row0, xa), comp) + ycc(load_rgb(row0, xb), comp) + ycc(load_rgb(row1, xa), comp) +
                                    ycc(load_rgb(row1, xb), comp);
                    s[i] = ((sum + 2) >> 2) - 128;
                }
            }
        }
        int a[8];
        dct8(s, a);
#pragma unroll
        for (int u = 0; u < 8; ++u) s_t[k][r * 8 + u] = (a[u] + (1 << (kRowShift - 1))) >> kRowShift;
        __syncthreads();
#pragma unroll
        for (int y = 0; y < 8; ++y) s[y] = s_t[k][y * 8 + r];  // column r of the block
        dct8(s, a);
        __syncthreads();
#pragma unroll
        for (int v = 0; v < 8; ++v) s_t[k][v * 8 + r] = a[v];
        __syncthreads();
        if (valid) {  // eight consecutive zig-zag positions of the block
            const uint16_t* q = f->q[comp != 0];
            uint32_t packed[4];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int zz = r * 8 + i;
                const int v = s_t[k][kZigzag[zz]];
                const uint32_t div = (uint32_t)q[zz] << (26 - kRowShift);
                const uint32_t m = ((uint32_t)(v < 0 ? -v : v) + (div >> 1)) / div;  // half away from zero
                int c = v < 0 ? -(int)m : (int)m;
                if (dummy) c = zz == 0 ? kDummyDC : 0;
                if (i & 1) packed[i >> 1] |= (uint32_t)(c & 0xFFFF) << 16;
                else packed[i >> 1] = (uint32_t)(c & 0xFFFF);
            }
            *reinterpret_cast<uint4*>(coef + ((size_t)grp * 8 + k) * 64 + r * 8) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
        }
        __syncthreads();
    }
}

// the block before j, in its interval, of j's component (below 0: none)
__device__ __forceinline__ int previous_block(int j, int layout) {
    if (layout == kGray) return j - 1;
    if (layout == k444) return j - 3;
    const int kb = j % 6;
    return kb >= 4 ? j - 6 : (kb == 0 ? j - 3 : j - 1);
}

// Counts the bits (kLength), writes the code (kWrite) or counts the symbols (kSymbols) of one block: `c` its 64
// coefficients, two to a word.  The writer keeps up to 31 bits in front of the next 32-bit boundary of the bit string and
// ors whole words into it.  The symbol counter takes a histogram in LDS where the others take the code table: a look-up
// adds one to the symbol's bin and nothing is put.
enum { kLength = 0, kWrite = 1, kSymbols = 2 };
template <int kMode>
struct BitSink {
    unsigned long long acc = 0;
    int n = 0, word = 0;
    uint32_t total = 0;
    uint32_t* out = nullptr;
    __device__ __forceinline__ uint32_t entry(const uint32_t* table, int symbol) { return table[symbol]; }
    __device__ __forceinline__ uint32_t entry(uint32_t* histogram, int symbol) {
        atomicAdd(&histogram[symbol], 1u);
        return 0;
    }
    __device__ __forceinline__ void put(uint32_t bits, int len) {
        if (kMode == kSymbols) return;
        if (kMode == kLength) {
            total += (uint32_t)len;
            return;
        }
        acc = (acc << len) | bits;
        n += len;
        if (n >= 32) {
            n -= 32;
            atomicOr(&out[word++], (uint32_t)(acc >> n));
        }
    }
    __device__ __forceinline__ void finish() {
        if (kMode == kWrite && n > 0) atomicOr(&out[word], (uint32_t)(acc << (32 - n)));
    }
};

__device__ __forceinline__ uint32_t with_magnitude(uint32_t entry, int v, int cat, int* len) {
    const uint32_t mag = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
    *len = (int)(entry >> 16) + cat;
    return ((entry & 0xFFFFu) << cat) | mag;
}

template <int kMode, typename Table>
__device__ __forceinline__ void encode_block(BitSink<kMode>& sink, const uint4* __restrict__ p, int diff, Table* huff) {
    uint32_t c[32];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = p[i];
        c[4 * i] = v.x;
        c[4 * i + 1] = v.y;
        c[4 * i + 2] = v.z;
        c[4 * i + 3] = v.w;
    }
    int len;
    {
        const int cat = 32 - __clz(diff < 0 ? -diff : diff);
        const uint32_t bits = with_magnitude(sink.entry(huff, 256 + cat), diff, cat, &len);
        sink.put(bits, len);
    }
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = (int)(int16_t)((k & 1) ? (c[k >> 1] >> 16) : (c[k >> 1] & 0xFFFFu));
        if (v == 0) {
            ++run;
        } else {
            while (run >= 16) {
                const uint32_t zrl = sink.entry(huff, 0xF0);
                sink.put(zrl & 0xFFFFu, (int)(zrl >> 16));
                run -= 16;
            }
            const int cat = 32 - __clz(v < 0 ? -v : v);
            const uint32_t bits = with_magnitude(sink.entry(huff, (run << 4) | cat), v, cat, &len);
            sink.put(bits, len);
            run = 0;
        }
    }
    if (run > 0) {
        const uint32_t eob = sink.entry(huff, 0x00);
        sink.put(eob & 0xFFFFu, (int)(eob >> 16));
    }
}

// both of a lane's blocks (2 lane, 2 lane + 1 of the interval's nb)
template <int kMode, typename Table>
__device__ __forceinline__ void encode_lane(BitSink<kMode>& sink, const int16_t* __restrict__ blocks, int lane, int nb, int layout,
                                            Table* s_huff) {
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
        const int j = 2 * lane + s;
        if (j >= nb) break;
        const int dc = (int)blocks[(size_t)j * 64];
        int diff = 0;
        if (dc != kDummyDC) {
            int p = previous_block(j, layout), pred = 0;
            while (p >= 0) {
                pred = (int)blocks[(size_t)p * 64];
                if (pred != kDummyDC) break;
                pred = 0;
                p = previous_block(p, layout);
            }
            diff = dc - pred;
        }
        int kb = 0;
        if (layout == k444) kb = j % 3;
        else if (layout == k420) kb = j % 6 < 4 ? 0 : 1;
        encode_block(sink, reinterpret_cast<const uint4*>(blocks + (size_t)j * 64), diff, s_huff + (kb != 0 ? 272 : 0));
    }
}

// kPerFrame: the frames' own code tables (JpegFrame::opt, table 0 Annex K's), loaded again when the interval's frame changes
template <bool kPlace, bool kPerFrame>
__global__ __launch_bounds__(kWave) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, int batch, int n_intervals,
                                                             const JpegFrame* __restrict__ frames, const int* __restrict__ ivl_start,
                                                             const int* __restrict__ grp_start, const uint32_t* __restrict__ huff,
                                                             uint32_t* __restrict__ len, const unsigned long long* __restrict__ place,
                                                             uint8_t* __restrict__ dst) {
    __shared__ uint32_t s_bits[kPerFrame ? kBitWordsOpt : kBitWords];
    __shared__ uint32_t s_huff[kHuffWords];
    const int lane = (int)threadIdx.x;
    int loaded = -1;
    if (!kPerFrame)
        for (int i = lane; i < kHuffWords; i += kWave) s_huff[i] = huff[i];
    for (int it = (int)blockIdx.x; it < n_intervals; it += (int)gridDim.x) {
        const int b = frame_of_tile(ivl_start, batch, it);
        const JpegFrame* f = frames + b;
        const int ii = it - ivl_start[b], layout = f->layout;
        const int first_mcu = ii * f->ri;
        const int nb = min(f->ri, f->n_mcus - first_mcu) * f->bpm;
        const int16_t* blocks = coef + ((size_t)grp_start[b] * 8 + (size_t)first_mcu * f->bpm) * 64;
        if (kPerFrame && f->opt != loaded) {
            __syncthreads();  // (the previous interval's codes have been looked up)
            loaded = f->opt;
            for (int i = lane; i < kHuffWords; i += kWave) s_huff[i] = huff[(size_t)loaded * kHuffWords + i];
        }
        __syncthreads();  // (the table is there; the previous interval's bytes have been read)

        BitSink<kLength> counter;
        encode_lane(counter, blocks, lane, nb, layout, static_cast<const uint32_t*>(s_huff));
        uint32_t incl = counter.total;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t total = __shfl(incl, kWave - 1), pos0 = incl - counter.total;
        const int n_words = (int)((total + 31u) >> 5) + 1;
        for (int i = lane; i < n_words; i += kWave) s_bits[i] = 0;
        __syncthreads();

        BitSink<kWrite> writer;
        writer.out = s_bits;
        writer.word = (int)(pos0 >> 5);
        writer.n = (int)(pos0 & 31u);
        encode_lane(writer, blocks, lane, nb, layout, static_cast<const uint32_t*>(s_huff));
        writer.finish();
        if (lane == 0 && (total & 7u)) {  // ones up to the byte boundary (which is never beyond the word's)
            const uint32_t o = total & 31u, padn = 8u - (total & 7u);
            atomicOr(&s_bits[total >> 5], ((1u << padn) - 1u) << (32u - o - padn));
        }
        __syncthreads();

        // the bytes, a zero behind every 0xFF
        const uint32_t n_bytes = (total + 7u) >> 3;
        const unsigned long long at = kPlace ? place[it] : 0ull, cap = f->cap;
        uint8_t* out = dst + (size_t)f->dst_off;
        uint32_t stuffed = 0;
        for (uint32_t base = 0; base < n_bytes; base += kWave) {
            const uint32_t j = base + (uint32_t)lane;
            const bool in = j < n_bytes;
            const uint32_t byte = in ? (s_bits[j >> 2] >> (24u - 8u * (j & 3u))) & 0xFFu : 0u;
            const unsigned long long ff = __ballot(in && byte == 0xFFu);
            if (kPlace && in) {
                const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(ff >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ff, 0u));
                const unsigned long long pos = at + j + stuffed + before;
                if (pos < cap) out[pos] = (uint8_t)byte;
                if (byte == 0xFFu && pos + 1 < cap) out[pos + 1] = 0;
            }
            stuffed += (uint32_t)__popcll(ff);
        }
        const uint32_t length = n_bytes + stuffed;
        if (!kPlace) {
            if (lane == 0) len[it] = length;
        } else if (ii != f->n_intervals - 1 && lane < 2) {  // RSTm, m cycling 0..7
            const unsigned long long pos = at + length + (unsigned)lane;
            if (pos < cap) out[pos] = lane == 0 ? (uint8_t)0xFF : (uint8_t)(0xD0 + (ii & 7));
        }
    }
}

// LR_JPEG_OPTIMIZE, the statistics: a wavefront takes `chunk` neighbouring intervals, so that it stays with a frame as long
// as it can; the bins are the code table's places.  Intervals of frames that did not ask are passed over.
__global__ __launch_bounds__(kWave) void jpeg_count_kernel(const int16_t* __restrict__ coef, int batch, int n_intervals, int chunk,
                                                           const JpegFrame* __restrict__ frames, const int* __restrict__ ivl_start,
                                                           const int* __restrict__ grp_start, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t s_hist[kHuffWords];
    const int lane = (int)threadIdx.x;
    for (int i = lane; i < kHuffWords; i += kWave) s_hist[i] = 0;
    int held = 0;  // the frame (its opt) whose symbols the histogram holds
    auto flush = [&]() {
        __syncthreads();
        if (held > 0)
            for (int i = lane; i < kHuffWords; i += kWave) {
                const uint32_t v = s_hist[i];
                if (v) atomicAdd(&counts[(size_t)(held - 1) * kHuffWords + i], (unsigned long long)v);
                s_hist[i] = 0;
            }
        __syncthreads();
    };
    const int first = (int)blockIdx.x * chunk, last = min(first + chunk, n_intervals);
    for (int it = first; it < last; ++it) {
        const int b = frame_of_tile(ivl_start, batch, it);
        const JpegFrame* f = frames + b;
        if (f->opt != held) {
            flush();
            held = f->opt;
        }
        if (held == 0) continue;
        const int first_mcu = (it - ivl_start[b]) * f->ri;
        const int nb = min(f->ri, f->n_mcus - first_mcu) * f->bpm;
        const int16_t* blocks = coef + ((size_t)grp_start[b] * 8 + (size_t)first_mcu * f->bpm) * 64;
        BitSink<kSymbols> sink;
        encode_lane(sink, blocks, lane, nb, f->layout, s_hist);
    }
    flush();
}

// one step of wave_min: the key of the lane the DPP control names (a lane the control or the row mask leaves out keeps its own)
template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t min_with_lane(uint32_t key) {
    const uint32_t other = (uint32_t)__builtin_amdgcn_update_dpp((int)key, (int)key, kCtrl, kRowMask, 0xF, false);
    return other < key ? other : key;
}
template <int kCtrl, int kRowMask>
__device__ __forceinline__ unsigned long long min_with_lane(unsigned long long key) {
    const int lo = (int)(uint32_t)key, hi = (int)(uint32_t)(key >> 32);
    const uint32_t other_lo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, kCtrl, kRowMask, 0xF, false);
    const uint32_t other_hi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, kCtrl, kRowMask, 0xF, false);
    const unsigned long long other = ((unsigned long long)other_hi << 32) | other_lo;
    return other < key ? other : key;
}
__device__ __forceinline__ uint32_t last_lane(uint32_t key) { return (uint32_t)__builtin_amdgcn_readlane((int)key, kWave - 1); }
__device__ __forceinline__ unsigned long long last_lane(unsigned long long key) {
    return ((unsigned long long)last_lane((uint32_t)(key >> 32)) << 32) | last_lane((uint32_t)key);
}
// The least of a wavefront's keys (32 or 64 bits), all 64 lanes active: within quads, half rows and rows of 16 lanes by DPP
// swaps, then row 0 into row 1 and row 2 into row 3 (row_bcast:15), rows 0..1 into rows 2..3 (row_bcast:31); lane 63 has
// it.  (A 64-bit __shfl_xor per step is two LDS round trips.)
template <typename Key>
__device__ __forceinline__ Key wave_min(Key key) {
    key = min_with_lane<0xB1, 0xF>(key);   // quad_perm:[1,0,3,2]
    key = min_with_lane<0x4E, 0xF>(key);   // quad_perm:[2,3,0,1]
    key = min_with_lane<0x141, 0xF>(key);  // row_half_mirror
    key = min_with_lane<0x140, 0xF>(key);  // row_mirror
    key = min_with_lane<0x142, 0xA>(key);  // row_bcast:15 into rows 1 and 3
    key = min_with_lane<0x143, 0xC>(key);  // row_bcast:31 into rows 2 and 3
    return last_lane(key);
}

constexpr int kEntries = 257;    // 256 symbols and the pseudo-symbol that keeps the all-ones code free
constexpr int kOwn = 5;          // entries of a lane: lane, lane + 64, ... (the fifth is lane 0's pseudo-symbol)
// Annex K.2 over a wavefront's 257 entries: merges the two least frequent entries until one
// is left and gives every entry its code length.  Of equal counts the larger index goes first, so an entry's key is its count
// with the index's complement below it (all ones: no count left); Key has room for the sum of all counts above those 9 bits.
// A lane keeps its two least keys, so the second reduction takes from every lane the least key that is not the first's.
// An entry remembers the entry its chain was merged into: a merge is a compare per entry, not a walk along a chain.
template <typename Key>
__device__ __forceinline__ void code_sizes(const unsigned long long (&freq)[kOwn], int lane, int (&size)[kOwn]) {
    constexpr Key kNoKey = ~(Key)0;
    Key key[kOwn];
    int root[kOwn];
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
        const int idx = lane + kWave * k;
        key[k] = freq[k] != 0 ? ((Key)freq[k] << 9) | (Key)(511 - idx) : kNoKey;
        root[k] = idx;
        size[k] = 0;
    }
    for (;;) {
        Key l1 = kNoKey, l2 = kNoKey;
#pragma unroll
        for (int k = 0; k < kOwn; ++k) {
            const Key v = key[k];
            l2 = v < l1 ? l1 : (v < l2 ? v : l2);
            l1 = v < l1 ? v : l1;
        }
        const Key m1 = wave_min(l1);
        const Key m2 = wave_min(l1 == m1 ? l2 : l1);
        if (m2 == kNoKey) break;
        const int c1 = 511 - (int)(m1 & 511u), c2 = 511 - (int)(m2 & 511u);
#pragma unroll
        for (int k = 0; k < kOwn; ++k) {
            if (key[k] == m1) key[k] += m2 & ~(Key)511;  // (the first keeps the sum, under its own index)
            else if (key[k] == m2) key[k] = kNoKey;
            if (root[k] == c1 || root[k] == c2) {  // every member of both chains gets one more bit
                ++size[k];
                root[k] = c1;
            }
        }
    }
}

constexpr int kCountWaves = 2048;  // of jpeg_count_kernel: eight to a compute unit; more would only flush more often
constexpr int kTableWaves = 4;   // DC 0, AC 0, DC 1, AC 1: the order of the DHT segments
constexpr int kUnused = 0x7FFFFFFF;
// LR_JPEG_OPTIMIZE, the tables of one frame from its counters: the code table (every word
// of it: symbols that do not occur get 0), the DHT segments, the header's length.
__global__ __launch_bounds__(kTableWaves* kWave) void jpeg_tables_kernel(JpegFrame* __restrict__ frames, const int* __restrict__ opt_frame,
                                                                        const unsigned long long* __restrict__ counts,
                                                                        uint32_t* __restrict__ huff) {
    // a symbol's place in HUFFVAL's order: its length before the limit, its value below it (kUnused: it does not occur)
    __shared__ __attribute__((aligned(16))) int s_order[kTableWaves][256];
    __shared__ int s_top[kTableWaves];                  // the longest length before the limit
    __shared__ int s_bits[kTableWaves][kEntries + 1];   // codes of a length (before the limit a length can be 256)
    __shared__ int s_cum[kTableWaves][17], s_code[kTableWaves][17];  // symbols shorter than or of a length; the length's first code
    __shared__ uint8_t s_dht[kTableWaves][16 + 256];    // BITS, HUFFVAL
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
    const int o = (int)blockIdx.x;
    JpegFrame* f = frames + opt_frame[o];
    const int n_tables = f->layout == kGray ? 2 : 4;
    const bool ac = wave & 1;
    const int n_symbols = wave >= n_tables ? 0 : (ac ? 256 : 16);  // (a wave without a table goes along with no symbols)
    const int at = (wave >> 1) * 272 + (ac ? 0 : 256);             // the table's place in the code table and the counters
    const int tail_len = f->hdr_len - f->tail_at;
    const uint8_t tail = tid < tail_len ? f->hdr[f->tail_at + tid] : (uint8_t)0;

    unsigned long long freq[kOwn], total = 0;
    int size[kOwn];
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
        const int idx = lane + kWave * k;
        freq[k] = idx < n_symbols ? counts[(size_t)o * kHuffWords + at + idx] : (idx == 256 ? 1ull : 0ull);
        total += freq[k];
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) total += __shfl_xor(total, d);
    // (keys of 32 bits while the sum of the table's counts stays below 2^22 -- a 4K frame's tables do -- cost a third)
    if (total < (1ull << 22)) code_sizes<uint32_t>(freq, lane, size);
    else code_sizes<unsigned long long>(freq, lane, size);
    for (int i = lane; i <= kEntries; i += kWave) s_bits[wave][i] = 0;
    if (lane == 0) s_top[wave] = 16;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
        const int idx = lane + kWave * k;
        if (idx < 256) s_order[wave][idx] = size[k] > 0 ? (size[k] << 9) | idx : kUnused;
        if (idx < kEntries && size[k] > 0) {
            atomicAdd(&s_bits[wave][size[k]], 1);
            atomicMax(&s_top[wave], size[k]);
        }
    }
    __syncthreads();
    if (lane == 0) {  // K.3: no code longer than 16 bits; then the pseudo-symbol's code leaves the longest length
        int* bits = s_bits[wave];
        for (int i = s_top[wave]; i > 16; --i)
            while (bits[i] > 0) {
                int j = i - 2;
                while (j > 0 && bits[j] == 0) --j;
                bits[i] -= 2;
                bits[i - 1] += 1;
                bits[j + 1] += 2;
                bits[j] -= 1;
            }
        int i = 16;
        while (i > 0 && bits[i] == 0) --i;
        if (i > 0) bits[i] -= 1;  // (a wave without a table has no code at all)
        int code = 0;
        s_cum[wave][0] = 0;
        for (int length = 1; length <= 16; ++length) {  // Annex C
            s_code[wave][length] = code;
            s_cum[wave][length] = s_cum[wave][length - 1] + bits[length];
            code = (code + bits[length]) << 1;
        }
    }
    __syncthreads();
    if (lane < 16) s_dht[wave][lane] = (uint8_t)s_bits[wave][lane + 1];
    // HUFFVAL: by the length before the limit, within one by the symbol; a symbol's place there -- the number of symbols in
    // front of it -- gives its length and code
    int mine[kOwn - 1], place[kOwn - 1];
#pragma unroll
    for (int k = 0; k < kOwn - 1; ++k) {
        mine[k] = size[k] > 0 ? (size[k] << 9) | (lane + kWave * k) : 0;
        place[k] = 0;
    }
    const int4* order = reinterpret_cast<const int4*>(s_order[wave]);
#pragma unroll 4
    for (int j = 0; j < n_symbols / 4; ++j) {
        const int4 v = order[j];
#pragma unroll
        for (int k = 0; k < kOwn - 1; ++k) place[k] += (v.x < mine[k]) + (v.y < mine[k]) + (v.z < mine[k]) + (v.w < mine[k]);
    }
#pragma unroll
    for (int k = 0; k < kOwn - 1; ++k) {
        const int idx = lane + kWave * k;
        if (idx >= n_symbols) continue;
        uint32_t word = 0;
        if (size[k] > 0) {
            int length = 1;
            while (s_cum[wave][length] <= place[k]) ++length;
            word = (uint32_t)(s_code[wave][length] + place[k] - s_cum[wave][length - 1]) | ((uint32_t)length << 16);
            s_dht[wave][16 + place[k]] = (uint8_t)idx;
        }
        huff[(size_t)(o + 1) * kHuffWords + at + idx] = word;
    }
    __syncthreads();

    // the DHT segments one behind the other, then what followed them
    int pos = f->dht_at;
    for (int t = 0; t < n_tables; ++t) {
        const int n = s_cum[t][16];
        for (int i = tid; i < 21 + n; i += kTableWaves * kWave) {
            uint8_t v;
            if (i == 0) v = 0xFF;
            else if (i == 1) v = 0xC4;
            else if (i == 2) v = (uint8_t)((19 + n) >> 8);
            else if (i == 3) v = (uint8_t)((19 + n) & 0xFF);
            else if (i == 4) v = (uint8_t)(((t & 1) << 4) | (t >> 1));
            else v = s_dht[t][i - 5];
            if (pos + i < kHeaderMax) f->hdr[pos + i] = v;  // (always: no table has more symbols than Annex K's)
        }
        pos += 21 + n;
    }
    if (tid < tail_len && pos + tid < kHeaderMax) f->hdr[pos + tid] = tail;
    if (tid == 0) f->hdr_len = pos + tail_len;
}

constexpr int kScanBlock = 256;
// a workgroup per frame: the intervals' places in the stream, the header, the EOI and the stream's length
__global__ __launch_bounds__(kScanBlock) void jpeg_place_kernel(const JpegFrame* __restrict__ frames, const int* __restrict__ ivl_start,
                                                                const uint32_t* __restrict__ len, unsigned long long* __restrict__ place,
                                                                unsigned long long* __restrict__ sizes, uint8_t* __restrict__ dst) {
    __shared__ unsigned long long s_scan[kScanBlock];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const JpegFrame* f = frames + b;
    const int first = ivl_start[b], n = f->n_intervals;
    const unsigned long long cap = f->cap;
    uint8_t* out = dst + (size_t)f->dst_off;
    unsigned long long carry = (unsigned long long)f->hdr_len;
    for (int base = 0; base < n; base += kScanBlock) {
        const int i = base + tid;
        const unsigned long long v = i < n ? (unsigned long long)len[first + i] + (i < n - 1 ? 2ull : 0ull) : 0ull;
        s_scan[tid] = v;
        __syncthreads();
        for (int d = 1; d < kScanBlock; d <<= 1) {
            const unsigned long long add = tid >= d ? s_scan[tid - d] : 0ull;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        if (i < n) place[first + i] = carry + s_scan[tid] - v;
        carry += s_scan[kScanBlock - 1];
        __syncthreads();
    }
    for (int i = tid; i < f->hdr_len; i += kScanBlock)
        if ((unsigned long long)i < cap) out[i] = f->hdr[i];
    if (tid < 2 && carry + (unsigned)tid < cap) out[carry + (unsigned)tid] = tid == 0 ? (uint8_t)0xFF : (uint8_t)0xD9;  // EOI
    if (tid == 0) sizes[b] = carry + 2;
}

// ---- the host's part: tables, headers, the check of the frame table ----

// ITU-T T.81 Annex K.1, natural order
const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                               69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                               81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kZigzagHost[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.3: BITS and HUFFVAL
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
    0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
    0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
    0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
    0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4,
    0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};

// the canonical codes of Annex C: table[symbol] = code | length << 16
void huffman_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* table) {
    uint32_t code = 0;
    int k = 0;
    for (int length = 1; length <= 16; ++length) {
        for (int i = 0; i < bits[length - 1]; ++i) table[vals[k++]] = code++ | ((uint32_t)length << 16);
        code <<= 1;
    }
}

// the IJG quality rule, in zig-zag order
void quant_table(const uint8_t* base, int quality, uint16_t* out) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) out[i] = (uint16_t)std::min(std::max(((int)base[kZigzagHost[i]] * s + 50) / 100, 1), 255);
}

struct HeaderWriter {
    uint8_t* p;
    int n = 0;
    void byte(int v) { p[n++] = (uint8_t)v; }
    void word(int v) {
        byte(v >> 8);
        byte(v & 0xFF);
    }
    void bytes(const uint8_t* v, int count) {
        for (int i = 0; i < count; ++i) byte(v[i]);
    }
    void marker(int m, int payload) {
        byte(0xFF);
        byte(m);
        word(payload + 2);
    }
    void dht(int id, const uint8_t* bits, const uint8_t* vals, int count) {
        marker(0xC4, 17 + count);
        byte(id);
        bytes(bits, 16);
        bytes(vals, count);
    }
};

// everything in front of the scan's first byte
int write_header(JpegFrame& f, int components) {  // (and dht_at, tail_at: where jpeg_tables_kernel puts a frame's own tables)
    HeaderWriter h{f.hdr};
    h.byte(0xFF);
    h.byte(0xD8);
    h.marker(0xE0, 14);  // JFIF 1.01, no units, 1 : 1, no thumbnail
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    h.bytes(jfif, 14);
    for (int t = 0; t < (components == 3 ? 2 : 1); ++t) {
        h.marker(0xDB, 65);
        h.byte(t);
        for (int i = 0; i < 64; ++i) h.byte(f.q[t][i]);
    }
    h.marker(0xC0, 6 + 3 * components);
    h.byte(8);
    h.word(f.h);
    h.word(f.w);
    h.byte(components);
    for (int c = 0; c < components; ++c) {
        h.byte(c + 1);
        h.byte(c == 0 && f.layout == k420 ? 0x22 : 0x11);
        h.byte(c == 0 ? 0 : 1);
    }
    f.dht_at = h.n;
    h.dht(0x00, kDcLumaBits, kDcVals, 12);
    h.dht(0x10, kAcLumaBits, kAcLumaVals, 162);
    if (components == 3) {
        h.dht(0x01, kDcChromaBits, kDcVals, 12);
        h.dht(0x11, kAcChromaBits, kAcChromaVals, 162);
    }
    f.tail_at = h.n;
    h.marker(0xDD, 2);
    h.word(f.ri);
    h.marker(0xDA, 4 + 2 * components);
    h.byte(components);
    for (int c = 0; c < components; ++c) {
        h.byte(c + 1);
        h.byte(c == 0 ? 0x00 : 0x11);
    }
    h.byte(0);
    h.byte(63);
    h.byte(0);
    return h.n;
}

}  // namespace

int ctx_encode_jpeg(lr_context* c, const void* d_src, size_t src_bytes, int format, const double* T, int batch, void* d_dst,
                    size_t dst_bytes, uint64_t* sizes) {
    auto fail = [](const std::string& what) {
        set_error("lr_encode_jpeg_device: " + what);
        return 1;
    };
    auto fail_at = [&](int b, int entry, const char* what) {
        return fail("frame " + std::to_string(b) + ": entry [" + std::to_string(entry) + "] " + what);
    };
    if (!c) return fail("no context");
    if (!d_src || !d_dst || !T || !sizes) return fail("null pointer (source, destination, frame table or sizes)");
    if (batch < 1) return fail("batch < 1");
    if (format != LR_PIX_U8 && format != LR_PIX_U8X3) return fail("format is LR_PIX_U8 or LR_PIX_U8X3");
    {
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
        if (s0 < d0 + dst_bytes && d0 < s0 + src_bytes) return fail("the destination region overlaps the source region");
    }

    // the table, as a whole
    const uint64_t bpp = format == LR_PIX_U8 ? 1 : 3;
    const int components = format == LR_PIX_U8 ? 1 : 3;
    std::vector<JpegFrame> fr((size_t)batch);
    std::vector<int> grp_start((size_t)batch + 1), ivl_start((size_t)batch + 1);
    std::vector<std::pair<uint64_t, uint64_t>> extent((size_t)batch);
    std::vector<int> opt_frame;  // the frames with LR_JPEG_OPTIMIZE
    int64_t n_groups = 0, n_intervals = 0;
    for (int b = 0; b < batch; ++b) {
        const double* t = T + (size_t)b * 8;
        JpegFrame& f = fr[(size_t)b];
        std::memset(&f, 0, sizeof f);
        uint64_t w, h, src_off, src_row, dst_off, cap, quality, layout;
        const uint64_t max_layout = components == 3 ? 1 : 0;
        if (!table_integer(t[0], 1, 65535, &w)) return fail_at(b, 0, "(width) is not an integer from 1 to 65535");
        if (!table_integer(t[1], 1, 65535, &h)) return fail_at(b, 1, "(height) is not an integer from 1 to 65535");
        if (!table_integer(t[2], 0, kExact, &src_off)) return fail_at(b, 2, "(source offset) is not an integer from 0 to 2^53");
        if (!table_integer(t[3], (double)(w * bpp), kExact, &src_row))
            return fail_at(b, 3, "(source row stride) is not an integer from a row's bytes to 2^53");
        if (!table_integer(t[4], 0, kExact, &dst_off)) return fail_at(b, 4, "(stream offset) is not an integer from 0 to 2^53");
        if (!table_integer(t[5], 0, kExact, &cap)) return fail_at(b, 5, "(capacity) is not an integer from 0 to 2^53");
        if (!table_integer(t[6], 1, 100, &quality)) return fail_at(b, 6, "(quality) is not an integer from 1 to 100");
        if (!table_integer(t[7], 0, (double)(LR_JPEG_OPTIMIZE | max_layout), &layout) || (layout & ~(uint64_t)LR_JPEG_OPTIMIZE) > max_layout)
            return fail_at(b, 7, components == 3 ? "(layout) is 0 (4:2:0) or 1 (4:4:4), LR_JPEG_OPTIMIZE added or not"
                                                 : "(layout) must be 0 or LR_JPEG_OPTIMIZE for LR_PIX_U8");
        if (layout & LR_JPEG_OPTIMIZE) {
            opt_frame.push_back(b);
            f.opt = (int)opt_frame.size();
            layout &= ~(uint64_t)LR_JPEG_OPTIMIZE;
        }
        uint64_t end;
        if (__builtin_mul_overflow(h - 1, src_row, &end) || __builtin_add_overflow(end, src_off, &end) ||
            __builtin_add_overflow(end, w * bpp, &end) || end > src_bytes)
            return fail_at(b, 2, "(source offset): the frame's source reaches beyond src_bytes");
        if (__builtin_add_overflow(dst_off, cap, &end) || end > dst_bytes)
            return fail_at(b, 4, "(stream offset): the frame's extent reaches beyond dst_bytes");
        extent[(size_t)b] = {dst_off, end};
        f.src_off = src_off;
        f.src_row = src_row;
        f.dst_off = dst_off;
        f.cap = cap;
        f.w = (int)w;
        f.h = (int)h;
        f.layout = components == 1 ? kGray : (layout == 1 ? k444 : k420);
        const int mcu = f.layout == k420 ? 16 : 8;
        f.bpm = f.layout == kGray ? 1 : (f.layout == k444 ? 3 : 6);
        f.ri = kIntervalBlocks / f.bpm;
        f.mcus_x = (f.w + mcu - 1) / mcu;
        const int64_t n_mcus = (int64_t)f.mcus_x * ((f.h + mcu - 1) / mcu);
        if (n_mcus * f.bpm > 0x7FFFFF00ll) return fail_at(b, 0, "(width): more than 2^31 blocks in a frame");
        f.n_mcus = (int)n_mcus;
        f.n_intervals = (int)((n_mcus + f.ri - 1) / f.ri);
        quant_table(kBaseLuma, (int)quality, f.q[0]);
        quant_table(kBaseChroma, (int)quality, f.q[1]);
        f.hdr_len = write_header(f, components);
        grp_start[(size_t)b] = (int)n_groups;
        ivl_start[(size_t)b] = (int)n_intervals;
        n_groups += (n_mcus * f.bpm + 7) / 8;
        n_intervals += f.n_intervals;
        if (n_groups > 0x0FFFFFF0ll) return fail_at(b, 0, "(width): the frames are larger than 2^31 blocks in total");
    }
    grp_start[(size_t)batch] = (int)n_groups;
    ivl_start[(size_t)batch] = (int)n_intervals;
    {
        std::vector<std::pair<uint64_t, uint64_t>> sorted = extent;
        if (const size_t at = extents_overlap(sorted)) {
            int which = 0;
            while (extent[(size_t)which] != sorted[at]) ++which;
            return fail_at(which, 4, "(stream offset): two frames' extents overlap");
        }
    }

    // one block of the mirror: frames | group prefix | interval prefix | the frames with LR_JPEG_OPTIMIZE | code tables: Annex
    // K's, then one per such frame (the device's alone: made there, never copied) | the streams' lengths (coming back)
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    const size_t n_opt = opt_frame.size();
    const size_t o_frames = 0, o_grp = o_frames + fr.size() * sizeof(JpegFrame);
    const size_t o_ivl = up8(o_grp + grp_start.size() * sizeof(int)), o_opt = up8(o_ivl + ivl_start.size() * sizeof(int));
    const size_t o_huff = up8(o_opt + n_opt * sizeof(int)), o_own = up8(o_huff + kHuffWords * sizeof(uint32_t));
    const size_t o_sizes = o_own + n_opt * kHuffWords * sizeof(uint32_t), need = o_sizes + (size_t)batch * sizeof(unsigned long long);
    LR_HIP(hipSetDevice(c->device));
    JpegStore& js = c->jpeg;
    // (the call is synchronous: nothing of an earlier one is in flight when these are replaced, so the block needs neither
    // the stream synchronise before a grow nor an event behind the copy, and upload_reserve / upload_send of tables.h,
    // which are that pair, are not used here)
    if (need > js.block.cap() && js.block.grow(need + need / 2)) return 1;
    const size_t n_coef = (size_t)n_groups * 8 * 64;
    if (n_coef > js.coef.cap() && js.coef.grow(n_coef)) return 1;
    if ((size_t)n_intervals > js.len.cap() && js.len.grow((size_t)n_intervals)) return 1;
    if ((size_t)n_intervals > js.place.cap() && js.place.grow((size_t)n_intervals)) return 1;
    if (n_opt * kHuffWords > js.counts.cap() && js.counts.grow(n_opt * kHuffWords)) return 1;
    unsigned char* m = js.block.h;
    std::memcpy(m + o_frames, fr.data(), fr.size() * sizeof(JpegFrame));
    std::memcpy(m + o_grp, grp_start.data(), grp_start.size() * sizeof(int));
    std::memcpy(m + o_ivl, ivl_start.data(), ivl_start.size() * sizeof(int));
    if (n_opt) std::memcpy(m + o_opt, opt_frame.data(), n_opt * sizeof(int));
    uint32_t* codes = reinterpret_cast<uint32_t*>(m + o_huff);
    std::memset(codes, 0, kHuffWords * sizeof(uint32_t));
    huffman_codes(kAcLumaBits, kAcLumaVals, codes);
    huffman_codes(kDcLumaBits, kDcVals, codes + 256);
    huffman_codes(kAcChromaBits, kAcChromaVals, codes + 272);
    huffman_codes(kDcChromaBits, kDcVals, codes + 272 + 256);
    LR_HIP(hipMemcpyAsync(js.block.d, m, o_own, hipMemcpyHostToDevice, c->stream));

    unsigned char* d = js.block.d.get();
    JpegFrame* d_frames = reinterpret_cast<JpegFrame*>(d + o_frames);
    const int* d_grp = reinterpret_cast<const int*>(d + o_grp);
    const int* d_ivl = reinterpret_cast<const int*>(d + o_ivl);
    uint32_t* d_huff = reinterpret_cast<uint32_t*>(d + o_huff);
    unsigned long long* d_sizes = reinterpret_cast<unsigned long long*>(d + o_sizes);
    const uint8_t* s8 = static_cast<const uint8_t*>(d_src);
    uint8_t* d8 = static_cast<uint8_t*>(d_dst);
    const int grid_t = (int)std::min<int64_t>(n_groups, 1 << 18), grid_e = (int)std::min<int64_t>(n_intervals, 1 << 16);
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3(grid_t), dim3(kWave), 0, c->stream, s8, batch, (int)n_groups, d_frames, d_grp,
                       js.coef.get());
    if (n_opt == 0) {
        hipLaunchKernelGGL((jpeg_entropy_kernel<false, false>), dim3(grid_e), dim3(kWave), 0, c->stream, js.coef.get(), batch,
                           (int)n_intervals, d_frames, d_ivl, d_grp, d_huff, js.len.get(), js.place.get(), d8);
        hipLaunchKernelGGL(jpeg_place_kernel, dim3(batch), dim3(kScanBlock), 0, c->stream, d_frames, d_ivl, js.len.get(), js.place.get(),
                           d_sizes, d8);
        hipLaunchKernelGGL((jpeg_entropy_kernel<true, false>), dim3(grid_e), dim3(kWave), 0, c->stream, js.coef.get(), batch,
                           (int)n_intervals, d_frames, d_ivl, d_grp, d_huff, js.len.get(), js.place.get(), d8);
    } else {  // LR_JPEG_OPTIMIZE: the symbols' counts and the tables made of them first, then the same with a table per frame
        const int* d_opt = reinterpret_cast<const int*>(d + o_opt);
        const int grid_c = (int)std::min<int64_t>(n_intervals, kCountWaves);
        const int chunk = (int)((n_intervals + grid_c - 1) / grid_c);
        LR_HIP(hipMemsetAsync(js.counts.get(), 0, n_opt * kHuffWords * sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)((n_intervals + chunk - 1) / chunk)), dim3(kWave), 0, c->stream,
                           js.coef.get(), batch, (int)n_intervals, chunk, d_frames, d_ivl, d_grp, js.counts.get());
        hipLaunchKernelGGL(jpeg_tables_kernel, dim3((unsigned)n_opt), dim3(kTableWaves * kWave), 0, c->stream, d_frames, d_opt,
                           js.counts.get(), d_huff);
        hipLaunchKernelGGL((jpeg_entropy_kernel<false, true>), dim3(grid_e), dim3(kWave), 0, c->stream, js.coef.get(), batch,
                           (int)n_intervals, d_frames, d_ivl, d_grp, d_huff, js.len.get(), js.place.get(), d8);
        hipLaunchKernelGGL(jpeg_place_kernel, dim3(batch), dim3(kScanBlock), 0, c->stream, d_frames, d_ivl, js.len.get(), js.place.get(),
                           d_sizes, d8);
        hipLaunchKernelGGL((jpeg_entropy_kernel<true, true>), dim3(grid_e), dim3(kWave), 0, c->stream, js.coef.get(), batch,
                           (int)n_intervals, d_frames, d_ivl, d_grp, d_huff, js.len.get(), js.place.get(), d8);
    }
    LR_HIP(hipGetLastError());
    LR_HIP(hipMemcpyAsync(m + o_sizes, d_sizes, (size_t)batch * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    LR_HIP(hipStreamSynchronize(c->stream));
    for (int b = 0; b < batch; ++b) sizes[b] = reinterpret_cast<const unsigned long long*>(m + o_sizes)[b];
    return 0;
}

}  // namespace lramd
