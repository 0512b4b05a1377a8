// Baseline JPEG streams in HBM to frames in HBM: lr_decode_jpeg_device for gfx950 (the demo's imread, autorectify.cpp).
//
// The arithmetic is the integer one of DESIGN.md section 3, item 14; tests/numpy_jpeg_decode_ref.py restates it.  The host
// reads the headers up to SOS (from the caller's host copy) and nothing behind them.  One chain of launches covers a batch of
// streams of different sizes and samplings:
//
//   1. sync        The scan is cut into parts of 128 bytes, a lane each, 256 to a workgroup.  A part's entry state is (byte,
//                  bit in it, block of the MCU, zig-zag index); the scan's first part starts from the true state, every other
//                  one from a guess (its first bit, a new MCU).  A lane decodes from its entry state to the first symbol
//                  that ends in a later part and hands that state to the next lane as ITS entry state; a lane whose entry
//                  state changed decodes again.  Inside a workgroup this repeats through LDS until nothing changes; the last
//                  lane's exit state goes to the next workgroup in the NEXT launch (no workgroup waits for another).  The
//                  host launches rounds until one in which no lane decoded: then every part's entry state is its
//                  predecessor's exit state -- a verified fixed point, and with the first part true the decode is the
//                  sequential one by induction, whatever the guesses were.  Huffman codes synchronise by themselves within
//                  a few symbols, so three launches are the rule.  (For a scan that never does, such as
//                  tests/jpeg_stream_cases.py's no_resync, the text above gives one launch per workgroup of its parts and
//                  one more that finds nothing to do; the call does not report its launches, so this is derived, not
//                  measured.)  An RSTm met by the bit reader
//                  byte-aligns and resets.
//   2. place       A workgroup per frame: the prefix sum of the parts' block counts gives every part its first block; the
//                  totals (blocks, markers) and the most decodes of any part go back to the host.
//   3. write       Step 1's decode once more from the final entry states, the coefficients now stored (int16, natural
//                  order, 128 bytes a block in coding order; DC still as differences) and the RSTm numbers checked.
//   4. dc          A workgroup per frame turns the DC differences into values: a segmented scan per component, the
//                  segments being the restart intervals.
//   5. transform   A wavefront takes eight blocks, a lane a row: dequantisation folded into the load, the first pass in
//                  registers, the transpose through LDS, the second pass; the 64 samples take the place of the block's
//                  first 64 bytes.
//   6. output      A thread per pixel: centred triangle upsampling of the chrominance from the blocks' samples, the colour
//                  rule, the store into the caller's picture -- where the frame's EXIF orientation puts it, if the caller
//                  asked for that (entry [7]).  Orientations 2..4 keep rows as rows and only move the address; 5..8 turn
//                  rows into columns, and such a frame's tiles are squares of 32 x 32 stored pixels that go through LDS,
//                  so that consecutive lanes still store consecutive bytes of one row of the picture.
//
// LR_JPEG_ANY_SAMPLING (or-ed into the call's format): three-component streams of any sampling whose factors are 1, 2 or 4,
// the luminance's the largest, at most 10 blocks to the MCU (4:4:0, 4:1:1, ...; tests/numpy_jpeg_sampling_ref.py restates it).
// The stages only need to know which component a block of the MCU belongs to (a table in the frame record) and where a
// component's sample lies (shifts by the factors); the upsampling is per axis by the ratio: the sample, the triangle, or
// replication for 4.  Those are the kAny instantiations of the kernels, which a call gets only if it has the bit and one of
// its frames needs them: every other call launches the kernels it always did (docs/jpeg_decode_bounds.md has the stores).
//
// LR_JPEG_SCALED (or-ed into the call's format): entry [6] of a frame's row is its scale denominator N, 1, 2, 4 or 8, and the
// picture is written at ceil(w / N) x ceil(h / N) (tests/numpy_jpeg_scale_ref.py restates it).  Steps 1 to 4 are the same at
// every scale.  Per component and axis, with rho the ratio of the largest factor to the component's, d = min(N, rho) of the
// scale is taken from the upsampling and r = N / d from the blocks: step 5 averages the block's 64 samples over cells of
// rx x ry (the rounded mean) and stores the (8 / rx) x (8 / ry) reduced samples densely in the slot's first bytes; step 6 runs
// over the reduced picture, a reduced block's sides being shifts, the upsampling that is left rho / d, the clamps the reduced
// grid's.  Those are the kScaled instantiations of the two kernels (on the general geometry, of which the three layouts are
// special cases), which a call gets only if it has the bit and a live frame with N > 1.
//
// Every loop on the device is bounded by the part's bits, the stream's length or the frame's block count; every read of the
// stream is clamped to [offset, offset + length), every coefficient store to the frame's blocks, every pixel store to the
// frame's size.  All device writes are ordinary C++ stores (and LDS).
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "jpeg_tables.h"
#include "tables.h"
#include "tiles.h"

namespace lramd {
namespace {

constexpr int kWave = 64;
constexpr int kPartBytes = 128;   // a part of a scan: one lane's
constexpr int kSyncBlock = 256;   // parts of a workgroup
constexpr int kTileW = 32, kTileH = 8;  // pixels of an output tile (a thread each)
constexpr int kSquare = 32;             // side of a transposing frame's tile: kSquare / kTileH passes of the thread shape
constexpr int kCoefLimit = 32767;  // |c q| saturates here (legitimate data stays below 2^12)
constexpr int kMidLimit = 65535;   // the first pass's result here: 21641 * 65535 < 2^31, 21641 the largest column sum of |T|
constexpr int kMidShift = 7, kEndShift = 19;
enum { kL420 = 0, kL444 = 1, kL422 = 2 };
enum { kOk = 0, kNotJpeg = 1, kUnsupported = 2, kSizeMismatch = 3, kDamaged = 4 };

// Annex F.2.2.3: a code of length l is a symbol if code <= maxcode[l] (-1: none of that length), vals[code + delta[l]]
struct HuffDec {
    int32_t maxcode[18];
    int32_t delta[18];
    uint8_t vals[256];
};
static_assert(sizeof(HuffDec) == 400, "copied by words");

struct JdFrame {
    unsigned long long src_off, dst_off, dst_row;
    uint32_t len, scan;  // the stream's length; offset of the scan's first byte in it
    int w, h, comps, layout;
    int ri, bpm, mcus_x, n_mcus;
    int hs, vs, n_parts, orient;  // orient: 0 or 1 as stored, 2..8 the EXIF orientation the output pass applies
    uint8_t q[3][64];  // divisors per component, natural order
    HuffDec dc[3], ac[3];
    // The general geometry (LR_JPEG_ANY_SAMPLING), filled for every frame and read by the kAny instantiations alone.  Every
    // factor is 1, 2 or 4, so the device shifts and masks and never divides.  Component i of the MCU is v_i rows of h_i
    // blocks from block first[i] on; its own grid is cw[i] x ch[i] samples.
    uint32_t comp_word;              // the table block of the MCU -> component: bits [2 kb, 2 kb + 2), kb < bpm <= 10
    uint8_t first[4];                // first block of the MCU of component i
    uint8_t hsh[4], vsh[4];          // log2 h_i, log2 v_i
    uint8_t rxs[4], rys[4];          // log2 (Hmax / h_i), log2 (Vmax / v_i): 0 the sample, 1 the triangle, 2 replication
    int cw[4], ch[4];
    // The reduced geometry (LR_JPEG_SCALED, scale denominator N), filled for every frame and read by the kScaled
    // instantiations alone.  Per component and axis, with rho the ratio above: d = min(N, rho), the blocks are reduced by
    // r = N / d and the upsampling that is left is rho / d.  N = 1 gives sides of 8, the ratios and the sizes above.
    int sw, sh;                      // the reduced picture: ceil(w / N) x ceil(h / N)
    uint8_t sbx[4], sby[4];          // log2 of a reduced block's sides, 3 - log2 r: 0..3
    uint8_t srx[4], sry[4];          // log2 (rho / d): 0 the sample, 1 the triangle, 2 replication
    int scw[4], sch[4];              // the component's reduced grid: ceil(cw / rx) x ceil(ch / ry)
};
static_assert(sizeof(JdFrame) % 8 == 0, "rows of the mirror block stay 8-byte aligned");

struct JdResult {
    uint32_t blocks, markers, tries, pad;
};

// ---- the entropy decoder ----

// A lane's place in its stream.  k is the byte that holds the next bit (a data byte, or k == len: the end), off the bits of
// it that are used (0..7), c the block of the MCU, z the zig-zag index that is due (0: the DC difference).
struct State {
    uint32_t k;
    int off, c, z;
};
__device__ __forceinline__ unsigned long long pack(const State& s) {
    return (unsigned long long)s.k | ((unsigned long long)s.off << 32) | ((unsigned long long)s.c << 35) | ((unsigned long long)s.z << 39);
}
__device__ __forceinline__ State unpack(unsigned long long v) {
    return State{(uint32_t)v, (int)((v >> 32) & 7u), (int)((v >> 35) & 15u), (int)((v >> 39) & 63u)};
}

// the component of block kb of the MCU.  kAny: from the frame's table (word); else the three layouts' rule
template <bool kAny>
__device__ __forceinline__ int component_of(int bpm, uint32_t word, int kb) {
    if (kAny) return (int)((word >> (2 * kb)) & 3u);
    const int ny = bpm - 2;
    return (bpm == 1 || kb < ny) ? 0 : kb - ny + 1;
}

struct Reader {
    const uint8_t* __restrict__ p;  // the stream
    uint32_t len, k;
    int off;
    uint32_t cur;  // the byte at k
    int rst;       // an RSTm that was passed and is not yet accounted for (its second byte), else 0
    bool bad;      // a bit was read behind an RSTm that no symbol boundary had accounted for
    bool over;     // a bit was read behind the end

    // k is where a byte is due: fill bytes and RSTm are passed, any other marker is the end
    __device__ __forceinline__ void enter() {
        while (k < len) {  // (every turn but the last moves k forward)
            cur = p[k];
            if (cur != 0xFFu) return;
            const uint32_t n = k + 1 < len ? (uint32_t)p[k + 1] : 0xD9u;
            if (n == 0u) return;  // a data byte 0xFF, its stuffed zero behind it
            if (n == 0xFFu) {
                k += 1;
            } else if (n >= 0xD0u && n <= 0xD7u) {
                if (rst) bad = true;  // (two markers and no symbol between them)
                rst = (int)n;
                k += 2;
            } else {
                k = len;
            }
        }
        k = len;
        cur = 0xFFu;
    }
    __device__ __forceinline__ void next_byte() {
        k += cur == 0xFFu ? 2u : 1u;
        off = 0;
        enter();
    }
    __device__ __forceinline__ bool ended() const { return k >= len; }
    __device__ __forceinline__ uint32_t bit() {  // (ones behind the end)
        if (rst) bad = true;
        if (k >= len) over = true;
        const uint32_t b = (cur >> (7 - off)) & 1u;
        if (k < len && ++off == 8) next_byte();
        return b;
    }
    __device__ __forceinline__ uint32_t bits(int n) {
        uint32_t v = 0;
        for (int i = 0; i < n; ++i) v = (v << 1) | bit();
        return v;
    }
    // at an MCU's end: what is left of the byte is padding if it is all ones and a marker or the end follows.  Any other
    // padding is read as the start of a symbol: in front of EOI that symbol runs over the end and is none (any padding is
    // taken there), in front of an RSTm it runs into the marker: damage (T.81 F.1.2.3 asks for 1-bits, and only 1-bits are
    // never a code, which is what a lane that enters on a guess needs; docs/jpeg_decode_bounds.md, "Padding").
    __device__ __forceinline__ void skip_padding() {
        if (off == 0 || k >= len) return;
        const uint32_t mask = (1u << (8 - off)) - 1u;
        if ((cur & mask) != mask) return;
        const uint32_t nk = k + (cur == 0xFFu ? 2u : 1u);
        if (nk >= len || (p[nk] == 0xFFu && (nk + 1 >= len || p[nk + 1] != 0u))) next_byte();
    }
};

// 0..255, or -1 for sixteen bits that are no code
__device__ __forceinline__ int huff_symbol(Reader& r, const HuffDec* t) {
    int code = 0;
    for (int l = 1; l <= 16; ++l) {
        code = (code << 1) | (int)r.bit();
        if (code <= t->maxcode[l]) return (int)t->vals[(code + t->delta[l]) & 255];
    }
    return -1;
}
__device__ __forceinline__ int extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// Decodes from `st` until a symbol ends at or behind byte `limit` (or the stream ends): `st` becomes that state, `blocks`
// the blocks completed, `markers` the RSTm passed.  kWrite: the coefficients of block first + (blocks so far) are stored
// and the markers' numbers checked; `err` is then what damages the scan.
template <bool kWrite, bool kAny>
__device__ void decode_part(const JdFrame* f, const HuffDec* s_huff, const uint8_t* __restrict__ stream, State& st, uint32_t limit,
                            uint32_t* blocks_out, uint32_t* markers_out, int16_t* __restrict__ coef, uint32_t first, uint32_t total,
                            bool* err_out) {
    Reader r{stream, f->len, st.k, st.off, 0u, 0, false, false};
    if (r.k >= r.len) r.k = r.len, r.cur = 0xFFu, r.off = 0;
    else if (r.k == f->scan && r.off == 0) r.enter();  // the scan's first byte (an RSTm in front of the first MCU stays pending: damage)
    else r.cur = stream[r.k];
    int c = st.c, z = st.z;
    const int bpm = f->bpm;
    const uint32_t word = kAny ? f->comp_word : 0u;
    uint32_t blocks = 0, markers = 0;
    bool err = false;
    // (a symbol is at least one bit, so a part's bits bound the turns; a lane never enters in front of its part)
    for (int turn = 0; turn < kPartBytes * 8 + 16 && r.k < limit && !r.ended(); ++turn) {
        const int comp = component_of<kAny>(bpm, word, c);
        bool done = false, wrong = false;
        if (z == 0) {
            int s = huff_symbol(r, s_huff + comp);
            if (s < 0 || s > 11) {
                wrong = true;
                done = s < 0;
                s = 0;
            }
            const int diff = s ? extend(r.bits(s), s) : 0;
            if (kWrite && first + blocks < total) coef[(size_t)(first + blocks) * 64] = (int16_t)diff;
            z = 1;
        } else {
            const int rs = huff_symbol(r, s_huff + 3 + comp);
            if (rs < 0) {
                wrong = true;
                done = true;
            } else {
                const int run = rs >> 4, s = rs & 15;
                if (s == 0) {
                    if (run == 15) {
                        z += 16;
                        if (z > 64) wrong = true;
                        done = z >= 64;
                    } else {
                        done = true;
                    }
                } else {
                    z += run;
                    if (z > 63) {
                        wrong = true;
                        done = true;
                    } else {
                        const int v = extend(r.bits(s), s);
                        if (kWrite && first + blocks < total) coef[(size_t)(first + blocks) * 64 + kZigzag[z]] = (int16_t)v;
                        done = ++z == 64;
                    }
                }
            }
        }
        if (r.over) break;  // (the stream ended inside the symbol: it is none, and no damage either)
        if (wrong || r.bad) err = true, r.bad = false;
        if (done) {
            z = 0;
            c = c + 1 == bpm ? 0 : c + 1;
            ++blocks;
            if (c == 0) r.skip_padding();
        }
        if (r.rst) {  // a symbol boundary behind an RSTm: a new interval
            if (c != 0 || z != 0) err = true;
            if (kWrite) {
                const uint32_t at = first + blocks, per = (uint32_t)f->ri * (uint32_t)bpm;
                if (per == 0 || at == 0 || at % per != 0 || (uint32_t)r.rst != 0xD0u + ((at / per - 1u) & 7u)) err = true;
            }
            c = z = 0;
            r.rst = 0;
            ++markers;
        }
    }
    if (r.ended()) r.off = 0, c = 0, z = 0;  // (one state for the end)
    st = State{r.k, r.off, c, z};
    *blocks_out = blocks;
    *markers_out = markers;
    if (kWrite) *err_out = err;
}

__device__ __forceinline__ void load_tables(const JdFrame* f, uint32_t* s_words, int tid, int n_threads) {
    const uint32_t* g = reinterpret_cast<const uint32_t*>(f->dc);
    for (int i = tid; i < (int)(6 * sizeof(HuffDec) / 4); i += n_threads) s_words[i] = g[i];
}

// the state of the scan's first part: its first byte (decode_part passes the fill bytes in front of the data)
__device__ __forceinline__ unsigned long long true_start(const JdFrame* f) { return pack(State{f->scan, 0, 0, 0}); }

// state: entry[n] | exit[n] | carry[2][n_wg], n = n_wg * kSyncBlock; part: counts[n] | tries[n] | first[n]
// kAny (here and below): the call has LR_JPEG_ANY_SAMPLING and a frame whose sampling is none of the three layouts; every
// other call gets the kernels without the general geometry.
template <bool kAny>
__global__ __launch_bounds__(kSyncBlock) void jd_sync_kernel(const uint8_t* __restrict__ src, int batch, int n_wg, int round,
                                                             const JdFrame* __restrict__ frames, const int* __restrict__ wg_start,
                                                             unsigned long long* __restrict__ state, uint32_t* __restrict__ part,
                                                             uint32_t* __restrict__ active) {
    __shared__ uint32_t s_huff[6 * sizeof(HuffDec) / 4];
    __shared__ unsigned long long s_entry[kSyncBlock];
    const int wg = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = frame_of_tile(wg_start, batch, wg);
    const JdFrame* f = frames + b;
    const int kw = wg - wg_start[b], i = kw * kSyncBlock + t;
    const bool valid = i < f->n_parts;
    const size_t n = (size_t)n_wg * kSyncBlock, g = (size_t)wg * kSyncBlock + t;
    unsigned long long* entry = state;
    unsigned long long* exitv = state + n;
    const unsigned long long* carry_in = state + 2 * n + (size_t)(round & 1) * n_wg;
    unsigned long long* carry_out = state + 2 * n + (size_t)((round + 1) & 1) * n_wg;
    const uint8_t* stream = src + (size_t)f->src_off;
    load_tables(f, s_huff, t, kSyncBlock);

    unsigned long long last = 0, mine = 0;
    uint32_t counts = 0, tries = 0;
    bool need = false;
    if (valid) {
        if (round == 0) {
            s_entry[t] = i == 0 ? true_start(f) : pack(State{f->scan + (uint32_t)i * kPartBytes, 0, 0, 0});
            need = true;
        } else {
            last = entry[g];
            mine = exitv[g];
            counts = part[g];
            tries = part[n + g];
            s_entry[t] = t == 0 && kw > 0 ? carry_in[wg] : last;
            need = s_entry[t] != last;
        }
    }
    __syncthreads();
    const uint32_t limit = (uint32_t)min((unsigned long long)f->len, (unsigned long long)f->scan + ((unsigned long long)i + 1) * kPartBytes);
    bool any = false;
    for (int turn = 0; turn <= kSyncBlock; ++turn) {  // (every turn but the last settles one more lane, from lane 0 on)
        if (valid && need) {
            last = s_entry[t];
            State st = unpack(last);
            uint32_t blocks, markers;
            decode_part<false, kAny>(f, reinterpret_cast<const HuffDec*>(s_huff), stream, st, limit, &blocks, &markers, nullptr, 0, 0, nullptr);
            mine = pack(st);
            counts = blocks | (markers << 16);
            ++tries;
            need = false;
            any = true;
        }
        __syncthreads();
        bool changed = false;
        if (valid && t + 1 < kSyncBlock && i + 1 < f->n_parts && s_entry[t + 1] != mine) {
            s_entry[t + 1] = mine;
            changed = true;
        }
        if (!__syncthreads_or(changed)) break;
        if (valid && s_entry[t] != last) need = true;
    }
    if (valid) {
        entry[g] = last;
        exitv[g] = mine;
        part[g] = counts;
        part[n + g] = tries;
        if (t == kSyncBlock - 1 && i + 1 < f->n_parts) carry_out[wg + 1] = mine;
    }
    if (__syncthreads_or(any) && t == 0) active[round & 1] = 1u;
}

constexpr int kScanBlock = 256;
// a workgroup per frame: every part's first block, the frame's totals
__global__ __launch_bounds__(kScanBlock) void jd_place_kernel(int n_wg, const JdFrame* __restrict__ frames, const int* __restrict__ wg_start,
                                                              uint32_t* __restrict__ part, JdResult* __restrict__ result) {
    __shared__ uint32_t s_scan[kScanBlock];
    __shared__ uint32_t s_mark[kScanBlock], s_tries[kScanBlock];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const JdFrame* f = frames + b;
    const size_t n = (size_t)n_wg * kSyncBlock, g0 = (size_t)wg_start[b] * kSyncBlock;
    uint32_t carry = 0, marks = 0, most = 0;
    for (int base = 0; base < f->n_parts; base += kScanBlock) {
        const int i = base + tid;
        const uint32_t cm = i < f->n_parts ? part[g0 + i] : 0u, v = cm & 0xFFFFu;
        s_scan[tid] = v;
        __syncthreads();
        for (int d = 1; d < kScanBlock; d <<= 1) {
            const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        if (i < f->n_parts) part[2 * n + g0 + i] = carry + s_scan[tid] - v;
        carry += s_scan[kScanBlock - 1];
        marks += cm >> 16;
        if (i < f->n_parts) most = max(most, part[n + g0 + i]);
        __syncthreads();
    }
    s_mark[tid] = marks;
    s_tries[tid] = most;
    __syncthreads();
    for (int d = kScanBlock / 2; d > 0; d >>= 1) {
        if (tid < d) {
            s_mark[tid] += s_mark[tid + d];
            s_tries[tid] = max(s_tries[tid], s_tries[tid + d]);
        }
        __syncthreads();
    }
    if (tid == 0) result[b] = JdResult{carry, s_mark[0], s_tries[0], 0u};
}

template <bool kAny>
__global__ __launch_bounds__(kSyncBlock) void jd_write_kernel(const uint8_t* __restrict__ src, int batch, int n_wg,
                                                              const JdFrame* __restrict__ frames, const int* __restrict__ wg_start,
                                                              const int* __restrict__ grp_start,
                                                              const unsigned long long* __restrict__ state,
                                                              const uint32_t* __restrict__ part, int16_t* __restrict__ coef,
                                                              uint32_t* __restrict__ damaged) {
    __shared__ uint32_t s_huff[6 * sizeof(HuffDec) / 4];
    const int wg = (int)blockIdx.x, t = (int)threadIdx.x;
    const int b = frame_of_tile(wg_start, batch, wg);
    const JdFrame* f = frames + b;
    const int i = (wg - wg_start[b]) * kSyncBlock + t;
    load_tables(f, s_huff, t, kSyncBlock);
    __syncthreads();
    if (i >= f->n_parts) return;
    const size_t n = (size_t)n_wg * kSyncBlock, g = (size_t)wg * kSyncBlock + t;
    State st = unpack(state[g]);
    const uint32_t limit = (uint32_t)min((unsigned long long)f->len, (unsigned long long)f->scan + ((unsigned long long)i + 1) * kPartBytes);
    uint32_t blocks, markers;
    bool err = false;
    decode_part<true, kAny>(f, reinterpret_cast<const HuffDec*>(s_huff), src + (size_t)f->src_off, st, limit, &blocks, &markers,
                      coef + (size_t)grp_start[b] * 8 * 64, part[2 * n + g], (uint32_t)f->n_mcus * (uint32_t)f->bpm, &err);
    if (err) damaged[b] = 1u;
}

// ---- DC differences to values ----

// the MCUs [m0, m0 + count) in order: kStore = false sums their differences per component into acc, kStore = true stores
// the running values (32-bit sums that wrap, saturated to int16 where stored; legitimate values stay below 2^11)
template <bool kStore, bool kAny>
__device__ __forceinline__ void dc_run(int16_t* __restrict__ coef, int bpm, uint32_t word, int m0, int count, uint32_t (&acc)[3]) {
    for (int m = m0; m < m0 + count; ++m)
        for (int kb = 0; kb < bpm; ++kb) {
            int16_t* at = coef + ((size_t)m * bpm + kb) * 64;
            const int comp = component_of<kAny>(bpm, word, kb);
            acc[comp] += (uint32_t)(int)*at;
            if (kStore) *at = (int16_t)min(max((int)acc[comp], -32768), 32767);
        }
}

template <bool kAny>
__global__ __launch_bounds__(kScanBlock) void jd_dc_kernel(const JdFrame* __restrict__ frames, const int* __restrict__ grp_start,
                                                           int16_t* __restrict__ coef_all) {
    __shared__ uint32_t s_sum[3][kScanBlock];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const JdFrame* f = frames + b;
    int16_t* coef = coef_all + (size_t)grp_start[b] * 8 * 64;
    const int bpm = f->bpm, n_mcus = f->n_mcus;
    const uint32_t word = kAny ? f->comp_word : 0u;
    const int seg = f->ri > 0 ? min(f->ri, n_mcus) : n_mcus, n_seg = (n_mcus + seg - 1) / seg;
    if (n_seg >= kScanBlock / 4) {  // many intervals: a thread takes whole ones
        for (int s = tid; s < n_seg; s += kScanBlock) {
            uint32_t acc[3] = {0u, 0u, 0u};
            dc_run<true, kAny>(coef, bpm, word, s * seg, min(seg, n_mcus - s * seg), acc);
        }
        return;
    }
    for (int s = 0; s < n_seg; ++s) {  // few: the workgroup scans each
        const int m0 = s * seg, nm = min(seg, n_mcus - m0), per = (nm + kScanBlock - 1) / kScanBlock;
        const int mine0 = min(tid * per, nm), mine_n = min(per, nm - mine0);
        uint32_t acc[3] = {0u, 0u, 0u};
        dc_run<false, kAny>(coef, bpm, word, m0 + mine0, mine_n, acc);
        for (int c = 0; c < 3; ++c) s_sum[c][tid] = acc[c];
        __syncthreads();
        for (int d = 1; d < kScanBlock; d <<= 1) {
            uint32_t add[3];
            for (int c = 0; c < 3; ++c) add[c] = tid >= d ? s_sum[c][tid - d] : 0u;
            __syncthreads();
            for (int c = 0; c < 3; ++c) s_sum[c][tid] += add[c];
            __syncthreads();
        }
        for (int c = 0; c < 3; ++c) acc[c] = s_sum[c][tid] - acc[c];  // what lies in front of this thread's run
        dc_run<true, kAny>(coef, bpm, word, m0 + mine0, mine_n, acc);
        __syncthreads();
    }
}

// ---- the inverse transform ----

// one pass over eight values: out[x] = sum_u T[u][x] s[u] (every |s| < 2^17 and every sum < 2^31)
__device__ __forceinline__ void idct8(const int (&s)[8], int (&out)[8]) {
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        int e = 0, o = 0;
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            e += __mul24(kDctHalf[u][x], s[u]);
            o += __mul24(kDctHalf[u + 1][x], s[u + 1]);
        }
        out[x] = e + o;
        out[7 - x] = e - o;
    }
}

// v[i] becomes the sum of cell i of 1 << l neighbours (l = 0..3); the entries from 8 >> l on are left over
__device__ __forceinline__ void sum_cells(int (&v)[8], int l) {
    if (l >= 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[2 * i] + v[2 * i + 1];
    }
    if (l >= 2) {
        v[0] = v[0] + v[1];
        v[1] = v[2] + v[3];
    }
    if (l >= 3) v[0] = v[0] + v[1];
}

// kScaled (with kAny: the general geometry throughout): the call has LR_JPEG_SCALED and a frame of scale 2, 4 or 8.  The
// block's 64 samples are then averaged over cells of rx x ry, the reductions of the block's component -- down a column in
// the registers of the lane that holds it, across a row behind the transpose -- and the (8 / rx) x (8 / ry) reduced samples
// stored densely, row by row, in the slot's first bytes (a frame of scale 1: all 64, as ever).
template <bool kAny, bool kScaled>
__global__ __launch_bounds__(kWave) void jd_transform_kernel(int batch, int n_groups, int luma_only, const JdFrame* __restrict__ frames,
                                                             const int* __restrict__ grp_start, int16_t* __restrict__ coef) {
    __shared__ int s_t[8][65];
    const int lane = (int)threadIdx.x, k = lane >> 3, r = lane & 7;
    for (int grp = (int)blockIdx.x; grp < n_groups; grp += (int)gridDim.x) {
        const int b = frame_of_tile(grp_start, batch, grp);
        const JdFrame* f = frames + b;
        const int blk = (grp - grp_start[b]) * 8 + k;
        const int comp = component_of<kAny>(f->bpm, kAny ? f->comp_word : 0u, blk % f->bpm);
        const bool valid = blk < f->n_mcus * f->bpm && !(luma_only && comp != 0);
        int16_t* slot = coef + ((size_t)grp * 8 + k) * 64;
        int s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a[8];
        if (valid) {  // row r of the block: F[r][u], times its divisors
            const uint4 v = *reinterpret_cast<const uint4*>(slot + r * 8);
            const uint32_t words[4] = {v.x, v.y, v.z, v.w};
            const uint8_t* q = f->q[comp] + r * 8;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int cf = (int)(int16_t)((u & 1) ? (words[u >> 1] >> 16) : (words[u >> 1] & 0xFFFFu));
                s[u] = min(max(cf * (int)q[u], -kCoefLimit), kCoefLimit);
            }
        }
        idct8(s, a);
#pragma unroll
        for (int x = 0; x < 8; ++x) s_t[k][r * 8 + x] = min(max((a[x] + (1 << (kMidShift - 1))) >> kMidShift, -kMidLimit), kMidLimit);
        __syncthreads();
#pragma unroll
        for (int v = 0; v < 8; ++v) s[v] = s_t[k][v * 8 + r];  // column r
        idct8(s, a);
        __syncthreads();
        const int lx = kScaled ? 3 - f->sbx[comp] : 0, ly = kScaled ? 3 - f->sby[comp] : 0;  // log2 of the component's cells
        if (kScaled) {  // column r is in registers: its cells' sums, ry samples each, go to LDS in the samples' place
            int v[8];
#pragma unroll
            for (int y = 0; y < 8; ++y) v[y] = min(max(((a[y] + (1 << (kEndShift - 1))) >> kEndShift) + 128, 0), 255);
            sum_cells(v, ly);
#pragma unroll
            for (int y = 0; y < 8; ++y) s_t[k][y * 8 + r] = v[y];  // (rows from 8 >> ly on are not read)
        } else {
#pragma unroll
            for (int y = 0; y < 8; ++y) s_t[k][y * 8 + r] = min(max(((a[y] + (1 << (kEndShift - 1))) >> kEndShift) + 128, 0), 255);
        }
        __syncthreads();
        if (kScaled) {
            if (valid && r < (8 >> ly)) {  // row r of the reduced samples: the cells' sums across, the rounded means, 8 >> lx bytes
                int w[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) w[x] = s_t[k][r * 8 + x];
                sum_cells(w, lx);
                const int shift = lx + ly, half = (1 << shift) >> 1;
                uint32_t lo = 0, hi = 0;
#pragma unroll
                for (int x = 0; x < 4; ++x) {  // (entries from 8 >> lx on are no means; they lie above the bytes that are stored)
                    lo |= (uint32_t)(((w[x] + half) >> shift) & 255) << (8 * x);
                    hi |= (uint32_t)(((w[4 + x] + half) >> shift) & 255) << (8 * x);
                }
                // rows are dense, (8 >> lx) bytes each: row r < 8 >> ly ends at or below byte 64 of the slot, all of which was read above
                uint8_t* out = reinterpret_cast<uint8_t*>(slot) + (r << (3 - lx));
                if (lx == 0) *reinterpret_cast<uint2*>(out) = make_uint2(lo, hi);
                else if (lx == 1) *reinterpret_cast<uint32_t*>(out) = lo;
                else if (lx == 2) *reinterpret_cast<uint16_t*>(out) = (uint16_t)lo;
                else *out = (uint8_t)lo;
            }
        } else if (valid) {  // row r of the samples, into the block's first 64 bytes (all of which were read above)
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                lo |= (uint32_t)s_t[k][r * 8 + x] << (8 * x);
                hi |= (uint32_t)s_t[k][r * 8 + 4 + x] << (8 * x);
            }
            *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(slot) + r * 8) = make_uint2(lo, hi);
        }
        __syncthreads();
    }
}

// ---- upsampling, colour, the picture ----

// sample (x, y) of component comp, in its own grid.  kAny: the MCU is the block's column and row shifted by the component's
// factors, the block in it row (by mod v) and column (bx mod h) of the component's v x h blocks
// kScaled: (x, y) in the component's reduced grid, a block's reduced samples being (1 << sby) rows of (1 << sbx)
template <bool kAny, bool kScaled = false>
__device__ __forceinline__ int sample_at(const uint8_t* __restrict__ blocks, const JdFrame* f, int comp, int x, int y) {
    const int sx = kScaled ? f->sbx[comp] : 3, sy = kScaled ? f->sby[comp] : 3;
    const int bx = x >> sx, by = y >> sy;
    size_t blk;
    if (kAny) {
        const int hsh = f->hsh[comp], vsh = f->vsh[comp];
        blk = ((size_t)(by >> vsh) * f->mcus_x + (bx >> hsh)) * f->bpm + f->first[comp] + ((by & ((1 << vsh) - 1)) << hsh) + (bx & ((1 << hsh) - 1));
    } else if (comp == 0) blk = ((size_t)(by / f->vs) * f->mcus_x + bx / f->hs) * f->bpm + (by % f->vs) * f->hs + bx % f->hs;
    else blk = ((size_t)by * f->mcus_x + bx) * f->bpm + f->hs * f->vs + comp - 1;
    return (int)blocks[blk * 128 + ((y & ((1 << sy) - 1)) << sx) + (x & ((1 << sx) - 1))];
}

// the chrominance at pixel (x, y): centred triangle filters, the edges replicated at the component's own size
// kAny, per axis by the ratio of the largest factor to the component's: 1 the sample, 2 the triangle, 4 the sample x >> 2
// (near and far are then one sample, and the triangle over the other axis is taken over the replicated samples)
// kScaled: (x, y) a pixel of the reduced picture, the ratios those that the reduction leaves, the clamps the reduced grid's
template <bool kAny, bool kScaled = false>
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ blocks, const JdFrame* f, int comp, int x, int y) {
    if (kAny) {
        const int rxs = kScaled ? f->srx[comp] : f->rxs[comp], rys = kScaled ? f->sry[comp] : f->rys[comp];
        const int cw = kScaled ? f->scw[comp] : f->cw[comp], ch = kScaled ? f->sch[comp] : f->ch[comp];
        const int nx = x >> rxs, ny = y >> rys;
        if (rxs != 1 && rys != 1) return sample_at<true, kScaled>(blocks, f, comp, nx, ny);
        const int fx = min(max(nx + ((x & 1) ? 1 : -1), 0), cw - 1), fy = min(max(ny + ((y & 1) ? 1 : -1), 0), ch - 1);
        if (rys != 1) return (3 * sample_at<true, kScaled>(blocks, f, comp, nx, ny) + sample_at<true, kScaled>(blocks, f, comp, fx, ny) + 2) >> 2;
        if (rxs != 1) return (3 * sample_at<true, kScaled>(blocks, f, comp, nx, ny) + sample_at<true, kScaled>(blocks, f, comp, nx, fy) + 2) >> 2;
        return (9 * sample_at<true, kScaled>(blocks, f, comp, nx, ny) + 3 * sample_at<true, kScaled>(blocks, f, comp, fx, ny) +
                3 * sample_at<true, kScaled>(blocks, f, comp, nx, fy) + sample_at<true, kScaled>(blocks, f, comp, fx, fy) + 8) >> 4;
    }
    if (f->hs == 1) return sample_at<false>(blocks, f, comp, x, y);
    const int cw = (f->w + 1) >> 1;
    const int nx = x >> 1, fx = min(max(nx + ((x & 1) ? 1 : -1), 0), cw - 1);
    if (f->vs == 1) return (3 * sample_at<false>(blocks, f, comp, nx, y) + sample_at<false>(blocks, f, comp, fx, y) + 2) >> 2;
    const int ch = (f->h + 1) >> 1;
    const int ny = y >> 1, fy = min(max(ny + ((y & 1) ? 1 : -1), 0), ch - 1);
    return (9 * sample_at<false>(blocks, f, comp, nx, ny) + 3 * sample_at<false>(blocks, f, comp, fx, ny) + 3 * sample_at<false>(blocks, f, comp, nx, fy) +
            sample_at<false>(blocks, f, comp, fx, fy) + 8) >> 4;
}

// pixel (x, y) of the stored picture: its luminance (kFormat LR_PIX_U8: all that is computed) and its three colour bytes
template <int kFormat, bool kAny, bool kScaled>
__device__ __forceinline__ void pixel_at(const uint8_t* __restrict__ blocks, const JdFrame* f, int x, int y, int (&c)[3]) {
    const int yy = sample_at<kAny, kScaled>(blocks, f, 0, x, y);
    c[0] = c[1] = c[2] = yy;
    if (kFormat == LR_PIX_U8X3 && f->comps == 3) {  // the IJG fixed-point inverse of the encoder's rule
        const int cb = chroma_at<kAny, kScaled>(blocks, f, 1, x, y) - 128, cr = chroma_at<kAny, kScaled>(blocks, f, 2, x, y) - 128;
        c[0] = min(max(yy + ((91881 * cr + 32768) >> 16), 0), 255);
        c[1] = min(max(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
        c[2] = min(max(yy + ((116130 * cb + 32768) >> 16), 0), 255);
    }
}

// the stored picture's size: kScaled the reduced one
template <bool kScaled>
__device__ __forceinline__ int pic_w(const JdFrame* f) { return kScaled ? f->sw : f->w; }
template <bool kScaled>
__device__ __forceinline__ int pic_h(const JdFrame* f) { return kScaled ? f->sh : f->h; }

// The EXIF orientations, S the stored w x h picture and O the one written:
//   2: O[y][x] = S[y][w-1-x]    3: S[h-1-y][w-1-x]    4: S[h-1-y][x]                 (O is w x h)
//   5: O[y][x] = S[x][y]        6: S[h-1-x][y]        7: S[h-1-x][w-1-y]    8: S[x][w-1-y]    (O is h x w)
// kTurn: the batch has a frame of orientation 5..8.  A batch without one -- every call that does not ask for orientations
// among them -- gets the kernel without the transposing path, its LDS and its registers.
// kScaled (with kAny): the stored picture is the reduced one, sw x sh, and its tiles are counted over that.
template <int kFormat, bool kTurn, bool kAny, bool kScaled>
__global__ __launch_bounds__(kTileW * kTileH) void jd_output_kernel(int batch, int n_tiles, const JdFrame* __restrict__ frames,
                                                                    const int* __restrict__ tile_start, const int* __restrict__ grp_start,
                                                                    const int16_t* __restrict__ coef, uint8_t* __restrict__ dst) {
    constexpr int kBpp = kFormat == LR_PIX_U8 ? 1 : 3;
    // a square of finished bytes, [stored x][stored y]: the pitch is an odd count of words (9 or 25), so the 32 lanes of a
    // store group, one stored x each, fall on 32 different banks
    constexpr int kPitch = kSquare * kBpp + 4;
    __shared__ uint8_t s_sq[kTurn ? kSquare * kPitch : 4];
    XcdBand band(n_tiles);
    for (int tile; band.next(&tile);) {
        const int b = frame_of_tile(tile_start, batch, tile);
        const JdFrame* f = frames + b;
        const int local = tile - tile_start[b], o = f->orient;
        const uint8_t* blocks = reinterpret_cast<const uint8_t*>(coef + (size_t)grp_start[b] * 8 * 64);
        const int tx = (int)threadIdx.x % kTileW, ty = (int)threadIdx.x / kTileW;
        int c[3];
        if (!kTurn || o < 5) {  // rows stay rows: a thread per pixel, its place mirrored
            const int tiles_x = (pic_w<kScaled>(f) + kTileW - 1) / kTileW;
            const int x = (local % tiles_x) * kTileW + tx, y = (local / tiles_x) * kTileH + ty;
            if (x >= pic_w<kScaled>(f) || y >= pic_h<kScaled>(f)) continue;
            pixel_at<kFormat, kAny, kScaled>(blocks, f, x, y, c);
            const int ox = (o == 2 || o == 3) ? pic_w<kScaled>(f) - 1 - x : x, oy = (o == 3 || o == 4) ? pic_h<kScaled>(f) - 1 - y : y;
            uint8_t* px = dst + (size_t)f->dst_off + (size_t)oy * (size_t)f->dst_row + (size_t)ox * kBpp;
#pragma unroll
            for (int i = 0; i < kBpp; ++i) px[i] = (uint8_t)c[i];
            continue;
        }
        if (!kTurn) continue;  // (not reached: the code below is left out of that kernel)
        // rows become columns (the branch is the workgroup's: every lane reaches both barriers)
        const int tiles_x = (pic_w<kScaled>(f) + kSquare - 1) / kSquare;
        const int x0 = (local % tiles_x) * kSquare, y0 = (local / tiles_x) * kSquare;
#pragma unroll
        for (int pass = 0; pass < kSquare / kTileH; ++pass) {
            const int j = ty + pass * kTileH;
            if (x0 + tx < pic_w<kScaled>(f) && y0 + j < pic_h<kScaled>(f)) {
                pixel_at<kFormat, kAny, kScaled>(blocks, f, x0 + tx, y0 + j, c);
#pragma unroll
                for (int i = 0; i < kBpp; ++i) s_sq[tx * kPitch + j * kBpp + i] = (uint8_t)c[i];
            }
        }
        __syncthreads();
        // stored column x0 + i is row oy of the picture, stored row y0 + j its pixel ox; lane order follows ox
        const bool flip_x = o == 6 || o == 7, flip_y = o == 7 || o == 8;
#pragma unroll 4  // (all twelve passes of u8x3 unrolled cost the kernel half its occupancy)
        for (int pass = 0; pass < kSquare * kBpp / kTileH; ++pass) {
            const int at = (int)threadIdx.x + pass * (kTileW * kTileH);
            const int i = at / (kSquare * kBpp), k = at % (kSquare * kBpp), ch = k % kBpp;
            const int j = flip_x ? kSquare - 1 - k / kBpp : k / kBpp;
            if (x0 + i < pic_w<kScaled>(f) && y0 + j < pic_h<kScaled>(f)) {
                const int ox = flip_x ? pic_h<kScaled>(f) - 1 - (y0 + j) : y0 + j, oy = flip_y ? pic_w<kScaled>(f) - 1 - (x0 + i) : x0 + i;
                dst[(size_t)f->dst_off + (size_t)oy * (size_t)f->dst_row + (size_t)ox * kBpp + ch] = s_sq[i * kPitch + j * kBpp + ch];
            }
        }
        __syncthreads();
    }
}

// ---- the host's part: the headers, the check of the frame table ----

struct Header {
    int status = kNotJpeg;
    std::string message = "no SOI";
    int w = 0, h = 0, comps = 0, layout = 0, ri = 0;
    int hf[3] = {1, 1, 1}, vf[3] = {1, 1, 1};  // the sampling factors the decoder works with (1 x 1 for one component)
    bool general = false;                      // a sampling that only LR_JPEG_ANY_SAMPLING admits
    int orientation = 0;  // the EXIF tag 0x0112 of the first Exif segment, 1..8; 0: none that counts
    uint32_t scan = 0;
    uint8_t q[3][64];
    HuffDec dc[3], ac[3];
};

void make_decoder(const uint8_t* bits, const uint8_t* vals, int count, HuffDec* t) {
    std::memset(t, 0, sizeof *t);
    std::memcpy(t->vals, vals, (size_t)count);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        // (a table that claims more codes than l bits have: the codes beyond them do not exist)
        const int usable = std::max(0, std::min(n, (1 << l) - code));
        t->maxcode[l] = usable > 0 ? code + usable - 1 : -1;
        t->delta[l] = k - code;
        code = (code + n) << 1;
        k += n;
        if (code > (1 << 17)) code = 1 << 17;
    }
    t->maxcode[0] = t->maxcode[17] = -1;
}

// The orientation an Exif APP1 payload tells: "Exif\0\0", then a TIFF block -- the byte order ("II*\0" little, "MM\0*" big
// endian), the offset of IFD0 from the block's start, there a 16-bit count and 12-byte entries (tag, type, count, value).
// The entry with tag 0x0112 counts if its type is 3 (SHORT), its count 1 and its value, the value field's first two bytes,
// 1..8.  Everything else is 0, none: a block or an IFD that does not lie within the n bytes, another type, count or value.
// Only IFD0 is read, and no read goes beyond t[0, n).
int exif_orientation(const uint8_t* t, size_t n) {
    if (n < 8) return 0;
    const bool little = t[0] == 'I' && t[1] == 'I' && t[2] == 0x2A && t[3] == 0;
    if (!little && !(t[0] == 'M' && t[1] == 'M' && t[2] == 0 && t[3] == 0x2A)) return 0;
    auto u16 = [&](size_t at) { return little ? (uint32_t)t[at] | ((uint32_t)t[at + 1] << 8) : ((uint32_t)t[at] << 8) | (uint32_t)t[at + 1]; };
    const size_t ifd = ((size_t)u16(little ? 6 : 4) << 16) | u16(little ? 4 : 6);
    if (ifd > n - 2) return 0;
    const size_t count = u16(ifd);
    if (count * 12 > n - 2 - ifd) return 0;
    for (size_t i = 0; i < count; ++i) {
        const size_t at = ifd + 2 + 12 * i;
        if (u16(at) != 0x0112) continue;
        const bool one = little ? (t[at + 4] == 1 && !t[at + 5] && !t[at + 6] && !t[at + 7]) : (!t[at + 4] && !t[at + 5] && !t[at + 6] && t[at + 7] == 1);
        const uint32_t v = u16(at + 8);
        return u16(at + 2) == 3 && one && v >= 1 && v <= 8 ? (int)v : 0;
    }
    return 0;
}

// the stream d[0, n) up to the first byte of its scan; any: LR_JPEG_ANY_SAMPLING
void read_header(const uint8_t* d, size_t n, bool any, Header& hd) {
    auto fail = [&](int status, const std::string& what) {
        hd.status = status;
        hd.message = what;
    };
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(kNotJpeg, "no SOI");
    struct Table {
        bool have = false;
        uint8_t bits[16], vals[256];
        int count = 0;
    };
    std::vector<Table> ht(8);
    bool have_q[4] = {false, false, false, false};
    uint8_t qt[4][64];
    const uint8_t* sof = nullptr;
    size_t p = 2;
    const uint8_t* seg = nullptr;
    size_t seg_len = 0;
    bool have_exif = false;
    bool have_jfif = false;
    int adobe = -1;  // the transform byte of the last Adobe APP14, -1: none
    for (;;) {
        if (p >= n) return fail(kNotJpeg, "truncated before SOS");
        if (d[p] != 0xFF) return fail(kNotJpeg, "no marker where one is due");
        while (p < n && d[p] == 0xFF) ++p;
        if (p >= n) return fail(kNotJpeg, "truncated before SOS");
        const int m = d[p++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9) return fail(kNotJpeg, "EOI before SOS");
        if (p + 2 > n) return fail(kNotJpeg, "truncated before SOS");
        const size_t length = ((size_t)d[p] << 8) | d[p + 1];
        if (length < 2 || p + length > n) return fail(kNotJpeg, "truncated before SOS");
        seg = d + p + 2;
        seg_len = length - 2;
        p += length;
        if (m == 0xDB) {
            for (size_t s = 0; s < seg_len; s += 65) {
                const int pq = seg[s] >> 4, tq = seg[s] & 15;
                if (pq != 0) return fail(kUnsupported, "16-bit quantisation table");
                if (tq > 3 || s + 65 > seg_len) return fail(kNotJpeg, "bad DQT");
                for (int i = 0; i < 64; ++i) qt[tq][kZigzagOrder[i]] = seg[s + 1 + i];
                have_q[tq] = true;
            }
        } else if (m == 0xC4) {
            for (size_t s = 0; s < seg_len;) {
                if (s + 17 > seg_len) return fail(kNotJpeg, "bad DHT");
                const int tc = seg[s] >> 4, th = seg[s] & 15;
                int count = 0;
                for (int i = 0; i < 16; ++i) count += seg[s + 1 + i];
                if (tc > 1 || th > 3 || count > 256 || s + 17 + count > seg_len) return fail(kNotJpeg, "bad DHT");
                Table& t = ht[(size_t)(tc * 4 + th)];
                t.have = true;
                t.count = count;
                std::memcpy(t.bits, seg + s + 1, 16);
                std::memcpy(t.vals, seg + s + 17, (size_t)count);
                s += 17 + (size_t)count;
            }
        } else if (m == 0xDD) {
            if (seg_len != 2) return fail(kNotJpeg, "bad DRI");
            hd.ri = (seg[0] << 8) | seg[1];
        } else if (m == 0xC0 || m == 0xC1) {
            if (sof) return fail(kUnsupported, "more than one frame header");
            if (seg_len < 6 || seg_len != 6 + 3 * (size_t)seg[5]) return fail(kNotJpeg, "bad SOF");
            sof = seg;
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC8) {  // (0xC4 was handled above)
            if (m != 0xCC && seg_len >= 6) {  // (the size and the components are told all the same)
                hd.h = (seg[1] << 8) | seg[2];
                hd.w = (seg[3] << 8) | seg[4];
                hd.comps = seg[5];
            }
            if (m == 0xC2) return fail(kUnsupported, "progressive (SOF2)");
            return fail(kUnsupported, "arithmetic, lossless or hierarchical coding (SOF" + std::to_string(m - 0xC0) + ")");
        } else if (m == 0xE1) {  // the first Exif segment tells the orientation, whatever it holds; XMP and the like are skipped
            if (!have_exif && seg_len >= 6 && std::memcmp(seg, "Exif\0\0", 6) == 0) {
                have_exif = true;
                hd.orientation = exif_orientation(seg + 6, seg_len - 6);
            }
        } else if (m == 0xE0) {
            if (seg_len >= 5 && std::memcmp(seg, "JFIF\0", 5) == 0) have_jfif = true;
        } else if (m == 0xEE) {
            if (seg_len >= 12 && std::memcmp(seg, "Adobe", 5) == 0) adobe = seg[11];
        } else if (m == 0xDA) {
            break;
        }
    }
    if (!sof) return fail(kNotJpeg, "SOS before SOF");
    if (sof[0] != 8) return fail(kUnsupported, std::to_string((int)sof[0]) + "-bit precision");
    hd.h = (sof[1] << 8) | sof[2];
    hd.w = (sof[3] << 8) | sof[4];
    const int nc = sof[5];
    if (hd.w < 1 || hd.h < 1) return fail(kUnsupported, "a size of 0 (DNL)");
    hd.comps = nc;
    if (nc != 1 && nc != 3) return fail(kUnsupported, std::to_string(nc) + " components");
    // libjpeg's rule for three components (default_decompress_parms): a JFIF segment says YCbCr; else an Adobe segment
    // decides (transform 0: RGB); else the ids 'R', 'G', 'B' say RGB.  The output pass knows YCbCr's colour rule alone: an
    // RGB file is refused.
    if (nc == 3 && !have_jfif && adobe == 0) return fail(kUnsupported, "an RGB file (Adobe segment with transform 0 and no JFIF segment)");
    if (nc == 3 && !have_jfif && adobe < 0 && sof[6] == 'R' && sof[9] == 'G' && sof[12] == 'B')
        return fail(kUnsupported, "an RGB file (component ids 'R', 'G', 'B' and neither a JFIF nor an Adobe segment)");
    if (nc == 3) {
        const int y = sof[7], cb = sof[10], cr = sof[13];
        const bool known = cb == 0x11 && cr == 0x11 && (y == 0x22 || y == 0x11 || y == 0x21);
        if (!known && !any) return fail(kUnsupported, "sampling other than 4:2:0, 4:4:4, 4:2:2");
        if (!known) {  // every factor 1, 2 or 4; component 0 the largest; at most 10 blocks to the MCU (T.81 B.2.3)
            int sum = 0;
            for (int i = 0; i < 3; ++i) {
                const int hi = sof[7 + 3 * i] >> 4, vi = sof[7 + 3 * i] & 15;
                if ((hi != 1 && hi != 2 && hi != 4) || (vi != 1 && vi != 2 && vi != 4))
                    return fail(kUnsupported, "a sampling factor other than 1, 2 or 4");
                if (hi > (y >> 4) || vi > (y & 15)) return fail(kUnsupported, "luminance sampled below chrominance");
                sum += hi * vi;
            }
            if (sum > 10) return fail(kUnsupported, "more than 10 blocks to the MCU");
        }
        for (int i = 0; i < 3; ++i) hd.hf[i] = sof[7 + 3 * i] >> 4, hd.vf[i] = sof[7 + 3 * i] & 15;
        hd.general = !known;
        hd.layout = !known ? y : (y == 0x22 ? kL420 : (y == 0x11 ? kL444 : kL422));  // (a sampling byte is never 0, 1 or 2)
    }
    if (seg_len < 1 || seg_len != 4 + 2 * (size_t)seg[0]) return fail(kNotJpeg, "bad SOS");
    if (seg[0] != nc) return fail(kUnsupported, "a non-interleaved or multi-scan file");
    for (int i = 0; i < nc; ++i) {
        const int cs = seg[1 + 2 * i], td = seg[2 + 2 * i] >> 4, ta = seg[2 + 2 * i] & 15, tq = sof[8 + 3 * i];
        if (cs != sof[6 + 3 * i]) return fail(kUnsupported, "the scan's components are not the frame's, in order");
        if (tq > 3 || td > 3 || ta > 3 || !have_q[tq] || !ht[(size_t)td].have || !ht[(size_t)(4 + ta)].have)
            return fail(kUnsupported, "a missing table");
        std::memcpy(hd.q[i], qt[tq], 64);
        make_decoder(ht[(size_t)td].bits, ht[(size_t)td].vals, ht[(size_t)td].count, &hd.dc[i]);
        make_decoder(ht[(size_t)(4 + ta)].bits, ht[(size_t)(4 + ta)].vals, ht[(size_t)(4 + ta)].count, &hd.ac[i]);
    }
    if (seg[seg_len - 3] != 0 || seg[seg_len - 2] != 63 || seg[seg_len - 1] != 0)
        return fail(kUnsupported, "a spectral selection or successive approximation");
    hd.scan = (uint32_t)p;
    hd.status = kOk;
    hd.message.clear();
}

}  // namespace

int ctx_decode_jpeg(lr_context* c, const void* d_src, const void* h_src, size_t src_bytes, int format, const double* T, int batch,
                    void* d_dst, size_t dst_bytes, int32_t* info) {
    const bool any_sampling = (format & LR_JPEG_ANY_SAMPLING) != 0;
    const bool scaled = (format & LR_JPEG_SCALED) != 0;
    format &= ~(LR_JPEG_ANY_SAMPLING | LR_JPEG_SCALED);
    auto fail = [](const std::string& what) {
        set_error("lr_decode_jpeg_device: " + what);
        return 1;
    };
    auto fail_at = [&](int b, int entry, const char* what) {
        return fail("frame " + std::to_string(b) + ": entry [" + std::to_string(entry) + "] " + what);
    };
    const bool probe = d_dst == nullptr;
    if (!probe && !c) return fail("no context");
    if (!h_src || !T || !info || (!probe && !d_src)) return fail("null pointer (source, its host copy, frame table or info)");
    if (batch < 1) return fail("batch < 1");
    if (format != LR_PIX_U8 && format != LR_PIX_U8X3) return fail("format is LR_PIX_U8 or LR_PIX_U8X3");
    if (!probe) {
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
        if (s0 < d0 + dst_bytes && d0 < s0 + src_bytes) return fail("the destination region overlaps the source region");
    }

    // the table, as a whole
    const uint64_t bpp = format == LR_PIX_U8 ? 1 : 3;
    struct Entry {
        uint64_t off, len, dst_off, dst_row, w, h;
        bool orient;
        int scale;  // the scale denominator: 1, 2, 4 or 8
    };
    std::vector<Entry> en((size_t)batch);
    std::vector<std::pair<uint64_t, uint64_t>> extent;
    std::vector<int> extent_of;
    for (int b = 0; b < batch; ++b) {
        const double* t = T + (size_t)b * 8;
        Entry& e = en[(size_t)b];
        if (!table_integer(t[0], 0, kExact, &e.off)) return fail_at(b, 0, "(stream offset) is not an integer from 0 to 2^53");
        if (!table_integer(t[1], 0, 2147483632.0, &e.len)) return fail_at(b, 1, "(stream length) is not an integer from 0 to 2^31 - 16");
        if (!table_integer(t[2], 0, kExact, &e.dst_off)) return fail_at(b, 2, "(picture offset) is not an integer from 0 to 2^53");
        if (!table_integer(t[4], probe ? 0 : 1, 65535, &e.w)) return fail_at(b, 4, "(width) is not an integer from 1 to 65535");
        if (!table_integer(t[5], probe ? 0 : 1, 65535, &e.h)) return fail_at(b, 5, "(height) is not an integer from 1 to 65535");
        if ((e.w == 0) != (e.h == 0)) return fail_at(b, 4, "(width) and [5] (height): one is 0 and the other is not");
        if (!table_integer(t[3], e.w ? (double)(e.w * bpp) : 0.0, kExact, &e.dst_row))
            return fail_at(b, 3, "(row stride) is not an integer from a row's bytes to 2^53");
        if (!scaled && !(t[6] == 0.0)) return fail_at(b, 6, "is reserved and must be 0");
        if (!(t[6] == 0.0 || t[6] == 1.0 || t[6] == 2.0 || t[6] == 4.0 || t[6] == 8.0))
            return fail_at(b, 6, "(scale denominator) is 0 or 1 (as stored), 2, 4 or 8");
        e.scale = t[6] == 0.0 ? 1 : (int)t[6];
        if (!(t[7] == 0.0 || t[7] == 1.0)) return fail_at(b, 7, "(EXIF orientation) is 0 (as stored) or 1 (applied)");
        e.orient = t[7] == 1.0;
        uint64_t end;
        if (__builtin_add_overflow(e.off, e.len, &end) || end > src_bytes)
            return fail_at(b, 0, "(stream offset): the stream reaches beyond src_bytes");
        if (e.w) {
            if (__builtin_mul_overflow(e.h - 1, e.dst_row, &end) || __builtin_add_overflow(end, e.dst_off, &end) ||
                __builtin_add_overflow(end, e.w * bpp, &end) || end > dst_bytes)
                return fail_at(b, 2, "(picture offset): the picture reaches beyond dst_bytes");
            extent.push_back({e.dst_off, end});
            extent_of.push_back(b);
        }
    }
    {
        std::vector<std::pair<uint64_t, uint64_t>> sorted = extent;
        if (const size_t at = extents_overlap(sorted)) {
            size_t which = 0;
            while (extent[which] != sorted[at]) ++which;
            return fail_at(extent_of[which], 2, "(picture offset): two frames' extents overlap");
        }
    }

    // the headers; what the device gets are the frames of status 0
    std::vector<JdFrame> fr;
    std::vector<int> frame_of;  // the caller's index of a device frame
    std::vector<int> grp_start, wg_start, tile_start;
    std::vector<int32_t> rows((size_t)batch * 8, 0);
    int64_t n_groups = 0, n_wg = 0, n_tiles = 0;
    int most_wg = 0;
    bool general = false;  // a frame that needs the kAny instantiations
    bool reduced = false;  // a frame of scale 2, 4 or 8: the kScaled instantiations
    Header hd;
    for (int b = 0; b < batch; ++b) {
        const Entry& e = en[(size_t)b];
        hd = Header{};
        read_header(static_cast<const uint8_t*>(h_src) + e.off, (size_t)e.len, any_sampling, hd);
        // the picture as written: with entry [7] the orientation the file tells (1 if none), and its size swapped for 5..8
        const int orient = e.orient ? std::max(hd.orientation, 1) : 0;
        // (and with LR_JPEG_SCALED the reduced one, reduced before it is turned)
        const int sw = lr_jpeg_scaled_size(hd.w, e.scale), sh = lr_jpeg_scaled_size(hd.h, e.scale);
        const int out_w = orient >= 5 ? sh : sw, out_h = orient >= 5 ? sw : sh;
        if (hd.status == kOk && e.w && ((uint64_t)out_w != e.w || (uint64_t)out_h != e.h)) {
            hd.status = kSizeMismatch;
            hd.message = "the stream is " + std::to_string(out_w) + " x " + std::to_string(out_h) + (e.scale > 1 ? " at 1/" + std::to_string(e.scale) : std::string()) + (orient >= 5 ? " (turned by its orientation)" : "");
        }
        int32_t* row = rows.data() + (size_t)b * 8;
        row[0] = out_w;
        row[1] = out_h;
        row[7] = orient;
        row[2] = hd.comps;
        row[3] = hd.layout;
        row[4] = hd.ri;
        row[5] = hd.status;
        if (hd.status != kOk) {
            set_error("lr_decode_jpeg_device: frame " + std::to_string(b) + ": status " + std::to_string(hd.status) + ": " + hd.message);
            continue;
        }
        if (probe) continue;
        JdFrame f;
        std::memset(&f, 0, sizeof f);
        f.src_off = e.off;
        f.dst_off = e.dst_off;
        f.dst_row = e.dst_row;
        f.len = (uint32_t)e.len;
        f.scan = hd.scan;
        f.w = hd.w;
        f.h = hd.h;
        f.comps = hd.comps;
        f.layout = hd.layout;
        f.ri = hd.ri;
        // an MCU is 8 Hmax x 8 Vmax pixels, component 0 having the largest factors; its blocks come component by component,
        // each as v_i rows of h_i blocks (T.81 A.2.3).  (For the three layouts this is what it was: hs x vs + 2 blocks.)
        f.hs = hd.hf[0];
        f.vs = hd.vf[0];
        auto log2_of = [](int v) { return v == 4 ? 2 : (v == 2 ? 1 : 0); };
        for (int i = 0; i < hd.comps; ++i) {
            f.first[i] = (uint8_t)f.bpm;
            for (int k = 0; k < hd.hf[i] * hd.vf[i]; ++k) f.comp_word |= (uint32_t)i << (2 * (f.bpm + k));
            f.bpm += hd.hf[i] * hd.vf[i];
            f.hsh[i] = (uint8_t)log2_of(hd.hf[i]);
            f.vsh[i] = (uint8_t)log2_of(hd.vf[i]);
            f.rxs[i] = (uint8_t)log2_of(f.hs / hd.hf[i]);
            f.rys[i] = (uint8_t)log2_of(f.vs / hd.vf[i]);
            f.cw[i] = (f.w * hd.hf[i] + f.hs - 1) / f.hs;  // ceil(w h_i / Hmax)
            f.ch[i] = (f.h * hd.vf[i] + f.vs - 1) / f.vs;
            // of the scale's log2 an axis' ratio takes what it can (the chrominance is then simply upsampled less); the
            // rest, log2 r, is the reduction of the component's blocks
            const int n = e.scale == 8 ? 3 : log2_of(e.scale), rx = n - std::min(n, (int)f.rxs[i]), ry = n - std::min(n, (int)f.rys[i]);
            f.sbx[i] = (uint8_t)(3 - rx);
            f.sby[i] = (uint8_t)(3 - ry);
            f.srx[i] = (uint8_t)(f.rxs[i] - (n - rx));
            f.sry[i] = (uint8_t)(f.rys[i] - (n - ry));
            f.scw[i] = (f.cw[i] + (1 << rx) - 1) >> rx;
            f.sch[i] = (f.ch[i] + (1 << ry) - 1) >> ry;
        }
        f.sw = sw;
        f.sh = sh;
        reduced = reduced || e.scale > 1;
        f.mcus_x = (f.w + 8 * f.hs - 1) / (8 * f.hs);
        f.n_mcus = f.mcus_x * ((f.h + 8 * f.vs - 1) / (8 * f.vs));  // (at most 2^26 of at most 10 blocks)
        general = general || hd.general;
        f.n_parts = (int)std::max<uint64_t>(1, (e.len - hd.scan + kPartBytes - 1) / kPartBytes);
        f.orient = orient;
        std::memcpy(f.q, hd.q, sizeof f.q);
        std::memcpy(f.dc, hd.dc, sizeof f.dc);
        std::memcpy(f.ac, hd.ac, sizeof f.ac);
        const int wgs = (f.n_parts + kSyncBlock - 1) / kSyncBlock;
        grp_start.push_back((int)n_groups);
        wg_start.push_back((int)n_wg);
        tile_start.push_back((int)n_tiles);
        n_groups += ((int64_t)f.n_mcus * f.bpm + 7) / 8;
        n_wg += wgs;
        const int tile_w = orient >= 5 ? kSquare : kTileW, tile_h = orient >= 5 ? kSquare : kTileH;
        n_tiles += (int64_t)((f.sw + tile_w - 1) / tile_w) * ((f.sh + tile_h - 1) / tile_h);  // (sw x sh is w x h at scale 1)
        most_wg = std::max(most_wg, wgs);
        if (n_groups > 0x0FFFFFF0ll || n_wg > 0x007FFFF0ll || n_tiles > 0x7FFFFFF0ll)
            return fail_at(b, 1, "(stream length): the frames are larger than 2^31 blocks, parts or tiles in total");
        fr.push_back(f);
        frame_of.push_back(b);
    }
    const int live = (int)fr.size();
    if (live == 0) {
        std::memcpy(info, rows.data(), rows.size() * sizeof(int32_t));
        return 0;
    }
    grp_start.push_back((int)n_groups);
    wg_start.push_back((int)n_wg);
    tile_start.push_back((int)n_tiles);

    // one block of the mirror: frames | three prefix tables | flags (damaged per frame, active[2]) | results (coming back)
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    const size_t n_pre = (size_t)live + 1;
    const size_t o_frames = 0, o_grp = o_frames + fr.size() * sizeof(JdFrame), o_wg = up8(o_grp + n_pre * sizeof(int));
    const size_t o_tile = up8(o_wg + n_pre * sizeof(int)), o_flags = up8(o_tile + n_pre * sizeof(int));
    const size_t o_result = up8(o_flags + ((size_t)live + 2) * sizeof(uint32_t)), need = o_result + (size_t)live * sizeof(JdResult);
    LR_HIP(hipSetDevice(c->device));
    JpegDecodeStore& js = c->jpeg_decode;
    // (the call is synchronous: nothing of an earlier one is in flight when these are replaced)
    if (need > js.block.cap() && js.block.grow(need + need / 2)) return 1;
    const size_t n_coef = (size_t)n_groups * 8 * 64, n_lanes = (size_t)n_wg * kSyncBlock;
    if (n_coef > js.coef.cap() && js.coef.grow(n_coef)) return 1;
    if (2 * n_lanes + 2 * (size_t)n_wg > js.state.cap() && js.state.grow(2 * n_lanes + 2 * (size_t)n_wg)) return 1;
    if (3 * n_lanes > js.part.cap() && js.part.grow(3 * n_lanes)) return 1;
    unsigned char* m = js.block.h;
    std::memset(m, 0, need);
    std::memcpy(m + o_frames, fr.data(), fr.size() * sizeof(JdFrame));
    std::memcpy(m + o_grp, grp_start.data(), n_pre * sizeof(int));
    std::memcpy(m + o_wg, wg_start.data(), n_pre * sizeof(int));
    std::memcpy(m + o_tile, tile_start.data(), n_pre * sizeof(int));
    LR_HIP(hipMemcpyAsync(js.block.d, m, o_result, hipMemcpyHostToDevice, c->stream));
    LR_HIP(hipMemsetAsync(js.coef.get(), 0, n_coef * sizeof(int16_t), c->stream));

    unsigned char* d = js.block.d.get();
    const JdFrame* d_frames = reinterpret_cast<const JdFrame*>(d + o_frames);
    const int* d_grp = reinterpret_cast<const int*>(d + o_grp);
    const int* d_wg = reinterpret_cast<const int*>(d + o_wg);
    const int* d_tile = reinterpret_cast<const int*>(d + o_tile);
    uint32_t* d_damaged = reinterpret_cast<uint32_t*>(d + o_flags);
    uint32_t* d_active = d_damaged + live;
    JdResult* d_result = reinterpret_cast<JdResult*>(d + o_result);
    const uint8_t* s8 = static_cast<const uint8_t*>(d_src);
    uint8_t* d8 = static_cast<uint8_t*>(d_dst);

    // the rounds: until one in which no lane decoded (a round settles at least one more workgroup of every chain)
    volatile uint32_t* h_active = reinterpret_cast<volatile uint32_t*>(m + o_flags) + live;
    bool settled = false;
    for (int round = 0; round < most_wg + 2 && !settled; ++round) {
        if (round >= 2) LR_HIP(hipMemsetAsync(d_active + (round & 1), 0, sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(general ? jd_sync_kernel<true> : jd_sync_kernel<false>, dim3((unsigned)n_wg), dim3(kSyncBlock), 0, c->stream, s8, live,
                           (int)n_wg, round, d_frames, d_wg, js.state.get(), js.part.get(), d_active);
        LR_HIP(hipGetLastError());
        LR_HIP(hipMemcpyAsync(const_cast<uint32_t*>(h_active) + (round & 1), d_active + (round & 1), sizeof(uint32_t), hipMemcpyDeviceToHost,
                              c->stream));
        LR_HIP(hipStreamSynchronize(c->stream));
        settled = h_active[round & 1] == 0;
    }
    if (!settled) return fail("the entropy decoder's rounds did not settle (this cannot happen)");

    hipLaunchKernelGGL(jd_place_kernel, dim3(live), dim3(kScanBlock), 0, c->stream, (int)n_wg, d_frames, d_wg, js.part.get(), d_result);
    hipLaunchKernelGGL(general ? jd_write_kernel<true> : jd_write_kernel<false>, dim3((unsigned)n_wg), dim3(kSyncBlock), 0, c->stream, s8, live,
                       (int)n_wg, d_frames, d_wg, d_grp, js.state.get(), js.part.get(), js.coef.get(), d_damaged);
    hipLaunchKernelGGL(general ? jd_dc_kernel<true> : jd_dc_kernel<false>, dim3(live), dim3(kScanBlock), 0, c->stream, d_frames, d_grp, js.coef.get());
    const int grid_t = (int)std::min<int64_t>(n_groups, 1 << 18);
    auto transform = general ? jd_transform_kernel<true, false> : jd_transform_kernel<false, false>;
    if (reduced) transform = jd_transform_kernel<true, true>;
    hipLaunchKernelGGL(transform, dim3(grid_t), dim3(kWave), 0, c->stream, live,
                       (int)n_groups, format == LR_PIX_U8 ? 1 : 0, d_frames, d_grp, js.coef.get());
    const int grid_o = (int)((std::min<int64_t>(n_tiles, 1 << 18) + 7) / 8 * 8);
    bool turn = false;
    for (const JdFrame& f : fr) turn = turn || f.orient >= 5;
    auto output = format == LR_PIX_U8 ? (turn ? jd_output_kernel<LR_PIX_U8, true, false, false> : jd_output_kernel<LR_PIX_U8, false, false, false>)
                                      : (turn ? jd_output_kernel<LR_PIX_U8X3, true, false, false> : jd_output_kernel<LR_PIX_U8X3, false, false, false>);
    if (general)
        output = format == LR_PIX_U8 ? (turn ? jd_output_kernel<LR_PIX_U8, true, true, false> : jd_output_kernel<LR_PIX_U8, false, true, false>)
                                     : (turn ? jd_output_kernel<LR_PIX_U8X3, true, true, false> : jd_output_kernel<LR_PIX_U8X3, false, true, false>);
    if (reduced)  // (the general geometry throughout: the three layouts are special cases of it)
        output = format == LR_PIX_U8 ? (turn ? jd_output_kernel<LR_PIX_U8, true, true, true> : jd_output_kernel<LR_PIX_U8, false, true, true>)
                                     : (turn ? jd_output_kernel<LR_PIX_U8X3, true, true, true> : jd_output_kernel<LR_PIX_U8X3, false, true, true>);
    hipLaunchKernelGGL(output, dim3(grid_o), dim3(kTileW * kTileH), 0, c->stream, live, (int)n_tiles, d_frames, d_tile, d_grp, js.coef.get(), d8);
    LR_HIP(hipGetLastError());
    LR_HIP(hipMemcpyAsync(m + o_flags, d + o_flags, need - o_flags, hipMemcpyDeviceToHost, c->stream));
    LR_HIP(hipStreamSynchronize(c->stream));
    const uint32_t* damaged = reinterpret_cast<const uint32_t*>(m + o_flags);
    const JdResult* result = reinterpret_cast<const JdResult*>(m + o_result);
    for (int i = 0; i < live; ++i) {
        const JdFrame& f = fr[(size_t)i];
        int32_t* row = rows.data() + (size_t)frame_of[(size_t)i] * 8;
        const uint32_t blocks = (uint32_t)f.n_mcus * (uint32_t)f.bpm;
        const uint32_t markers = f.ri > 0 ? (uint32_t)((f.n_mcus + f.ri - 1) / f.ri - 1) : 0u;
        row[6] = (int32_t)result[i].tries;
        if (damaged[i] || result[i].blocks != blocks || result[i].markers != markers) {
            row[5] = kDamaged;
            set_error("lr_decode_jpeg_device: frame " + std::to_string(frame_of[(size_t)i]) + ": status 4: the scan is damaged (" +
                      std::to_string(result[i].blocks) + " blocks of " + std::to_string(blocks) + ", " + std::to_string(result[i].markers) +
                      " RSTm of " + std::to_string(markers) + (damaged[i] ? ", an invalid code or a misplaced marker)" : ")"));
        }
    }
    std::memcpy(info, rows.data(), rows.size() * sizeof(int32_t));
    return 0;
}

}  // namespace lramd
