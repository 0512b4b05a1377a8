// The detector's front end: lr_warp_perspective_device with LR_WARP_PREPARE for gfx950.
//
// luma / 256 of an 8-bit (or f32) frame, area-averaged down to the detector's size: the reference demo's first step
// (BGR to gray, / 256, INTER_AREA prescale).  A streaming reduction: every source byte is read once, about s^2 source
// pixels make one destination pixel, so what matters is that the source goes through the memory pipe in full-width
// coalesced loads and that nothing else stands in their way.
//
//   * a workgroup takes one 64 x 4 tile of the destination (a wavefront a row, a lane a pixel), so its source footprint
//     is a band of about 4 s rows by 64 s pixels;
//   * the band goes through LDS eight source rows (by at most 512 source pixels) at a time: all 256 lanes fetch the
//     rows' bytes as aligned dwords, four to a lane in flight (the ragged ends of a row, which u8 and u8x3 rows have,
//     byte by byte, so nothing outside a row is touched), u8x3 is turned into luma ONCE per source pixel on the way,
//     and then every lane runs its own taps over the staged rows;
//   * the tiles of all frames, row-major frame by frame, are cut into eight contiguous runs, one per XCD (the XCD band
//     order of kernels_warp.hip), so neighbouring tiles, which share a source row where the scale is not whole, share
//     an L2;
//   * a wavefront's 64 results are 256 consecutive bytes: one coalesced dword store per lane.
//
// The arithmetic is the canonical one of DESIGN.md section 3 (mirrored by tests/numpy_prepare_ref.py).  Per axis a
// destination sample's taps are `first .. first + count - 1`; every tap strictly inside covers a whole source sample,
// so its weight is (float)(1.0 / s) whatever the sample; only the first and the last tap have weights of their own.
// The host makes that table (four words per destination column and row) in double, as examples/rectify_recipe.cpp
// does, and the kernel accumulates h = h + w_x * p over a row's taps in order, then v = v + w_y * h over the rows in
// order, each multiply and add rounded on its own (-ffp-contract=off).  The tap count has no bound (8192 to 1 is
// legal): both loops run over chunks of the band.
//
// One tile body, two kernels: prepare_tile is a workgroup's work on a tile; prepare_kernel (one size for all frames: the
// frame is tile / tiles per frame, everything else a kernel argument) and prepare_ragged_kernel (LR_WARP_RAGGED |
// LR_WARP_PREPARE: frames that each have their own source size, output size, span tables and places, found through the
// tiles' prefix table and a record per frame) only find the values it takes.
//
// Measured (profiles/prepare_*.txt): 24-40 us for a 4K frame, three to six times a device copy of
// the same bytes -- bound by the bytes the workgroups keep in flight (a chunk each, nothing fetched ahead), not yet cured.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "tables.h"
#include "tiles.h"

namespace lramd {
namespace {

constexpr int kTileW = 64;   // destination pixels per tile row (a lane each)
constexpr int kTileH = 4;    // destination rows per tile (a wavefront each)
constexpr int kBlock = 256;
constexpr int kRows = 8;     // source rows staged at a time
constexpr int kCols = 512;   // source pixels of a row staged at a time
constexpr int kFetch = 4;    // dwords a lane has in flight while staging
constexpr int kMaxGrid = 8 * 8192;  // beyond that the workgroups of an XCD loop over its run of tiles

// one destination sample of one axis: its taps and the weights of the two that differ from 1 / s
struct Span {
    int first, count;
    float w_first, w_last;
};

struct PrepareArgs {
    const uint8_t* src;
    size_t src_image_bytes, src_row_bytes;
    uint8_t* dst;
    size_t dst_image_bytes, dst_row_bytes;
    int ow, oh;
    const Span* sx;  // ow entries
    const Span* sy;  // oh entries
    float wx_in, wy_in;  // (float)(1.0 / s) of each axis
    int tiles_x, tiles_per_frame, n_tiles;
};

// LR_WARP_RAGGED | LR_WARP_PREPARE: a frame's record
struct PrepareFrame {
    unsigned long long src_offset, src_row_bytes;  // of its source, from the source pointer
    unsigned long long dst_offset, dst_row_bytes;  // of its output, from the destination pointer
    int ow, oh, tiles_x;
    unsigned span0;      // its ow + oh spans begin here in the call's span table
    float wx_in, wy_in;  // (float)(1.0 / s) of each axis
    int pad[2];
};
static_assert(sizeof(PrepareFrame) == 64, "records are read as they lie");

struct RaggedPrepareArgs {
    const uint8_t* src;
    int batch, n_tiles;
};

template <int kFormat>
struct Staged {  // what a lane's tap reads from LDS
    using type = uint8_t;
};
template <>
struct Staged<LR_PIX_F32> {
    using type = float;
};

// One tile: the 64 x 4 destination pixels from (x0, y0) of a frame whose source begins at `src`, whose span tables are sx
// (ow entries) and sy (oh entries) and whose output begins at `out`.  Everything but the lane's own spans is uniform across
// the workgroup.  The two kernels below differ only in where they find these values.
template <int kFormat>
__device__ __forceinline__ void prepare_tile(const uint8_t* src, size_t src_row_bytes, const Span* sx, const Span* sy, float wx_in,
                                             float wy_in, int ow, int oh, int x0, int y0, uint8_t* out, size_t dst_row_bytes) {
    using Lum = typename Staged<kFormat>::type;
    constexpr int kBpp = kFormat == LR_PIX_U8 ? 1 : (kFormat == LR_PIX_U8X3 ? 3 : 4);
    // raw: a chunk's bytes as fetched, every row from the aligned dword that holds its first byte (u8, f32: the taps
    // read it where it lies).  lum (u8x3 only): the chunk's luma.
    constexpr int kRawPitch = kCols * kBpp + 8;  // bytes; a multiple of 4
    constexpr int kLumPitch = kFormat == LR_PIX_U8X3 ? kCols : 1;
    __shared__ __attribute__((aligned(16))) uint8_t raw[kRows * kRawPitch];
    __shared__ uint8_t lum[kFormat == LR_PIX_U8X3 ? kRows * kLumPitch : 4];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x1 = min(x0 + kTileW, ow) - 1, y1 = min(y0 + kTileH, oh) - 1;  // last column and row of the tile

    // the band of the source this tile reads (the same for the whole workgroup) ...
    const Span sxa = sx[x0], sxb = sx[x1], sya = sy[y0], syb = sy[y1];
    const int col_a = sxa.first, col_b = sxb.first + sxb.count - 1;
    const int row_a = sya.first, row_b = syb.first + syb.count - 1;
    // ... and this lane's pixel in it (lanes and wavefronts past the edge carry an empty span and store nothing)
    const int x = x0 + lane, y = y0 + wave;
    const bool live = x <= x1 && y <= y1;
    Span mx = {0, 0, 0.f, 0.f}, my = {0, 0, 0.f, 0.f};
    if (live) {
        mx = sx[x];
        my = sy[y];
    }
    const int mx_last = mx.first + mx.count - 1, my_last = my.first + my.count - 1;

    float v = 0.f;
    for (int r0 = row_a; r0 <= row_b; r0 += kRows) {
        const int nr = min(kRows, row_b - r0 + 1);
        float h[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) h[k] = 0.f;
        for (int c0 = col_a; c0 <= col_b; c0 += kCols) {
            const int nc = min(kCols, col_b - c0 + 1);
            // first byte of the chunk in its first row; row k's first byte is k row strides further
            const uint8_t* chunk = src + (size_t)r0 * src_row_bytes + (size_t)c0 * kBpp;
            __syncthreads();  // the previous chunk has been read
            // fetch rows r0 .. r0 + nr - 1, bytes [c0 * kBpp, (c0 + nc) * kBpp) of each: words_row dwords cover a
            // row wherever its first byte lies in its dword (<= kRawPitch / 4)
            const int words_row = ((nc * kBpp + 3) >> 2) + 1, words = nr * words_row;
            for (int i0 = tid; i0 < words; i0 += kFetch * kBlock) {
                uint32_t word[kFetch];
#pragma unroll
                for (int u = 0; u < kFetch; ++u) {
                    const int idx = i0 + u * kBlock;
                    word[u] = 0;
                    if (idx < words) {
                        const int k = idx / words_row, d = idx - k * words_row;
                        const uint8_t* beg = chunk + (size_t)k * src_row_bytes;
                        const uint8_t* end = beg + (size_t)nc * kBpp;
                        const uint8_t* p = beg - (reinterpret_cast<uintptr_t>(beg) & 3u) + 4 * (size_t)d;
                        if (p >= beg && p + 4 <= end) {
                            word[u] = *reinterpret_cast<const uint32_t*>(p);
                        } else {
                            for (int i = 0; i < 4; ++i)
                                if (p + i >= beg && p + i < end) word[u] |= (uint32_t)p[i] << (8 * i);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < kFetch; ++u) {
                    const int idx = i0 + u * kBlock;
                    if (idx < words) {
                        const int k = idx / words_row, d = idx - k * words_row;
                        reinterpret_cast<uint32_t*>(raw + k * kRawPitch)[d] = word[u];
                    }
                }
            }
            if (kFormat == LR_PIX_U8X3) {
                __syncthreads();
                for (int idx = tid; idx < nr * nc; idx += kBlock) {
                    const int k = idx / nc, i = idx - k * nc;
                    const uint8_t* beg = chunk + (size_t)k * src_row_bytes;
                    const uint8_t* px = raw + k * kRawPitch + (reinterpret_cast<uintptr_t>(beg) & 3u) + 3 * i;
                    const uint32_t c0v = px[0], c1v = px[1], c2v = px[2];
                    lum[k * kLumPitch + i] = (uint8_t)((4899u * c0v + 9617u * c1v + 1868u * c2v + 8192u) >> 14);
                }
            }
            __syncthreads();
            // this lane's taps inside the chunk
            const int ja = max(mx.first, c0), jb = min(mx_last, c0 + nc - 1);
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                const int row = r0 + k;
                if (k < nr && row >= my.first && row <= my_last && ja <= jb) {
                    const Lum* line;
                    if (kFormat == LR_PIX_U8X3) {
                        line = reinterpret_cast<const Lum*>(lum + k * kLumPitch);
                    } else {
                        const uint8_t* beg = chunk + (size_t)k * src_row_bytes;
                        line = reinterpret_cast<const Lum*>(raw + k * kRawPitch + (reinterpret_cast<uintptr_t>(beg) & 3u));
                    }
                    float acc = h[k];
                    for (int j = ja; j <= jb; ++j) {
                        const float w = j == mx.first ? mx.w_first : (j == mx_last ? mx.w_last : wx_in);
                        const float p = kFormat == LR_PIX_F32 ? (float)line[j - c0] : (float)line[j - c0] * (1.0f / 256.0f);
                        acc = acc + w * p;
                    }
                    h[k] = acc;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const int row = r0 + k;
            if (k < nr && row >= my.first && row <= my_last) {
                const float w = row == my.first ? my.w_first : (row == my_last ? my.w_last : wy_in);
                v = v + w * h[k];
            }
        }
    }
    if (live) reinterpret_cast<float*>(out + (size_t)y * dst_row_bytes)[x] = v;
}

template <int kFormat>
__global__ __launch_bounds__(kBlock) void prepare_kernel(PrepareArgs g) {
    XcdBand band(g.n_tiles);
    for (int tile; band.next(&tile);) {
        const int b = tile / g.tiles_per_frame;
        const int r = tile - b * g.tiles_per_frame;
        const int ty = r / g.tiles_x, tx = r - ty * g.tiles_x;
        prepare_tile<kFormat>(g.src + (size_t)b * g.src_image_bytes, g.src_row_bytes, g.sx, g.sy, g.wx_in, g.wy_in, g.ow, g.oh,
                              tx * kTileW, ty * kTileH, g.dst + (size_t)b * g.dst_image_bytes, g.dst_row_bytes);
    }
}

// LR_WARP_RAGGED | LR_WARP_PREPARE: the same tiles over a ragged list.  Every frame has its own source (place, size, stride),
// output (place, size, stride), span tables and (float)(1 / s) pair, all found through its record; tile to frame goes by
// the scalar binary search of tiles.h.  Records, prefix table and spans are restrict-qualified arguments of their own: the
// stores to dst cannot change them, so their uniform reads stay scalar loads.
template <int kFormat>
__global__ __launch_bounds__(kBlock) void prepare_ragged_kernel(RaggedPrepareArgs g, const PrepareFrame* __restrict__ frames,
                                                                const int* __restrict__ start, const Span* __restrict__ spans,
                                                                uint8_t* __restrict__ dst) {
    XcdBand band(g.n_tiles);
    for (int tile; band.next(&tile);) {
        const int b = frame_of_tile(start, g.batch, tile);
        const PrepareFrame* f = frames + b;
        const int ow = f->ow, tiles_x = f->tiles_x;
        const Span* sx = spans + f->span0;  // ow entries, then the rows' oh
        const int r = tile - start[b];
        const int ty = r / tiles_x, tx = r - ty * tiles_x;
        prepare_tile<kFormat>(g.src + (size_t)f->src_offset, (size_t)f->src_row_bytes, sx, sx + ow, f->wx_in, f->wy_in, ow, f->oh,
                              tx * kTileW, ty * kTileH, dst + (size_t)f->dst_offset, (size_t)f->dst_row_bytes);
    }
}

// One axis of the table: destination sample i covers [i s, min(n_src, (i + 1) s)), s = n_src / n_dst; tap j weighs
// (float)(overlap / s).  Returns (float)(1.0 / s), the weight of every tap strictly inside.
float make_spans(int n_src, int n_dst, Span* out) {
    const double s = (double)n_src / n_dst;
    auto weight = [&](double lo, double hi, int j) {
        const double ov = std::min(hi, (double)j + 1) - std::max(lo, (double)j);
        return (float)(std::max(0.0, ov) / s);
    };
    for (int i = 0; i < n_dst; ++i) {
        const double lo = i * s, hi = std::min((double)n_src, (i + 1) * s);
        const int a = (int)std::floor(lo), b = std::min(n_src - 1, (int)std::ceil(hi) - 1);
        out[i].first = a;
        out[i].count = b - a + 1;
        out[i].w_first = weight(lo, hi, a);
        out[i].w_last = weight(lo, hi, b);
    }
    return (float)(1.0 / s);
}

}  // namespace

int ctx_prepare_frames(lr_context* c, const void* d_src, size_t src_image_bytes, int batch, int width, int height,
                       size_t src_row_bytes, int format, void* d_dst, size_t dst_image_bytes, int out_width,
                       int out_height, size_t dst_row_bytes) {
    auto fail = [](const char* what) {
        set_error(std::string("lr_warp_perspective_device: LR_WARP_PREPARE: ") + what);
        return 1;
    };
    if (!c) return fail("no context");
    if (!d_src || !d_dst) return fail("null pointer (source or destination)");
    if (batch < 1) return fail("batch < 1");
    if (width < 1 || height < 1 || out_width < 1 || out_height < 1) return fail("source or output size below 1");
    if (format != LR_PIX_U8 && format != LR_PIX_U8X3 && format != LR_PIX_F32) return fail("unknown pixel format");
    if (out_width > width || out_height > height) return fail("output larger than the source (no upscaling)");
    const size_t bpp = format == LR_PIX_U8 ? 1 : (format == LR_PIX_U8X3 ? 3 : 4);
    if (src_row_bytes < (size_t)width * bpp) return fail("source row stride shorter than a row");
    if (dst_row_bytes < (size_t)out_width * 4) return fail("destination row stride shorter than a row");
    size_t src_span, dst_span;
    if (!frame_span(height, src_row_bytes, (size_t)width * bpp, &src_span) ||
        !frame_span(out_height, dst_row_bytes, (size_t)out_width * 4, &dst_span))
        return fail("frame larger than the address space");
    if (batch > 1 && (src_image_bytes < src_span || dst_image_bytes < dst_span))
        return fail("image stride shorter than a frame");
    if ((reinterpret_cast<uintptr_t>(d_dst) | dst_row_bytes | (batch > 1 ? dst_image_bytes : 0)) & 3u)
        return fail("destination pointer or stride not 4-byte aligned");
    if (format == LR_PIX_F32 && ((reinterpret_cast<uintptr_t>(d_src) | src_row_bytes | (batch > 1 ? src_image_bytes : 0)) & 3u))
        return fail("f32 pointer or stride not 4-byte aligned");
    const int64_t tiles_x = ((int64_t)out_width + kTileW - 1) / kTileW, tiles_y = ((int64_t)out_height + kTileH - 1) / kTileH;
    const int64_t n_tiles = tiles_x * tiles_y * (int64_t)batch;
    if (n_tiles > 0x7FFFFFF0ll) return fail("output larger than 2^31 tiles of 64 x 4 pixels");

    LR_HIP(hipSetDevice(c->device));
    // The span table is made once per (source size, output size) and kept.  The launches that read the device copy and
    // the upload that overwrites it are all on the context's stream; the page-locked copy waits for its last upload.
    const size_t n_spans = (size_t)out_width + (size_t)out_height;
    const bool same = c->prep.spans.d && c->prep.key[0] == width && c->prep.key[1] == out_width &&
                      c->prep.key[2] == height && c->prep.key[3] == out_height;
    if (!same) {
        c->prep.key[0] = 0;  // (no table while this is under way)
        if (upload_reserve(c, c->prep.spans, c->ev_prep_spans, n_spans * sizeof(Span))) return 1;
        Span* hs = reinterpret_cast<Span*>(c->prep.spans.h.get());
        c->prep.w_in[0] = make_spans(width, out_width, hs);
        c->prep.w_in[1] = make_spans(height, out_height, hs + out_width);
        if (upload_send(c, c->prep.spans, c->ev_prep_spans, n_spans * sizeof(Span))) return 1;
        c->prep.key[0] = width;
        c->prep.key[1] = out_width;
        c->prep.key[2] = height;
        c->prep.key[3] = out_height;
    }

    PrepareArgs g;
    g.src = static_cast<const uint8_t*>(d_src);
    g.src_image_bytes = src_image_bytes;
    g.src_row_bytes = src_row_bytes;
    g.dst = static_cast<uint8_t*>(d_dst);
    g.dst_image_bytes = dst_image_bytes;
    g.dst_row_bytes = dst_row_bytes;
    g.ow = out_width;
    g.oh = out_height;
    g.sx = reinterpret_cast<const Span*>(c->prep.spans.d.get());
    g.sy = g.sx + out_width;
    g.wx_in = c->prep.w_in[0];
    g.wy_in = c->prep.w_in[1];
    g.tiles_x = (int)tiles_x;
    g.tiles_per_frame = (int)(tiles_x * tiles_y);
    g.n_tiles = (int)n_tiles;
    const int grid = (int)std::min<int64_t>((n_tiles + 7) / 8 * 8, kMaxGrid);
    launch_by_format(format, [&](auto fmt) {
        hipLaunchKernelGGL(prepare_kernel<decltype(fmt)::value>, dim3(grid), dim3(kBlock), 0, c->stream, g);
    });
    LR_HIP(hipGetLastError());
    return 0;
}

// LR_WARP_RAGGED | LR_WARP_PREPARE: the table's check is the ragged warp's (ragged_parse); the span tables are made per
// call, in make_spans' arithmetic, one per (source size, output size) pair of the call, and go up with the records and the
// tiles' prefix table in one transfer from one mirrored buffer.
int ctx_prepare_ragged(lr_context* c, const void* d_src, size_t src_bytes, int batch, int width, int height, size_t src_row_bytes,
                       int format, const double* T, void* d_dst, size_t dst_bytes, int out_width, int out_height,
                       size_t dst_row_bytes) {
    auto fail = [](const char* what) {
        set_error(std::string("lr_warp_perspective_device: LR_WARP_RAGGED: ") + what);
        return 1;
    };
    std::vector<RaggedEntry> e;
    int64_t n_tiles = 0;
    if (ragged_parse(d_src, src_bytes, batch, width, height, src_row_bytes, format, true, T, d_dst, dst_bytes, out_width,
                     out_height, dst_row_bytes, kTileW, kTileH, e, &n_tiles))
        return 1;
    // which span table each frame reads: frames of one (source size, output size) share one
    struct Table {
        size_t span0;  // its first span: ow for the columns, then oh for the rows
        int first;     // the first frame that reads it
        float w_in[2];
    };
    std::map<std::array<uint64_t, 4>, Table> tables;
    std::vector<Table*> table_of((size_t)batch);
    size_t n_spans = 0;
    for (int b = 0; b < batch; ++b) {
        const RaggedEntry& s = e[(size_t)b];
        const auto ins = tables.insert({{s.w, s.ow, s.h, s.oh}, Table{n_spans, b, {0.f, 0.f}}});
        if (ins.second) n_spans += (size_t)(s.ow + s.oh);
        table_of[(size_t)b] = &ins.first->second;
    }
    if (n_spans > 0x7FFFFFF0u) return fail("span tables of more than 2^31 entries");
    // records | prefix table (padded to 16 bytes) | spans
    const size_t rec_bytes = (size_t)batch * sizeof(PrepareFrame);
    const size_t start_bytes = (((size_t)batch + 1) * sizeof(int) + 15) / 16 * 16;
    const size_t bytes = rec_bytes + start_bytes + n_spans * sizeof(Span);
    LR_HIP(hipSetDevice(c->device));
    if (upload_reserve(c, c->prep.ragged, c->ev_prep_ragged, bytes)) return 1;
    unsigned char* hb = c->prep.ragged.h.get();
    PrepareFrame* rec = reinterpret_cast<PrepareFrame*>(hb);
    int* start = reinterpret_cast<int*>(hb + rec_bytes);
    Span* hs = reinterpret_cast<Span*>(hb + rec_bytes + start_bytes);
    int tiles = 0;
    for (int b = 0; b < batch; ++b) {
        const RaggedEntry& s = e[(size_t)b];
        Table& t = *table_of[(size_t)b];
        if (t.first == b) {
            t.w_in[0] = make_spans((int)s.w, (int)s.ow, hs + t.span0);
            t.w_in[1] = make_spans((int)s.h, (int)s.oh, hs + t.span0 + s.ow);
        }
        PrepareFrame& f = rec[b];
        std::memset(&f, 0, sizeof f);
        f.src_offset = s.src_off;
        f.src_row_bytes = s.src_row;
        f.dst_offset = s.dst_off;
        f.dst_row_bytes = s.dst_row;
        f.ow = (int)s.ow;
        f.oh = (int)s.oh;
        f.tiles_x = (int)((s.ow + kTileW - 1) / kTileW);
        f.span0 = (unsigned)t.span0;
        f.wx_in = t.w_in[0];
        f.wy_in = t.w_in[1];
        start[b] = tiles;
        tiles += f.tiles_x * (int)((s.oh + kTileH - 1) / kTileH);
    }
    start[batch] = tiles;
    if (upload_send(c, c->prep.ragged, c->ev_prep_ragged, bytes)) return 1;

    RaggedPrepareArgs g;
    g.src = static_cast<const uint8_t*>(d_src);
    g.batch = batch;
    g.n_tiles = (int)n_tiles;
    const unsigned char* db = c->prep.ragged.d.get();
    const PrepareFrame* d_rec = reinterpret_cast<const PrepareFrame*>(db);
    const int* d_start = reinterpret_cast<const int*>(db + rec_bytes);
    const Span* d_spans = reinterpret_cast<const Span*>(db + rec_bytes + start_bytes);
    uint8_t* dst = static_cast<uint8_t*>(d_dst);
    const int grid = (int)std::min<int64_t>((n_tiles + 7) / 8 * 8, kMaxGrid);
    launch_by_format(format, [&](auto fmt) {
        hipLaunchKernelGGL(prepare_ragged_kernel<decltype(fmt)::value>, dim3(grid), dim3(kBlock), 0, c->stream, g, d_rec, d_start,
                           d_spans, dst);
    });
    LR_HIP(hipGetLastError());
    return 0;
}

}  // namespace lramd
