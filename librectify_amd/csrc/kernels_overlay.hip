// The demo's lines picture: lr_draw_lines_device for gfx950 (autorectify.cpp:72-110, draw_lines).
//
// Every detected segment is a 3-pixel stroke with a disc of radius 5 at each end, in its group's colour, later segments
// over earlier ones, on the gray frame as RGB.  The rule is the integer one of DESIGN.md section 3 (mirrored by
// tests/numpy_overlay_ref.py as the demo's loop); this file finds, for every pixel, the HIGHEST-index segment whose shape
// contains it, which is the same picture.
//
//   * The host turns the segments into records of integers while it validates (endpoints truncated, through H first if
//     there is one; the colour; a flag for segments that are not drawn) and sorts their indices into bins of 256 x 256
//     pixels by bounding box grown by the disc's radius (a frame whose segments would fill more than 8 entries each
//     keeps one list of all of them: every bin then points to it).  Records, bins and lists go up in one copy.
//   * A workgroup of 256 lanes takes a 64 x 16 tile: the warp's tile, flat tile index, per-frame prefix table and XCD bands
//     (kernels_warp.hip).  A lane has four neighbouring pixels of a row, twelve contiguous bytes of u8x3.
//   * The workgroup walks its bin's list from the end in chunks of 256, a record per lane: bounding box against the
//     tile, survivors compacted into LDS in order (ballot + mbcnt inside a wavefront, four counts across them).  The
//     list in LDS holds a chunk, so a list longer than it is simply walked in several rounds.
//   * Every lane runs its pixels down the LDS list and stops a pixel at its first hit.  When all pixels of the tile are
//     owned the walk ends.
//
// The test of a pixel against a record, with p = pixel - end 1, d = end 2 - end 1, t = p.d, c = p x d, dd = d.d:
//   |p|^2 <= 25  or  |p - d|^2 <= 25  or  (0 < t < dd and 4 c^2 <= 9 dd).
// The rule's round caps of the stroke (4 |p|^2 <= 9 where t <= 0, 4 |p - d|^2 <= 9 where t >= dd) lie inside the discs, so
// they need no test of their own.  A pixel that reaches the test lies within 5 of the record's bounding box, so |p| <=
// 2^25 + 5 per axis and t, c and dd fit in int64; 4 c^2 is formed only where |c| <= 3 max(|d.x|, |d.y|) < 2^27.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "tables.h"
#include "tiles.h"

namespace lramd {
namespace {

constexpr int kTileW = 64;  // pixels per tile row (16 lanes x 4 pixels)
constexpr int kTileH = 16;  // rows per tile (4 wavefronts x 4 rows)
constexpr int kBlock = 256;
constexpr int kMaxGrid = 8 * 8192;  // beyond that the workgroups of an XCD loop over its run of tiles
constexpr int kList = kBlock;       // records the LDS list holds: one chunk of the walk
constexpr int kBin = 256;           // pixels per side of a bin (4 x 16 tiles)
constexpr int kReach = 5;           // the disc's radius: how far a shape reaches beyond its endpoints' bounding box
constexpr uint32_t kSkip = 0x80000000u;  // in a record's colour: not drawn

struct OverlayRec {
    int x1, y1, x2, y2;
    uint32_t colour;  // c0 | c1 << 8 | c2 << 16, or kSkip
    int frame;
};
static_assert(sizeof(OverlayRec) == 24, "six words");

struct OverlayFrame {
    unsigned long long dst_off, dst_row, src_off, src_row;  // bytes, from d_dst and d_src
    int w, h, tiles_x, bins_x;
    uint32_t bin_base, pad[3];  // the frame's first bin in the bin table
};
static_assert(sizeof(OverlayFrame) == 64, "eight doubles");

enum { kFromU8 = 0, kFromU8X3 = 1, kInPlace = 2 };

__device__ __forceinline__ bool in_disc(long long px, long long py) {
    // (|p| per axis first: the squares then fit in 32 bits whatever the pixel)
    return px >= -kReach && px <= kReach && py >= -kReach && py <= kReach && (int)(px * px + py * py) <= kOverlayDiscR2;
}

template <int kMode>
__global__ __launch_bounds__(kBlock) void overlay_kernel(const uint8_t* __restrict__ src, int batch, int n_tiles,
                                                         const OverlayFrame* __restrict__ frames, const int* __restrict__ start,
                                                         const uint2* __restrict__ bins, const uint32_t* __restrict__ list,
                                                         const OverlayRec* __restrict__ recs, uint8_t* __restrict__ dst) {
    __shared__ int s_rec[kList][5];
    __shared__ int s_cnt[kBlock / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lx = lane & 15, row_in_tile = wave * 4 + (lane >> 4);
    XcdBand band(n_tiles);
    for (int tile; band.next(&tile);) {
        const int b = frame_of_tile(start, batch, tile);
        const OverlayFrame* f = frames + b;
        const int w = f->w, h = f->h, tiles_x = f->tiles_x;
        const int r = tile - start[b];
        const int ty = r / tiles_x, tx = r - ty * tiles_x;
        const int tile_x0 = tx * kTileW, tile_y0 = ty * kTileH;
        const int y = tile_y0 + row_in_tile, x0 = tile_x0 + lx * 4;
        const uint2 bin = bins[f->bin_base + (uint32_t)(ty / (kBin / kTileH)) * (uint32_t)f->bins_x + (uint32_t)(tx / (kBin / kTileW))];
        const uint32_t l_first = bin.x, l_count = bin.y;
        const int n = y < h ? min(4, max(0, w - x0)) : 0;  // pixels of this lane inside the frame
        if (kMode == kInPlace && l_count == 0) continue;   // (uniform: nothing to draw here)

        // the background, asked for before the walk
        uint32_t bg[4] = {0, 0, 0, 0};
        if (kMode == kFromU8 && n > 0) {
            const uint8_t* p = src + (size_t)f->src_off + (size_t)y * (size_t)f->src_row + (size_t)x0;
            uint32_t v = 0;
            if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
                v = *reinterpret_cast<const uint32_t*>(p);
            } else {
                for (int k = 0; k < n; ++k) v |= (uint32_t)p[k] << (8 * k);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) bg[k] = ((v >> (8 * k)) & 0xFFu) * 0x010101u;
        } else if (kMode == kFromU8X3 && n > 0) {
            const uint8_t* p = src + (size_t)f->src_off + (size_t)y * (size_t)f->src_row + (size_t)x0 * 3;
            if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
                const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
                bg[0] = d0 & 0xFFFFFFu;
                bg[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
                bg[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16);
                bg[3] = d2 >> 8;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) bg[k] = (uint32_t)p[3 * k] | ((uint32_t)p[3 * k + 1] << 8) | ((uint32_t)p[3 * k + 2] << 16);
            }
        }

        uint32_t col[4] = {0, 0, 0, 0};
        uint32_t hit = 0;                              // pixels of this lane that a segment owns
        const uint32_t outside = 15u & ~((1u << n) - 1u);  // ... and those that are no pixels of the frame
        for (uint32_t done = 0; done < l_count; done += kBlock) {
            // a chunk of the list, highest index first: a record per lane, its box grown by the reach against the tile
            const uint32_t k = done + (uint32_t)tid;
            bool keep = false;
            OverlayRec rec = {};
            if (k < l_count) {
                rec = recs[list[l_first + (l_count - 1u - k)]];
                const int lo_x = min(rec.x1, rec.x2) - kReach, hi_x = max(rec.x1, rec.x2) + kReach;
                const int lo_y = min(rec.y1, rec.y2) - kReach, hi_y = max(rec.y1, rec.y2) + kReach;
                keep = !(rec.colour & kSkip) && hi_x >= tile_x0 && lo_x < tile_x0 + kTileW && hi_y >= tile_y0 && lo_y < tile_y0 + kTileH;
            }
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_cnt[wave] = __popcll(m);
            __syncthreads();
            int base = 0, total = 0;
#pragma unroll
            for (int v = 0; v < kBlock / 64; ++v) {
                const int c = s_cnt[v];
                base += v < wave ? c : 0;
                total += c;
            }
            if (keep) {
                const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                s_rec[pos][0] = rec.x1;
                s_rec[pos][1] = rec.y1;
                s_rec[pos][2] = rec.x2;
                s_rec[pos][3] = rec.y2;
                s_rec[pos][4] = (int)rec.colour;
            }
            __syncthreads();

            // this lane's pixels down the list: a pixel stops at its first hit
            for (int q = 0; q < total && (hit | outside) != 15u; ++q) {
                const int X1 = s_rec[q][0], Y1 = s_rec[q][1], X2 = s_rec[q][2], Y2 = s_rec[q][3];
                if (y < min(Y1, Y2) - kReach || y > max(Y1, Y2) + kReach || x0 + 3 < min(X1, X2) - kReach || x0 > max(X1, X2) + kReach)
                    continue;
                const long long dx = (long long)X2 - X1, dy = (long long)Y2 - Y1, dd = dx * dx + dy * dy;
                const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
                const long long lim = 3 * (adx > ady ? adx : ady);  // the stroke needs |c| <= 1.5 |d|
                const long long py = (long long)y - Y1;
                long long px = (long long)x0 - X1;
                long long t = px * dx + py * dy, c = px * dy - py * dx;
                uint32_t got = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long long ac = c < 0 ? -c : c;
                    const bool stroke = t > 0 && t < dd && ac <= lim &&
                                        kOverlayStrokeDen * ac * ac <= kOverlayStrokeNum * dd;
                    if (stroke || in_disc(px, py) || in_disc(px - dx, py - dy)) got |= 1u << i;
                    px += 1;
                    t += dx;
                    c += dy;
                }
                got &= ~(hit | outside);
                if (got) {
                    const uint32_t colour = (uint32_t)s_rec[q][4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (got & (1u << i)) col[i] = colour;
                    hit |= got;
                }
            }
            // (also the barrier in front of the next chunk's writes to the list)
            if (__syncthreads_and((hit | outside) == 15u)) break;
        }

        if (n == 0) continue;
        uint8_t* p = dst + (size_t)f->dst_off + (size_t)y * (size_t)f->dst_row + (size_t)x0 * 3;
        if (kMode == kInPlace) {  // only covered pixels are written
            if (hit == 15u && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
                uint32_t* q = reinterpret_cast<uint32_t*>(p);
                q[0] = col[0] | (col[1] << 24);
                q[1] = (col[1] >> 8) | (col[2] << 16);
                q[2] = (col[2] >> 16) | (col[3] << 8);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (hit & (1u << k)) {
                        p[3 * k] = (uint8_t)col[k];
                        p[3 * k + 1] = (uint8_t)(col[k] >> 8);
                        p[3 * k + 2] = (uint8_t)(col[k] >> 16);
                    }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!(hit & (1u << k))) col[k] = bg[k];
            if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
                uint32_t* q = reinterpret_cast<uint32_t*>(p);
                q[0] = col[0] | (col[1] << 24);
                q[1] = (col[1] >> 8) | (col[2] << 16);
                q[2] = (col[2] >> 16) | (col[3] << 8);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) {
                        p[3 * k] = (uint8_t)col[k];
                        p[3 * k + 1] = (uint8_t)(col[k] >> 8);
                        p[3 * k + 2] = (uint8_t)(col[k] >> 16);
                    }
            }
        }
    }
}

// a coordinate truncated toward zero, as the demo's int(l.x1); false if it is not drawn (not finite, or beyond 2^24)
bool truncated(double v, int* out) {
    if (!std::isfinite(v)) return false;
    const double t = std::trunc(v);
    if (std::fabs(t) > (double)kOverlayMaxCoord) return false;
    *out = (int)t;
    return true;
}

uint32_t group_colour(int g) { return g < 0 ? kOverlayUngrouped : kOverlayPalette[g % kOverlayColours]; }

// a segment as a record: its endpoints through H (or as they are) and truncated, its colour, or kSkip
OverlayRec make_record(const LineSegment& l, const double* Hm, int frame) {
    OverlayRec r = {0, 0, 0, 0, kSkip, frame};
    double x[2] = {(double)l.x1, (double)l.x2}, y[2] = {(double)l.y1, (double)l.y2};
    if (Hm) {
        double den[2];
        for (int e = 0; e < 2; ++e) den[e] = (Hm[6] * x[e] + Hm[7] * y[e]) + Hm[8];
        // (a NaN denominator fails both comparisons: skipped like a non-finite coordinate)
        if (!((den[0] > 0.0 && den[1] > 0.0) || (den[0] < 0.0 && den[1] < 0.0))) return r;
        for (int e = 0; e < 2; ++e) {
            const double u = ((Hm[0] * x[e] + Hm[1] * y[e]) + Hm[2]) / den[e];
            const double v = ((Hm[3] * x[e] + Hm[4] * y[e]) + Hm[5]) / den[e];
            x[e] = u;
            y[e] = v;
        }
    }
    if (!truncated(x[0], &r.x1) || !truncated(y[0], &r.y1) || !truncated(x[1], &r.x2) || !truncated(y[1], &r.y2)) return r;
    r.colour = group_colour(l.group_id);
    return r;
}

struct FrameEntry {
    uint64_t w, h, src_off, src_row, dst_off, dst_row, first, count;
};

}  // namespace

int ctx_draw_lines(lr_context* c, const void* d_src, size_t src_bytes, int format, const LineSegment* lines, size_t n_lines,
                   const double* T, int batch, const double* H, void* d_dst, size_t dst_bytes) {
    auto fail = [](const std::string& what) {
        set_error("lr_draw_lines_device: " + what);
        return 1;
    };
    auto fail_at = [&](int b, int entry, const char* what) {
        return fail("frame " + std::to_string(b) + ": entry [" + std::to_string(entry) + "] " + what);
    };
    if (!c) return fail("no context");
    if (!d_dst || !T) return fail("null pointer (destination or frame table)");
    if (batch < 1) return fail("batch < 1");
    if (format != LR_PIX_U8 && format != LR_PIX_U8X3) return fail("format is LR_PIX_U8 or LR_PIX_U8X3");
    const bool in_place = d_src == nullptr;
    if (in_place && format != LR_PIX_U8X3) return fail("in place (d_src == NULL) the format is LR_PIX_U8X3");
    if (in_place && src_bytes != 0) return fail("in place (d_src == NULL) src_bytes must be 0");
    if (!lines && n_lines != 0) return fail("null lines with a non-zero count");
    if (n_lines > ((size_t)1 << 28)) return fail("more than 2^28 segments");
    if (!in_place) {
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
        if (s0 < d0 + dst_bytes && d0 < s0 + src_bytes) return fail("the destination region overlaps the source region");
    }
    if (H)
        for (size_t i = 0; i < (size_t)batch * 9; ++i)
            if (!std::isfinite(H[i])) return fail("frame " + std::to_string(i / 9) + ": H is not finite");

    // the table, as a whole
    const uint64_t bpp = format == LR_PIX_U8 ? 1 : 3;
    std::vector<FrameEntry> e((size_t)batch);
    std::vector<std::pair<uint64_t, uint64_t>> extent((size_t)batch);  // of the outputs: [first byte, end)
    int64_t n_tiles = 0;
    uint64_t n_recs = 0, n_bins = 0;
    for (int b = 0; b < batch; ++b) {
        const double* t = T + (size_t)b * 8;
        FrameEntry& s = e[(size_t)b];
        // (2^30: a tile's last column, x0 + 3 and the like stay ints)
        if (!table_integer(t[0], 1, 1073741824.0, &s.w)) return fail_at(b, 0, "(width) is not an integer from 1 to 2^30");
        if (!table_integer(t[1], 1, 1073741824.0, &s.h)) return fail_at(b, 1, "(height) is not an integer from 1 to 2^30");
        if (in_place) {
            if (!(t[2] == 0.0)) return fail_at(b, 2, "(source offset) must be 0 in place");
            if (!(t[3] == 0.0)) return fail_at(b, 3, "(source row stride) must be 0 in place");
            s.src_off = s.src_row = 0;
        } else {
            if (!table_integer(t[2], 0, kExact, &s.src_off)) return fail_at(b, 2, "(source offset) is not an integer from 0 to 2^53");
            if (!table_integer(t[3], (double)(s.w * bpp), kExact, &s.src_row))
                return fail_at(b, 3, "(source row stride) is not an integer from a row's bytes to 2^53");
        }
        if (!table_integer(t[4], 0, kExact, &s.dst_off)) return fail_at(b, 4, "(output offset) is not an integer from 0 to 2^53");
        if (!table_integer(t[5], (double)(s.w * 3), kExact, &s.dst_row))
            return fail_at(b, 5, "(output row stride) is not an integer from a row's bytes to 2^53");
        if (!table_integer(t[6], 0, kExact, &s.first)) return fail_at(b, 6, "(first segment) is not an integer from 0 to 2^53");
        if (!table_integer(t[7], 0, kExact, &s.count)) return fail_at(b, 7, "(segment count) is not an integer from 0 to 2^53");
        if (s.first + s.count > n_lines) return fail_at(b, 7, "(segment count): [6] + [7] reaches beyond n_lines");
        uint64_t end;
        if (!in_place && (__builtin_mul_overflow(s.h - 1, s.src_row, &end) || __builtin_add_overflow(end, s.src_off, &end) ||
                          __builtin_add_overflow(end, s.w * bpp, &end) || end > src_bytes))
            return fail_at(b, 2, "(source offset): the frame's source reaches beyond src_bytes");
        if (__builtin_mul_overflow(s.h - 1, s.dst_row, &end) || __builtin_add_overflow(end, s.dst_off, &end) ||
            __builtin_add_overflow(end, s.w * 3, &end) || end > dst_bytes)
            return fail_at(b, 4, "(output offset): the frame's output reaches beyond dst_bytes");
        extent[(size_t)b] = {s.dst_off, end};
        n_tiles += (int64_t)((s.w + kTileW - 1) / kTileW) * (int64_t)((s.h + kTileH - 1) / kTileH);
        if (n_tiles > 0x7FFFFFF0ll) return fail_at(b, 0, "(width): the outputs are larger than 2^31 tiles of 64 x 16 pixels");
        n_recs += s.count;
        n_bins += ((s.w + kBin - 1) / kBin) * ((s.h + kBin - 1) / kBin);
    }
    {
        std::vector<std::pair<uint64_t, uint64_t>> sorted = extent;
        if (const size_t at = extents_overlap(sorted)) {
            int which = 0;
            while (extent[(size_t)which] != sorted[at]) ++which;
            return fail_at(which, 4, "(output offset): two frames' output extents overlap");
        }
    }
    if (n_recs > ((uint64_t)1 << 28)) return fail("more than 2^28 segments in the frames' ranges together");

    // records, bins and lists.  A frame's bins hold, in ascending order, the records whose grown box touches them; a frame
    // whose boxes would make more than 8 entries a record keeps ONE list of all its records, and every bin points to it.
    std::vector<OverlayFrame> fr((size_t)batch);
    std::vector<int> start((size_t)batch + 1);
    std::vector<OverlayRec> recs;
    recs.reserve((size_t)n_recs);
    std::vector<uint2> bins((size_t)n_bins);
    std::vector<uint32_t> list;
    std::vector<uint32_t> fill;
    struct Box {
        int bx0, bx1, by0, by1;
    };
    std::vector<Box> boxes;
    int tiles = 0;
    uint32_t bin_base = 0;
    for (int b = 0; b < batch; ++b) {
        const FrameEntry& s = e[(size_t)b];
        OverlayFrame& f = fr[(size_t)b];
        std::memset(&f, 0, sizeof f);
        f.dst_off = s.dst_off;
        f.dst_row = s.dst_row;
        f.src_off = s.src_off;
        f.src_row = s.src_row;
        f.w = (int)s.w;
        f.h = (int)s.h;
        f.tiles_x = (int)((s.w + kTileW - 1) / kTileW);
        f.bins_x = (int)((s.w + kBin - 1) / kBin);
        f.bin_base = bin_base;
        start[(size_t)b] = tiles;
        tiles += f.tiles_x * (int)((s.h + kTileH - 1) / kTileH);
        const uint32_t nb = (uint32_t)f.bins_x * (uint32_t)((s.h + kBin - 1) / kBin);
        uint2* fb = bins.data() + bin_base;
        bin_base += nb;

        const uint32_t rec_base = (uint32_t)recs.size(), n = (uint32_t)s.count;
        boxes.assign(n, Box{0, -1, 0, -1});
        uint64_t entries = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const OverlayRec r = make_record(lines[s.first + i], H ? H + (size_t)b * 9 : nullptr, b);
            recs.push_back(r);
            if (r.colour & kSkip) continue;
            // the grown box, cut to the frame (all within +-(2^24 + 5))
            const int64_t lo_x = std::max<int64_t>(std::min(r.x1, r.x2) - kReach, 0), hi_x = std::min<int64_t>(std::max(r.x1, r.x2) + kReach, (int64_t)s.w - 1);
            const int64_t lo_y = std::max<int64_t>(std::min(r.y1, r.y2) - kReach, 0), hi_y = std::min<int64_t>(std::max(r.y1, r.y2) + kReach, (int64_t)s.h - 1);
            if (lo_x > hi_x || lo_y > hi_y) continue;  // wholly outside
            Box& bx = boxes[i];
            bx = Box{(int)(lo_x / kBin), (int)(hi_x / kBin), (int)(lo_y / kBin), (int)(hi_y / kBin)};
            entries += (uint64_t)(bx.bx1 - bx.bx0 + 1) * (uint64_t)(bx.by1 - bx.by0 + 1);
        }
        if (entries > 8ull * n) {  // one list of all
            const uint32_t first = (uint32_t)list.size();
            for (uint32_t i = 0; i < n; ++i) list.push_back(rec_base + i);
            for (uint32_t k = 0; k < nb; ++k) fb[k] = make_uint2(first, n);
            continue;
        }
        for (uint32_t k = 0; k < nb; ++k) fb[k] = make_uint2(0, 0);
        for (uint32_t i = 0; i < n; ++i)
            for (int by = boxes[i].by0; by <= boxes[i].by1; ++by)
                for (int bx = boxes[i].bx0; bx <= boxes[i].bx1; ++bx) ++fb[(size_t)by * f.bins_x + bx].y;
        uint32_t at = (uint32_t)list.size();
        for (uint32_t k = 0; k < nb; ++k) {
            fb[k].x = at;
            at += fb[k].y;
        }
        list.resize(at);
        fill.assign(nb, 0);
        for (uint32_t i = 0; i < n; ++i)
            for (int by = boxes[i].by0; by <= boxes[i].by1; ++by)
                for (int bx = boxes[i].bx0; bx <= boxes[i].bx1; ++bx) {
                    const size_t k = (size_t)by * f.bins_x + bx;
                    list[fb[k].x + fill[k]++] = rec_base + i;
                }
    }
    start[(size_t)batch] = tiles;

    // one block of the mirror: frames | tile prefix | bins | lists | records, each from a multiple of 8 bytes
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    const size_t o_frames = 0, o_start = o_frames + fr.size() * sizeof(OverlayFrame);
    const size_t o_bins = up8(o_start + start.size() * sizeof(int)), o_list = o_bins + bins.size() * sizeof(uint2);
    const size_t o_recs = up8(o_list + list.size() * sizeof(uint32_t)), need = o_recs + recs.size() * sizeof(OverlayRec);
    LR_HIP(hipSetDevice(c->device));
    MirroredBuffer<unsigned char>& m = c->overlay.block;
    if (upload_reserve(c, m, c->ev_overlay, need, need + need / 2)) return 1;
    std::memcpy(m.h + o_frames, fr.data(), fr.size() * sizeof(OverlayFrame));
    std::memcpy(m.h + o_start, start.data(), start.size() * sizeof(int));
    if (!bins.empty()) std::memcpy(m.h + o_bins, bins.data(), bins.size() * sizeof(uint2));
    if (!list.empty()) std::memcpy(m.h + o_list, list.data(), list.size() * sizeof(uint32_t));
    if (!recs.empty()) std::memcpy(m.h + o_recs, recs.data(), recs.size() * sizeof(OverlayRec));
    if (upload_send(c, m, c->ev_overlay, need)) return 1;

    const unsigned char* d = m.d.get();
    const OverlayFrame* d_frames = reinterpret_cast<const OverlayFrame*>(d + o_frames);
    const int* d_start = reinterpret_cast<const int*>(d + o_start);
    const uint2* d_bins = reinterpret_cast<const uint2*>(d + o_bins);
    const uint32_t* d_list = reinterpret_cast<const uint32_t*>(d + o_list);
    const OverlayRec* d_recs = reinterpret_cast<const OverlayRec*>(d + o_recs);
    const uint8_t* s8 = static_cast<const uint8_t*>(d_src);
    uint8_t* d8 = static_cast<uint8_t*>(d_dst);
    const int grid = (int)std::min<int64_t>((n_tiles + 7) / 8 * 8, kMaxGrid);
    if (in_place)
        hipLaunchKernelGGL(overlay_kernel<kInPlace>, dim3(grid), dim3(kBlock), 0, c->stream, s8, batch, (int)n_tiles, d_frames,
                           d_start, d_bins, d_list, d_recs, d8);
    else if (format == LR_PIX_U8)
        hipLaunchKernelGGL(overlay_kernel<kFromU8>, dim3(grid), dim3(kBlock), 0, c->stream, s8, batch, (int)n_tiles, d_frames,
                           d_start, d_bins, d_list, d_recs, d8);
    else
        hipLaunchKernelGGL(overlay_kernel<kFromU8X3>, dim3(grid), dim3(kBlock), 0, c->stream, s8, batch, (int)n_tiles, d_frames,
                           d_start, d_bins, d_list, d_recs, d8);
    LR_HIP(hipGetLastError());
    return 0;
}

}  // namespace lramd
