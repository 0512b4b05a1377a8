// The caller's recipe around the C API, without OpenCV (behaviour of the reference demo,
// autorectify.cpp:56-68,113-148,322-376): gray conversion, scale by 1/256, area-averaging prescale to at most
// `--max-size` pixels on the long side, find_line_segment_groups with min_length = max(w,h)/100, endpoints scaled
// back, compute_rectification_transform with horizontal_vp_min_distance = 2, and the two CSV files the demo writes
// (<prefix>_lines.csv: x1,y1,x2,y2,weight,err,group_id per row; <prefix>_tform.csv: TL, TR, BL, BR, hvp, vvp).
//
//   rectify_recipe in.pgm|in.ppm out_prefix [--max-size N|fraction] [--refine] [--threads N]
//                  [--h-strategy rotate_h|rotate_v|rectify|keep] [--v-strategy ...] [--warp] [--device-prepare] [--lines]
//                  [--jpeg Q] [--optimize] [--jpeg-in] [--orient] [--any-sampling] [--scale N] [--cubic] [--border MODE[:VALUE]] [--crop]
//                  [--lens fx,fy,cx,cy,k1,k2,p1,p2,k3[,k4,k5,k6,s1,s2,s3,s4,model]] [--fisheye fx,fy,cx,cy,k1,k2,k3,k4]
//                  [--lens-scale S] [--out-max N]
//
// Input is a binary PGM (P5, 8 bit) or PPM (P6, 8 bit; converted with the usual integer luma weights
// (4899 R + 9617 G + 1868 B + 8192) >> 14).  Image decoding stays with the caller's imaging library.
// --warp: the demo's last step too (autorectify.cpp:357-360) -- lr_rectification_homography with clip 3.0, the 8-bit
// frame as read warped on the GPU (lr_warp_perspective_device), written as <out_prefix>_warp.pgm or .ppm
// (INTEGRATION.md §6).
// --device-prepare: the first step on the GPU as well -- the file's 8-bit pixels go up as they are, luma, / 256 and the
// prescale are one lr_warp_perspective_device call with LR_WARP_PREPARE, and lr_find_line_segment_groups_device runs
// on the prepared frame where it lies.  Same CSV files, byte for byte.
// --lines: the demo's lines picture (autorectify.cpp:72-110,364-366) -- the segments, in the full frame's coordinates as
// written to the CSV, drawn on the gray frame on the GPU (lr_draw_lines_device), written as <out_prefix>_lines.ppm; with
// --warp also <out_prefix>_warp_lines.ppm: the rectified picture with the segments drawn through H.
// --jpeg Q: the demo's products as it writes them (autorectify.cpp:368-369, imwrite) -- implies --warp; the rectified picture
// is compressed where the warp left it in HBM (lr_encode_jpeg_device, quality Q, 4:2:0 for colour) and only the stream comes
// back: <out_prefix>_warp.jpg, and with --lines also <out_prefix>_warp_lines.jpg.
// --optimize (with --jpeg Q alone): the files are coded with Huffman tables made from their own symbols (LR_JPEG_OPTIMIZE added
// to entry [7] of the frame's row and to lr_jpeg_bound's layout; cv::IMWRITE_JPEG_OPTIMIZE): the same pixels in fewer bytes.
// --jpeg-in: the input file is a baseline JPEG file (the demo's imread) -- lr_jpeg_info tells its size from the headers, the
// file goes up as it is and lr_decode_jpeg_device decodes it in HBM (RGB, or gray for a one-component file).  The example
// then downloads the picture and goes on exactly as --device-prepare does with a PPM it has read, so here the pixels do
// cross the link (once down, once up): a caller who wants them to stay in HBM passes the decoder's output on, as
// Context.rectify_batch does with a list of files.
// --orient (with --jpeg-in alone): the file's EXIF orientation is applied as the demo's imread applies it -- entry [7] of the
// frame's row is 1 for lr_jpeg_info, which then tells the upright size, and for lr_decode_jpeg_device, whose output pass
// writes the upright picture; that one goes on to prepare, detect and warp.  Without it the picture is the stored one.
// --any-sampling (with --jpeg-in alone): LR_JPEG_ANY_SAMPLING is or-ed into the format of lr_decode_jpeg_device (lr_jpeg_info
// is that call in probe mode, so the same word goes to both): a file of 4:4:0 (a losslessly rotated 4:2:2 photograph), 4:1:1 or
// any other sampling with factors 1, 2 or 4 is decoded, which without the option is refused with status 2.
// --scale N (with --jpeg-in alone; N = 1, 2, 4 or 8): the file is decoded at 1/N of its size -- LR_JPEG_SCALED is or-ed into the
// format and entry [6] of the frame's row is N, for lr_jpeg_info's probe call, which then tells the reduced size ceil(w / N) x
// ceil(h / N), and for lr_decode_jpeg_device, which averages the blocks' samples in its transform.  Everything behind the
// decoder works on the reduced picture, so the segments and the homography are in its coordinates (the file's, divided by N).
// --border MODE[:VALUE] (with --warp or --jpeg alone): what lies outside the source in the rectified picture, LR_WARP_BORDER --
// MODE constant, replicate, reflect or reflect101; VALUE (constant only) a gray level 0 .. 255 or R,G,B, default 0.
// --crop (likewise): the rectified picture is its constrained crop (lr_crop_homography: the largest upright rectangle of the
// source's aspect that holds no border; the margin follows --cubic); the segments of --lines are drawn through the crop's H.
// --cubic (with --warp or --jpeg alone; it implies neither): the warp samples 4 x 4 bicubic, cv::warpPerspective's INTER_CUBIC
// (LR_WARP_CUBIC or-ed into the warp's format word), instead of bilinear.  Everything else is as without it.
// --out-max N (with --warp or --jpeg alone): the rectified picture is at most N pixels on its longer side -- lr_shrink_homography
// gives the map, the size and the sampling factor S, and the warp averages S x S samples per pixel (LR_WARP_AREA): shrunk without
// aliasing in the one resampling there is; applied after --crop, and the segments of --lines are drawn through the small picture's H.
// --lens fx,fy,cx,cy,k1,k2,p1,p2,k3 (with --warp or --jpeg alone; not with --crop): the frame's camera matrix and distortion
// vector, OpenCV's, in the pixel units of the frame as read (LR_WARP_LENS).  One warp with the identity map and the lens writes
// the frame without its distortion; prescale, detector and the CSV files work on that one, so segments and transform are in
// ideal coordinates (lr_lens_distort takes a point back onto the photograph); the rectified picture is then warped from the
// frame AS READ with the lens and the homography: one resampling.  Seventeen values instead of nine (k4, k5, k6, s1, s2, s3,
// s4 and the model behind k3) are OpenCV's rational and thin-prism model, or with model 1 cv::fisheye's (LR_WARP_LENS_MODEL).
// --fisheye fx,fy,cx,cy,k1,k2,k3,k4: cv::fisheye's camera matrix and D, the same as --lens with model 1.
// --lens-scale S (with --lens or --fisheye; S > 0): prescale and detector see the ideal picture scaled by S about (cx, cy) --
// below 1 brings more of a fisheye's view into the frame -- and the rectified picture's map goes through the same scaling.
// Segments and transform are then in the scaled ideal picture's coordinates.
// Links against librectify_amd.so exactly like a program written for the reference.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "librectify_amd.h"

using namespace librectify;

namespace {

struct Gray {
    int w = 0, h = 0;
    std::vector<float> px;  // row-major
    int ch = 1;               // the 8-bit frame as read (gray or interleaved RGB), for --warp
    std::vector<uint8_t> raw;
};

bool read_token(std::istream& f, std::string& tok) {
    tok.clear();
    int c;
    while ((c = f.get()) != EOF) {
        if (c == '#') {
            while ((c = f.get()) != EOF && c != '\n') {
            }
        } else if (!std::isspace(c)) {
            break;
        }
    }
    if (c == EOF) return false;
    do {
        tok.push_back((char)c);
        c = f.get();
    } while (c != EOF && !std::isspace(c));
    return true;
}

// 8-bit gray levels as floats in [0, 1): value / 256 (autorectify.cpp:119)
bool load_pnm(const std::string& path, Gray& g) {
    std::ifstream f(path, std::ios::binary);
    std::string magic, tw, th, tm;
    if (!f || !read_token(f, magic) || !read_token(f, tw) || !read_token(f, th) || !read_token(f, tm)) return false;
    const int ch = magic == "P5" ? 1 : (magic == "P6" ? 3 : 0);
    if (!ch || std::atoi(tm.c_str()) != 255) return false;
    g.w = std::atoi(tw.c_str());
    g.h = std::atoi(th.c_str());
    if (g.w <= 0 || g.h <= 0) return false;
    g.ch = ch;
    std::vector<uint8_t>& raw = g.raw;
    raw.resize((size_t)g.w * g.h * ch);
    f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)raw.size());
    if ((size_t)f.gcount() != raw.size()) return false;
    g.px.resize((size_t)g.w * g.h);
    for (size_t i = 0; i < g.px.size(); ++i) {
        int v = raw[i * ch];
        if (ch == 3) v = (4899 * raw[i * 3] + 9617 * raw[i * 3 + 1] + 1868 * raw[i * 3 + 2] + 8192) >> 14;
        g.px[i] = (float)v * (1.0f / 256.0f);
    }
    return true;
}

// --jpeg-in: the file decoded on the GPU into g.raw (and g.px, for --lines).  Returns false with the reason on stderr.
bool load_jpeg(const std::string& path, bool orient, bool any_sampling, int scale, Gray& g) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (!f || file.empty()) {
        std::fprintf(stderr, "cannot read %s\n", path.c_str());
        return false;
    }
    double frame[8] = {0, (double)file.size(), 0, 0, 0, 0, (double)scale, orient ? 1.0 : 0.0};
    int32_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int option = (any_sampling ? LR_JPEG_ANY_SAMPLING : 0) | (scale ? LR_JPEG_SCALED : 0);
    // (lr_jpeg_info spelled out, for the option: the decoder call without a destination and without a context)
    if (lr_decode_jpeg_device(nullptr, nullptr, file.data(), file.size(), LR_PIX_U8X3 | option, frame, 1, nullptr, 0, info) != 0 || info[5] != 0) {
        std::fprintf(stderr, "jpeg input failed: %s\n", lr_last_error());
        return false;
    }
    g.w = info[0];
    g.h = info[1];
    g.ch = info[2] == 1 ? 1 : 3;
    g.raw.resize((size_t)g.w * g.h * g.ch);
    frame[3] = (double)g.w * g.ch;
    frame[4] = g.w;
    frame[5] = g.h;
    lr_context* ctx = nullptr;
    void* d_file = nullptr;
    void* d_img = nullptr;
    const bool ok = lr_context_create(0, &ctx) == 0 && lr_device_malloc(ctx, file.size(), &d_file) == 0 &&
                    lr_device_malloc(ctx, g.raw.size(), &d_img) == 0 && lr_memcpy_h2d(ctx, d_file, file.data(), file.size()) == 0 &&
                    lr_decode_jpeg_device(ctx, d_file, file.data(), file.size(), (g.ch == 3 ? LR_PIX_U8X3 : LR_PIX_U8) | option, frame, 1, d_img,
                                          g.raw.size(), info) == 0 &&
                    info[5] == 0 && lr_memcpy_d2h(ctx, g.raw.data(), d_img, g.raw.size()) == 0;
    if (!ok) std::fprintf(stderr, "jpeg input failed: %s\n", lr_last_error());
    if (ctx) {
        if (d_file) lr_device_free(ctx, d_file);
        if (d_img) lr_device_free(ctx, d_img);
        lr_context_destroy(ctx);
    }
    if (!ok) return false;
    g.px.resize((size_t)g.w * g.h);
    for (size_t i = 0; i < g.px.size(); ++i) {
        int v = g.raw[i * g.ch];
        if (g.ch == 3) v = (4899 * g.raw[i * 3] + 9617 * g.raw[i * 3 + 1] + 1868 * g.raw[i * 3 + 2] + 8192) >> 14;
        g.px[i] = (float)v * (1.0f / 256.0f);
    }
    return true;
}

// One axis of an area-averaging downscale: destination sample i is the mean of the source interval
// [i*s, (i+1)*s), s = n_src / n_dst, partially covered source samples weighted by their overlap.
struct Span {
    int first;
    std::vector<float> wgt;
};
std::vector<Span> area_spans(int n_src, int n_dst) {
    std::vector<Span> spans(n_dst);
    const double s = (double)n_src / n_dst;
    for (int i = 0; i < n_dst; ++i) {
        const double lo = i * s, hi = std::min((double)n_src, (i + 1) * s);
        const int a = (int)std::floor(lo), b = std::min(n_src - 1, (int)std::ceil(hi) - 1);
        spans[i].first = a;
        for (int j = a; j <= b; ++j) {
            const double ov = std::min(hi, (double)j + 1) - std::max(lo, (double)j);
            spans[i].wgt.push_back((float)(std::max(0.0, ov) / s));
        }
    }
    return spans;
}

// The demo's prescale (autorectify.cpp:56-68): scale = min(max_size / max(w, h), 1); area interpolation.
Gray prescale(const Gray& in, int max_size, float& scale) {
    scale = std::min((float)max_size / (float)std::max(in.w, in.h), 1.0f);
    if (scale == 1.0f) return in;
    Gray out;
    out.w = std::max(1, (int)std::lround(in.w * (double)scale));
    out.h = std::max(1, (int)std::lround(in.h * (double)scale));
    const std::vector<Span> sx = area_spans(in.w, out.w), sy = area_spans(in.h, out.h);
    std::vector<float> tmp((size_t)in.h * out.w);
    for (int y = 0; y < in.h; ++y)
        for (int x = 0; x < out.w; ++x) {
            float acc = 0.f;
            const float* row = &in.px[(size_t)y * in.w + sx[x].first];
            for (size_t j = 0; j < sx[x].wgt.size(); ++j) acc += sx[x].wgt[j] * row[j];
            tmp[(size_t)y * out.w + x] = acc;
        }
    out.px.assign((size_t)out.w * out.h, 0.f);
    for (int y = 0; y < out.h; ++y)
        for (size_t j = 0; j < sy[y].wgt.size(); ++j) {
            const float wj = sy[y].wgt[j];
            const float* row = &tmp[(size_t)(sy[y].first + (int)j) * out.w];
            float* dst = &out.px[(size_t)y * out.w];
            for (int x = 0; x < out.w; ++x) dst[x] += wj * row[x];
        }
    return out;
}

// --device-prepare: the prescaled size by the rule of prescale() above, the raw frame uploaded, prepared on the device
// and searched there.  Fills `found`, `out_w`, `out_h` and `scale`; returns false with the reason on stderr.
bool find_groups_device_prepared(const Gray& g, int max_size, bool refine, int threads,
                                 std::vector<LineSegment>& found, int& out_w, int& out_h, float& scale) {
    scale = std::min((float)max_size / (float)std::max(g.w, g.h), 1.0f);
    out_w = scale == 1.0f ? g.w : std::max(1, (int)std::lround(g.w * (double)scale));
    out_h = scale == 1.0f ? g.h : std::max(1, (int)std::lround(g.h * (double)scale));
    lr_context* ctx = nullptr;
    void* d_src = nullptr;
    void* d_img = nullptr;
    const size_t img_bytes = (size_t)out_w * out_h * sizeof(float);
    found.resize((size_t)out_w * out_h / 6 + 16);
    int n = 0;
    // (a frame that needs no prescale is searched where it lies: the detector reads 8-bit frames itself -- LR_FRAMES_*)
    const bool in_place = scale == 1.0f;
    const float min_length = (float)std::max(out_w, out_h) / 100.0f;
    bool ok = lr_context_create(0, &ctx) == 0 && lr_device_malloc(ctx, g.raw.size(), &d_src) == 0 &&
              lr_memcpy_h2d(ctx, d_src, g.raw.data(), g.raw.size()) == 0;
    if (ok && in_place)
        ok = lr_find_line_segment_groups_device(ctx, static_cast<const float*>(d_src), g.w, g.h, g.w, min_length,
                                                (g.ch == 3 ? LR_FRAMES_U8X3 : LR_FRAMES_U8) | (refine ? 1 : 0), threads,
                                                found.data(), (int)found.size(), &n) == 0;
    else if (ok)
        ok = lr_device_malloc(ctx, img_bytes, &d_img) == 0 &&
             lr_warp_perspective_device(ctx, d_src, g.raw.size(), 1, g.w, g.h, (size_t)g.w * g.ch,
                                        (g.ch == 3 ? LR_PIX_U8X3 : LR_PIX_U8) | LR_WARP_PREPARE, nullptr, d_img, img_bytes, out_w,
                                        out_h, (size_t)out_w * sizeof(float)) == 0 &&
             lr_find_line_segment_groups_device(ctx, static_cast<const float*>(d_img), out_w, out_h, out_w, min_length, refine,
                                                threads, found.data(), (int)found.size(), &n) == 0;
    if (!ok) std::fprintf(stderr, "device prepare failed: %s\n", lr_last_error());
    if (ctx) {
        if (d_src) lr_device_free(ctx, d_src);
        if (d_img) lr_device_free(ctx, d_img);
        lr_context_destroy(ctx);
    }
    found.resize(ok ? (size_t)std::min(n, (int)found.size()) : 0);
    return ok;
}

// A picture that lies in HBM (ch 1: gray, ch 3: RGB, rows packed) as a baseline JPEG file: an extent of lr_jpeg_bound bytes,
// one lr_encode_jpeg_device call, and the stream alone comes back.  optimize: with Huffman tables of the picture's own.
// Returns false with the reason on stderr.
bool write_jpeg(lr_context* ctx, const void* d_img, int w, int h, int ch, int quality, bool optimize, const std::string& path) {
    const int format = ch == 3 ? LR_PIX_U8X3 : LR_PIX_U8;
    const int layout = optimize ? LR_JPEG_OPTIMIZE : 0;  // (4:2:0 for colour)
    const size_t cap = lr_jpeg_bound(w, h, format, layout);
    const double frame[8] = {(double)w, (double)h, 0, (double)w * ch, 0, (double)cap, (double)quality, (double)layout};
    void* d_jpg = nullptr;
    uint64_t size = 0;
    std::vector<uint8_t> stream;
    bool ok = cap != 0 && lr_device_malloc(ctx, cap, &d_jpg) == 0 &&
              lr_encode_jpeg_device(ctx, d_img, (size_t)w * h * ch, format, frame, 1, d_jpg, cap, &size) == 0 && size <= cap;
    if (ok) {
        stream.resize((size_t)size);
        ok = lr_memcpy_d2h(ctx, stream.data(), d_jpg, stream.size()) == 0;
    }
    if (!ok) std::fprintf(stderr, "jpeg failed: %s\n", cap == 0 ? "a picture beyond 65535 pixels a side" : lr_last_error());
    if (d_jpg) lr_device_free(ctx, d_jpg);
    if (!ok) return false;
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(stream.data()), (std::streamsize)stream.size());
    if (!f) {
        std::fprintf(stderr, "jpeg failed: cannot write %s\n", path.c_str());
        return false;
    }
    std::printf("wrote %s (%dx%d, quality %d%s, %zu bytes)\n", path.c_str(), w, h, quality, optimize ? ", optimised tables" : "",
                stream.size());
    return true;
}

// The demo's homography_from_corners(t, 3.0) + warpPerspective of the frame as read, on the GPU; writes
// <prefix>_warp.pgm / .ppm.  Returns false with the reason on stderr.
// `out`, `ow`, `oh` and `H` (source to rectified picture) are kept for --lines.  jpeg > 0: <prefix>_warp.jpg as well.
// (optimize: with Huffman tables of its own.)  cubic: the bicubic sampling rule.  border: --border's rule, or null.  crop: the
// picture is the constrained crop, and H, ow, oh are the crop's.
struct Border {
    int mode = LR_BORDER_CONSTANT;
    unsigned v[3] = {0, 0, 0};
};

// --lens, --fisheye and --lens-scale: the frame's lens entries, nine (LR_WARP_LENS) or seventeen (with LR_WARP_LENS_MODEL), and
// the scale s of the ideal picture about (cx, cy) that the detector sees
struct LensArg {
    double v[17];
    int n = 0;  // 0: no lens
    double scale = 1.0;
    int bits() const { return n == 17 ? LR_WARP_LENS | LR_WARP_LENS_MODEL : LR_WARP_LENS; }
    // the map from the scaled ideal picture to the ideal picture, [[1/s, 0, cx (1 - 1/s)], [0, 1/s, cy (1 - 1/s)], [0, 0, 1]],
    // in front of M: every product and sum rounded on its own, as the Python package composes them
    void scaled(double* M) const {
        if (scale == 1.0) return;
        const double q = 1.0 / scale, tx = v[2] * (1.0 - q), ty = v[3] * (1.0 - q);
        for (int j = 0; j < 3; ++j) {
            M[j] = q * M[j] + tx * M[6 + j];
            M[3 + j] = q * M[3 + j] + ty * M[6 + j];
        }
    }
};

// lens: the frame's lens, or null; its entries travel behind the border word.  out_max: --out-max's bound, or 0;
// the sampling factor travels at the very end (LR_WARP_AREA), and H, ow, oh are the small picture's.
bool warp_frame(const Gray& g, const ImageTransform& t, const std::string& prefix, std::vector<uint8_t>& out, int& ow, int& oh,
                double* H, int jpeg, bool optimize, bool cubic, const Border* border, bool crop, const LensArg* lens, int out_max) {
    double M[28];  // (the tenth: the border word of LR_WARP_BORDER; then nine or seventeen: the lens; the last: LR_WARP_AREA's S)
    lr_context* ctx = nullptr;
    void* d_src = nullptr;
    void* d_dst = nullptr;
    const size_t bpp = (size_t)g.ch;
    bool ok = lr_rectification_homography(&t, 3.0f, H, M, &ow, &oh) == 0;
    if (ok && crop) {
        int x0 = 0, y0 = 0, cw = 0, ch = 0;
        const int rc = lr_crop_homography(H, M, g.w, g.h, ow, oh, cubic ? 1 : 0, 0.0, H, M, &x0, &y0, &cw, &ch);
        if (rc != 0) {
            std::fprintf(stderr, "warp failed: no constrained crop (lr_crop_homography: %d)\n", rc);
            return false;
        }
        std::printf("crop %dx%d at (%d, %d) of %dx%d\n", cw, ch, x0, y0, ow, oh);
        ow = cw;
        oh = ch;
    }
    int options = cubic ? LR_WARP_CUBIC : 0;
    if (border) {
        const unsigned value = g.ch == 3 ? (border->v[0] | border->v[1] << 8 | border->v[2] << 16) : border->v[0];
        M[9] = (double)border->mode + 8.0 * (double)(border->mode == LR_BORDER_CONSTANT ? value : 0u);
        options |= LR_WARP_BORDER;
    }
    if (lens) {
        std::memcpy(M + (border ? 10 : 9), lens->v, (size_t)lens->n * sizeof(double));
        options |= lens->bits();
    }
    if (ok && out_max > 0) {
        int S = 1;
        const int full_w = ow, full_h = oh;
        if (lr_shrink_homography(H, M, ow, oh, out_max, H, M, &ow, &oh, &S) != 0) {
            std::fprintf(stderr, "warp failed: lr_shrink_homography refused the picture\n");
            return false;
        }
        std::printf("out-max %d: %dx%d written as %dx%d, %d x %d samples per pixel\n", out_max, full_w, full_h, ow, oh, S, S);
        M[9 + (border ? 1 : 0) + (lens ? lens->n : 0)] = (double)S;
        options |= LR_WARP_AREA;
    }
    if (ok && lens) lens->scaled(M);  // (H, the lines and the transform stay in the scaled ideal picture's coordinates)
    ok = ok && lr_context_create(0, &ctx) == 0;
    if (ok) {
        out.resize((size_t)ow * oh * bpp);
        ok = lr_device_malloc(ctx, g.raw.size(), &d_src) == 0 && lr_device_malloc(ctx, out.size(), &d_dst) == 0 &&
             lr_memcpy_h2d(ctx, d_src, g.raw.data(), g.raw.size()) == 0 &&
             lr_warp_perspective_device(ctx, d_src, g.raw.size(), 1, g.w, g.h, (size_t)g.w * bpp,
                                        (g.ch == 3 ? LR_PIX_U8X3 : LR_PIX_U8) | options, M, d_dst, out.size(),
                                        ow, oh, (size_t)ow * bpp) == 0 &&
             lr_memcpy_d2h(ctx, out.data(), d_dst, out.size()) == 0;
    }
    if (!ok) std::fprintf(stderr, "warp failed: %s\n", lr_last_error());
    const bool jpeg_ok = !ok || jpeg <= 0 || write_jpeg(ctx, d_dst, ow, oh, g.ch, jpeg, optimize, prefix + "_warp.jpg");
    if (ctx) {
        if (d_src) lr_device_free(ctx, d_src);
        if (d_dst) lr_device_free(ctx, d_dst);
        lr_context_destroy(ctx);
    }
    if (!ok || !jpeg_ok) return false;
    const std::string path = prefix + (g.ch == 3 ? "_warp.ppm" : "_warp.pgm");
    std::ofstream f(path, std::ios::binary);
    f << (g.ch == 3 ? "P6" : "P5") << "\n" << ow << " " << oh << "\n255\n";
    f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)out.size());
    if (!f) {
        std::fprintf(stderr, "warp failed: cannot write %s\n", path.c_str());
        return false;
    }
    std::printf("wrote %s (%dx%d)\n", path.c_str(), ow, oh);
    return true;
}

// --lens: the frame without its distortion (the identity map or --lens-scale's, bilinear, zero border: LR_WARP_LENS), for
// prescale and detector.  Returns false with the reason on stderr.
bool undistort_frame(const Gray& g, const LensArg& lens, Gray& out) {
    double M[26] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    lens.scaled(M);
    std::memcpy(M + 9, lens.v, (size_t)lens.n * sizeof(double));
    lr_context* ctx = nullptr;
    void* d_src = nullptr;
    void* d_dst = nullptr;
    const size_t bpp = (size_t)g.ch;
    out.w = g.w;
    out.h = g.h;
    out.ch = g.ch;
    out.raw.resize(g.raw.size());
    const bool ok = lr_context_create(0, &ctx) == 0 && lr_device_malloc(ctx, g.raw.size(), &d_src) == 0 &&
                    lr_device_malloc(ctx, g.raw.size(), &d_dst) == 0 && lr_memcpy_h2d(ctx, d_src, g.raw.data(), g.raw.size()) == 0 &&
                    lr_warp_perspective_device(ctx, d_src, g.raw.size(), 1, g.w, g.h, (size_t)g.w * bpp,
                                               (g.ch == 3 ? LR_PIX_U8X3 : LR_PIX_U8) | lens.bits(), M, d_dst, g.raw.size(), g.w, g.h,
                                               (size_t)g.w * bpp) == 0 &&
                    lr_memcpy_d2h(ctx, out.raw.data(), d_dst, out.raw.size()) == 0;
    if (!ok) std::fprintf(stderr, "undistorting failed: %s\n", lr_last_error());
    if (ctx) {
        if (d_src) lr_device_free(ctx, d_src);
        if (d_dst) lr_device_free(ctx, d_dst);
        lr_context_destroy(ctx);
    }
    if (!ok) return false;
    out.px.resize((size_t)out.w * out.h);
    for (size_t i = 0; i < out.px.size(); ++i) {
        int v = out.raw[i * out.ch];
        if (out.ch == 3) v = (4899 * out.raw[i * 3] + 9617 * out.raw[i * 3 + 1] + 1868 * out.raw[i * 3 + 2] + 8192) >> 14;
        out.px[i] = (float)v * (1.0f / 256.0f);
    }
    return true;
}

// `count` numbers separated by commas, all finite; returns how many there were (0: a fault, or more than `most`)
int parse_numbers(const char* text, double* out, int most) {
    const char* p = text;
    for (int i = 0; i < most; ++i) {
        char* end = nullptr;
        out[i] = std::strtod(p, &end);
        if (end == p || !std::isfinite(out[i])) return 0;
        if (*end == '\0') return i + 1;
        if (*end != ',') return 0;
        p = end + 1;
    }
    return 0;
}

// --lens's argument: nine numbers (LR_WARP_LENS) or seventeen (LR_WARP_LENS_MODEL: the last is the model, 0 or 1, and a
// fisheye's entries [8..15] are zero), fx and fy above 0
bool parse_lens(const char* text, LensArg& lens) {
    const int n = parse_numbers(text, lens.v, 17);
    if ((n != 9 && n != 17) || !(lens.v[0] > 0.0) || !(lens.v[1] > 0.0)) return false;
    if (n == 17) {
        if (lens.v[16] != 0.0 && lens.v[16] != 1.0) return false;
        for (int i = 8; i < 16; ++i)
            if (lens.v[16] == 1.0 && lens.v[i] != 0.0) return false;
    }
    lens.n = n;
    return true;
}

// --fisheye's argument: fx,fy,cx,cy,k1,k2,k3,k4 of cv::fisheye, as the seventeen entries of model 1
bool parse_fisheye(const char* text, LensArg& lens) {
    double v[8];
    if (parse_numbers(text, v, 8) != 8 || !(v[0] > 0.0) || !(v[1] > 0.0)) return false;
    for (int i = 0; i < 17; ++i) lens.v[i] = i < 8 ? v[i] : 0.0;
    lens.v[16] = (double)LR_LENS_FISHEYE;
    lens.n = 17;
    return true;
}

// --border's argument: MODE[:VALUE], VALUE a gray level or R,G,B (a gray level serves all three channels)
bool parse_border(const char* text, Border& b) {
    const std::string s = text;
    const size_t colon = s.find(':');
    const std::string mode = s.substr(0, colon);
    if (mode == "constant") b.mode = LR_BORDER_CONSTANT;
    else if (mode == "replicate") b.mode = LR_BORDER_REPLICATE;
    else if (mode == "reflect") b.mode = LR_BORDER_REFLECT;
    else if (mode == "reflect101") b.mode = LR_BORDER_REFLECT_101;
    else return false;
    if (colon == std::string::npos) return true;
    if (b.mode != LR_BORDER_CONSTANT) return false;
    int v[3] = {0, 0, 0}, used = 0;
    const int n = std::sscanf(s.c_str() + colon + 1, "%d,%d,%d%n", &v[0], &v[1], &v[2], &used);
    if (n == 1) {
        if (std::sscanf(s.c_str() + colon + 1, "%d%n", &v[0], &used) != 1) return false;
        v[1] = v[2] = v[0];
    } else if (n != 3) {
        return false;
    }
    if (s.c_str()[colon + 1 + (size_t)used] != 0) return false;
    for (int i = 0; i < 3; ++i) {
        if (v[i] < 0 || v[i] > 255) return false;
        b.v[i] = (unsigned)v[i];
    }
    return true;
}

// The demo's draw_lines on an 8-bit picture (ch 1: gray, every pixel v as (v, v, v); ch 3: drawn upon in place), the
// segments through H if it is not null; writes `path` as a PPM, and with jpeg > 0 `jpg_path` as a JPEG file compressed
// where the picture was drawn.  Returns false with the reason on stderr.
bool lines_picture(const uint8_t* img, int w, int h, int ch, const LineSegment* lines, int n, const double* H,
                   const std::string& path, int jpeg = 0, bool optimize = false, const std::string& jpg_path = std::string()) {
    lr_context* ctx = nullptr;
    void* d_img = nullptr;
    void* d_rgb = nullptr;
    const size_t img_bytes = (size_t)w * h * ch, rgb_bytes = (size_t)w * h * 3;
    const double in_place[8] = {(double)w, (double)h, 0, 0, 0, (double)w * 3, 0, (double)n};
    const double from_gray[8] = {(double)w, (double)h, 0, (double)w, 0, (double)w * 3, 0, (double)n};
    std::vector<uint8_t> out(rgb_bytes);
    bool ok = lr_context_create(0, &ctx) == 0 && lr_device_malloc(ctx, img_bytes, &d_img) == 0 &&
              lr_memcpy_h2d(ctx, d_img, img, img_bytes) == 0;
    if (ok && ch == 3)
        ok = lr_draw_lines_device(ctx, nullptr, 0, LR_PIX_U8X3, lines, (size_t)n, in_place, 1, H, d_img, rgb_bytes) == 0 &&
             lr_memcpy_d2h(ctx, out.data(), d_img, rgb_bytes) == 0;
    else if (ok)
        ok = lr_device_malloc(ctx, rgb_bytes, &d_rgb) == 0 &&
             lr_draw_lines_device(ctx, d_img, img_bytes, LR_PIX_U8, lines, (size_t)n, from_gray, 1, H, d_rgb, rgb_bytes) == 0 &&
             lr_memcpy_d2h(ctx, out.data(), d_rgb, rgb_bytes) == 0;
    if (!ok) std::fprintf(stderr, "lines picture failed: %s\n", lr_last_error());
    if (ok && jpeg > 0) ok = write_jpeg(ctx, ch == 3 ? d_img : d_rgb, w, h, 3, jpeg, optimize, jpg_path);
    if (ctx) {
        if (d_img) lr_device_free(ctx, d_img);
        if (d_rgb) lr_device_free(ctx, d_rgb);
        lr_context_destroy(ctx);
    }
    if (!ok) return false;
    std::ofstream f(path, std::ios::binary);
    f << "P6\n" << w << " " << h << "\n255\n";
    f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)out.size());
    if (!f) {
        std::fprintf(stderr, "lines picture failed: cannot write %s\n", path.c_str());
        return false;
    }
    std::printf("wrote %s (%dx%d, %d segments)\n", path.c_str(), w, h, n);
    return true;
}

bool parse_strategy(const std::string& s, RectificationStrategy& out) {
    if (s == "rotate_h") out = ROTATE_H;
    else if (s == "rotate_v") out = ROTATE_V;
    else if (s == "rectify") out = RECTIFY;
    else if (s == "keep") out = KEEP;
    else return false;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr,
                     "usage: %s in.pgm|in.ppm out_prefix [--max-size N|fraction] [--refine] [--threads N]\n"
                     "          [--h-strategy rotate_h|rotate_v|rectify|keep] [--v-strategy ...] [--warp] [--device-prepare]\n"
                     "          [--lines] [--jpeg Q] [--optimize] [--jpeg-in] [--orient] [--any-sampling] [--scale 1|2|4|8]\n"
                     "          [--cubic] [--border constant|replicate|reflect|reflect101[:VALUE]] [--crop]\n"
                     "          [--lens fx,fy,cx,cy,k1,k2,p1,p2,k3[,k4,k5,k6,s1,s2,s3,s4,model]] [--fisheye fx,fy,cx,cy,k1,k2,k3,k4]\n"
                     "          [--lens-scale S] [--out-max N]\n",
                     argv[0]);
        return 2;
    }
    float max_size = 1200.f;  // the demo's default
    bool refine = false, warp = false, device_prepare = false, lines_pictures = false, jpeg_in = false, orient = false, any_sampling = false, cubic = false;
    bool optimize = false, bordered = false, crop = false, lensed = false, lens_scaled = false;
    Border border;
    LensArg lens;
    int threads = -1, jpeg = 0, decode_scale = 0, out_max = 0;
    RectificationConfig cfg;
    cfg.horizontal_vp_min_distance = 2;  // autorectify.cpp:347
    for (int i = 3; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has_val = i + 1 < argc;
        if (a == "--refine") refine = true;
        else if (a == "--warp") warp = true;
        else if (a == "--device-prepare") device_prepare = true;
        else if (a == "--lines") lines_pictures = true;
        else if (a == "--jpeg-in") jpeg_in = device_prepare = true;
        else if (a == "--orient") orient = true;
        else if (a == "--any-sampling") any_sampling = true;
        else if (a == "--scale" && has_val && lr_jpeg_scaled_size(1, std::atoi(argv[i + 1])) == 1 && std::atoi(argv[i + 1]) != 0)
            decode_scale = std::atoi(argv[++i]);
        else if (a == "--cubic") cubic = true;
        else if (a == "--optimize") optimize = true;
        else if (a == "--crop") crop = true;
        else if (a == "--border" && has_val && parse_border(argv[i + 1], border)) {
            bordered = true;
            ++i;
        }
        else if (a == "--lens" && has_val && parse_lens(argv[i + 1], lens)) {
            lensed = true;
            ++i;
        }
        else if (a == "--fisheye" && has_val && parse_fisheye(argv[i + 1], lens)) {
            lensed = true;
            ++i;
        }
        else if (a == "--lens-scale" && has_val && parse_numbers(argv[i + 1], &lens.scale, 1) == 1 && lens.scale > 0.0) {
            lens_scaled = true;
            ++i;
        }
        else if (a == "--out-max" && has_val && std::atoi(argv[i + 1]) >= 1) out_max = std::atoi(argv[++i]);
        else if (a == "--max-size" && has_val) max_size = (float)std::atof(argv[++i]);
        else if (a == "--threads" && has_val) threads = std::atoi(argv[++i]);
        else if (a == "--jpeg" && has_val && std::atoi(argv[i + 1]) >= 1 && std::atoi(argv[i + 1]) <= 100) {
            jpeg = std::atoi(argv[++i]);
            warp = true;
        }
        else if (a == "--h-strategy" && has_val && parse_strategy(argv[i + 1], cfg.h_strategy)) ++i;
        else if (a == "--v-strategy" && has_val && parse_strategy(argv[i + 1], cfg.v_strategy)) ++i;
        else {
            std::fprintf(stderr, "unknown or incomplete option: %s\n", a.c_str());
            return 2;
        }
    }
    if (orient && !jpeg_in) {
        std::fprintf(stderr, "--orient goes with --jpeg-in: a PGM or PPM file carries no EXIF orientation\n");
        return 2;
    }
    if (any_sampling && !jpeg_in) {
        std::fprintf(stderr, "--any-sampling goes with --jpeg-in: a PGM or PPM file has no chroma sampling\n");
        return 2;
    }
    if (decode_scale && !jpeg_in) {
        std::fprintf(stderr, "--scale goes with --jpeg-in: it is the decoder's reduction, and a PGM or PPM file is not decoded\n");
        return 2;
    }
    if (optimize && jpeg <= 0) {
        std::fprintf(stderr, "--optimize goes with --jpeg Q: it is the encoder's choice of Huffman tables\n");
        return 2;
    }
    if (cubic && !warp) {
        std::fprintf(stderr, "--cubic goes with --warp or --jpeg: it is the warp's sampling rule and implies neither\n");
        return 2;
    }
    if ((bordered || crop) && !warp) {
        std::fprintf(stderr, "--border and --crop go with --warp or --jpeg: they shape the rectified picture and imply neither\n");
        return 2;
    }
    if (lensed && (!warp || crop)) {
        std::fprintf(stderr, "--lens goes with --warp or --jpeg and not with --crop: the crop's rectangle assumes straight source edges\n");
        return 2;
    }
    if (lens_scaled && !lensed) {
        std::fprintf(stderr, "--lens-scale goes with --lens or --fisheye: it scales the ideal picture about the lens's centre\n");
        return 2;
    }
    if (out_max && !warp) {
        std::fprintf(stderr, "--out-max goes with --warp or --jpeg: it bounds the rectified picture's size and implies neither\n");
        return 2;
    }
    Gray full;
    if (jpeg_in) {
        if (!load_jpeg(argv[1], orient, any_sampling, decode_scale, full)) return 1;
    } else if (!load_pnm(argv[1], full)) {
        std::fprintf(stderr, "cannot read %s (binary PGM/PPM, 8 bit, expected)\n", argv[1]);
        return 1;
    }
    // --lens: prescale, detector and the lines picture see the frame without its distortion; the warp reads it as read
    Gray ideal;
    if (lensed && !undistort_frame(full, lens, ideal)) return 1;
    const Gray& seen = lensed ? ideal : full;
    // a value below 1 is a fraction of the long side (autorectify.cpp:121-125)
    const int max_px = max_size < 1.f ? (int)(std::max(full.w, full.h) * max_size) : (int)max_size;
    float scale = 1.f;
    int n = 0, small_w = 0, small_h = 0;
    LineSegment* lines = nullptr;
    std::vector<LineSegment> found;  // --device-prepare: the caller's array
    if (device_prepare) {
        if (!find_groups_device_prepared(seen, std::max(1, max_px), refine, threads, found, small_w, small_h, scale))
            return 1;
        n = (int)found.size();
        lines = found.data();
    } else {
        Gray img = prescale(seen, std::max(1, max_px), scale);
        small_w = img.w;
        small_h = img.h;
        lines = find_line_segment_groups(img.px.data(), img.w, img.h, img.w, (float)std::max(img.w, img.h) / 100.0f,
                                         refine, threads, &n);
    }
    for (int i = 0; i < n; ++i) {  // back to the coordinates of the full image
        lines[i].x1 /= scale;
        lines[i].y1 /= scale;
        lines[i].x2 /= scale;
        lines[i].y2 /= scale;
    }
    const ImageTransform t = compute_rectification_transform(lines, n, full.w, full.h, cfg);

    const std::string prefix = argv[2];
    std::ofstream lf(prefix + "_lines.csv");
    for (int i = 0; i < n; ++i) {
        const LineSegment& l = lines[i];
        lf << l.x1 << "," << l.y1 << "," << l.x2 << "," << l.y2 << "," << l.weight << "," << l.err << "," << l.group_id
           << "\n";
    }
    std::ofstream tf(prefix + "_tform.csv");
    tf << t.top_left.x << "," << t.top_left.y << "\n";
    tf << t.top_right.x << "," << t.top_right.y << "\n";
    tf << t.bottom_left.x << "," << t.bottom_left.y << "\n";
    tf << t.bottom_right.x << "," << t.bottom_right.y << "\n";
    tf << t.horizontal_vp.x << "," << t.horizontal_vp.y << "," << t.horizontal_vp.z << "\n";
    tf << t.vertical_vp.x << "," << t.vertical_vp.y << "," << t.vertical_vp.z << "\n";
    std::printf("%dx%d -> %dx%d (scale %g), %d segments, wrote %s_lines.csv and %s_tform.csv\n", full.w, full.h, small_w,
                small_h, (double)scale, n, prefix.c_str(), prefix.c_str());
    std::vector<uint8_t> warped;
    int ow = 0, oh = 0;
    double H[9];
    bool ok = !warp || warp_frame(full, t, prefix, warped, ow, oh, H, jpeg, optimize, cubic, bordered ? &border : nullptr, crop, lensed ? &lens : nullptr, out_max);
    if (ok && lines_pictures) {  // on the gray frame, as the demo draws (autorectify.cpp:364)
        std::vector<uint8_t> gray(seen.px.size());
        for (size_t i = 0; i < gray.size(); ++i) gray[i] = (uint8_t)(seen.px[i] * 256.0f);
        ok = lines_picture(gray.data(), full.w, full.h, 1, lines, n, nullptr, prefix + "_lines.ppm") &&
             (!warp || lines_picture(warped.data(), ow, oh, full.ch, lines, n, H, prefix + "_warp_lines.ppm", jpeg, optimize, prefix + "_warp_lines.jpg"));
    }
    if (!device_prepare) release_line_segments(&lines);
    if (!ok) return 1;
    return device_prepare || lines == nullptr ? 0 : 1;
}
