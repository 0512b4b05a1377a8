// The host side of lr_encode_jpeg_device under a host sanitizer, as a program of its own (no Python, no GPU): the check of the
// frame table -- entry [7] with and without LR_JPEG_OPTIMIZE, every other entry's refusal, overlapping extents -- and
// lr_jpeg_bound's arithmetic over the sizes' whole range.  Every call here is refused on the host before anything would be
// enqueued; the context is a bare lr_context that never touches a device.
//
// Build and run, from the repository's root (the library's own sources, host code instrumented):
//
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   mkdir -p /tmp/lr_asan && for s in librectify_amd/csrc/*.hip librectify_amd/csrc/*.cpp tools/jpeg_table_check_main.cpp; do
//       hipcc $F -Iinclude -Ilibrectify_amd/csrc -x hip -c $s -o /tmp/lr_asan/$(basename $s).o & done; wait
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/lr_asan/*.o -o /tmp/lr_asan/jpeg_table_check
//   /tmp/lr_asan/jpeg_table_check        (prints the number of refusals checked and "ok"; a sanitizer report ends it)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"
#include "librectify_amd.h"

namespace {

int failures = 0, checked = 0;

void expect(bool ok, const char* what) {
    ++checked;
    if (!ok) {
        ++failures;
        std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, lr_last_error());
    }
}

// the call with a table of `batch` rows; nothing behind the pointers is ever read: every table here is refused
int encode(lr_context* ctx, int format, const std::vector<double>& table, int batch, uint64_t* sizes) {
    static unsigned char src[4096], dst[8];
    return lr_encode_jpeg_device(ctx, src, sizeof src, format, table.data(), batch, dst, 0 /* no room: see below */, sizes);
}

}  // namespace

int main() {
    // ---- lr_jpeg_bound ----
    const int formats[3] = {LR_PIX_U8, LR_PIX_U8X3, LR_PIX_F32};
    const int sizes_px[] = {-1, 0, 1, 7, 8, 9, 15, 16, 17, 255, 4096, 65534, 65535, 65536};
    for (int format : formats)
        for (int layout : {0, 1, 2, 15, 16, 17, 18, 32, 33, -1, -16})
            for (int w : sizes_px)
                for (int h : sizes_px) {
                    const size_t plain = lr_jpeg_bound(w, h, format, layout & ~LR_JPEG_OPTIMIZE), got = lr_jpeg_bound(w, h, format, layout);
                    const bool size_ok = w >= 1 && h >= 1 && w <= 65535 && h <= 65535;
                    const int base = layout & ~LR_JPEG_OPTIMIZE;
                    const bool valid = size_ok && layout >= 0 && ((format == LR_PIX_U8 && base == 0) || (format == LR_PIX_U8X3 && (base == 0 || base == 1)));
                    if (!valid) {
                        expect(got == 0, "lr_jpeg_bound is 0 for arguments that are not valid");
                        continue;
                    }
                    const size_t mcu = format == LR_PIX_U8X3 && base == 0 ? 16 : 8, bpm = format == LR_PIX_U8 ? 1 : (base == 0 ? 6 : 3);
                    const size_t mcus = (((size_t)w + mcu - 1) / mcu) * (((size_t)h + mcu - 1) / mcu), ri = 96 / bpm;
                    const size_t per_block = (layout & LR_JPEG_OPTIMIZE) ? 418 : 416;
                    expect(got == 640 + 2 * ((mcus + ri - 1) / ri) + per_block * mcus * bpm, "lr_jpeg_bound's value");
                    expect(got >= plain && plain != 0, "the optimised bound is no smaller");
                }
    for (size_t n = 1; n <= 96; ++n) expect(2 * ((1665 * n + 7) / 8) <= 418 * n, "418 bytes a block cover n blocks of 1665 bits, every byte stuffed");

    // ---- the table check ----
    lr_context ctx;  // (never used on a device)
    uint64_t sizes[2] = {0xDEADBEEF, 0xDEADBEEF};
    // two frames with extents of 100 bytes in a destination of 0 bytes: a row that is valid up to [7] is refused at entry [4]
    // (the extent's end lies beyond dst_bytes), which is checked after [7]
    const double row[8] = {40, 24, 0, 120, 0, 100, 90, 0};
    auto table_with = [&](int b, int entry, double v) {
        std::vector<double> t(16);
        std::memcpy(&t[0], row, sizeof row);
        std::memcpy(&t[8], row, sizeof row);
        t[(size_t)b * 8 + entry] = v;
        return t;
    };
    auto refused_at = [&](int format, int b, int entry, double v, int want_frame, int want_entry, const char* what) {
        const int rc = encode(&ctx, format, table_with(b, entry, v), 2, sizes);
        const std::string msg = lr_last_error();
        const std::string want = "lr_encode_jpeg_device: frame " + std::to_string(want_frame) + ": entry [" + std::to_string(want_entry) + "]";
        expect(rc != 0 && msg.compare(0, want.size(), want) == 0, what);
        expect(sizes[0] == 0xDEADBEEF && sizes[1] == 0xDEADBEEF, "sizes are untouched");
    };
    // [7] that is valid passes on to the extent's check (entry [4] of frame 0, the first row); one that is not is named
    for (double v : {0.0, 1.0, 16.0, 17.0}) refused_at(LR_PIX_U8X3, 0, 7, v, 0, 4, "a valid [7] for LR_PIX_U8X3 is not what is refused");
    for (double v : {2.0, 3.0, 15.0, 18.0, 19.0, 32.0, 33.0, 48.0, 0.5, 16.5, -1.0, -16.0, 1e300, (double)NAN, (double)INFINITY})
        refused_at(LR_PIX_U8X3, 0, 7, v, 0, 7, "an invalid [7] for LR_PIX_U8X3 is refused at [7]");
    for (double v : {0.0, 16.0}) refused_at(LR_PIX_U8, 0, 7, v, 0, 4, "a valid [7] for LR_PIX_U8 is not what is refused");
    for (double v : {1.0, 2.0, 17.0, 32.0, 15.0, 16.5}) refused_at(LR_PIX_U8, 0, 7, v, 0, 7, "an invalid [7] for LR_PIX_U8 is refused at [7]");
    refused_at(LR_PIX_U8X3, 1, 7, 18.0, 0, 4, "rows are checked in order: frame 0's extent comes before frame 1's [7]");
    refused_at(LR_PIX_U8X3, 0, 6, 101.0, 0, 6, "quality");
    refused_at(LR_PIX_U8X3, 0, 0, 65536.0, 0, 0, "width");
    refused_at(LR_PIX_U8X3, 0, 3, 119.0, 0, 3, "stride");
    {   // many optimised rows (the list of optimised frames grows), the last one bad
        const int batch = 1000;
        std::vector<double> t((size_t)batch * 8);
        std::vector<uint64_t> many((size_t)batch, 7);
        for (int b = 0; b < batch; ++b) {
            std::memcpy(&t[(size_t)b * 8], row, sizeof row);
            t[(size_t)b * 8 + 5] = 0;  // (capacity 0: every extent is empty and inside a region of 0 bytes)
            t[(size_t)b * 8 + 7] = 16 + (b & 1);
        }
        t[(size_t)(batch - 1) * 8 + 7] = 34;
        const int rc = encode(&ctx, LR_PIX_U8X3, t, batch, many.data());
        expect(rc != 0 && std::string(lr_last_error()).find("frame 999: entry [7]") != std::string::npos, "the last of 1000 rows");
        expect(many[0] == 7 && many[999] == 7, "sizes are untouched");
    }
    std::printf("%d checks, %d failed: %s\n", checked, failures, failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
