// csrc/reg_plan.h against a brute-force restatement of its rules (loops over rows and over pages, no division), on cases in
// which each rule decides at least once.  Addresses are numbers: nothing is read through them.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "reg_plan.h"

using lramd::RegPlan;

static const uintptr_t kPage = 4096;
static int failures = 0;

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            ++failures;                           \
            std::printf("FAIL %s: ", #cond);      \
            std::printf(__VA_ARGS__);             \
            std::printf("\n");                    \
        }                                         \
    } while (0)

struct Expect {  // what the table of the case says about one frame (offsets from the frame's address; -1: not stated)
    int frame;
    bool planned;
    long lo_off, hi_off;
    int r_lo, r_hi;
};

struct Case {
    std::string name;
    std::vector<uintptr_t> addr;
    int h;
    size_t pitch, row_bytes;
    std::vector<char> may;
    std::vector<Expect> expect;
};

static std::vector<uintptr_t> array_of(uintptr_t base, size_t step, int n) {
    std::vector<uintptr_t> a;
    for (int i = 0; i < n; ++i) a.push_back(base + (size_t)i * step);
    return a;
}

static int n_frames = 0;

static std::vector<RegPlan> check_case(const Case& c) {
    const int n = (int)c.addr.size();
    std::vector<const void*> ptrs;
    for (uintptr_t a : c.addr) ptrs.push_back(reinterpret_cast<const void*>(a));
    const std::vector<RegPlan> plan = lramd::plan_registrations(ptrs.data(), n, c.h, c.pitch, c.row_bytes, kPage, c.may.data());
    CHECK((int)plan.size() == n, "%s: %d plans for %d frames", c.name.c_str(), (int)plan.size(), n);
    std::map<uintptr_t, int> owner;  // page -> the frame whose (restated) plan holds it
    for (int i = 0; i < n && i < (int)plan.size(); ++i, ++n_frames) {
        const char* nm = c.name.c_str();
        const RegPlan& p = plan[(size_t)i];
        const uintptr_t a = c.addr[(size_t)i];
        uintptr_t e = a + c.row_bytes;
        for (int r = 1; r < c.h; ++r) e += c.pitch;
        // the whole pages inside [a, e)
        uintptr_t lo = 0, hi = 0;
        bool pages = false, shared = false;
        for (uintptr_t q = 0; q + kPage <= e; q += kPage) {
            if (q < a) continue;
            if (!pages) lo = q;
            pages = true;
            hi = q + kPage;
            shared = shared || owner.count(q) != 0;
        }
        // the rows that lie wholly inside [lo, hi)
        int first = -1, last = -1, inside = 0;
        uintptr_t s = a;
        for (int r = 0; r < c.h; ++r, s += c.pitch) {
            if (!pages || s < lo || s + c.row_bytes > hi) continue;
            if (first < 0) first = r;
            last = r;
            ++inside;
        }
        const bool want = c.may[(size_t)i] && pages && !(inside < c.h / 2) && !shared;
        const bool got = p.hi > p.lo;
        CHECK(got == want, "%s frame %d: planned %d, restated %d", nm, i, (int)got, (int)want);
        if (!c.may[(size_t)i]) CHECK(!got, "%s frame %d: a plan without the flag", nm, i);
        if (!got) {
            CHECK(p.lo == 0 && p.hi == 0 && p.r_lo == 0 && p.r_hi == 0, "%s frame %d: an empty plan is all zeros", nm, i);
        } else {
            CHECK(p.lo == lo && p.hi == hi, "%s frame %d: pages [%lu, %lu), restated [%lu, %lu)", nm, i, (unsigned long)p.lo, (unsigned long)p.hi,
                  (unsigned long)lo, (unsigned long)hi);
            bool lo_mult = false, hi_mult = false;  // (page multiples, by counting)
            for (uintptr_t q = 0; q <= p.hi; q += kPage) {
                lo_mult = lo_mult || q == p.lo;
                hi_mult = hi_mult || q == p.hi;
            }
            CHECK(lo_mult && hi_mult, "%s frame %d: lo and hi are page multiples", nm, i);
            CHECK(p.lo >= a && p.hi <= e, "%s frame %d: pages inside the frame", nm, i);
            CHECK(p.r_lo == first && p.r_hi == last + 1 && p.r_hi - p.r_lo == inside, "%s frame %d: rows [%d, %d), restated [%d, %d) (%d inside)", nm, i,
                  p.r_lo, p.r_hi, first, last + 1, inside);
            CHECK(p.r_hi - p.r_lo >= c.h / 2, "%s frame %d: at least half the rows", nm, i);
            for (uintptr_t q = p.lo; q < p.hi; q += kPage) {
                CHECK(owner.count(q) == 0, "%s frame %d: page %lu belongs to frame %d's plan too", nm, i, (unsigned long)q, owner.count(q) ? owner[q] : -1);
                owner[q] = i;
            }
        }
    }
    for (const Expect& x : c.expect) {
        const RegPlan& p = plan[(size_t)x.frame];
        const uintptr_t a = c.addr[(size_t)x.frame];
        const char* nm = c.name.c_str();
        CHECK((p.hi > p.lo) == x.planned, "%s frame %d: planned %d, the table says %d", nm, x.frame, (int)(p.hi > p.lo), (int)x.planned);
        if (x.lo_off >= 0) CHECK((long)(p.lo - a) == x.lo_off && (long)(p.hi - a) == x.hi_off, "%s frame %d: lo - a = %ld, hi - a = %ld", nm, x.frame, (long)(p.lo - a), (long)(p.hi - a));
        if (x.r_lo >= 0) CHECK(p.r_lo == x.r_lo && p.r_hi == x.r_hi, "%s frame %d: rows [%d, %d), the table says [%d, %d)", nm, x.frame, p.r_lo, p.r_hi, x.r_lo, x.r_hi);
    }
    return plan;
}

int main() {
    std::vector<Case> cases;
    cases.push_back({"u8 1920x1080, contiguous, base 7 pages + 1", array_of(7 * kPage + 1, (size_t)1920 * 1080, 3), 1080, 1920, 1920, {1, 1, 1},
                     {{1, true, 3071, 2071551, 2, 1078}}});
    cases.push_back({"the same, frame 2 without the flag", array_of(7 * kPage + 1, (size_t)1920 * 1080, 3), 1080, 1920, 1920, {1, 1, 0},
                     {{1, true, 3071, 2071551, 2, 1078}, {2, false, -1, -1, -1, -1}}});
    cases.push_back({"f32 960x540, pitch 4000, base 5 pages", array_of(5 * kPage, (size_t)4000 * 540, 4), 540, 4000, 3840, {1, 1, 1, 1},
                     {{3, true, 3968, 2158464, 1, 539}}});
    cases.push_back({"u8 517x131, base 3 pages + 1", array_of(3 * kPage + 1, (size_t)517 * 131, 3), 131, 517, 517, {1, 1, 1}, {{2, true, -1, -1, 8, 126}}});
    cases.push_back({"u8x3 333x190, base 2 pages + 64", array_of(2 * kPage + 64, (size_t)999 * 190, 2), 190, 999, 999, {1, 1}, {{1, true, -1, -1, 3, 187}}});
    cases.push_back({"rows of 5000 bytes, pitch 8192, h = 3", {9 * kPage + 17}, 3, 8192, 5000, {1}, {{0, true, -1, -1, 1, 2}}});
    cases.push_back({"rows of 5000 bytes, pitch 8192, h = 2", {9 * kPage + 4095}, 2, 8192, 5000, {1}, {{0, false, -1, -1, -1, -1}}});
    cases.push_back({"f32 40x6 inside one page", {4 * kPage + 100}, 6, 160, 160, {1}, {{0, false, -1, -1, -1, -1}}});
    cases.push_back({"a frame listed twice", {6 * kPage + 9, 6 * kPage + 9}, 480, 640, 640, {1, 1}, {{0, true, -1, -1, -1, -1}, {1, false, -1, -1, -1, -1}}});
    cases.push_back({"sliding windows, half a frame apart", array_of(3 * kPage + 5, (size_t)640 * 240, 7), 480, 640, 640, {1, 1, 1, 1, 1, 1, 1},
                     {{0, true, -1, -1, -1, -1}}});
    cases.push_back({"twelve contiguous u8 1920x1080 frames", array_of(11 * kPage, (size_t)1920 * 1080, 12), 1080, 1920, 1920, std::vector<char>(12, 1), {}});
    std::vector<std::vector<RegPlan>> plans;
    for (const Case& c : cases) plans.push_back(check_case(c));
    const std::vector<RegPlan>& win = plans[9];
    for (size_t i = 1; i < win.size(); ++i)
        CHECK(!(win[i].hi > win[i].lo && win[i - 1].hi > win[i - 1].lo), "sliding windows: frames %d and %d both planned", (int)i - 1, (int)i);
    for (size_t i = 0; i < plans[10].size(); ++i) CHECK(plans[10][i].hi > plans[10][i].lo, "twelve frames: frame %d has no plan", (int)i);
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok %d cases %d frames\n", (int)cases.size(), n_frames);
    return 0;
}
