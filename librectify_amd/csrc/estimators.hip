// The vanishing-point estimators around their GPU kernels: RANSAC (the default), the opt-in PROSAC, Direct and diamond-space
// estimators with their host replays, the peeling loop they share, and the refinement of the raw segments.
#include "host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

namespace lramd {

namespace {

// the lines `order` of a model the way the kernels read them: packed into the page-locked mirror and sent to the device
int upload_model(lr_context* c, const PencilModel& model, const std::vector<int>& order, PencilSoA* out) {
    const size_t n = order.size();
    if (ctx_ensure_ransac_capacity(c, n)) return 1;
    float* hm = c->model.h;
    for (size_t j = 0; j < n; ++j) {
        const int i = order[j];
        hm[0 * n + j] = model.anchor[i].x;
        hm[1 * n + j] = model.anchor[i].y;
        hm[2 * n + j] = model.direction[i].x;
        hm[3 * n + j] = model.direction[i].y;
        hm[4 * n + j] = model.length[i];
        hm[5 * n + j] = model.h[i].x;
        hm[6 * n + j] = model.h[i].y;
        hm[7 * n + j] = model.h[i].z;
    }
    float* dm = c->model.d;
    LR_HIP(hipMemcpyAsync(dm, hm, 8 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    *out = PencilSoA{dm + 0 * n, dm + 1 * n, dm + 2 * n, dm + 3 * n, dm + 4 * n, dm + 5 * n, dm + 6 * n, dm + 7 * n};
    return 0;
}

}  // namespace

// ---- RANSAC ------------------------------------------------------------------------------

int ctx_ransac_best(lr_context* c, const PencilModel& model, const std::vector<int>& indices, float tol, int n_iter,
                    uint64_t seed, uint32_t round, Vec3* best_h, float* best_score, int* best_iter) {
    LR_HIP(hipSetDevice(c->device));
    const size_t n = indices.size();
    *best_h = {0.f, 0.f, 0.f};  // the reference leaves best_h uninitialised when nothing scores (estimator.h:39)
    *best_score = 0.f;
    *best_iter = -1;
    if (n < 2 || n_iter <= 0) return 0;
    PencilSoA m;
    if (upload_model(c, model, indices, &m)) return 1;
    // scoring launch + read-out: (score bits, iteration) arrive in the page-locked pair, no copy commands
    if (launch_ransac_score(m, (uint32_t)n, tol, model.degeneracy_tol, (uint32_t)n_iter, seed, round, c->d_best_slots,
                            reinterpret_cast<uint32_t*>(c->h_best.get()), c->stream))
        return 1;
    LR_HIP(hipStreamSynchronize(c->stream));
    int32_t it;
    std::memcpy(&it, &c->h_best[1], sizeof(it));
    *best_score = c->h_best[0];
    *best_iter = it;
    if (it >= 0) {
        uint32_t a, b;
        sample_pair(seed, round, (uint32_t)it, (uint32_t)n, a, b);
        *best_h = model.fit(indices[a], indices[b]);
    }
    return 0;
}

// estimate_line_pencils (line_pencil.cpp:148-177) for lines the host holds: upload, peel on the device, download.
int ctx_estimate_line_pencils(lr_context* c, std::vector<LineSegment>& lines, int max_models, float inlier_deg,
                              float garbage_deg, int n_iter, uint64_t seed) {
    if (lines.empty()) return 0;
    LR_HIP(hipSetDevice(c->device));
    const size_t n = lines.size();
    if (ensure_group_capacity(c, n)) return 1;
    LR_HIP(hipMemcpyAsync(c->d_flines, lines.data(), n * sizeof(LineSegment), hipMemcpyHostToDevice, c->stream));
    if (launch_lines_bbox(c->d_flines, (uint32_t)n, c->d_gctl, c->d_gnorm, c->stream)) return 1;
    if (enqueue_groups(c, (uint32_t)n, max_models, inlier_deg, garbage_deg, n_iter, seed)) return 1;
    LR_HIP(hipMemcpyAsync(lines.data(), c->d_flines, n * sizeof(LineSegment), hipMemcpyDeviceToHost, c->stream));
    LR_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- PROSAC (opt-in; reference prosac.h, never instantiated there) ---------------------------------

namespace {

constexpr uint32_t kProsacRecCap = 32;  // new-best iterations of a chunk whose inlier flags come back with its counts

// (each group's capacity is read off the buffer it grows last)
int ensure_prosac_buffers(lr_context* c, size_t n_lines, size_t n_pairs, size_t chunk) {
    if (2 * n_pairs > c->pairs.cap()) {
        LR_HIP(hipStreamSynchronize(c->stream));
        if ((!c->d_peak && c->d_peak.grow(4)) || c->pairs.grow(2 * n_pairs)) return 1;
    }
    if (n_lines > c->weights.cap()) {
        LR_HIP(hipStreamSynchronize(c->stream));
        if (c->weights.grow(std::max<size_t>(n_lines, 4096))) return 1;
    }
    // (two of everything a chunk of hypotheses uses: the next chunk is on the GPU while the host goes through the last one)
    if (2 * n_lines * kProsacRecCap > c->recflags.cap()) {
        LR_HIP(hipStreamSynchronize(c->stream));
        if (c->rec.grow(2 * (kProsacRecCap + 1)) || c->recflags.grow(2 * std::max<size_t>(n_lines, 4096) * kProsacRecCap)) return 1;
    }
    if (2 * chunk > c->hcounts.cap()) {
        LR_HIP(hipStreamSynchronize(c->stream));
        if (c->samples.grow(4 * chunk) || c->hcounts.grow(2 * chunk)) return 1;
    }
    for (Event& e : c->prosac_ev)
        if (e.ensure(hipEventDisableTiming)) return 1;
    return 0;
}

// Stable argsort by weight, descending (reference utils.h:36-44 uses std::stable_sort with a > comparator).  The weights
// are fourth powers (>= +0), so the order of their bit patterns is their order: three stable 11-bit counting passes over
// the complemented bits, a fifth of std::stable_sort's time on 24 000 lines.  A NaN weight (a line through the peak
// itself) has no place in that order: then the comparison sort decides, with the NaNs last in their own order.
void stable_order_descending(const std::vector<float>& w, std::vector<int>& order) {
    const size_t n = w.size();
    order.resize(n);
    bool plain = true;
    for (size_t i = 0; i < n; ++i) plain = plain && w[i] >= 0.0f && !std::signbit(w[i]);  // (false for NaN and -0)
    if (!plain || n < 256) {
        for (size_t i = 0; i < n; ++i) order[i] = (int)i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {  // NaN last, stably: a strict weak ordering
            if (std::isnan(w[a])) return false;
            if (std::isnan(w[b])) return true;
            return w[a] > w[b];
        });
        return;
    }
    std::vector<uint32_t> key(n), key2(n);
    std::vector<int> idx(n), idx2(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t b;
        std::memcpy(&b, &w[i], 4);
        key[i] = ~b;
        idx[i] = (int)i;
    }
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass * 11;
        uint32_t cnt[2049] = {0};
        for (size_t i = 0; i < n; ++i) cnt[((key[i] >> shift) & 2047u) + 1]++;
        for (int b = 0; b < 2048; ++b) cnt[b + 1] += cnt[b];
        for (size_t i = 0; i < n; ++i) {
            const uint32_t p = cnt[(key[i] >> shift) & 2047u]++;
            key2[p] = key[i];
            idx2[p] = idx[i];
        }
        key.swap(key2);
        idx.swap(idx2);
    }
    order = idx;
}

// prosac.h:31-55
int niter_ransac(double p, double epsilon, int s, int Nmax) {
    if (Nmax == -1) Nmax = INT32_MAX;
    if (epsilon <= 0.) return 1;
    const double logarg = -std::exp(s * std::log(1. - epsilon));
    const double logval = std::log(1. + logarg);
    const double N = std::log(1. - p) / logval;
    if (logval < 0. && N < Nmax) return (int)std::ceil(N);
    return Nmax;
}

const float kChi2[20] = {INFINITY,   6.6348966f,  5.41189443f, 4.70929225f, 4.21788459f, 3.84145882f, 3.5373846f,
                         3.28302029f, 3.06490172f, 2.8743734f,  2.70554345f, 2.55422131f, 2.41732093f, 2.29250453f,
                         2.17795916f, 2.07225086f, 1.97422609f, 1.88294329f, 1.79762406f, 1.71761761f};

inline uint32_t sample_one(uint64_t seed, uint32_t round, uint32_t iter, uint32_t n) {
    const uint64_t z = splitmix64(seed ^ splitmix64(((uint64_t)round << 32) | iter));
    return (uint32_t)(((uint64_t)(uint32_t)z * n) >> 32);
}

// the growth function of PROSAC (prosac.h:150-166): pure bookkeeping, no data
struct Growth {
    int t, n, T_n_prime;
    double T_n;
    void advance(int n_star, int m) {
        t = t + 1;
        if ((t > T_n_prime) && (n < n_star)) {
            const double T_nplus1 = (T_n * (n + 1)) / (n + 1 - m);
            n = n + 1;
            T_n_prime = T_n_prime + (int)std::ceil(T_nplus1 - T_n);
            T_n = T_nplus1;
        }
    }
};

}  // namespace

// get_weights (line_pencil.cpp:47-86): vote pairs from the host's std::mt19937 (default seed, as the
// reference), accumulator and peak on the GPU, weights back on the host (positions follow `indices`).
int ctx_ht_weights(lr_context* c, const PencilModel& model, const std::vector<int>& indices, std::vector<float>& weights) {
    LR_HIP(hipSetDevice(c->device));
    const size_t n = indices.size();
    weights.assign(n, 0.f);
    if (n == 0) return 0;
    const int n_pairs = 20000, ht = 65;  // line_pencil.h:26-27
    if (ensure_prosac_buffers(c, n, (size_t)n_pairs, 1)) return 1;
    {
        std::mt19937 rng;
        std::uniform_int_distribution<int> rand_idx(0, (int)n - 1);
        for (int i = 0; i < n_pairs; ++i) {
            c->pairs.h[i] = rand_idx(rng);
            c->pairs.h[n_pairs + i] = rand_idx(rng);
        }
    }
    PencilSoA m;
    if (upload_model(c, model, indices, &m)) return 1;
    LR_HIP(hipMemcpyAsync(c->pairs.d, c->pairs.h, 2 * (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (launch_ht_weights(m, (uint32_t)n, c->pairs.d, c->pairs.d + n_pairs, n_pairs, ht, c->d_peak, c->weights.d, c->stream))
        return 1;
    LR_HIP(hipMemcpyAsync(c->weights.h, c->weights.d, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    LR_HIP(hipStreamSynchronize(c->stream));
    std::copy(c->weights.h.get(), c->weights.h + n, weights.begin());
    return 0;
}

// PROSAC_Estimator::solve (prosac.h:104-299).  The sequential loop is replayed on the host exactly as
// written; only "support of the model" (the inlier count of every sample against all lines) runs on the
// GPU, for a speculative chunk of upcoming iterations at a time.  The sample of iteration t depends on
// earlier results only through n_star, which changes when a new best hypothesis appears: the chunk is
// then cut at that iteration and the rest regenerated, so the outcome equals the sequential run.
int ctx_prosac_solve(lr_context* c, const PencilModel& model, const std::vector<int>& indices, float tol, int T_N_in,
                     uint64_t seed, uint32_t round, Vec3* h_out, ProsacTrace* trace) {
    static const bool pdebug = std::getenv("LIBRECTIFY_PROSAC_DEBUG") != nullptr;
    double t_w = now_ms(), t_events = 0, t_gen = 0, t_gpu = 0, t_flags = 0, t_len = 0;
    int n_events = 0, n_chunks = 0, n_single = 0;
    std::vector<float> weights;
    if (ctx_ht_weights(c, model, indices, weights)) return 1;
    const double t_w1 = now_ms();
    const int N = (int)indices.size();
    std::vector<int> order(N);
    stable_order_descending(weights, order);  // utils.h:36-44 (argsort, stable, by weight descending)
    const double t_s1 = now_ms();
    std::vector<int> idx(N);
    for (int i = 0; i < N; ++i) idx[i] = indices[order[i]];
    const int m = 2;
    const float eta = 0.05f, beta = 0.01f, psi = 0.02f, p_good = 0.9f, max_outlier = 0.5f;  // prosac.h:62-66
    const int T_N = T_N_in > 0 ? T_N_in : niter_ransac(p_good, max_outlier, m, -1);
    float chi2_value;
    {
        const float p2 = 2 * psi;
        chi2_value = kChi2[(int)std::floor(std::max(std::min(p2, 0.2f), 0.01f) * 100)];
    }
    auto Imin = [&](int mm, int n) {
        const double mu = n * beta;
        const double sigma = std::sqrt(n * beta * (1 - beta));
        return (int)std::ceil(mm + mu + sigma * std::sqrt(chi2_value));
    };
    int n_star = N, I_n_star = 0, I_N_best = 0, k_n_star = T_N, best_iter = -1;
    const int I_N_min = (int)((1. - max_outlier) * N);
    Growth g{0, m, 1, (double)T_N};
    for (int i = 0; i < m; i++) g.T_n *= (double)(g.n - i) / (N - i);
    Vec3 p_best{0, 0, 0};
    std::vector<uint8_t> best_inl(N, 0), isInlier(N);
    std::vector<int> pre;
    PencilSoA soa;
    if (N >= 2 && upload_model(c, model, idx, &soa)) return 1;
    // sample of iteration s.t from the growth state (prosac.h:170-190)
    auto sample_of = [&](const Growth& s, uint32_t& sa, uint32_t& sb) {
        if (s.t > s.T_n_prime) {
            sample_pair(seed, round, (uint32_t)s.t, (uint32_t)s.n, sa, sb);
        } else {
            sa = sample_one(seed, round, (uint32_t)s.t, (uint32_t)(s.n - 1));
            sb = (uint32_t)(s.n - 1);  // prosac.h:186 writes n (one past U_n); n-1 is meant
        }
    };
    // Chunks of upcoming iterations, two in flight: while the host goes through the counts of one, the GPU works on the
    // next, which was generated as if the first held no new best.  Nothing of a chunk is used without the check below
    // (iteration by iteration: does the true state still draw this sample?), so a chunk generated under a wrong guess
    // costs GPU time and never a result.
    constexpr size_t kChunkMax = 1u << 16;
    struct Chunk {
        size_t cnt = 0;
        int buf = 0;
        Growth start{0, 0, 0, 0.0}, end{0, 0, 0, 0.0};  // growth state before its first / behind its last sample
        int n_star = 0;                                  // ... and the n_star it was drawn with
        bool live = false;
    };
    if (N >= 2 && ensure_prosac_buffers(c, (size_t)N, 1, kChunkMax)) return 1;
    const size_t rf_bytes = c->recflags.cap() / 2;  // (per chunk buffer)
    auto running = [&](const Growth& s) { return ((I_N_best < I_N_min) || s.t <= k_n_star) && s.t < T_N; };
    size_t chunk = 2048;
    auto start_chunk = [&](const Growth& from, int buf, Chunk& ch) -> int {
        const double tg0 = now_ms();
        uint32_t* hs = c->samples.h + (size_t)buf * 2 * kChunkMax;
        uint32_t* ds = c->samples.d + (size_t)buf * 2 * kChunkMax;
        Growth s = from;
        // the second sample of the pairs follows the first ones directly: the length is not known before the loop ends,
        // so they are written at the far end first (cheap: one pass over 4 bytes per iteration)
        size_t cnt = 0;
        while (cnt < chunk && running(s)) {
            s.advance(n_star, m);
            uint32_t sa, sb;
            sample_of(s, sa, sb);
            hs[cnt] = sa;
            hs[kChunkMax + cnt] = sb;
            ++cnt;
        }
        ch.cnt = cnt;
        ch.buf = buf;
        ch.start = from;
        ch.end = s;
        ch.n_star = n_star;
        ch.live = cnt > 0;
        t_gen += now_ms() - tg0;
        if (!ch.live) return 0;
        ++n_chunks;
        if (cnt < kChunkMax) std::memmove(hs + cnt, hs + kChunkMax, cnt * sizeof(uint32_t));
        uint32_t* dcnt = c->hcounts.d + (size_t)buf * kChunkMax;
        uint32_t* drec = c->rec.d + (size_t)buf * (kProsacRecCap + 1);
        uint8_t* dflags = c->recflags.d + (size_t)buf * rf_bytes;
        LR_HIP(hipMemcpyAsync(ds, hs, 2 * cnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (launch_prosac_count(soa, (uint32_t)N, tol, model.degeneracy_tol, ds, ds + cnt, (uint32_t)cnt, dcnt, c->stream)) return 1;
        LR_HIP(hipMemcpyAsync(c->hcounts.h + (size_t)buf * kChunkMax, dcnt, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        // the chunk's new-best iterations (they follow from the counts and the best count known when it is enqueued: a
        // best found in the chunk before it can only strike some of them off) and the inlier flags of each come back
        // with the counts: one wait per chunk, not one per new best
        if (launch_prosac_records(soa, (uint32_t)N, ds, ds + cnt, dcnt, (uint32_t)cnt, (uint32_t)std::max(I_N_best, 0), tol, drec,
                                  kProsacRecCap, dflags, c->stream))
            return 1;
        LR_HIP(hipMemcpyAsync(c->rec.h + (size_t)buf * (kProsacRecCap + 1), drec, (kProsacRecCap + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        LR_HIP(hipMemcpyAsync(c->recflags.h + (size_t)buf * rf_bytes, dflags, (size_t)N * kProsacRecCap, hipMemcpyDeviceToHost, c->stream));
        LR_HIP(hipEventRecord(c->prosac_ev[buf], c->stream));
        chunk = std::min<size_t>(chunk * 4, kChunkMax);
        return 0;
    };
    Chunk cur, nxt;
    while (N >= 2 && running(g)) {
        if (!cur.live) {
            if (start_chunk(g, 0, cur)) return 1;
            if (!cur.live) break;
        }
        if (!nxt.live && start_chunk(cur.end, cur.buf ^ 1, nxt)) return 1;
        const double tg1 = now_ms();
        LR_HIP(hipEventSynchronize(c->prosac_ev[cur.buf]));
        const double tg2 = now_ms();
        t_gpu += tg2 - tg1;
        const uint32_t* hs = c->samples.h + (size_t)cur.buf * 2 * kChunkMax;
        const uint32_t* hsb = hs + cur.cnt;
        const uint32_t* hcnt = c->hcounts.h + (size_t)cur.buf * kChunkMax;
        const uint32_t* hrec = c->rec.h + (size_t)cur.buf * (kProsacRecCap + 1);
        const uint8_t* hflags = c->recflags.h + (size_t)cur.buf * rf_bytes;
        const uint32_t n_rec = std::min<uint32_t>(hrec[0], kProsacRecCap);
        uint32_t rec_pos = 0;
        // The chunk was generated under the state at its start (or an earlier one).  A new best hypothesis changes n_star
        // and k_n_star; what follows it in the chunk is still the sequential algorithm's as long as the loop would go on
        // and would draw the same sample: checked iteration by iteration, and the chunk is cut where that stops being true.
        // (Drawn from this very state with this n_star, the samples ARE the sequence: nothing to compare until a new best
        // changes n_star.)
        bool same = cur.n_star == n_star && cur.start.t == g.t && cur.start.n == g.n && cur.start.T_n_prime == g.T_n_prime &&
                    cur.start.T_n == g.T_n;
        size_t j = 0;
        for (; j < cur.cnt; ++j) {
            if (!running(g)) break;
            Growth gn = g;
            gn.advance(n_star, m);
            if (!same) {
                uint32_t ea, eb;
                sample_of(gn, ea, eb);
                if (ea != hs[j] || eb != hsb[j]) break;
            }
            g = gn;
            const uint32_t I = hcnt[j];
            if (I == 0xFFFFFFFFu) continue;  // degenerate sample
            if ((int)I > I_N_best) {
                const int ia = idx[hs[j]], ib = idx[hsb[j]];
                const Vec3 p_t = model.fit(ia, ib);
                int I_N = 0;
                const double te0 = pdebug ? now_ms() : 0.;
                while (rec_pos < n_rec && hrec[1 + rec_pos] < (uint32_t)j) ++rec_pos;
                if (rec_pos < n_rec && hrec[1 + rec_pos] == (uint32_t)j) {  // its flags came with the chunk
                    std::memcpy(isInlier.data(), hflags + (size_t)rec_pos * N, (size_t)N);
                    for (int i = 0; i < N; ++i) I_N += isInlier[i];
                } else if (N >= 4096) {  // (more new bests in the chunk than flag rows: one by one)
                    if (launch_prosac_flags(soa, (uint32_t)N, p_t.x, p_t.y, p_t.z, tol, reinterpret_cast<uint8_t*>(c->weights.d.get()), c->stream))  // (the weights buffer is free by now)
                        return 1;
                    LR_HIP(hipMemcpyAsync(isInlier.data(), c->weights.d, (size_t)N, hipMemcpyDeviceToHost, c->stream));
                    LR_HIP(hipStreamSynchronize(c->stream));
                    for (int i = 0; i < N; ++i) I_N += isInlier[i];
                    ++n_single;
                } else {
                    for (int i = 0; i < N; ++i) {
                        isInlier[i] = model.error(p_t, idx[i]) < tol;
                        I_N += isInlier[i];
                    }
                }
                I_N_best = I_N;
                p_best = p_t;
                best_inl = isInlier;
                best_iter = g.t;
                const double te1 = pdebug ? now_ms() : 0.;
                t_flags += te1 - te0;
                int n_best = N, I_n_best = I_N;
                double epsilon_n_best = (double)I_n_best / n_best;
                // prosac.h:236-262, the search for the best termination length, as written -- but lengths that could pass
                // its two conditions (more inliers per line among the first n_test than among the first n_best, and
                // more than chance explains) are looked for 64 at a time on the prefix counts (a loop without exits,
                // which the compiler vectorises): few lengths do, and the scalar loop took a square root for most of
                // the N of them, for every new best
                // (Imin depends on the length alone, not on the lines: two roots per length once per context, not per new best)
                std::vector<int>& imin_tab = c->prosac_imin;
                for (int n = (int)imin_tab.size(); n <= N; ++n) imin_tab.push_back(n > m ? Imin(m, n) : 0);
                pre.resize((size_t)N + 1);
                pre[0] = 0;
                for (int i = 0; i < N; ++i) pre[(size_t)i + 1] = pre[(size_t)i] + isInlier[i];
                int n_test = N;
                bool stop = false;
                while (n_test > m && !stop) {
                    const int lo = std::max(m + 1, n_test - 63);
                    // (the second condition without its root, in single precision with room for every rounding -- the sum
                    // I - eps n is off by less than 4e-7 n + 0.02 for any line count the interface allows: lengths whose
                    // upper bound of (I - eps n)^2 is clearly below the variance term cannot pass; the expression as
                    // written decides in the scalar loop.  Four lengths per SSE instruction.)
                    const float e_b = (float)epsilon_n_best;
                    const float q_b = (float)(epsilon_n_best * (1. - epsilon_n_best) * 2.706 * (1. - 1e-3));
                    int any = 0;
                    for (int n = lo; n <= n_test; ++n) {
                        const float dn = (float)n, dd = ((float)pre[(size_t)n] - e_b * dn) + (4e-7f * dn + 0.02f);
                        any |= (dd > 0.f) & (dd * dd >= dn * q_b);
                    }
                    if (!any) {
                        n_test = lo - 1;
                        continue;
                    }
                    for (; n_test >= lo; n_test--) {
                        const int I_n_test = pre[(size_t)n_test];
                        if (!(I_n_test * n_best > I_n_best * n_test)) continue;
                        // I > eps n + sqrt(v): decided on (I - eps n)^2 against v where that is clear of every rounding,
                        // by the expression as written otherwise (the root is what this loop's time went into)
                        const double en = epsilon_n_best * n_test, v = n_test * epsilon_n_best * (1. - epsilon_n_best) * 2.706;
                        const double dd = (double)I_n_test - en;
                        bool second;
                        if (!(dd > 0.) || dd * dd < v * (1. - 1e-9)) second = false;
                        else if (dd * dd > v * (1. + 1e-9)) second = true;
                        else second = I_n_test > en + std::sqrt(v);
                        if (second) {
                            if (I_n_test < imin_tab[(size_t)n_test]) {
                                stop = true;
                                break;
                            }
                            n_best = n_test;
                            I_n_best = I_n_test;
                            epsilon_n_best = (double)I_n_best / n_best;
                        }
                    }
                }
                if (pdebug) t_len += now_ms() - te1;
                if (I_n_best * n_star > I_n_star * n_best) {
                    same = same && n_best == n_star;
                    n_star = n_best;
                    I_n_star = I_n_best;
                    k_n_star = niter_ransac(1. - eta, 1. - I_n_star / (double)n_star, m, T_N);
                }
                ++n_events;
            }
        }
        t_events += now_ms() - tg2;
        if (j == cur.cnt && nxt.live) {
            cur = nxt;  // its first iteration is the one after this chunk's last: still in step
            nxt.live = false;
        } else {
            // cut (or over): what is in flight continues a sequence that was not drawn; its buffers are free once it is done
            if (nxt.live) LR_HIP(hipEventSynchronize(c->prosac_ev[nxt.buf]));
            cur.live = nxt.live = false;
        }
    }
    if (cur.live || nxt.live) LR_HIP(hipStreamSynchronize(c->stream));
    if (pdebug)
        std::fprintf(stderr, "prosac round %u: N %d, weights %.2f ms, sort %.2f, chunks %d (generate %.2f, gpu+sync %.2f, scan+events %.2f of which flags %.2f, lengths %.2f; %d events, %d with a wait of their own), total %.2f ms\n",
                     round, N, t_w1 - t_w, t_s1 - t_w1, n_chunks, t_gen, t_gpu, t_events, t_flags, t_len, n_events, n_single, now_ms() - t_w);
    if (trace) {
        trace->iterations = g.t;
        trace->n_star = n_star;
        trace->best_iter = best_iter;
        trace->I_N_best = I_N_best;
    }
    std::vector<int> inl;
    for (int i = 0; i < N; ++i)
        if (best_inl[i]) inl.push_back(idx[i]);
    *h_out = model.fit_optimal(inl);
    return 0;
}

namespace {

// The peeling loop of estimate_multiple_structures (estimator.h:99-145) for the estimators whose verdicts stay on the host:
// solve(obs, k, &h) gives round k's model from the lines still in play (ascending); the lines within tol of it become group
// k, those within garbage_tol are discarded.  taken(out, more) sees the lines a round took out (ascending) and whether
// another round follows.
template <class Solve, class Taken>
int peel_models(const PencilModel& model, std::vector<LineSegment>& lines, int max_models, float inlier_deg, float garbage_deg,
                Solve solve, Taken taken) {
    const float tol = cos_threshold(inlier_deg), garbage_tol = cos_threshold(garbage_deg);
    const int N = model.size();
    std::vector<int> inlier_flag(N, -1), garbage_flag(N, 0), obs, out;
    int remaining = N, k = 0;
    while (remaining >= 2 && k < max_models) {  // estimator.h:115
        obs.clear();
        for (int i = 0; i < N; ++i)
            if (inlier_flag[i] < 0 && garbage_flag[i] == 0) obs.push_back(i);
        Vec3 h;
        if (solve(obs, k, &h)) return 1;
        out.clear();
        for (int i : obs) {
            const float e = model.error(h, i);
            if (e < tol) {
                inlier_flag[i] = k;
                out.push_back(i);
            } else if (e >= tol && e < garbage_tol) {
                garbage_flag[i] = 1;
                out.push_back(i);
            }
        }
        remaining -= (int)out.size();
        ++k;
        if (taken(out, remaining >= 2 && k < max_models)) return 1;
    }
    for (int i = 0; i < N; ++i) lines[i].group_id = garbage_flag[i] == 1 ? -1 : inlier_flag[i];
    return 0;
}

int nothing_taken(const std::vector<int>&, bool) { return 0; }

PencilModel normalised_model(const std::vector<LineSegment>& lines) {
    return PencilModel(normalise(lines, bbox_normalisation(lines)));
}

}  // namespace

int ctx_estimate_line_pencils_prosac(lr_context* c, std::vector<LineSegment>& lines, int max_models, float inlier_deg,
                                     float garbage_deg, int T_N, uint64_t seed) {
    if (lines.empty()) return 0;
    const PencilModel model = normalised_model(lines);
    const float tol = cos_threshold(inlier_deg);
    return peel_models(model, lines, max_models, inlier_deg, garbage_deg, [&](const std::vector<int>& obs, int k, Vec3* h) {
        return ctx_prosac_solve(c, model, obs, tol, T_N, seed, (uint32_t)k, h, nullptr);
    }, nothing_taken);
}

// DirectEstimator (estimator.h:82-96; compiled by the reference, never instantiated): the lines whose Hough weight
// (GPU: ctx_ht_weights) exceeds 0.95 decide the refit; an empty set means every line (line_pencil.cpp:114-117).
int ctx_direct_solve(lr_context* c, const PencilModel& model, const std::vector<int>& indices, Vec3* h) {
    std::vector<float> weights;
    if (ctx_ht_weights(c, model, indices, weights)) return 1;
    std::vector<int> inl;
    for (size_t j = 0; j < indices.size(); ++j)
        if (weights[j] > 0.95f) inl.push_back(indices[j]);
    *h = model.fit_optimal(inl);
    return 0;
}

int ctx_estimate_line_pencils_direct(lr_context* c, std::vector<LineSegment>& lines, int max_models, float inlier_deg,
                                     float garbage_deg) {
    if (lines.empty()) return 0;
    const PencilModel model = normalised_model(lines);
    return peel_models(model, lines, max_models, inlier_deg, garbage_deg, [&](const std::vector<int>& obs, int, Vec3* h) {
        return ctx_direct_solve(c, model, obs, h);
    }, nothing_taken);
}

namespace {

// every line of the model on the device, and an accumulator of d x d cells kept in the context (no allocation on the path of a call)
int cht_setup(lr_context* c, const PencilModel& model, int d, PencilSoA* soa) {
    std::vector<int> all(model.size());
    for (int i = 0; i < model.size(); ++i) all[i] = i;
    if (upload_model(c, model, all, soa)) return 1;
    const size_t cells = (size_t)d * d;
    if (cells > c->d_cht_acc.cap()) {
        LR_HIP(hipStreamSynchronize(c->stream));
        if (c->d_cht_acc.grow(cells)) return 1;
    }
    return 0;
}

// the point (in the model's normalised coordinates) that accumulator cell `cell` of a d x d diamond space stands for
Vec3 diamond_cell_point(size_t cell, int d) {
    const int iy = (int)(cell / (size_t)d), ix = (int)(cell % (size_t)d);
    const float u = (float)ix / (float)(d - 1) * 2.f - 1.f, v = (float)iy / (float)(d - 1) * 2.f - 1.f;
    return Vec3{v, (u >= 0.f ? 1.f : -1.f) * u + (v >= 0.f ? 1.f : -1.f) * v - 1.f, u};
}

}  // namespace

// Diamond-space accumulator (opt-in; cht.h:13-24): de-normalised vanishing point of the strongest pencil.
int ctx_cht_vanishing_point(lr_context* c, const std::vector<LineSegment>& lines, int d, Vec3* vp,
                            std::vector<uint64_t>* acc_out) {
    LR_HIP(hipSetDevice(c->device));
    const Normalisation nrm = bbox_normalisation(lines);
    const PencilModel model(normalise(lines, nrm));
    PencilSoA soa;
    if (cht_setup(c, model, d, &soa)) return 1;
    if (launch_cht_accumulate(soa, (uint32_t)model.size(), d, c->d_cht_acc, c->stream)) return 1;
    std::vector<uint64_t> acc((size_t)d * d);
    LR_HIP(hipMemcpyAsync(acc.data(), c->d_cht_acc, acc.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    LR_HIP(hipStreamSynchronize(c->stream));
    size_t best = 0;
    for (size_t i = 1; i < acc.size(); ++i)
        if (acc[i] > acc[best]) best = i;
    Vec3 p = diamond_cell_point(best, d);
    if (std::fabs(p.z) < kEps) {
        p.z = 0.f;
    } else {
        p = {p.x / p.z, p.y / p.z, 1.f};
        p.x = nrm.scale * p.x + nrm.center.x;
        p.y = nrm.scale * p.y + nrm.center.y;
    }
    *vp = p;
    if (acc_out) acc_out->swap(acc);
    return 0;
}

// The diamond-space accumulator as an ESTIMATOR of the path (opt-in, lr_set_estimator(3, d); cht.h:13-24 describes
// accumulate -> argmax -> de-normalise, "the weights can be negative (so lines can be removed!)"): the peeling loop of
// estimate_multiple_structures (estimator.h:99-145) around a solve() that reads
//     hypothesis = point of the accumulator's strongest cell (first maximum in row-major order)
//     inliers    = remaining lines whose inclination error against it is below tol   (as estimator.h:74)
//     model      = fit_optimal(inliers)                                              (as estimator.h:75-76)
// The votes of every line go into the accumulator once; after a round the lines it has grouped or discarded are taken
// back out of it with negative votes (exact: the votes are integers), instead of accumulating the rest again -- the
// oracle re-accumulates, so the two check each other.  Accumulation and argmax run on the GPU, one 12-byte peak comes
// back per round; the O(n) verdicts stay on the host like PROSAC's and Direct's.  Parity unpinned: the reference's
// cht.cpp does not compile.
int ctx_estimate_line_pencils_cht(lr_context* c, std::vector<LineSegment>& lines, int max_models, float inlier_deg,
                                  float garbage_deg, int d, ChtTrace* trace) {
    if (lines.empty()) return 0;
    LR_HIP(hipSetDevice(c->device));
    if (d <= 0) d = 128;
    const PencilModel model = normalised_model(lines);
    const float tol = cos_threshold(inlier_deg);
    const int N = model.size();
    PencilSoA soa;
    if (cht_setup(c, model, d, &soa)) return 1;
    if ((size_t)N > c->cht_idx.cap()) {
        LR_HIP(hipStreamSynchronize(c->stream));
        if (c->cht_idx.grow(std::max<size_t>((size_t)N, 4096))) return 1;
    }
    if (!c->cht_peak.cap() && c->cht_peak.grow(8)) return 1;
    uint32_t* const peak = c->cht_peak.h;
    unsigned long long* d_votes = reinterpret_cast<unsigned long long*>(c->cht_peak.d + 4);
    LR_HIP(hipMemsetAsync(c->cht_peak.d, 0, 8 * sizeof(uint32_t), c->stream));
    LR_HIP(hipMemsetAsync(c->d_cht_acc, 0, (size_t)d * d * sizeof(unsigned long long), c->stream));
    if (launch_cht_votes(soa, nullptr, (uint32_t)N, d, c->d_cht_acc, false, d_votes, c->stream)) return 1;
    auto solve = [&](const std::vector<int>& obs, int, Vec3* h) -> int {
        if (launch_cht_peak(c->d_cht_acc, d, c->cht_peak.d, c->stream)) return 1;
        LR_HIP(hipMemcpyAsync(peak, c->cht_peak.d, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        LR_HIP(hipStreamSynchronize(c->stream));
        const Vec3 p = diamond_cell_point(peak[0], d);
        std::vector<int> inl;
        for (int i : obs)
            if (model.error(p, i) < tol) inl.push_back(i);
        *h = model.fit_optimal(inl);
        if (trace) {
            trace->models.push_back(*h);
            trace->peak_cell.push_back(peak[0]);
        }
        return 0;
    };
    auto taken = [&](const std::vector<int>& out, bool more) -> int {  // the next round votes without them
        if (!more || out.empty()) return 0;
        std::copy(out.begin(), out.end(), c->cht_idx.h.get());
        LR_HIP(hipMemcpyAsync(c->cht_idx.d, c->cht_idx.h, out.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        return launch_cht_votes(soa, c->cht_idx.d, (uint32_t)out.size(), d, c->d_cht_acc, true, d_votes, c->stream);
    };
    if (peel_models(model, lines, max_models, inlier_deg, garbage_deg, solve, taken)) return 1;
    if (trace) {
        LR_HIP(hipMemcpyAsync(peak, c->cht_peak.d, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        LR_HIP(hipStreamSynchronize(c->stream));
        trace->votes = ((uint64_t)peak[5] << 32) | peak[4];
    }
    return 0;
}

// postprocess_lines_segments (line_detector.cpp:332-444): pair test on the GPU for large n, graph walk and
// merges on the host.
int ctx_refine(lr_context* c, std::vector<LineSegment>& lines) {
    const size_t n = lines.size();
    if (n < 2048) {
        lines = refine_lines(lines);
        return 0;
    }
    LR_HIP(hipSetDevice(c->device));
    std::vector<float> table;
    refine_segment_table(lines, table);
    // segment table and edge list live in the context and grow on demand (no allocation on the path of a call)
    if (table.size() > c->d_refine_table.cap()) {
        LR_HIP(hipStreamSynchronize(c->stream));
        if (c->d_refine_table.grow(table.size())) return 1;
    }
    size_t cap = std::max<size_t>(16 * n, c->d_refine_edges.cap());
    std::vector<std::pair<uint32_t, uint32_t>> edges;
    static_assert(sizeof(std::pair<uint32_t, uint32_t>) == sizeof(uint2), "edge layout");
    LR_HIP(hipMemcpyAsync(c->d_refine_table, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    for (;;) {
        if (cap > c->d_refine_edges.cap()) {
            LR_HIP(hipStreamSynchronize(c->stream));
            if (c->d_refine_edges.grow(cap)) return 1;
        }
        LR_HIP(hipMemsetAsync(c->d_counts + 8, 0, sizeof(uint32_t), c->stream));
        if (launch_refine_pairs(c->d_refine_table, (uint32_t)n, c->d_refine_edges, c->d_counts + 8,
                                (uint32_t)std::min<size_t>(c->d_refine_edges.cap(), 0xFFFFFFFFu), c->stream))
            return 1;
        LR_HIP(hipMemcpyAsync(c->h_counts + 8, c->d_counts + 8, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        LR_HIP(hipStreamSynchronize(c->stream));
        const size_t ne = c->h_counts[8];
        if (ne <= c->d_refine_edges.cap()) {
            edges.resize(ne);
            if (ne) {
                LR_HIP(hipMemcpyAsync(edges.data(), c->d_refine_edges, ne * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
                LR_HIP(hipStreamSynchronize(c->stream));
            }
            break;
        }
        cap = ne;  // the kernel counted every edge: exactly enough next time
    }
    lines = refine_lines_from_edges(lines, edges);
    return 0;
}

}  // namespace lramd
