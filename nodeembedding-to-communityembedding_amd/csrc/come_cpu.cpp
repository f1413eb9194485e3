// come_cpu.cpp -- the CPU twins of the hot-path entry points ("a CPU twin of each
// entry point, come_cpu_*(..., int threads)"), plain host C++ in libcome.so.
//
// They are separate entry points on host memory, for callers without a GPU and as the product's
// own CPU path; no GPU entry point ever calls them (there is no fallback: a GPU call without a
// usable device fails with COME_E_HIP).  Semantics follow the reference's CPU path:
//   come_cpu_sgns_o2 / _o1   train_o2 / train_o1 (utils/training_sdg_inner.pyx:407-509) driven by
//                            `threads` worker threads that take jobs of kJobItems walks (edges)
//                            and update the shared tables without locks, as Context2Vec /
//                            Node2Vec's workers do (ADSCModel/context_embeddings.py:72-102,
//                            node_embeddings.py:58-95).  COME_MODE_SEQUENTIAL (= workers=1)
//                            runs the walks in order on the calling thread.  The dot product is
//                            in the GPU kernels' WAVE64 order (lane l sums elements l, l+64, ...
//                            by an fma chain, then an xor butterfly over the 64 lanes), so the
//                            sequential mode equals come_sgns_o2's sequential mode bit for bit.
//   come_cpu_community_grad  Community2Vec.train (community_embeddings.py:61-78) in the
//                            arithmetic order of the VALU kernel k_community_grad, rows split
//                            over the threads (each row's update reads only its own row).
//   come_cpu_gmm_resp/_estep GaussianMixture.predict_proba (community_embeddings.py:37) and the
//                            E-step's per-row log-sum-exp, rows split over the threads.
//   come_cpu_community_loss  the community objective (what community_embeddings.py:40-59 means),
//                            float64 arithmetic, one partial sum per thread's block of rows.
//   come_cpu_sgns_o2_loss / _pairs_loss  the SGNS objectives as come_sgns_o2_loss /
//                            come_sgns_pairs_loss define them: the trainer's fp32 WAVE64 dot, a
//                            float64 softplus on it, terms added in k order, pairs in the
//                            trainer's order; one partial sum per thread's block of walks (pairs).
//   come_cpu_random_walks_pq the node2vec (p, q) walker: come_walk_pq.h's step body, which the
//                            kernel k_random_walks_pq compiles too, so the walks are the device's
//                            bit for bit; walks split over the threads.
//   come_cpu_walk_cdf / come_cpu_random_walks_w  edge-weighted walks: the same header's CDF
//                            arithmetic and pq_step<true>, as k_walk_cdf / k_random_walks_w.
//   come_cpu_edge_cdf / come_cpu_edge_sample / come_cpu_edge_pick  edge sampling by weight for
//                            O1: come_edge_sample.h's CDF and draw, as k_edge_cdf / k_edge_sample.
// Each compute body is built twice, for AVX2+FMA and for the baseline ISA (explicit fmaf either
// way, -ffp-contract=off: identical results), and the first call picks one from the CPU.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <immintrin.h>

#include <atomic>
#include <cmath>
#include <thread>
#include <vector>

#include "../../include/come.h"
#include "come_edge_sample.h"
#include "come_walk_pq.h"

namespace come {
int set_error(int code, const char *fmt, ...);
}
using come::set_error;

namespace {

constexpr int kExpTableSize = 1000;
constexpr int kMaxSentenceLen = 10000;  // pyx:18,480
constexpr int kMaxNegative = 20, kMaxDim = 512, kMaxThreads = 1024;
constexpr uint64_t kLcgMul = 25214903917ULL, kLcgAdd = 11ULL, kLcgMask = (1ULL << 48) - 1;
constexpr int64_t kJobItems = 150;  // the reference trainers' default chunksize

const float *exp_table() {
    static const struct T {
        float v[kExpTableSize];
        T() { come_exp_table(v); }  // pyx:531-533: the library's one definition
    } t;
    return t.v;
}

bool have_fma() {
    static const bool f = [] {
        __builtin_cpu_init();
        return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    }();
    return f;
}

#define COME_FMA_CLONE __attribute__((target("avx2,fma")))
#define HOT inline __attribute__((always_inline))

// The GPU kernels' dot-product order (come_wave.h; oracle/come_oracle.c COME_DOT_WAVE64).
HOT float dot_wave64(const float *a, const float *b, int d) {
    float lane[64];
    for (int l = 0; l < 64; ++l) lane[l] = 0.0f;
    for (int v = 0; v < d; v += 64) {
        const int n = d - v < 64 ? d - v : 64;
        for (int l = 0; l < n; ++l) lane[l] = fmaf(a[v + l], b[v + l], lane[l]);
    }
    for (int off = 1; off <= 32; off <<= 1) {
        float t[64];
        for (int l = 0; l < 64; ++l) t[l] = lane[l] + lane[l ^ off];
        memcpy(lane, t, sizeof(t));
    }
    return lane[0];
}

// The same value with AVX2: eight 8-lane accumulators hold the 64 lanes (fma chains over d in
// steps of 64, as above), then the butterfly's reduction tree.  The xor butterfly's lane 0 is the
// pairwise tree over lanes 0..63 in index order (stage `off` adds the neighbouring groups of size
// off) and float addition is commutative, so any evaluation of that tree is bit-identical:
// hadd(A, B) forms the off=1 pairs of two accumulators, a second hadd the off=2 pairs, adding the
// 128-bit halves the off=4 groups (one sum per accumulator), and the last three stages pair the
// eight sums (0,1) (2,3) (4,5) (6,7), then (01,23) (45,67), then the two halves.
// (Out of line: an always_inline target("avx2,fma") function cannot be inlined into the generic
// template chain; the call costs nothing beside d = 128 of work.)
__attribute__((target("avx2,fma"))) float dot_wave64_avx2(
    const float *a, const float *b, int d) {
    __m256 acc[8];
    for (int j = 0; j < 8; ++j) acc[j] = _mm256_setzero_ps();
    for (int v = 0; v < d; v += 64)
        for (int j = 0; j < 8; ++j)
            acc[j] = _mm256_fmadd_ps(_mm256_loadu_ps(a + v + 8 * j),
                                     _mm256_loadu_ps(b + v + 8 * j), acc[j]);
    const __m256 h0 = _mm256_hadd_ps(_mm256_hadd_ps(acc[0], acc[1]),
                                     _mm256_hadd_ps(acc[2], acc[3]));
    const __m256 h1 = _mm256_hadd_ps(_mm256_hadd_ps(acc[4], acc[5]),
                                     _mm256_hadd_ps(acc[6], acc[7]));
    // s0 = [S0 S1 S2 S3], s1 = [S4 S5 S6 S7]: the per-accumulator sums (stage off=4)
    const __m128 s0 = _mm_add_ps(_mm256_castps256_ps128(h0), _mm256_extractf128_ps(h0, 1));
    const __m128 s1 = _mm_add_ps(_mm256_castps256_ps128(h1), _mm256_extractf128_ps(h1, 1));
    const __m128 p = _mm_hadd_ps(s0, s1);  // [S0+S1, S2+S3, S4+S5, S6+S7]   (off=8)
    const __m128 q = _mm_hadd_ps(p, p);    // [S0..3, S4..7, ...]             (off=16)
    return _mm_cvtss_f32(_mm_add_ss(q, _mm_movehdup_ps(q)));  //              (off=32)
}

struct Sgns {
    float *in_tab, *out_tab;  // O1: the same table (pyx:444)
    int64_t V;
    int d, negative, window, L;
    const int32_t *items;     // walks [P x L] or edges [E x 2]
    const uint64_t *seeds;
    const uint32_t *table;
    uint64_t T;
    float lr, alpha;
};

// Rows not yet in cache are the cost at the benchmarked sizes (a 1M x 128 table is 512 MB, a 1e8
// table 400 MB): every row a pair touches is prefetched before the first is read.
HOT void prefetch_row(const float *row, int d) {
    for (int i = 0; i < d; i += 16) __builtin_prefetch(row + i, 1, 3);
}

// One pair (pyx:105-151 for O2, pyx:205-249 for O1: no alpha, output rows not written).  The
// negative draws depend only on nr (pyx:133-134), so they are taken first -- the table reads and
// the target rows then overlap instead of queueing behind each dot product; the update sequence
// itself is unchanged.
template <bool O2, bool Simd>
HOT uint64_t pair_update(const Sgns &a, uint32_t word_index, uint32_t word2_index, uint64_t nr,
                         float *work, const float *expt) {
    float *in = a.in_tab + (int64_t)word2_index * a.d;
    uint32_t target[kMaxNegative + 1];
    target[0] = word_index;
    for (int k = 1; k <= a.negative; ++k) {
        target[k] = a.table[(nr >> 16) % a.T];
        nr = (nr * kLcgMul + kLcgAdd) & kLcgMask;  // pyx:134
    }
    prefetch_row(in, a.d);
    for (int k = 0; k <= a.negative; ++k)
        if ((int64_t)target[k] < a.V) prefetch_row(a.out_tab + (int64_t)target[k] * a.d, a.d);
    for (int i = 0; i < a.d; ++i) work[i] = 0.0f;
    for (int k = 0; k <= a.negative; ++k) {
        float label = 1.0f;
        if (k > 0) {
            if (target[k] == word_index) continue;     // pyx:135: the draw is consumed
            if ((int64_t)target[k] >= a.V) continue;   // a table value outside [0, V): skipped
            label = 0.0f;
        }
        float *out = a.out_tab + (int64_t)target[k] * a.d;
        float f;
        if constexpr (Simd)
            f = (a.d & 63) == 0 ? dot_wave64_avx2(in, out, a.d) : dot_wave64(in, out, a.d);
        else
            f = dot_wave64(in, out, a.d);
        if (f <= -6.0f || f >= 6.0f) continue;         // pyx:141: skip, not clamp
        const float s = expt[(int)(((double)f + 6.0) * 83.0)];
        const float g = O2 ? ((label - s) * a.lr) * a.alpha : (label - s) * a.lr;
        for (int i = 0; i < a.d; ++i) work[i] = fmaf(g, out[i], work[i]);    // pyx:146
        if (O2)
            for (int i = 0; i < a.d; ++i) out[i] = fmaf(g, in[i], out[i]);   // pyx:147
    }
    for (int i = 0; i < a.d; ++i) in[i] = in[i] + work[i];                  // pyx:149
    return nr;
}

// train_o2 on walk p (pyx:479-508): fixed window, j ascending, j != i; entries outside [0, V) are
// None (pyx:435-436).  Returns its pair updates.
template <bool Simd>
HOT int64_t walk_o2(const Sgns &a, int64_t p, float *work, const float *expt) {
    const int32_t *idx = a.items + p * (int64_t)a.L;
    const int n = a.L < kMaxSentenceLen ? a.L : kMaxSentenceLen;
    auto ok = [&](int j) { return idx[j] >= 0 && (int64_t)idx[j] < a.V; };
    uint64_t nr = a.seeds[p];
    int64_t pairs = 0;
    for (int i = 0; i < n; ++i) {
        if (!ok(i)) continue;
        const int j0 = i - a.window < 0 ? 0 : i - a.window;
        const int j1 = i + a.window + 1 > n ? n : i + a.window + 1;
        for (int j = j0; j < j1; ++j) {
            if (j == i || !ok(j)) continue;
            nr = pair_update<true, Simd>(a, (uint32_t)idx[i], (uint32_t)idx[j], nr, work, expt);
            ++pairs;
        }
    }
    return pairs;
}

// train_o1 on edge e (pyx:425-450): (input u, positive v) then (input v, positive u), the RNG
// state carried across both.  An edge with an endpoint outside [0, V) is skipped.
template <bool Simd>
HOT int64_t edge_o1(const Sgns &a, int64_t e, float *work, const float *expt) {
    const int32_t u = a.items[2 * e], v = a.items[2 * e + 1];
    if (u < 0 || v < 0 || (int64_t)u >= a.V || (int64_t)v >= a.V) return 0;
    uint64_t nr = a.seeds[e];
    nr = pair_update<false, Simd>(a, (uint32_t)v, (uint32_t)u, nr, work, expt);
    pair_update<false, Simd>(a, (uint32_t)u, (uint32_t)v, nr, work, expt);
    return 2;
}

template <bool O2, bool Simd>
HOT int64_t run_items(const Sgns &a, int64_t lo, int64_t hi, float *work) {
    const float *expt = exp_table();
    int64_t pairs = 0;
    for (int64_t i = lo; i < hi; ++i)
        pairs += O2 ? walk_o2<Simd>(a, i, work, expt) : edge_o1<Simd>(a, i, work, expt);
    return pairs;
}
template <bool O2>
COME_FMA_CLONE int64_t run_items_fma(const Sgns &a, int64_t lo, int64_t hi, float *work) {
    return run_items<O2, true>(a, lo, hi, work);
}
template <bool O2>
int64_t run_items_base(const Sgns &a, int64_t lo, int64_t hi, float *work) {
    return run_items<O2, false>(a, lo, hi, work);
}

// `threads` workers claim jobs of kJobItems consecutive items from a shared counter and race on
// the tables as the reference's Hogwild threads do; sequential = the calling thread, in order.
template <bool O2>
int64_t drive(const Sgns &a, int64_t n_items, bool sequential, int threads) {
    auto body = have_fma() ? run_items_fma<O2> : run_items_base<O2>;
    if (sequential || threads <= 1 || n_items <= kJobItems) {
        std::vector<float> work(a.d);
        return body(a, 0, n_items, work.data());
    }
    std::atomic<int64_t> next(0), total(0);
    auto worker = [&] {
        std::vector<float> work(a.d);
        int64_t mine = 0;
        for (;;) {
            const int64_t lo = next.fetch_add(kJobItems);
            if (lo >= n_items) break;
            mine += body(a, lo, lo + kJobItems < n_items ? lo + kJobItems : n_items, work.data());
        }
        total += mine;
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back(worker);
    for (auto &t : pool) t.join();
    return total.load();
}

// Rows [0, V) split into `threads` contiguous blocks, fn(lo, hi) on each.
template <class F>
void parallel_rows(int64_t V, int threads, F fn) {
    if (threads <= 1 || V < 64) {
        fn((int64_t)0, V);
        return;
    }
    std::vector<std::thread> pool;
    const int64_t per = (V + threads - 1) / threads;
    for (int t = 0; t < threads; ++t) {
        const int64_t lo = t * per, hi = lo + per < V ? lo + per : V;
        if (lo < hi) pool.emplace_back(fn, lo, hi);
    }
    for (auto &t : pool) t.join();
}

struct Comm {
    float *x;
    const float *pi, *mu, *inv_cov;
    int64_t V;
    int d, K, iters;
    float coef, lr;
};

// k_community_grad's arithmetic per row: G[c] = fma(pi_k, sum_j (x - mu_k)[j] M_k[c][j], G[c])
// over k (the inner sum an fma chain in j), g = clip(G * coef, -5, 5), x = x - g * lr.
HOT void community_rows(const Comm &a, int64_t lo, int64_t hi) {
    std::vector<float> dx(a.d), G(a.d);
    for (int64_t r = lo; r < hi; ++r) {
        float *x = a.x + r * a.d;
        for (int it = 0; it < a.iters; ++it) {
            for (int c = 0; c < a.d; ++c) G[c] = 0.0f;
            for (int k = 0; k < a.K; ++k) {
                const float *M = a.inv_cov + (int64_t)k * a.d * a.d;
                for (int j = 0; j < a.d; ++j) dx[j] = x[j] - a.mu[(int64_t)k * a.d + j];
                const float p = a.pi[r * a.K + k];
                for (int c = 0; c < a.d; ++c) {
                    float acc = 0.0f;
                    for (int j = 0; j < a.d; ++j) acc = fmaf(dx[j], M[(int64_t)c * a.d + j], acc);
                    G[c] = fmaf(p, acc, G[c]);
                }
            }
            for (int c = 0; c < a.d; ++c) {
                float g = G[c] * a.coef;
                g = g < -5.0f ? -5.0f : (g > 5.0f ? 5.0f : g);  // clip(min=-5, max=5), :79
                x[c] = x[c] - g * a.lr;
            }
        }
    }
}
COME_FMA_CLONE void community_rows_fma(const Comm &a, int64_t lo, int64_t hi) {
    community_rows(a, lo, hi);
}
void community_rows_base(const Comm &a, int64_t lo, int64_t hi) { community_rows(a, lo, hi); }

struct Resp {
    const float *x, *prec_chol, *mu_prec, *log_norm;
    float *resp, *lse;
    int64_t V;
    int d, K;
};

// Per row: y_c = sum_j x_j P_k[j][c] - (mu_k P_k)_c, lp_k = log_norm_k - 0.5 sum_c y_c^2, then
// resp = exp(lp - logsumexp(lp)) (sklearn _estimate_weighted_log_prob + _estimate_log_prob_resp).
HOT void resp_rows(const Resp &a, int64_t lo, int64_t hi) {
    std::vector<float> lp(a.K);
    for (int64_t r = lo; r < hi; ++r) {
        const float *x = a.x + r * a.d;
        float m = -INFINITY;
        for (int k = 0; k < a.K; ++k) {
            const float *P = a.prec_chol + (int64_t)k * a.d * a.d;
            float sq = 0.0f;
            for (int c = 0; c < a.d; ++c) {
                float y = 0.0f;
                for (int j = 0; j < a.d; ++j) y = fmaf(x[j], P[(int64_t)j * a.d + c], y);
                y = y - a.mu_prec[(int64_t)k * a.d + c];
                sq = fmaf(y, y, sq);
            }
            lp[k] = a.log_norm[k] - 0.5f * sq;
            m = fmaxf(m, lp[k]);
        }
        float s = 0.0f;
        for (int k = 0; k < a.K; ++k) s += expf(lp[k] - m);
        const float lse = m + logf(s);
        for (int k = 0; k < a.K; ++k) a.resp[r * a.K + k] = expf(lp[k] - lse);
        if (a.lse) a.lse[r] = lse;
    }
}
COME_FMA_CLONE void resp_rows_fma(const Resp &a, int64_t lo, int64_t hi) { resp_rows(a, lo, hi); }
void resp_rows_base(const Resp &a, int64_t lo, int64_t hi) { resp_rows(a, lo, hi); }

struct Loss {
    const float *x, *pi, *prec_chol, *mu_prec, *log_norm;
    float *row_out;
    int64_t V;
    int d, K;
};

// come_community_loss in float64: y_c = sum_{j <= c} x_j P_k[j][c] - (mu_k P_k)_c (the factors are
// upper-triangular by the entry's contract), row = sum_k pi_k (log_norm_k - 0.5 sum_c y_c^2);
// returns the sum of the rows lo .. hi - 1 in row order.
double loss_rows(const Loss &a, int64_t lo, int64_t hi) {
    double total = 0.0;
    for (int64_t r = lo; r < hi; ++r) {
        const float *x = a.x + r * a.d;
        double row = 0.0;
        for (int k = 0; k < a.K; ++k) {
            const float *P = a.prec_chol + (int64_t)k * a.d * a.d;
            double sq = 0.0;
            for (int c = 0; c < a.d; ++c) {
                double y = 0.0;
                for (int j = 0; j <= c; ++j) y += (double)x[j] * (double)P[(int64_t)j * a.d + c];
                y -= (double)a.mu_prec[(int64_t)k * a.d + c];
                sq += y * y;
            }
            row += (double)a.pi[r * a.K + k] * ((double)a.log_norm[k] - 0.5 * sq);
        }
        if (a.row_out) a.row_out[r] = (float)row;
        total += row;
    }
    return total;
}

int check_threads(int threads) {
    if (threads < 1 || threads > kMaxThreads)
        return set_error(COME_E_INVALID, "threads must be in [1, %d]", kMaxThreads);
    return COME_OK;
}

int check_sgns(int64_t V, int d, int negative, const uint32_t *table, uint64_t T, int mode,
               int threads) {
    if (V < 0 || d < 1 || d > kMaxDim || negative < 0 || negative > kMaxNegative)
        return set_error(COME_E_INVALID, "need V>=0, 1<=d<=%d, 0<=negative<=%d", kMaxDim,
                         kMaxNegative);
    if (negative > 0 && (!table || T == 0))
        return set_error(COME_E_INVALID, "negative sampling needs a table with T >= 1");
    if (mode & COME_TABLE_PACKED)
        return set_error(COME_E_INVALID, "CPU twins take the uint32 table (not the packed form)");
    if ((mode & 0xFF) != COME_MODE_HOGWILD && (mode & 0xFF) != COME_MODE_SEQUENTIAL)
        return set_error(COME_E_INVALID, "mode must be COME_MODE_HOGWILD or COME_MODE_SEQUENTIAL");
    return check_threads(threads);
}

// ---- the SGNS objectives as losses (come_sgns_loss.hip's arithmetic and summation order) ----
struct SgnsLoss {
    const float *in_tab, *out_tab;
    int64_t V;
    int d, negative, window, L;
    const int32_t *walks;      // O2: [P x L]
    const uint64_t *seeds;     // O2: [P]
    const uint32_t *table;     // O2
    uint64_t T;
    const int32_t *rows_in, *rows_pos, *rows_neg;  // explicit pairs
    double *unit_out;          // per walk / per pair, or null
};

HOT double softplus64(double z) { return std::fmax(z, 0.0) + std::log1p(std::exp(-std::fabs(z))); }

// softplus(-f(in, pos)) + sum_k softplus(f(in, t_k)) added in k order from the positive; a target
// equal to `skip` or outside [0, V) adds nothing.
template <bool Simd>
HOT double pair_loss(const SgnsLoss &a, int64_t ri, int64_t rp, const uint32_t *target, int64_t skip) {
    const float *in = a.in_tab + ri * a.d;
    auto dot = [&](const float *o) {
        if constexpr (Simd) return (a.d & 63) == 0 ? dot_wave64_avx2(in, o, a.d) : dot_wave64(in, o, a.d);
        else return dot_wave64(in, o, a.d);
    };
    double s = 0.0;
    s += softplus64(-(double)dot(a.out_tab + rp * a.d));
    for (int k = 0; k < a.negative; ++k) {
        const int64_t t = (int64_t)target[k];
        if (t == skip || t >= a.V) continue;
        s += softplus64((double)dot(a.out_tab + t * a.d));
    }
    return s;
}

// train_o2's enumeration and draws on walk p (walk_o2 above), nothing written: the walk's value.
template <bool Simd>
HOT double walk_loss(const SgnsLoss &a, int64_t p, int64_t *pairs) {
    const int32_t *idx = a.walks + p * (int64_t)a.L;
    const int n = a.L < kMaxSentenceLen ? a.L : kMaxSentenceLen;
    auto ok = [&](int j) { return idx[j] >= 0 && (int64_t)idx[j] < a.V; };
    uint64_t nr = a.seeds[p];
    uint32_t target[kMaxNegative];
    double total = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!ok(i)) continue;
        const int j0 = i - a.window < 0 ? 0 : i - a.window;
        const int j1 = (int64_t)i + a.window + 1 > n ? n : i + a.window + 1;
        for (int j = j0; j < j1; ++j) {
            if (j == i || !ok(j)) continue;
            for (int k = 0; k < a.negative; ++k) {
                target[k] = a.table[(nr >> 16) % a.T];
                nr = (nr * kLcgMul + kLcgAdd) & kLcgMask;  // pyx:134: every draw advances
            }
            total += pair_loss<Simd>(a, idx[j], idx[i], target, idx[i]);
            ++*pairs;
        }
    }
    return total;
}

// units lo .. hi - 1 (walks, or explicit pairs when a.walks is null), added in index order
template <bool Simd>
HOT double loss_units(const SgnsLoss &a, int64_t lo, int64_t hi, int64_t *pairs) {
    double total = 0.0;
    for (int64_t u = lo; u < hi; ++u) {
        double v = 0.0;
        if (a.walks || a.seeds) {
            v = walk_loss<Simd>(a, u, pairs);
        } else {
            const int64_t ri = a.rows_in[u], rp = a.rows_pos[u];
            if (ri >= 0 && ri < a.V && rp >= 0 && rp < a.V) {
                v = pair_loss<Simd>(a, ri, rp, reinterpret_cast<const uint32_t *>(a.rows_neg) +
                                                   u * (int64_t)a.negative, -1);
                ++*pairs;
            }
        }
        if (a.unit_out) a.unit_out[u] = v;
        total += v;
    }
    return total;
}
COME_FMA_CLONE double loss_units_fma(const SgnsLoss &a, int64_t lo, int64_t hi, int64_t *pairs) {
    return loss_units<true>(a, lo, hi, pairs);
}
double loss_units_base(const SgnsLoss &a, int64_t lo, int64_t hi, int64_t *pairs) {
    return loss_units<false>(a, lo, hi, pairs);
}

// one partial per block of units (parallel_rows' split), added in block order
void loss_drive(const SgnsLoss &a, int64_t units, int threads, double *loss_out,
                int64_t *pairs_out) {
    auto fn = have_fma() ? loss_units_fma : loss_units_base;
    const int64_t per = threads <= 1 || units < 64 ? units : (units + threads - 1) / threads;
    const size_t blocks = (size_t)((units + per - 1) / per);
    std::vector<double> part(blocks, 0.0);
    std::vector<int64_t> cnt(blocks, 0);
    parallel_rows(units, threads, [&](int64_t lo, int64_t hi) {
        part[lo / per] = fn(a, lo, hi, &cnt[lo / per]);
    });
    double total = 0.0;
    int64_t pairs = 0;
    for (size_t b = 0; b < blocks; ++b) {
        total += part[b];
        pairs += cnt[b];
    }
    *loss_out = total;
    if (pairs_out) *pairs_out = pairs;
}

// come_sgns_o2_loss's messages (the GPU entry validates the same way)
int check_loss_tables(const char *who, int64_t V, int d, int negative) {
    if (V <= 0) return set_error(COME_E_INVALID, "%s: V must be > 0 (got %lld)", who, (long long)V);
    if (V > INT32_MAX)
        return set_error(COME_E_INVALID, "%s: V must fit int32 row indices (got %lld)", who,
                         (long long)V);
    if (d < 1 || d > kMaxDim)
        return set_error(COME_E_INVALID, "%s: d must be in [1, %d] (got %d)", who, kMaxDim, d);
    if (negative < 0 || negative > kMaxNegative)
        return set_error(COME_E_INVALID, "%s: negative must be in [0, %d] (got %d)", who,
                         kMaxNegative, negative);
    return COME_OK;
}

}  // namespace

extern "C" int come_cpu_sgns_o2(float *node, float *ctx, int64_t V, int d, const int32_t *walks,
                                int64_t P, int L, const uint64_t *seeds, int window, int negative,
                                const uint32_t *table, uint64_t T, float lr, float alpha, int mode,
                                int threads, int64_t *pairs_out) {
    int rc = check_sgns(V, d, negative, table, T, mode, threads);
    if (rc) return rc;
    if (P < 0 || L < 0 || window < 0) return set_error(COME_E_INVALID, "need P, L, window >= 0");
    if (pairs_out) *pairs_out = 0;
    if (P == 0 || L == 0 || V == 0) return COME_OK;
    if (!node || !ctx || !walks || !seeds) return set_error(COME_E_INVALID, "null pointer");
    const Sgns a{node, ctx, V, d, negative, window, L, walks, seeds, table, T, lr, alpha};
    const int64_t pairs =
        drive<true>(a, P, (mode & 0xFF) == COME_MODE_SEQUENTIAL, threads);
    if (pairs_out) *pairs_out = pairs;
    return COME_OK;
}

extern "C" int come_cpu_sgns_o1(float *node, int64_t V, int d, const int32_t *edges, int64_t E,
                                const uint64_t *seeds, int negative, const uint32_t *table,
                                uint64_t T, float lr, int mode, int threads, int64_t *pairs_out) {
    int rc = check_sgns(V, d, negative, table, T, mode, threads);
    if (rc) return rc;
    if (E < 0) return set_error(COME_E_INVALID, "need E >= 0");
    if (pairs_out) *pairs_out = 0;
    if (E == 0 || V == 0) return COME_OK;
    if (!node || !edges || !seeds) return set_error(COME_E_INVALID, "null pointer");
    const Sgns a{node, node, V, d, negative, 0, 2, edges, seeds, table, T, lr, 0.0f};
    const int64_t pairs =
        drive<false>(a, E, (mode & 0xFF) == COME_MODE_SEQUENTIAL, threads);
    if (pairs_out) *pairs_out = pairs;
    return COME_OK;
}

extern "C" int come_cpu_community_grad(float *x, int64_t V, int d, const float *pi,
                                       const float *mu, const float *inv_cov, int K, float beta,
                                       float lr, int iters, int threads) {
    if (V < 0 || d < 1 || d > kMaxDim || K < 1 || iters < 0)
        return set_error(COME_E_INVALID, "need V>=0, 1<=d<=%d, K>=1, iters>=0", kMaxDim);
    int rc = check_threads(threads);
    if (rc) return rc;
    if (V == 0 || iters == 0) return COME_OK;
    if (!x || !pi || !mu || !inv_cov) return set_error(COME_E_INVALID, "null pointer");
    // (float)(beta / K): community_embeddings.py:77 (numpy casts the Python float to fp32)
    const Comm a{x, pi, mu, inv_cov, V, d, K, iters, (float)((double)beta / K), lr};
    auto fn = have_fma() ? community_rows_fma : community_rows_base;
    parallel_rows(V, threads, [&](int64_t lo, int64_t hi) { fn(a, lo, hi); });
    return COME_OK;
}

extern "C" int come_cpu_gmm_estep(const float *x, int64_t V, int d, const float *prec_chol,
                                  const float *mu_prec, const float *log_norm, int K,
                                  float *resp_out, float *lse_out, int threads) {
    if (V < 0 || d < 1 || d > kMaxDim || K < 1)
        return set_error(COME_E_INVALID, "need V>=0, 1<=d<=%d, K>=1", kMaxDim);
    int rc = check_threads(threads);
    if (rc) return rc;
    if (V == 0) return COME_OK;
    if (!x || !prec_chol || !mu_prec || !log_norm || !resp_out)
        return set_error(COME_E_INVALID, "null pointer");
    const Resp a{x, prec_chol, mu_prec, log_norm, resp_out, lse_out, V, d, K};
    auto fn = have_fma() ? resp_rows_fma : resp_rows_base;
    parallel_rows(V, threads, [&](int64_t lo, int64_t hi) { fn(a, lo, hi); });
    return COME_OK;
}

extern "C" int come_cpu_community_loss(const float *x, int64_t V, int d, const float *pi,
                                       const float *prec_chol, const float *mu_prec,
                                       const float *log_norm, int K, float *row_out,
                                       double *loss_out, int threads) {
    if (V < 0 || d < 1 || d > kMaxDim || K < 1 || K > 4096)
        return set_error(COME_E_INVALID, "community_loss: need V>=0, 1<=d<=%d, 1<=K<=4096",
                         kMaxDim);
    int rc = check_threads(threads);
    if (rc) return rc;
    if (V == 0) return COME_OK;
    if (!x || !pi || !prec_chol || !mu_prec || !log_norm || !loss_out)
        return set_error(COME_E_INVALID, "community_loss: null pointer");
    const Loss a{x, pi, prec_chol, mu_prec, log_norm, row_out, V, d, K};
    // one partial per block of rows (parallel_rows' split), added in block order
    const int64_t per = threads <= 1 || V < 64 ? V : (V + threads - 1) / threads;
    std::vector<double> part((size_t)((V + per - 1) / per), 0.0);
    parallel_rows(V, threads, [&](int64_t lo, int64_t hi) { part[lo / per] = loss_rows(a, lo, hi); });
    double total = 0.0;
    for (double p : part) total += p;
    *loss_out = total;
    return COME_OK;
}

extern "C" int come_cpu_gmm_resp(const float *x, int64_t V, int d, const float *prec_chol,
                                 const float *mu_prec, const float *log_norm, int K,
                                 float *resp_out, int threads) {
    return come_cpu_gmm_estep(x, V, d, prec_chol, mu_prec, log_norm, K, resp_out, nullptr,
                              threads);
}

extern "C" int come_cpu_sgns_o2_loss(const float *node, const float *ctx, int64_t V, int d,
                                     const int32_t *walks, int64_t P, int L,
                                     const uint64_t *seeds, int window, int negative,
                                     const uint32_t *table, uint64_t T, double *walk_out,
                                     double *loss_out, int64_t *pairs_out, int threads) {
    int rc = check_loss_tables("cpu_sgns_o2_loss", V, d, negative);
    if (rc) return rc;
    if (negative > 0 && (!table || T == 0))
        return set_error(COME_E_INVALID,
                         "cpu_sgns_o2_loss: negative sampling needs a non-empty table");
    if (P < 0 || L < 0 || window < 0)
        return set_error(COME_E_INVALID, "cpu_sgns_o2_loss: P, L and window must be >= 0");
    if (L > kMaxSentenceLen)
        return set_error(COME_E_INVALID, "cpu_sgns_o2_loss: L must be <= %d (got %d)",
                         kMaxSentenceLen, L);
    if (P > INT32_MAX) return set_error(COME_E_INVALID, "cpu_sgns_o2_loss: P too large");
    rc = check_threads(threads);
    if (rc) return rc;
    if (P == 0) return COME_OK;
    if (!node || !ctx || (!walks && L > 0) || !seeds || !loss_out)
        return set_error(COME_E_INVALID,
                         "cpu_sgns_o2_loss: null node/ctx/walks/seeds/loss_out pointer");
    const SgnsLoss a{node,  ctx, V,       d,       negative, window,  L,       walks,
                     seeds, table, T, nullptr, nullptr,  nullptr, walk_out};
    loss_drive(a, P, threads, loss_out, pairs_out);
    return COME_OK;
}

extern "C" int come_cpu_sgns_pairs_loss(const float *inp, const float *out, int64_t V, int d,
                                        const int32_t *rows_in, const int32_t *rows_pos,
                                        const int32_t *rows_neg, int64_t M, int negative,
                                        double *pair_out, double *loss_out, int64_t *pairs_out,
                                        int threads) {
    int rc = check_loss_tables("cpu_sgns_pairs_loss", V, d, negative);
    if (rc) return rc;
    if (M < 0) return set_error(COME_E_INVALID, "cpu_sgns_pairs_loss: M must be >= 0");
    if (M > INT32_MAX) return set_error(COME_E_INVALID, "cpu_sgns_pairs_loss: M too large");
    rc = check_threads(threads);
    if (rc) return rc;
    if (M == 0) return COME_OK;
    if (!inp || !out || !rows_in || !rows_pos || (!rows_neg && negative > 0) || !loss_out)
        return set_error(COME_E_INVALID, "cpu_sgns_pairs_loss: null inp/out/rows_in/rows_pos/"
                                         "rows_neg/loss_out pointer");
    const SgnsLoss a{inp,     out,     V, d,       negative, 0,        0,       nullptr,
                     nullptr, nullptr, 0, rows_in, rows_pos, rows_neg, pair_out};
    loss_drive(a, M, threads, loss_out, pairs_out);
    return COME_OK;
}

// The (p, q) and weighted walkers on host memory: come_walk_pq.h's pq_step<W>, the kernels' own
// step body, walk by walk.  A walk depends only on its global index, so the split over threads
// changes nothing.
template <bool W>
static void cpu_walks(const come::PqGraph &g, const come::PqParams &pp, int64_t V,
                      const int32_t *starts, int64_t P, int L, uint64_t seed, int64_t walk_offset,
                      const int32_t *emit, int32_t *out, uint64_t *trials_out, int threads) {
    using namespace come;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    std::atomic<uint64_t> total(0);
    parallel_rows(P, threads, [&](int64_t lo, int64_t hi) {
        uint64_t trials = 0;
        for (int64_t w = lo; w < hi; ++w) {
            int32_t *row = out + w * (int64_t)L;
            const int32_t start = starts[w];
            const uint64_t gw = (uint64_t)(walk_offset + w);
            bool alive = start >= 0 && start < V;  // not a node: an empty walk
            PqWalk s{alive ? start : -1, -1, 0, 0};
            for (int t = 0; t < L; ++t) {
                if (alive && t > 0)
                    trials += pq_step<W>(g, pp, start, (uint32_t)t, gw, k0, k1, s, alive);
                row[t] = alive ? (emit ? emit[s.cur] : s.cur) : -1;
            }
        }
        total += trials;
    });
    if (trials_out) *trials_out += total.load();
}

extern "C" int come_cpu_random_walks_pq(const int64_t *rowptr, const int32_t *col,
                                        const int32_t *col_sorted, int64_t V,
                                        const int32_t *starts, int64_t P, int L, float alpha,
                                        float p, float q, uint64_t seed, int64_t walk_offset,
                                        const int32_t *emit, int32_t *out, uint64_t *trials_out,
                                        int threads) {
    using namespace come;
    bool run;
    int rc = walk_check_args("cpu_random_walks_pq: ", V, P, L, walk_offset, alpha, p, q,
                             rowptr && col && starts && out, &run,
                             [&] { return check_threads(threads); });
    if (rc || !run) return rc;
    if (!col_sorted && pq_needs_sorted(p, q))
        return set_error(COME_E_INVALID,
                         "cpu_random_walks_pq: col_sorted may be NULL only with q == 1 and p >= 1");
    cpu_walks<false>(PqGraph{rowptr, col, col_sorted, rowptr[V], nullptr},
                     pq_make_params(alpha, p, q), V, starts, P, L, seed, walk_offset, emit, out,
                     trials_out, threads);
    return COME_OK;
}

// come_walk_cdf on host memory: come_walk_pq.h's cdf_units / cdf_threshold, row by row.  The
// prefix sums are integers and the maximum does not depend on an order, so this is the kernel's
// wcdf bit for bit, whatever its split of rows over lanes and wavefronts or `threads` here.
extern "C" int come_cpu_walk_cdf(const int64_t *rowptr, const float *weights, int64_t V,
                                 uint32_t *wcdf_out, int32_t *status_out, int threads) {
    using namespace come;
    if (V <= 0 || V > INT32_MAX)
        return set_error(COME_E_INVALID, "cpu_walk_cdf: V must be in [1, 2^31)");
    int rc = check_threads(threads);
    if (rc) return rc;
    if (!rowptr || !weights || !wcdf_out || !status_out)
        return set_error(COME_E_INVALID, "cpu_walk_cdf: null pointer");
    const int64_t nnz = rowptr[V];
    std::atomic<int32_t> status(0);
    parallel_rows(V, threads, [&](int64_t lo, int64_t hi) {
        for (int64_t v = lo; v < hi; ++v) {
            const int64_t b = rowptr[v], deg = rowptr[v + 1] - b;
            if (b < 0 || deg <= 0 || b + deg > nnz) continue;  // empty, or not a CSR
            float wmax = 0.0f;
            bool ok = true;
            for (int64_t i = 0; i < deg; ++i) {
                const float x = weights[b + i];
                ok = ok && cdf_weight_ok(x);
                wmax = x > wmax ? x : wmax;
            }
            if (!ok || !(wmax > 0.0f)) {
                for (int64_t i = 0; i < deg; ++i) wcdf_out[b + i] = 0xFFFFFFFFu;
                status = 1;
                continue;
            }
            uint64_t total = 0, U = 0;
            for (int64_t i = 0; i < deg; ++i) total += cdf_units(weights[b + i], wmax);
            for (int64_t i = 0; i < deg; ++i) {
                U += cdf_units(weights[b + i], wmax);
                wcdf_out[b + i] = cdf_threshold(U, total);
            }
        }
    });
    *status_out = status.load();
    return COME_OK;
}

extern "C" int come_cpu_random_walks_w(const int64_t *rowptr, const int32_t *col,
                                       const uint32_t *wcdf, int64_t V, const int32_t *starts,
                                       int64_t P, int L, float alpha, float p, float q,
                                       uint64_t seed, int64_t walk_offset, const int32_t *emit,
                                       int32_t *out, uint64_t *trials_out, int threads) {
    using namespace come;
    bool run;
    int rc = walk_check_args("cpu_random_walks_w: ", V, P, L, walk_offset, alpha, p, q,
                             rowptr && col && wcdf && starts && out, &run,
                             [&] { return check_threads(threads); });
    if (rc || !run) return rc;
    cpu_walks<true>(PqGraph{rowptr, col, col, rowptr[V], wcdf}, pq_make_params(alpha, p, q), V,
                    starts, P, L, seed, walk_offset, emit, out, trials_out, threads);
    return COME_OK;
}

// come_edge_cdf on host memory: cdf_units and an exact uint64 running sum.  The maximum does not
// depend on an order and the sums are integers, so this is the device scan's ecdf bit for bit,
// whatever its tiling.  One pass per phase; `threads` splits the maximum only (the sum is one
// sequential pass, memory-bound).
extern "C" int come_cpu_edge_cdf(const float *weights, int64_t E, uint64_t *ecdf_out,
                                 int32_t *status_out, int threads) {
    using namespace come;
    if (E <= 0 || E > INT32_MAX)
        return set_error(COME_E_INVALID, "cpu_edge_cdf: E must be in [1, 2^31)");
    int rc = check_threads(threads);
    if (rc) return rc;
    if (!weights || !ecdf_out || !status_out)
        return set_error(COME_E_INVALID, "cpu_edge_cdf: null pointer");
    std::atomic<int32_t> bad(0);
    std::atomic<uint32_t> wmax_bits(0);  // non-negative floats order as their bits
    parallel_rows(E, threads, [&](int64_t lo, int64_t hi) {
        float m = 0.0f;
        bool ok = true;
        for (int64_t i = lo; i < hi; ++i) {
            const float x = weights[i];
            ok = ok && cdf_weight_ok(x);
            m = x > m ? x : m;
        }
        if (!ok) bad = 1;
        uint32_t bits, seen = wmax_bits.load();
        memcpy(&bits, &m, sizeof bits);
        while (m > 0.0f && bits > seen && !wmax_bits.compare_exchange_weak(seen, bits)) {
        }
    });
    float wmax;
    const uint32_t bits = wmax_bits.load();
    memcpy(&wmax, &bits, sizeof wmax);
    if (bad.load() || !(wmax > 0.0f)) {
        *status_out = 1;
        return COME_OK;
    }
    uint64_t U = 0;
    for (int64_t i = 0; i < E; ++i) {
        U += cdf_units(weights[i], wmax);
        ecdf_out[i] = U;
    }
    *status_out = 0;
    return COME_OK;
}

// Test support: the sampler's pick for given 64-bit uniforms, idx_out[k] = edge_pick(r64[k]).
extern "C" int come_cpu_edge_pick(const uint64_t *ecdf, int64_t E, const uint64_t *r64, int64_t n,
                                  int64_t *idx_out) {
    using namespace come;
    if (E <= 0 || E > INT32_MAX)
        return set_error(COME_E_INVALID, "cpu_edge_pick: E must be in [1, 2^31)");
    if (n < 0) return set_error(COME_E_INVALID, "cpu_edge_pick: n must be >= 0");
    if (n == 0) return COME_OK;
    if (!ecdf || !r64 || !idx_out) return set_error(COME_E_INVALID, "cpu_edge_pick: null pointer");
    for (int64_t k = 0; k < n; ++k) idx_out[k] = edge_pick(ecdf, E, r64[k]);
    return COME_OK;
}

// The sampler on host memory: edge_r64 and edge_pick, the kernel's own draw.
extern "C" int come_cpu_edge_sample(const int32_t *edges, const uint64_t *ecdf, int64_t E,
                                    int64_t S, uint64_t seed, int64_t sample_offset, int32_t *out,
                                    int64_t *index_out, int threads) {
    using namespace come;
    if (E <= 0 || E > INT32_MAX)
        return set_error(COME_E_INVALID, "cpu_edge_sample: E must be in [1, 2^31)");
    if (S < 0 || sample_offset < 0)
        return set_error(COME_E_INVALID, "cpu_edge_sample: S and sample_offset must be >= 0");
    int rc = check_threads(threads);
    if (rc) return rc;
    if (S == 0) return COME_OK;
    if (!edges || !ecdf || !out) return set_error(COME_E_INVALID, "cpu_edge_sample: null pointer");
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    parallel_rows(S, threads, [&](int64_t lo, int64_t hi) {
        for (int64_t s = lo; s < hi; ++s) {
            const int64_t pick = edge_pick(ecdf, E, edge_r64((uint64_t)(sample_offset + s), k0, k1));
            out[2 * s] = edges[2 * pick];
            out[2 * s + 1] = edges[2 * pick + 1];
            if (index_out) index_out[s] = pick;
        }
    });
    return COME_OK;
}

// ---- top-k neighbour search (come_topk's contract on host arrays) ----
namespace come {
namespace {

struct Topk {
    const float *q, *base, *bsq;
    const int32_t *exclude;
    int32_t *idx;
    float *score;
    int64_t V;
    int d, k, metric;
};

// |x|^2 by an fmaf chain in feature order (k_row_sqnorms)
HOT float row_sqnorm(const float *x, int d) {
    float s = 0.0f;
    for (int c = 0; c < d; ++c) s = fmaf(x[c], x[c], s);
    return s;
}

inline float inv_norm(float sq) { return sq > 0.0f ? 1.0f / std::sqrt(sq) : (sq == 0.0f ? 0.0f : sq); }

// The kernels' arithmetic per pair: dot by an fmaf chain in feature order, key = fmaf(dot, mul_j,
// add_j), rank value v = key (dot), key / |q| (cosine), -max(0, |q|^2 - key) (L2); the list holds
// the k best (v descending, index ascending), kept sorted.  A NaN passes no comparison.
HOT void topk_rows(const Topk &a, int64_t lo, int64_t hi) {
    const int d = a.d, k = a.k;
    std::vector<float> lv(k);
    std::vector<int32_t> li(k);
    for (int64_t r = lo; r < hi; ++r) {
        const float *q = a.q + r * d;
        const float qsq = a.metric == COME_TOPK_DOT ? 0.0f : row_sqnorm(q, d);
        const float qf = a.metric == COME_TOPK_COSINE ? inv_norm(qsq) : qsq;
        const int32_t ex = a.exclude ? a.exclude[r] : -1;
        int n = 0;
        for (int64_t j0 = 0; j0 < a.V; j0 += 4) {
            float dot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const float *bp[4];
            for (int u = 0; u < 4; ++u) bp[u] = a.base + (j0 + u < a.V ? j0 + u : a.V - 1) * d;
            for (int c = 0; c < d; ++c) {
                const float qc = q[c];
                for (int u = 0; u < 4; ++u) dot[u] = fmaf(qc, bp[u][c], dot[u]);
            }
            for (int u = 0; u < 4 && j0 + u < a.V; ++u) {
                const int32_t j = (int32_t)(j0 + u);
                if (j == ex) continue;
                float v = dot[u];
                if (a.metric == COME_TOPK_COSINE) v = fmaf(v, inv_norm(a.bsq[j]), 0.0f) * qf;
                if (a.metric == COME_TOPK_L2) {
                    const float d2 = qf - fmaf(v, 2.0f, -a.bsq[j]);
                    v = -(d2 > 0.0f ? d2 : (d2 <= 0.0f ? 0.0f : d2));
                }
                // rows come in ascending index: an equal value loses to every entry held
                if (n == k && !(v > lv[k - 1])) continue;
                if (!(v > -INFINITY)) continue;  // NaN, or the score of an empty entry
                int p = n < k ? n++ : k - 1;
                for (; p > 0 && v > lv[p - 1]; --p) {
                    lv[p] = lv[p - 1];
                    li[p] = li[p - 1];
                }
                lv[p] = v;
                li[p] = j;
            }
        }
        const bool l2 = a.metric == COME_TOPK_L2;
        for (int e = 0; e < k; ++e) {
            a.idx[r * k + e] = e < n ? li[e] : -1;
            a.score[r * k + e] = e < n ? (l2 ? -lv[e] : lv[e]) : (l2 ? INFINITY : -INFINITY);
        }
    }
}
COME_FMA_CLONE void topk_rows_fma(const Topk &a, int64_t lo, int64_t hi) { topk_rows(a, lo, hi); }
void topk_rows_base(const Topk &a, int64_t lo, int64_t hi) { topk_rows(a, lo, hi); }

}  // namespace
}  // namespace come

extern "C" int come_cpu_topk(const float *q, int64_t Q, const float *base, int64_t V, int d, int k,
                             int metric, const int32_t *exclude, const float *base_sq,
                             int32_t *idx_out, float *score_out, int threads) {
    using namespace come;
    if (Q < 1 || V < 1 || V > INT32_MAX)
        return set_error(COME_E_INVALID, "cpu_topk: need Q >= 1 and V in [1, 2^31)");
    if (d < 1 || d > kMaxDim)
        return set_error(COME_E_INVALID, "cpu_topk: d must be in [1, %d] (got %d)", kMaxDim, d);
    if (k < 1 || k > 64) return set_error(COME_E_INVALID, "cpu_topk: k must be in [1, 64] (got %d)", k);
    if (metric != COME_TOPK_DOT && metric != COME_TOPK_COSINE && metric != COME_TOPK_L2)
        return set_error(COME_E_INVALID, "cpu_topk: unknown metric %d", metric);
    int rc = check_threads(threads);
    if (rc) return rc;
    if (!q || !base || !idx_out || !score_out)
        return set_error(COME_E_INVALID, "cpu_topk: null pointer");
    std::vector<float> own;
    if (!base_sq && metric != COME_TOPK_DOT) {
        own.resize((size_t)V);
        parallel_rows(V, threads, [&](int64_t lo, int64_t hi) {
            for (int64_t r = lo; r < hi; ++r) own[(size_t)r] = row_sqnorm(base + r * d, d);
        });
        base_sq = own.data();
    }
    const Topk a{q, base, base_sq, exclude, idx_out, score_out, V, d, k, metric};
    auto fn = have_fma() ? topk_rows_fma : topk_rows_base;
    parallel_rows(Q, threads, [&](int64_t lo, int64_t hi) { fn(a, lo, hi); });
    return COME_OK;
}
