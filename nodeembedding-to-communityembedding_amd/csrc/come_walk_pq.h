// come_walk_pq.h -- the walkers' random stream (Philox-4x32-10) and the node2vec (p, q)
// second-order step: one copy, compiled as device code by come_walk.hip (the walkers) and
// come_walk_cdf.hip (the CDF build) and as plain host C++ by come_cpu.cpp (the CPU twins), so the
// two are the same walks bit for bit.  Also the one check of the walkers' common arguments.
//
// Semantics.  A walk is c_0 = start.  Its first step, and the first step after a restart, is
// uniform over N(c_0): the first-order walker's step (come_walk.hip), same Philox block, same
// draws.  Every later step goes from cur = c_{t-1} with prev = c_{t-2} to x in N(cur) with
// probability proportional to
//     wr = 1/p   if x == prev,
//     wa = 1     if x is in N(prev),
//     wf = 1/q   otherwise.
// A node without neighbours ends the walk.  With probability alpha a step is instead a jump to
// `start`, after which the walk has no prev.
//
// Sampling: rejection against the envelope M = max(wa, wf), which p does not enter, with the part
// of the return weight above the envelope handled as an "outlier" (Knuth-Yao style mixture), so a
// step never costs O(degree) and a large 1/p never makes the other neighbours' acceptance small.
// Fixed point, units of 2^-32, computed once per call on the host in double (pq_make_params):
//     ta = wa / M,  tf = wf / M,  tr = min(wr, M) / M     each rounded, clamped to [1, 2^32] and
//                                                         stored minus one (a uint32)
//     e  = max(wr - M, 0) / M                             an integer < 2^45 (here <= 255 * 2^32)
// Step t of global walk gw (= walk_offset + w) runs trials j = 0, 1, ...; trial j draws one Philox
// block r[0..3] with counter (t, gw low, gw high, j) and the call's key (seed low, seed high):
//     j == 0 only: restart iff (r[1] >> 8) < ceil(alpha * 2^24)          (the first-order test)
//     no prev, or deg(cur) == 1: take col[b + ((r[0] * deg) >> 32)]      (the first-order pick);
//         for deg == 1 that is the only neighbour -- exact, and a leaf never spins for large p
//     otherwise
//       1. if e > 0 and prev is in N(cur): return to prev iff r[3] * (deg * 2^32 + e) < e * 2^32,
//          compared exactly in 128 bits, i.e. with probability e / (deg * 2^32 + e) to within the
//          2^-32 grain of r[3];
//       2. else the candidate x = col[b + ((r[0] * deg) >> 32)] is taken iff r[2] <= t(x) - 1,
//          t(x) = tr, ta or tf by the three cases above;
//       3. else trial j + 1.  After kPqMaxTrials trials the last candidate is taken.
// Exactness: one trial ends at neighbour x with probability min(w_x, M) / M / (deg + e 2^-32), plus
// e 2^-32 / (deg + e 2^-32) at prev, i.e. proportional to w_x for every x.  Acceptance for
// deg >= 2 is at least min(q, 1/q) / 2 whatever p and the degree (at most one neighbour is prev,
// and every other one is accepted with at least min(wa, wf) / M), so the expected trials per step
// are at most 2 max(q, 1/q) <= 32, and the cap is reached with probability < (1 - 1/32)^4096 <
// e^-100.  With p = q = 1 every threshold is 2^32 and e = 0: trial 0 always accepts, the walk is
// the first-order walker's.
//
// Membership (x in N(prev), prev in N(cur)) is a binary search in col_sorted: the rowptr of col,
// each row ascending.  At most 32 iterations, every index clamped to [0, rowptr[V]).  The N(prev)
// search is skipped when ta == tf (q == 1), the N(cur) search when e == 0 (p >= 1 / M); prev's
// (begin, degree) are carried from the step before.  Candidates always come from col, so with a
// col_sorted whose rows hold the right nodes in the wrong order the distribution is off but every
// step is still an edge.
//
// Edge weights (pq_step<true>, come_random_walks_w).  The same step with two substitutions; the
// Philox blocks, the thresholds ta / tf / tr and the outlier test are the code above.  Entry i of
// a row carries a 32-bit cumulative threshold wcdf[b + i] (come_walk_cdf builds them, cdf_units /
// cdf_threshold below are its arithmetic), and the search of r[0] in it replaces the multiply-shift
// pick: the candidate is the first i with max(r[0], 1) <= wcdf[b + i], a lower-bound search of at
// most kPqSearchSteps iterations with indices clamped to [0, nnz).  Write m_i for the number of
// 32-bit values of r[0] that end at i (pq_wmass); sum_i m_i = 2^32, an entry of weight 0 has
// m_i = 0, and with H = max(wcdf[i] + 1, 1), L = max(wcdf[i-1] + 1, 1) (L = 1 for i = 0)
// m_i = H - L + (L == 1 && H >= 2): the draw 0 counts as 1, so a threshold 0 at the head of a row
// -- entries of weight 0 before the first positive one -- is never selected.
//     no prev, or deg(cur) == 1: the candidate is taken: probability m_x / 2^32.
//     otherwise, with E' = floor(m_prev e / 2^32) (a 96-bit product; 0 when prev is not in the row):
//       1. if E' > 0: return to prev iff r[3] * (2^32 + E') < E' * 2^32   (pq_outlier; E' < 2^45);
//       2. else the candidate x is taken iff r[2] <= t(x) - 1;  3. else the next trial, capped.
// Exactness: one trial ends at x != prev with probability 2^32 / (2^32 + E') * m_x / 2^32 *
// t(x) / 2^32 = m_x t(x) / (2^32 (2^32 + E')), and at prev with (E' 2^32 + m_prev tr) / (2^32 (2^32
// + E')) = m_prev (e + tr) / (2^32 (2^32 + E')) up to the floor in E' (less than 2^-32 of a trial).
// t(x) / 2^32 = min(beta_x, M) / M and (e + tr) / 2^32 = (1/p) / M, so a trial ends at x with
// probability proportional to m_x beta_x for every x, prev included.  With equal weights m_i is
// the multiply-shift pick's count (come.h, come_walk_cdf), so candidates and acceptances are
// pq_step<false>'s and at p = q = 1 the walks are come_random_walks' bit for bit.  With e > 0 the
// outlier probability E' / (2^32 + E') equals e / (deg 2^32 + e) only to within e 2^-64 (m_prev is
// 2^32 / deg rounded to an integer), so on equal weights the walks at p < 1 / M are
// come_random_walks_pq's except where r[3] falls between the two, fewer than 2^-24 of the steps;
// tests pin them equal on the test graphs.
// Acceptance is WEAKER than above.  prev can hold almost all of a row's mass, so "at most one
// neighbour is prev" bounds nothing: with f = m_prev / 2^32 a trial succeeds with probability at
// least f tr' + (1 - f) min(ta, tf) / 2^32 where tr' = tr / 2^32 = min(1/p, M) / M, and for f -> 1
// only min(ta, tf, tr) / 2^32 remains.  That is min(1/q, 1, 1/p) / max(1, 1/q): at least 2^-8
// whenever q >= 1 or p <= 16, i.e. at most 256 expected trials, the cap reached with probability
// < (1 - 2^-8)^4096 < e^-16; in the corner p > 16 and q < 1 it falls to 2^-12 at (256, 1/16),
// 4096 expected trials, and there the cap can be reached with probability up to e^-1 on a row whose
// mass sits on prev (the last candidate is then taken: prev, almost surely).  For p <= 1 the
// bound is min(q, 1/q) whatever the weights, twice the unweighted walker's.
// Rows must be ascending: the outlier needs prev's INDEX in cur's row to read m_prev, so the
// weighted entry points take one adjacency array, each row ascending, with wcdf in that order; the
// membership search returns the index and there is no separate col_sorted.  A mis-ordered row
// gives wrong probabilities, but every step is still an entry of the row.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/come.h"

#if defined(__HIPCC__)
#define COME_HD __host__ __device__
#else
#define COME_HD
#endif

namespace come {

int set_error(int code, const char *fmt, ...);  // returns code (come_host.cpp)

struct Philox {
    uint32_t r[4];
};

COME_HD inline uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

COME_HD inline Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                    uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 10; ++i) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = mulhi32(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = mulhi32(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

// restart iff the 24-bit uniform (r[1] >> 8) < this
inline uint32_t walk_restart_threshold(float alpha) {
    return (uint32_t)ceil((double)alpha * 16777216.0);
}

constexpr int kPqMaxTrials = 4096;
constexpr int kPqSearchSteps = 32;
constexpr float kPqMinP = 1.0f / 256.0f, kPqMaxP = 256.0f;
constexpr float kPqMinQ = 1.0f / 16.0f, kPqMaxQ = 16.0f;

struct PqParams {
    uint64_t e;                  // outlier mass of the return edge, units of 2^-32
    uint32_t ta, tf, tr;         // acceptance thresholds minus one: accept iff r[2] <= t
    uint32_t restart_threshold;  // walk_restart_threshold(alpha)
};

// NaN fails both comparisons' conjunction
inline bool pq_in_range(float p, float q) {
    return p >= kPqMinP && p <= kPqMaxP && q >= kPqMinQ && q <= kPqMaxQ;
}

// does this (p, q) ever search col_sorted?
inline bool pq_needs_sorted(float p, float q) { return !(q == 1.0f && p >= 1.0f); }

inline uint32_t pq_threshold(double w) {  // w in (0, 1] -> round(w * 2^32) in [1, 2^32], minus 1
    double t = floor(w * 4294967296.0 + 0.5);
    if (!(t >= 1.0)) t = 1.0;
    if (t > 4294967296.0) t = 4294967296.0;
    return (uint32_t)((uint64_t)t - 1u);
}

inline PqParams pq_make_params(float alpha, float p, float q) {
    const double wr = 1.0 / (double)p, wa = 1.0, wf = 1.0 / (double)q;
    const double M = wa > wf ? wa : wf;
    PqParams pp;
    pp.ta = pq_threshold(wa / M);
    pp.tf = pq_threshold(wf / M);
    pp.tr = pq_threshold((wr < M ? wr : M) / M);
    pp.e = wr > M ? (uint64_t)floor((wr - M) / M * 4294967296.0 + 0.5) : 0u;
    pp.restart_threshold = walk_restart_threshold(alpha);
    return pp;
}

// The arguments every walker entry point takes, device or host, checked in the one order they
// all report them in.  `prefix` starts each message ("" for the device entries).  The first-order
// entry passes p = q = 1.  `pointers`: the entry's required pointers are all non-null -- looked at
// only when there is work, *run: P == 0 or L == 0 is COME_OK with nothing to do whatever the
// pointers are.  `also`: a check of the caller's own between the ranges and that early return (the
// CPU twins' `threads`).
template <class Also>
inline int walk_check_args(const char *prefix, int64_t V, int64_t P, int L, int64_t walk_offset,
                           float alpha, float p, float q, bool pointers, bool *run, Also also) {
    *run = false;
    if (V <= 0 || V > INT32_MAX)
        return set_error(COME_E_INVALID, "%sV must be in [1, 2^31)", prefix);
    if (P < 0 || L < 0 || walk_offset < 0)
        return set_error(COME_E_INVALID, "%sP, L and walk_offset must be >= 0", prefix);
    if (!(alpha >= 0.0f && alpha <= 1.0f))
        return set_error(COME_E_INVALID, "%salpha not in [0,1]", prefix);
    if (!pq_in_range(p, q))
        return set_error(COME_E_INVALID, "%sp must be in [2^-8, 2^8] and q in [2^-4, 2^4]", prefix);
    const int rc = also();
    if (rc) return rc;
    if (P == 0 || L == 0) return COME_OK;
    if (!pointers) return set_error(COME_E_INVALID, "%snull pointer", prefix);
    *run = true;
    return COME_OK;
}

inline int walk_check_args(const char *prefix, int64_t V, int64_t P, int L, int64_t walk_offset,
                           float alpha, float p, float q, bool pointers, bool *run) {
    return walk_check_args(prefix, V, P, L, walk_offset, alpha, p, q, pointers, run,
                           [] { return (int)COME_OK; });
}

struct PqGraph {
    const int64_t *rowptr;
    const int32_t *col;
    const int32_t *col_sorted;  // may be NULL when no (p, q) search runs (pq_needs_sorted)
    int64_t nnz;                // rowptr[V]: search indices are clamped below it
    const uint32_t *wcdf;       // pq_step<true> only: per-entry thresholds, col's rows ascending
};

struct PqWalk {
    int32_t cur, prev;  // prev = -1: none (first step, or the step after a restart)
    int64_t pb, pdeg;   // N(prev) = col_sorted[pb, pb + pdeg)
};

// v's index in col_sorted[b, b + deg), or -1.  A bounded binary search; an unsorted row gives some
// answer.
COME_HD inline int64_t pq_index(const PqGraph &g, int64_t b, int64_t deg, int32_t v) {
    if (g.nnz <= 0) return -1;
    int64_t lo = 0, hi = deg;
    for (int i = 0; i < kPqSearchSteps && lo < hi; ++i) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        int64_t idx = b + mid;
        idx = idx < 0 ? 0 : idx;
        idx = idx < g.nnz ? idx : g.nnz - 1;
        const int32_t c = g.col_sorted[idx];
        if (c == v) return mid;
        if (c < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return -1;
}

COME_HD inline bool pq_contains(const PqGraph &g, int64_t b, int64_t deg, int32_t v) {
    return pq_index(g, b, deg, v) >= 0;
}

// ---- edge weights: the per-row CDF's arithmetic (come_walk_cdf) and its search ----

// u_i: the weight in units of 2^-32 of the row's largest.  The division is correctly rounded and
// the scaling exact, so the device and the host agree (nothing here is built with fast-math).
COME_HD inline uint64_t cdf_units(float w, float wmax) {
    return (uint64_t)llrint((double)w / (double)wmax * 4294967296.0);
}

// T_i - 1 (saturating at 0) from the exact prefix sum U_i and the row's total U_last > 0
COME_HD inline uint32_t cdf_threshold(uint64_t U, uint64_t Ulast) {
    double t = ceil((double)U / (double)Ulast * 4294967296.0);
    if (U >= Ulast || t > 4294967296.0) t = 4294967296.0;
    const uint64_t T = (uint64_t)t;
    return (uint32_t)(T > 0 ? T - 1 : 0);
}

// finite and >= 0 (NaN fails the comparison)
COME_HD inline bool cdf_weight_ok(float w) { return w >= 0.0f && w <= 3.4028234663852886e38f; }

COME_HD inline uint32_t pq_wcdf_at(const PqGraph &g, int64_t idx) {
    idx = idx < 0 ? 0 : idx;
    idx = idx < g.nnz ? idx : g.nnz - 1;
    return g.wcdf[idx];
}

// The first i in [0, deg) with max(r0, 1) <= wcdf[b + i]; deg - 1 if there is none (a row whose
// last threshold is not 2^32 - 1: not come_walk_cdf's).  deg >= 1, nnz >= 1.
COME_HD inline int64_t pq_wpick(const PqGraph &g, int64_t b, int64_t deg, uint32_t r0) {
    r0 |= (uint32_t)(r0 == 0);
    int64_t lo = 0, hi = deg - 1;
    for (int i = 0; i < kPqSearchSteps && lo < hi; ++i) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (r0 <= pq_wcdf_at(g, b + mid))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// m_i: how many of the 2^32 values of r0 pq_wpick sends to entry i of the row at b
COME_HD inline uint64_t pq_wmass(const PqGraph &g, int64_t b, int64_t i) {
    uint64_t H = (uint64_t)pq_wcdf_at(g, b + i) + 1u;
    uint64_t L = i > 0 ? (uint64_t)pq_wcdf_at(g, b + i - 1) + 1u : 1u;
    L = L < 1u ? 1u : L;
    H = H < L ? L : H;  // a threshold array that is not monotone: no mass
    return H - L + (uint64_t)(L == 1u && H >= 2u);
}

// floor(m * e / 2^32), m <= 2^32, e < 2^45: a 96-bit product
COME_HD inline uint64_t pq_scale_outlier(uint64_t m, uint64_t e) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t hi = __umul64hi(m, e);
#else
    const uint64_t hi = (uint64_t)(((unsigned __int128)m * (unsigned __int128)e) >> 64);
#endif
    return (hi << 32) | ((m * e) >> 32);
}

// r3 * den < e * 2^32, exactly (den < 2^64, r3 < 2^32, e < 2^45: both sides below 2^96)
COME_HD inline bool pq_outlier(uint32_t r3, uint64_t den, uint64_t e) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t hi = __umul64hi((uint64_t)r3, den);
#else
    const uint64_t hi = (uint64_t)(((unsigned __int128)r3 * (unsigned __int128)den) >> 64);
#endif
    const uint64_t lo = (uint64_t)r3 * den;
    const uint64_t ehi = e >> 32, elo = e << 32;
    return hi < ehi || (hi == ehi && lo < elo);
}

// The candidate's index in the row for the draw r0: by weight (the CDF search), or uniform (:40):
// multiply-shift of a 32-bit uniform, bias <= deg / 2^32
template <bool W>
COME_HD inline int64_t pq_pick(const PqGraph &g, int64_t b, int64_t deg, uint32_t r0) {
    if constexpr (W)
        return pq_wpick(g, b, deg, r0);
    else
        return (int64_t)(((uint64_t)r0 * (uint64_t)deg) >> 32);
}

// One step (t >= 1) of global walk gw from s.cur.  Returns the Philox blocks drawn: 0 at a node
// without neighbours (the walk ends: alive = false, s unchanged), else 1 + the rejected trials.
// W: edge weights -- candidates by pq_wpick in g.wcdf, the outlier mass scaled by prev's mass;
// g.col == g.col_sorted then, each row ascending.
template <bool W = false>
COME_HD inline uint32_t pq_step(const PqGraph &g, const PqParams &pp, int32_t start, uint32_t t,
                                uint64_t gw, uint32_t k0, uint32_t k1, PqWalk &s, bool &alive) {
    const int32_t cur = s.cur;
    const int64_t b = g.rowptr[cur];
    const int64_t deg = g.rowptr[cur + 1] - b;
    if (deg <= 0) {  // graph_utils.py:44-45
        alive = false;
        return 0;
    }
    const uint32_t c1 = (uint32_t)gw, c2 = (uint32_t)(gw >> 32);
    Philox x = philox4x32_10(t, c1, c2, 0u, k0, k1);
    if ((x.r[1] >> 8) < pp.restart_threshold) {  // rand.random() < alpha (:39): restart (:42)
        s.cur = start;
        s.prev = -1;
        return 1;
    }
    int64_t pick = pq_pick<W>(g, b, deg, x.r[0]);
    const int32_t prev = s.prev;
    uint32_t trials = 1;
    int32_t nxt;
    if (prev < 0 || deg == 1) {
        nxt = g.col[b + pick];
    } else {
        bool back;
        uint64_t e = pp.e, den;
        if constexpr (W) {
            const int64_t at = e > 0 ? pq_index(g, b, deg, prev) : -1;
            e = at >= 0 ? pq_scale_outlier(pq_wmass(g, b, at), e) : 0u;
            back = e > 0;
            den = 4294967296ull + e;
        } else {
            back = e > 0 && pq_contains(g, b, deg, prev);
            den = ((uint64_t)(deg < INT32_MAX ? deg : INT32_MAX) << 32) + e;
        }
        // by value: a select between fields of the by-reference struct becomes an indexed load
        const uint32_t ta = pp.ta, tf = pp.tf, tr = pp.tr;
        const bool split = ta != tf;
        for (;;) {
            if (back && pq_outlier(x.r[3], den, e)) {
                nxt = prev;
                break;
            }
            nxt = g.col[b + pick];
            uint32_t thr = ta;
            if (nxt == prev)
                thr = tr;
            else if (split && !pq_contains(g, s.pb, s.pdeg, nxt))
                thr = tf;
            if (x.r[2] <= thr || trials == (uint32_t)kPqMaxTrials) break;
            x = philox4x32_10(t, c1, c2, trials, k0, k1);
            pick = pq_pick<W>(g, b, deg, x.r[0]);
            ++trials;
        }
    }
    s.prev = cur;
    s.pb = b;
    s.pdeg = deg;
    s.cur = nxt;
    return trials;
}

}  // namespace come
