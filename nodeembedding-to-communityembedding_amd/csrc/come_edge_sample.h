// come_edge_sample.h -- edge sampling by weight for the first-order (O1) trainer: the arithmetic
// of the global edge CDF and of one draw from it.  One copy, compiled as device code by
// come_edge_sample.hip (k_edge_cdf_*, k_edge_sample) and as plain host C++ by come_cpu.cpp
// (come_cpu_edge_cdf, come_cpu_edge_sample, come_cpu_edge_pick), so the CDF words, the sampled
// rows and their indices are the same on both sides bit for bit.
//
// CDF.  With wmax the largest of the E weights, edge i carries u_i = cdf_units(w_i, wmax) =
// llrint(w_i / wmax * 2^32) <= 2^32 units (come_walk_pq.h: a correctly rounded division and an
// exact scaling) and ecdf[i] = U_i = u_0 + ... + u_i, an exact uint64 sum: E < 2^31 keeps
// U_E < 2^63.  Only an order-free maximum and integer sums enter, so any scan order gives the same
// words.  The sums themselves are stored -- no thresholds, no second rounding.
//
// Draw.  Global sample gs draws ONE Philox-4x32-10 block with
//     counter (c0, c1, c2, c3) = (gs low 32 bits, gs high 32 bits, 0, kEdgeStream)
//     key     (k0, k1)         = (seed low 32 bits, seed high 32 bits).
// The walkers' counters are (t, gw low, gw high, j) with a trial index j < kPqMaxTrials = 4096 in
// c3, so c3 = kEdgeStream = 0x45444745 ("EDGE") is a block no walk of the same seed ever draws.
//     r64 = r[0] << 32 | r[1]
//     x   = mulhi64(r64, U_E) = floor(r64 * U_E / 2^64)            in [0, U_E)
//     pick = the first i with x < ecdf[i]
// a lower-bound search of at most kEdgeSearchSteps iterations, every index clamped to [0, E).
// Exactness: edge i is the pick for U_{i-1} <= x < U_i, i.e. for the r64 in
// [ceil(U_{i-1} 2^64 / U_E), ceil(U_i 2^64 / U_E)): it receives
//     ceil(U_i 2^64 / U_E) - ceil(U_{i-1} 2^64 / U_E)
// of the 2^64 values of r64 (U_{-1} = 0), which is u_i / U_E to within 2^-64.  An edge with
// u_i = 0 (weight 0, or below 2^-33 wmax) repeats its predecessor's sum, owns no x and is never
// drawn, at the head of the array included (there U_i = 0 and x < 0 never holds).
#pragma once
#include <stdint.h>

#include "come_walk_pq.h"

namespace come {

constexpr uint32_t kEdgeStream = 0x45444745u;
constexpr int kEdgeSearchSteps = 32;  // E < 2^31: 31 halvings reach one entry

COME_HD inline uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// the 64-bit uniform of global sample gs
COME_HD inline uint64_t edge_r64(uint64_t gs, uint32_t k0, uint32_t k1) {
    const Philox x = philox4x32_10((uint32_t)gs, (uint32_t)(gs >> 32), 0u, kEdgeStream, k0, k1);
    return ((uint64_t)x.r[0] << 32) | (uint64_t)x.r[1];
}

COME_HD inline uint64_t edge_cdf_at(const uint64_t *ecdf, int64_t E, int64_t idx) {
    idx = idx < 0 ? 0 : idx;
    idx = idx < E ? idx : E - 1;
    return ecdf[idx];
}

// The first i in [0, E) with mulhi64(r64, ecdf[E - 1]) < ecdf[i]; E - 1 if there is none (an array
// that is not come_edge_cdf's).  E >= 1.
COME_HD inline int64_t edge_pick(const uint64_t *ecdf, int64_t E, uint64_t r64) {
    const uint64_t x = mulhi64(r64, ecdf[E - 1]);
    int64_t lo = 0, hi = E - 1;
    for (int i = 0; i < kEdgeSearchSteps && lo < hi; ++i) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (x < edge_cdf_at(ecdf, E, mid))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

}  // namespace come
