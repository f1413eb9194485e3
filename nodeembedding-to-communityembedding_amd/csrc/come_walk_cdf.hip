// come_walk_cdf.hip -- the per-row CDF build of the edge-weighted walks (gfx950): k_walk_cdf.  The
// walker that reads it is k_random_walks_w (come_walk.hip).
//
// The CDF's arithmetic is cdf_units / cdf_threshold of come_walk_pq.h, shared with the CPU twin
// (come_cpu.cpp), so the thresholds are the host's bit for bit.
//
// k_walk_cdf.  Per row: the largest weight, u_i = llrint(w_i / wmax * 2^32), the exact uint64
// prefix sums U_i, and T_i = ceil(U_i / U_last * 2^32).  Only the maximum (order-free) and integer
// sums enter, so how a row is split over lanes cannot change a bit.  Rows differ by four orders of
// magnitude in length: a lane takes its own row when it has at most CDF_SHORT entries, and the
// longer rows of a wavefront's 64 are then taken one after another by the whole wavefront (a
// shuffle scan per 64 entries, the carry in a register).  Three passes over the row (maximum,
// total, thresholds); a one-off pass per graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "come_internal.h"
#include "come_walk_pq.h"

namespace come {

constexpr int CDF_BLOCK = 256;
constexpr int CDF_SHORT = 32;  // rows up to this long are built by one lane

// One lane, one row of `deg` entries at `b`.  Returns false for a row that must not be used.
__device__ inline bool cdf_row_lane(const float *w, uint32_t *out, int64_t b, int deg) {
    float wmax = 0.0f;
    bool ok = true;
    for (int i = 0; i < deg; ++i) {
        const float x = w[b + i];
        ok = ok && cdf_weight_ok(x);
        wmax = x > wmax ? x : wmax;
    }
    ok = ok && wmax > 0.0f;
    if (!ok) {
        for (int i = 0; i < deg; ++i) out[b + i] = 0xFFFFFFFFu;
        return false;
    }
    uint64_t total = 0;
    for (int i = 0; i < deg; ++i) total += cdf_units(w[b + i], wmax);
    uint64_t U = 0;
    for (int i = 0; i < deg; ++i) {
        U += cdf_units(w[b + i], wmax);
        out[b + i] = cdf_threshold(U, total);
    }
    return true;
}

__device__ inline uint64_t wave_sum_u64(uint64_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor((unsigned long long)v, off, 64);
    return v;
}

// A whole wavefront, one row (uniform b, deg across the lanes).
__device__ inline bool cdf_row_wave(const float *w, uint32_t *out, int64_t b, int64_t deg,
                                    int lane) {
    float wmax = 0.0f;
    int bad = 0;
    for (int64_t i = lane; i < deg; i += 64) {
        const float x = w[b + i];
        bad |= !cdf_weight_ok(x);
        wmax = x > wmax ? x : wmax;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(wmax, off, 64);
        wmax = o > wmax ? o : wmax;
        bad |= __shfl_xor(bad, off, 64);
    }
    if (bad || !(wmax > 0.0f)) {
        for (int64_t i = lane; i < deg; i += 64) out[b + i] = 0xFFFFFFFFu;
        return false;
    }
    uint64_t total = 0;
    for (int64_t i = lane; i < deg; i += 64) total += cdf_units(w[b + i], wmax);
    total = wave_sum_u64(total);
    uint64_t carry = 0;
    for (int64_t i0 = 0; i0 < deg; i0 += 64) {  // uniform trip count: every lane shuffles
        const int64_t i = i0 + lane;
        uint64_t U = i < deg ? cdf_units(w[b + i], wmax) : 0u;
        for (int off = 1; off < 64; off <<= 1) {  // inclusive scan over the 64 lanes
            const uint64_t o = __shfl_up((unsigned long long)U, off, 64);
            if (lane >= off) U += o;
        }
        U += carry;
        if (i < deg) out[b + i] = cdf_threshold(U, total);
        carry = __shfl((unsigned long long)U, 63, 64);
    }
    return true;
}

__global__ void __launch_bounds__(CDF_BLOCK) k_walk_cdf(const int64_t *__restrict__ rowptr,
                                                        const float *__restrict__ weights,
                                                        int64_t V, uint32_t *__restrict__ wcdf,
                                                        int32_t *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * CDF_BLOCK + threadIdx.x;
    const int64_t nnz = rowptr[V];
    int64_t b = 0, deg = 0;
    if (v < V) {
        b = rowptr[v];
        deg = rowptr[v + 1] - b;
        if (b < 0 || deg < 0 || b + deg > nnz) deg = 0;  // not a CSR: touch nothing
    }
    bool ok = true;
    if (deg > 0 && deg <= CDF_SHORT) ok = cdf_row_lane(weights, wcdf, b, (int)deg);
    // the long rows among this wavefront's 64, one at a time, all lanes on each
    unsigned long long longs = __ballot(deg > CDF_SHORT);
    while (longs) {
        const int src = __ffsll(longs) - 1;
        longs &= longs - 1;
        const int64_t rb = __shfl((unsigned long long)b, src, 64);
        const int64_t rd = __shfl((unsigned long long)deg, src, 64);
        if (!cdf_row_wave(weights, wcdf, rb, rd, lane)) ok = false;
    }
    if (!ok) *status = 1;  // a plain (vector) store: every writer writes the same word
}

}  // namespace come

using namespace come;

extern "C" int come_walk_cdf(const int64_t *rowptr, const float *weights, int64_t V,
                             uint32_t *wcdf_out, int32_t *status, void *stream) {
    if (V <= 0 || V > INT32_MAX) return set_error(COME_E_INVALID, "V must be in [1, 2^31)");
    if (!rowptr || !weights || !wcdf_out || !status)
        return set_error(COME_E_INVALID, "walk_cdf: null pointer");
    int dev = 0;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) return hip_error(e, "walk_cdf status memset");
    const int64_t blocks = (V + CDF_BLOCK - 1) / CDF_BLOCK;
    hipLaunchKernelGGL(k_walk_cdf, dim3((unsigned)blocks), dim3(CDF_BLOCK), 0,
                       (hipStream_t)stream, rowptr, weights, V, wcdf_out, status);
    return hip_error(hipGetLastError(), "k_walk_cdf launch");
}
