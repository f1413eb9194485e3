// come_walk_w.hip -- edge-weighted random walks on the device (gfx950): the per-row CDF build
// (k_walk_cdf) and the weighted (p, q) walker (k_random_walks_w).
//
// The step is come_walk_pq.h's pq_step<true> and the CDF's arithmetic is cdf_units / cdf_threshold
// of the same header, both shared with the CPU twins (come_cpu.cpp), so thresholds, walks and trial
// counts are the host's bit for bit.
//
// k_walk_cdf.  Per row: the largest weight, u_i = llrint(w_i / wmax * 2^32), the exact uint64
// prefix sums U_i, and T_i = ceil(U_i / U_last * 2^32).  Only the maximum (order-free) and integer
// sums enter, so how a row is split over lanes cannot change a bit.  Rows differ by four orders of
// magnitude in length: a lane takes its own row when it has at most CDF_SHORT entries, and the
// longer rows of a wavefront's 64 are then taken one after another by the whole wavefront (a
// shuffle scan per 64 entries, the carry in a register).  Three passes over the row (maximum,
// total, thresholds); a one-off pass per graph.
//
// k_random_walks_w is k_random_walks_pq's launch: one lane per walk, 256-lane workgroups, the
// output staged through LDS in 16-step slices.  Per trial a lane additionally walks about
// log2(deg) dependent wcdf entries for its candidate.
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

struct WalkWArgs {
    const int64_t *rowptr;
    const int32_t *col;
    const uint32_t *wcdf;
    const int32_t *starts;
    const int32_t *emit;
    int32_t *out;
    unsigned long long *trials_out;  // += the Philox blocks this launch drew, or NULL
    int64_t V;
    int64_t P;
    int64_t walk_offset;
    uint64_t seed;
    int L;
    PqParams pp;
};

constexpr int WALK_W_BLOCK = 256;
constexpr int WALK_W_CHUNK = 16;

__global__ void __launch_bounds__(WALK_W_BLOCK) k_random_walks_w(WalkWArgs a) {
    // +1: column writes hit distinct banks
    __shared__ alignas(8) int32_t tile[WALK_W_BLOCK][WALK_W_CHUNK + 1];
    const int tid = threadIdx.x;
    const int64_t w0 = (int64_t)blockIdx.x * WALK_W_BLOCK;
    const int64_t w = w0 + tid;
    const uint64_t gw = (uint64_t)(a.walk_offset + w);
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const PqGraph g{a.rowptr, a.col, a.col, a.rowptr[a.V], a.wcdf};
    int32_t start = -1;
    if (w < a.P) start = a.starts[w];
    bool alive = start >= 0 && start < a.V;  // not a node: an empty walk
    PqWalk s{alive ? start : -1, -1, 0, 0};
    uint64_t trials = 0;
    const int64_t rows = a.P - w0 < WALK_W_BLOCK ? a.P - w0 : WALK_W_BLOCK;
    // dead lanes and lanes past P keep going through the chunk loop (they emit -1), so every
    // lane reaches the barriers
    for (int c0 = 0; c0 < a.L; c0 += WALK_W_CHUNK) {
        const int cn = a.L - c0 < WALK_W_CHUNK ? a.L - c0 : WALK_W_CHUNK;
        for (int j = 0; j < cn; ++j) {
            const int t = c0 + j;
            if (alive && t > 0)
                trials += pq_step<true>(g, a.pp, start, (uint32_t)t, gw, k0, k1, s, alive);
            tile[tid][j] = alive ? (a.emit ? a.emit[s.cur] : s.cur) : -1;
        }
        __syncthreads();
        // rows x cn slice -> global, consecutive lanes on consecutive columns of one row
        for (int i = tid; i < (int)rows * cn; i += WALK_W_BLOCK) {
            const int r = i / cn, j = i - r * cn;
            a.out[(w0 + r) * (int64_t)a.L + c0 + j] = tile[r][j];
        }
        __syncthreads();
    }
    if (a.trials_out) {  // uniform: one LDS add per walk (the tile is free now), one global add
        unsigned long long *block_trials = (unsigned long long *)&tile[0][0];
        if (tid == 0) *block_trials = 0;
        __syncthreads();
        if (trials) atomicAdd(block_trials, (unsigned long long)trials);
        __syncthreads();
        if (tid == 0 && *block_trials) atomicAdd(a.trials_out, *block_trials);
    }
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

extern "C" int come_random_walks_w(const int64_t *rowptr, const int32_t *col,
                                   const uint32_t *wcdf, int64_t V, const int32_t *starts,
                                   int64_t P, int L, float alpha, float p, float q, uint64_t seed,
                                   int64_t walk_offset, const int32_t *emit, int32_t *out,
                                   uint64_t *trials_out, void *stream) {
    if (V <= 0 || V > INT32_MAX) return set_error(COME_E_INVALID, "V must be in [1, 2^31)");
    if (P < 0 || L < 0 || walk_offset < 0)
        return set_error(COME_E_INVALID, "P, L and walk_offset must be >= 0");
    if (!(alpha >= 0.0f && alpha <= 1.0f)) return set_error(COME_E_INVALID, "alpha not in [0,1]");
    if (!pq_in_range(p, q))
        return set_error(COME_E_INVALID, "p must be in [2^-8, 2^8] and q in [2^-4, 2^4]");
    if (P == 0 || L == 0) return COME_OK;
    if (!rowptr || !col || !wcdf || !starts || !out)
        return set_error(COME_E_INVALID, "null pointer");
    int dev = 0;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    WalkWArgs a{rowptr, col, wcdf, starts, emit, out, (unsigned long long *)trials_out,
                V, P, walk_offset, seed, L, pq_make_params(alpha, p, q)};
    const int64_t blocks = (P + WALK_W_BLOCK - 1) / WALK_W_BLOCK;
    if (blocks > INT32_MAX) return set_error(COME_E_INVALID, "too many walks in one launch");
    void *kargs[] = {&a};
    hipError_t e = hipLaunchKernel((const void *)k_random_walks_w, dim3((unsigned)blocks),
                                   dim3(WALK_W_BLOCK), kargs, 0, (hipStream_t)stream);
    return hip_error(e, "k_random_walks_w launch");
}
