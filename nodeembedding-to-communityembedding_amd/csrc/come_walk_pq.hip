// come_walk_pq.hip -- node2vec (p, q) second-order walks on the device (gfx950).
//
// The step itself -- semantics, the rejection sampler, the random stream -- is come_walk_pq.h's
// pq_step, shared with the CPU twin (come_cpu.cpp).  This file is the launch around it: one lane
// per walk, 256-lane workgroups, the output staged through LDS in 16-step slices exactly as
// k_random_walks_staged<16> (come_walk.hip) does.  Per trial a lane reads one rowptr pair, one col
// entry and up to log2(deg(prev)) col_sorted entries: latency-bound gathers, hidden by the
// thousands of walks in flight per CU.  Lanes of a wavefront run different numbers of trials;
// the trial loop is capped (kPqMaxTrials) and the searches are bounded (kPqSearchSteps), so no
// lane can keep a wavefront spinning.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "come_internal.h"
#include "come_walk_pq.h"

namespace come {

struct WalkPqArgs {
    const int64_t *rowptr;
    const int32_t *col;
    const int32_t *col_sorted;
    const int32_t *starts;
    const int32_t *emit;
    int32_t *out;
    unsigned long long *trials_out;  // += the Philox blocks this launch drew, or NULL
    int64_t V;
    int64_t P;
    int64_t walk_offset;  // global index of walk 0 of this launch (counter of the stream)
    uint64_t seed;
    int L;
    PqParams pp;
};

constexpr int WALK_PQ_BLOCK = 256;
constexpr int WALK_PQ_CHUNK = 16;

__global__ void __launch_bounds__(WALK_PQ_BLOCK) k_random_walks_pq(WalkPqArgs a) {
    // +1: column writes hit distinct banks
    __shared__ alignas(8) int32_t tile[WALK_PQ_BLOCK][WALK_PQ_CHUNK + 1];
    const int tid = threadIdx.x;
    const int64_t w0 = (int64_t)blockIdx.x * WALK_PQ_BLOCK;
    const int64_t w = w0 + tid;
    const uint64_t gw = (uint64_t)(a.walk_offset + w);
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const PqGraph g{a.rowptr, a.col, a.col_sorted, a.rowptr[a.V], nullptr};
    int32_t start = -1;
    if (w < a.P) start = a.starts[w];
    bool alive = start >= 0 && start < a.V;  // not a node: an empty walk
    PqWalk s{alive ? start : -1, -1, 0, 0};
    uint64_t trials = 0;
    const int64_t rows = a.P - w0 < WALK_PQ_BLOCK ? a.P - w0 : WALK_PQ_BLOCK;
    // dead lanes and lanes past P keep going through the chunk loop (they emit -1), so every
    // lane reaches the barriers
    for (int c0 = 0; c0 < a.L; c0 += WALK_PQ_CHUNK) {
        const int cn = a.L - c0 < WALK_PQ_CHUNK ? a.L - c0 : WALK_PQ_CHUNK;
        for (int j = 0; j < cn; ++j) {
            const int t = c0 + j;
            if (alive && t > 0) trials += pq_step(g, a.pp, start, (uint32_t)t, gw, k0, k1, s, alive);
            tile[tid][j] = alive ? (a.emit ? a.emit[s.cur] : s.cur) : -1;
        }
        __syncthreads();
        // rows x cn slice -> global, consecutive lanes on consecutive columns of one row
        for (int i = tid; i < (int)rows * cn; i += WALK_PQ_BLOCK) {
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

extern "C" int come_random_walks_pq(const int64_t *rowptr, const int32_t *col,
                                    const int32_t *col_sorted, int64_t V, const int32_t *starts,
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
    if (!rowptr || !col || !starts || !out) return set_error(COME_E_INVALID, "null pointer");
    if (!col_sorted && pq_needs_sorted(p, q))
        return set_error(COME_E_INVALID, "col_sorted may be NULL only with q == 1 and p >= 1");
    int dev = 0;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    WalkPqArgs a{rowptr, col, col_sorted, starts, emit, out, (unsigned long long *)trials_out,
                 V, P, walk_offset, seed, L, pq_make_params(alpha, p, q)};
    const int64_t blocks = (P + WALK_PQ_BLOCK - 1) / WALK_PQ_BLOCK;
    if (blocks > INT32_MAX) return set_error(COME_E_INVALID, "too many walks in one launch");
    void *kargs[] = {&a};
    hipError_t e = hipLaunchKernel((const void *)k_random_walks_pq, dim3((unsigned)blocks),
                                   dim3(WALK_PQ_BLOCK), kargs, 0, (hipStream_t)stream);
    return hip_error(e, "k_random_walks_pq launch");
}
