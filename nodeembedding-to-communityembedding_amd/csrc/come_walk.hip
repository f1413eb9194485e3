// come_walk.hip -- device random-walk generators (gfx950): the producer of train_o2's input.
// The first-order walker (come_random_walks), node2vec's (p, q) second-order walker
// (come_random_walks_pq) and the edge-weighted one (come_random_walks_w): one launch body, one
// step policy per walker.
//
// Reference: utils/graph_utils.py __random_walk__ (:20-46) driven by build_deepwalk_corpus_iter
// (:187-192).  Same distribution as the reference walker -- from the current node, with
// probability alpha jump back to the walk's first node, otherwise move to a uniformly chosen
// neighbour; a node without neighbours ends the walk -- but not the same random stream: the
// reference's CPython MT19937 stream is restated exactly on the host (come_walks_reference).
// The (p, q) and weighted steps -- semantics, the rejection sampler, the random stream -- are
// come_walk_pq.h's pq_step<W>, shared with the CPU twins (come_cpu.cpp).
//
// One lane per walk.  The random numbers come from Philox-4x32-10 keyed by the seed and counted
// by (walk, step), so a walk's path does not depend on the launch shape, the batch it is in or
// the device.  Per step a first-order lane reads rowptr[cur], rowptr[cur + 1] (one 16-B pair) and
// one col entry; a (p, q) trial adds up to log2(deg(prev)) col_sorted entries and a weighted one
// about log2(deg) dependent wcdf entries for its candidate: latency-bound gathers with thousands
// of walks in flight per CU.  Lanes of a wavefront run different numbers of trials; the trial
// loop is capped (kPqMaxTrials) and the searches are bounded (kPqSearchSteps), so no lane can
// keep a wavefront spinning.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "come_internal.h"
#include "come_walk_pq.h"  // Philox, pq_step and walk_check_args, shared with the CPU twins

namespace come {

// Two argument structs, in the member order the kernels had as separate files: a kernel argument's
// offset steers the scalar loads and with them the register allocation of the whole kernel, and
// one struct for all three renumbered the first-order kernel's scalar registers throughout
// (profiles/r17_walk_refactor.txt).
struct WalkArgs {  // first-order
    const int64_t *rowptr;
    const int32_t *col;
    const int32_t *starts;
    const int32_t *emit;
    int32_t *out;
    int64_t V;
    int64_t P;
    int64_t walk_offset;  // global index of walk 0 of this launch (counter of the stream)
    uint64_t seed;
    int L;
    uint32_t restart_threshold;  // walk_restart_threshold(alpha)
};

struct WalkPqArgs {  // (p, q) and weighted
    const int64_t *rowptr;
    const int32_t *col;
    union {  // one slot: the weighted walker has no col_sorted of its own (col's rows ascend)
        const int32_t *col_sorted;
        const uint32_t *wcdf;
    };
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

// ---- step policies ----
// A policy object holds what a launch's steps share; State is a lane's walk, node() the node it
// stands on.  step(): advance one step (t >= 1); returns the Philox blocks drawn and clears `alive`
// at a node without neighbours.  kTrials: whether the launch body adds those blocks up for
// trials_out.

struct StepFirstOrder {
    using Args = WalkArgs;
    using State = int32_t;  // cur
    static constexpr bool kTrials = false;
    const WalkArgs &a;
    __device__ __forceinline__ explicit StepFirstOrder(const WalkArgs &args) : a(args) {}
    __device__ __forceinline__ State begin(int32_t start) const { return start; }
    __device__ __forceinline__ int32_t node(const State &cur) const { return cur; }
    __device__ __forceinline__ uint32_t step(State &cur, int32_t start, uint32_t t, uint64_t gw,
                                             uint32_t k0, uint32_t k1, bool &alive) const {
        const int64_t b = a.rowptr[cur];
        const int64_t deg = a.rowptr[cur + 1] - b;
        if (deg <= 0) {  // graph_utils.py:44-45
            alive = false;
        } else {
            const Philox x = philox4x32_10(t, (uint32_t)gw, (uint32_t)(gw >> 32), 0u, k0, k1);
            if ((x.r[1] >> 8) >= a.restart_threshold) {  // rand.random() >= alpha (:39)
                // uniform neighbour (:40): multiply-shift of a 32-bit uniform, bias <= deg / 2^32
                const uint32_t pick = (uint32_t)(((uint64_t)x.r[0] * (uint64_t)deg) >> 32);
                cur = a.col[b + pick];
            } else {
                cur = start;  // restart (:42)
            }
        }
        return alive;  // one block, unless the walk ended
    }
};

template <bool W>
struct StepPq {
    using Args = WalkPqArgs;
    using State = PqWalk;
    static constexpr bool kTrials = true;
    const PqGraph g;
    const PqParams &pp;  // the kernel's own argument: pq_step reads its fields by value
    __device__ __forceinline__ explicit StepPq(const WalkPqArgs &a)
        : g{a.rowptr, a.col, W ? a.col : a.col_sorted, a.rowptr[a.V], W ? a.wcdf : nullptr},
          pp(a.pp) {}
    __device__ __forceinline__ State begin(int32_t start) const { return {start, -1, 0, 0}; }
    __device__ __forceinline__ int32_t node(const State &s) const { return s.cur; }
    __device__ __forceinline__ uint32_t step(State &s, int32_t start, uint32_t t, uint64_t gw,
                                             uint32_t k0, uint32_t k1, bool &alive) const {
        return pq_step<W>(g, pp, start, t, gw, k0, k1, s, alive);
    }
};

constexpr int WALK_BLOCK = 256;
constexpr int WALK_CHUNK = 16;  // 8 and 32 measured within 1% (profiles/r01i_ab_walks_staged.txt)

// The launch body of the three staged kernels.  A lane's row is L ints at a 4L-byte stride, so a
// store per lane per step (k_random_walks below) touches 64 cache lines per wavefront.  Here each
// lane fills a WALK_CHUNK-step slice of its row in LDS and the workgroup then writes the slice
// out as 64-B row segments, 16 lanes per segment.  Lanes past P or past a dead end keep going
// through the chunk loop (they emit -1) so every lane reaches the barriers.
// `a` by value, as the kernels take it, and the lane's state declared after `alive`: both decide
// the generated code (profiles/r17_walk_refactor.txt).
template <class Step>
__device__ __forceinline__ void walk_staged(const typename Step::Args a) {
    // +1: column writes hit distinct banks
    __shared__ alignas(Step::kTrials ? 8 : 4) int32_t tile[WALK_BLOCK][WALK_CHUNK + 1];
    const int tid = threadIdx.x;
    const int64_t w0 = (int64_t)blockIdx.x * WALK_BLOCK;
    const int64_t w = w0 + tid;
    const uint64_t gw = (uint64_t)(a.walk_offset + w);
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const Step step(a);
    int32_t start = -1;
    if (w < a.P) start = a.starts[w];
    bool alive = start >= 0 && start < a.V;  // not a node: an empty walk
    typename Step::State s = step.begin(alive ? start : -1);
    uint64_t trials = 0;
    const int64_t rows = a.P - w0 < WALK_BLOCK ? a.P - w0 : WALK_BLOCK;
    for (int c0 = 0; c0 < a.L; c0 += WALK_CHUNK) {
        const int cn = a.L - c0 < WALK_CHUNK ? a.L - c0 : WALK_CHUNK;
        for (int j = 0; j < cn; ++j) {
            const int t = c0 + j;
            if (alive && t > 0) trials += step.step(s, start, (uint32_t)t, gw, k0, k1, alive);
            tile[tid][j] = alive ? (a.emit ? a.emit[step.node(s)] : step.node(s)) : -1;
        }
        __syncthreads();
        // rows x cn slice -> global, consecutive lanes on consecutive columns of one row
        for (int i = tid; i < (int)rows * cn; i += WALK_BLOCK) {
            const int r = i / cn, j = i - r * cn;
            a.out[(w0 + r) * (int64_t)a.L + c0 + j] = tile[r][j];
        }
        __syncthreads();
    }
    if constexpr (Step::kTrials) {
        if (a.trials_out) {  // uniform: one LDS add per walk (the tile is free now), one global add
            unsigned long long *block_trials = (unsigned long long *)&tile[0][0];
            if (tid == 0) *block_trials = 0;
            __syncthreads();
            if (trials) atomicAdd(block_trials, (unsigned long long)trials);
            __syncthreads();
            if (tid == 0 && *block_trials) atomicAdd(a.trials_out, *block_trials);
        }
    }
}

__global__ void __launch_bounds__(WALK_BLOCK) k_random_walks_staged(WalkArgs a) {
    walk_staged<StepFirstOrder>(a);
}

__global__ void __launch_bounds__(WALK_BLOCK) k_random_walks_pq(WalkPqArgs a) {
    walk_staged<StepPq<false>>(a);
}

__global__ void __launch_bounds__(WALK_BLOCK) k_random_walks_w(WalkPqArgs a) {
    walk_staged<StepPq<true>>(a);
}

// The first-order walks again (same policy, same Philox counters), one store per lane per step
// and no LDS (walk_staged = 0): the structurally different kernel the staged one is tested against.
__global__ void __launch_bounds__(WALK_BLOCK) k_random_walks(WalkArgs a) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.P) return;
    int32_t *row = a.out + w * (int64_t)a.L;
    const int32_t start = a.starts[w];
    const uint64_t gw = (uint64_t)(a.walk_offset + w);
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    int t = 0;
    if (start < 0 || start >= a.V) {  // not a node: an empty walk
        for (; t < a.L; ++t) row[t] = -1;
        return;
    }
    const StepFirstOrder step(a);
    bool alive = true;
    int32_t cur = start;
    row[t++] = a.emit ? a.emit[cur] : cur;
    for (; t < a.L; ++t) {
        step.step(cur, start, (uint32_t)t, gw, k0, k1, alive);
        if (!alive) break;
        row[t] = a.emit ? a.emit[cur] : cur;
    }
    for (; t < a.L; ++t) row[t] = -1;
}

}  // namespace come

using namespace come;

template <class Args>
static int launch_walks(const void *kernel, const char *what, Args a, void *stream) {
    int dev = 0;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    const int64_t blocks = (a.P + WALK_BLOCK - 1) / WALK_BLOCK;
    if (blocks > INT32_MAX) return set_error(COME_E_INVALID, "too many walks in one launch");
    void *kargs[] = {&a};
    hipError_t e = hipLaunchKernel(kernel, dim3((unsigned)blocks), dim3(WALK_BLOCK), kargs, 0,
                                   (hipStream_t)stream);
    return hip_error(e, what);
}

extern "C" int come_random_walks(const int64_t *rowptr, const int32_t *col, int64_t V,
                                 const int32_t *starts, int64_t P, int L, float alpha,
                                 uint64_t seed, int64_t walk_offset, const int32_t *emit,
                                 int32_t *out, void *stream) {
    bool run;  // p = q = 1: in range
    int rc = walk_check_args("", V, P, L, walk_offset, alpha, 1.0f, 1.0f,
                             rowptr && col && starts && out, &run);
    if (rc || !run) return rc;
    // walk_staged: 1 = LDS-staged output (default), 0 = one store per lane per step
    const int staged = current_opts().walk_staged;
    if (staged != 0 && staged != 1)
        return set_error(COME_E_INVALID, "walk_staged must be 0 or 1 (got %d)", staged);
    const WalkArgs a{rowptr, col,         starts, emit, out, V,
                     P,      walk_offset, seed,   L,    walk_restart_threshold(alpha)};
    return launch_walks(staged ? (const void *)k_random_walks_staged : (const void *)k_random_walks,
                        "k_random_walks launch", a, stream);
}

extern "C" int come_random_walks_pq(const int64_t *rowptr, const int32_t *col,
                                    const int32_t *col_sorted, int64_t V, const int32_t *starts,
                                    int64_t P, int L, float alpha, float p, float q, uint64_t seed,
                                    int64_t walk_offset, const int32_t *emit, int32_t *out,
                                    uint64_t *trials_out, void *stream) {
    bool run;
    int rc = walk_check_args("", V, P, L, walk_offset, alpha, p, q,
                             rowptr && col && starts && out, &run);
    if (rc || !run) return rc;
    if (!col_sorted && pq_needs_sorted(p, q))
        return set_error(COME_E_INVALID, "col_sorted may be NULL only with q == 1 and p >= 1");
    const WalkPqArgs a{rowptr, col, {col_sorted}, starts, emit, out,
                       (unsigned long long *)trials_out, V, P, walk_offset, seed, L,
                       pq_make_params(alpha, p, q)};
    return launch_walks((const void *)k_random_walks_pq, "k_random_walks_pq launch", a, stream);
}

extern "C" int come_random_walks_w(const int64_t *rowptr, const int32_t *col,
                                   const uint32_t *wcdf, int64_t V, const int32_t *starts,
                                   int64_t P, int L, float alpha, float p, float q, uint64_t seed,
                                   int64_t walk_offset, const int32_t *emit, int32_t *out,
                                   uint64_t *trials_out, void *stream) {
    bool run;
    int rc = walk_check_args("", V, P, L, walk_offset, alpha, p, q,
                             rowptr && col && wcdf && starts && out, &run);
    if (rc || !run) return rc;
    WalkPqArgs a{rowptr, col, {nullptr}, starts, emit, out, (unsigned long long *)trials_out,
                 V, P, walk_offset, seed, L, pq_make_params(alpha, p, q)};
    a.wcdf = wcdf;
    return launch_walks((const void *)k_random_walks_w, "k_random_walks_w launch", a, stream);
}
