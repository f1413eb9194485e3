// come_sgns_o1.h -- the O1 (edge) trainer kernels: k_sgns_o1 and k_sgns_o1_runs (the input row
// held over runs of edges).  Execution model: come_sgns_common.h.
#pragma once
#include "come_sgns_common.h"

namespace come {

// ---- O1: one wavefront per edge ------------------------------------------------------------
struct O1Args {
    float *node;
    const int32_t *edges;
    const uint64_t *seeds;
    const uint32_t *table;
    int64_t V;
    int64_t E;
    int d;
    int negative;
    float lr;
    FastMod fm;
    int packed;
    const uint32_t *hot;  // HOG, optional: contended rows (come_hot_rows), updated atomically
    int64_t chunk;        // k_sgns_o1_runs: consecutive edges per wavefront unit
};

// The targets of edge e = (u, v): its 2n draws -- pair 1 uses draws 0..n-1, pair 2 draws n..2n-1
// (state carried, pyx:444-448) -- and for each pair the rows t[k] with valid[k] (a draw equal to
// the pair's positive is skipped as in the reference, one outside [0, V) so that nothing is read
// out of bounds).
template <int MAXN>
__device__ inline void o1_targets(const O1Args &a, const LcgLane &lc, int64_t e, int u, int v,
                                  int (&t1)[MAXN + 1], int (&t2)[MAXN + 1], bool (&v1)[MAXN + 1],
                                  bool (&v2)[MAXN + 1]) {
    const int n = a.negative;
    DrawBatch db;
    db.used = 0;
    db.base = uniform64(a.seeds[e]);
    db.target = 0;
    if (n > 0) draws_fill(db, db.base, lc, a, 2 * n);  // only the 2n draws the edge uses
    t1[0] = v;  // pair 1: input u, positive v (pyx:444)
    t2[0] = u;  // pair 2: input v, positive u (pyx:447)
    v1[0] = v2[0] = true;
#pragma unroll
    for (int k = 1; k <= MAXN; ++k) {
        if (k <= n) {
            t1[k] = (int)readlane_u32(db.target, k - 1);
            t2[k] = (int)readlane_u32(db.target, n + k - 1);
            v1[k] = t1[k] != v && t1[k] >= 0 && t1[k] < a.V;
            v2[k] = t2[k] != u && t2[k] >= 0 && t2[k] < a.V;
        } else {
            t1[k] = t2[k] = -1;
            v1[k] = v2[k] = false;
        }
    }
}

// One O1 pair (pyx:225-245): the dots of the input row `in` against the positive r[0] and the
// negatives r[1..n] (entries with !valid[k] skipped), and `work`, the pair's change of the input
// row.  O1 updates no target row, so every dot is against the rows as gathered; the caller applies
// in += work (pyx:247).
template <int VEC, bool FULL, int MAXN>
__device__ inline void o1_pair(const Row<VEC, FULL> &in, const Row<VEC, FULL> (&r)[MAXN + 1],
                               const bool (&valid)[MAXN + 1], int n, float lr,
                               Row<VEC, FULL> &work) {
    float part[MAXN + 1];
#pragma unroll
    for (int k = 0; k <= MAXN; ++k) part[k] = valid[k] ? lane_partial(in, r[k]) : 0.0f;
    wave_sum_n(part, n + 1);
#pragma unroll
    for (int q = 0; q < VEC; ++q) work.v[q] = 0.0f;
#pragma unroll
    for (int k = 0; k <= MAXN; ++k) {
        if (!valid[k]) continue;
        float sig;
        if (!sigmoid_tab(c_exp_table, uniformf(part[k]), &sig)) continue;
        const float g = ((k == 0 ? 1.0f : 0.0f) - sig) * lr;  // pyx:243
#pragma unroll
        for (int q = 0; q < VEC; ++q) work.v[q] = __builtin_fmaf(g, r[k].v[q], work.v[q]);
    }
}

template <int VEC, bool FULL, int MAXN>
__global__ void __launch_bounds__(256) k_sgns_o1(O1Args a) {
    using R = Row<VEC, FULL>;
    const int lane = threadIdx.x & 63;
    const int64_t waves_per_block = blockDim.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * waves_per_block;
    const LcgLane lc = lcg_lane_constants(lane);
    const int n = a.negative;
    const int d = a.d;

    for (int64_t e = gw; e < a.E; e += nwaves) {
        const int u = uniform(a.edges[2 * e]);
        const int v = uniform(a.edges[2 * e + 1]);
        if (u < 0 || u >= a.V || v < 0 || v >= a.V) continue;  // reference: undefined behaviour
        int t1[MAXN + 1], t2[MAXN + 1];
        bool v1[MAXN + 1], v2[MAXN + 1];
        o1_targets<MAXN>(a, lc, e, u, v, t1, t2, v1, v2);
        // Every row both pairs read can be gathered up front: pair 1 writes only node[u]; pair 2
        // never reads node[u] through a negative (skipped, == its positive) and gets its positive
        // (and, for a self-loop, its input) forwarded from pair 1's registers.
        R in1, in2;
        in1.load(a.node + (int64_t)u * d, lane, d);
        if (v != u) in2.load(a.node + (int64_t)v * d, lane, d);
        const bool hot_u = is_hot(a, u), hot_v = is_hot(a, v);
        R r1[MAXN + 1], r2[MAXN + 1];
#pragma unroll
        for (int k = 1; k <= MAXN; ++k) {
            if (v1[k]) r1[k].load(a.node + (int64_t)t1[k] * d, lane, d);
            if (v2[k]) r2[k].load(a.node + (int64_t)t2[k] * d, lane, d);
        }
        if (v != u) r1[0] = in2; else r1[0] = in1;  // positive of pair 1 = node[v] (pre-update)

        // pair 1
        {
            R work;
            o1_pair<VEC, FULL, MAXN>(in1, r1, v1, n, a.lr, work);
#pragma unroll
            for (int q = 0; q < VEC; ++q) in1.v[q] = in1.v[q] + work.v[q];  // pyx:247
            if (hot_u) work.atomic_add(a.node + (int64_t)u * d, lane, d);
            else in1.store(a.node + (int64_t)u * d, lane, d);
        }
        // pair 2: positive = node[u] as pair 1 left it; self-loop: the input is that row too.
        r2[0] = in1;
        if (v == u) in2 = in1;
        {
            R work;
            o1_pair<VEC, FULL, MAXN>(in2, r2, v2, n, a.lr, work);
#pragma unroll
            for (int q = 0; q < VEC; ++q) in2.v[q] = in2.v[q] + work.v[q];
            if (hot_v) work.atomic_add(a.node + (int64_t)v * d, lane, d);
            else in2.store(a.node + (int64_t)v * d, lane, d);
        }
    }
}

// O1 with the input row held over runs of edges (a.chunk > 0; option o1_chunk): a wavefront takes
// `chunk` consecutive edges and processes them in order, as one of the reference's worker
// threads does with its job of consecutive edges (node_embeddings.py:58-95).  Edge lists come
// grouped by their first endpoint (G.edges() order: all (u, *) of a node together), so the
// wavefront keeps node[u] in registers for the run of edges sharing u -- read once, updated by
// every pair-1 of the run (pyx:444: input u) and read as pair 2's positive (pyx:447) -- and writes
// it back once when u changes or the chunk ends: a float-atomic delta of the run's updates if u is
// contended, else a plain store.  A contended u's delta also goes out before the second update of
// a self-loop (u, u), so that edge's two changes reach memory as two adds in order, exactly as
// k_sgns_o1 sends them (tests/test_gpu_o1_hogwild.py: edges that share no row are bit-identical to
// the sequential order under either kernel).  Any target row equal to the held u is taken from
// the registers.
// One wavefront in sequential mode: bit-identical to k_sgns_o1 (the held row is what memory holds).
// Wavefronts per SIMD the run kernel is compiled for: latency-bound like the stream kernel (one
// edge's rows in flight per wavefront), so at d <= 128, n <= 5 it is held to 64 VGPRs (a 12-byte
// prologue spill) for 8 waves per SIMD and launched 8 four-wave workgroups per CU: C2 at lr 0.1
// 1.161 vs 1.277 ms per pass at its natural 79 VGPRs / 6 waves (7 waves: 1.186 ms;
// profiles/r05_ab_o1_waves.txt).
template <int VEC, int MAXN>
constexpr int o1_runs_waves_per_eu() {
    return (VEC <= 2 && MAXN <= 5) ? 8 : 1;
}

template <int VEC, bool FULL, int MAXN>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(o1_runs_waves_per_eu<VEC, MAXN>())))
    k_sgns_o1_runs(O1Args a) {
    using R = Row<VEC, FULL>;
    const int lane = threadIdx.x & 63;
    const int64_t waves_per_block = blockDim.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * waves_per_block;
    const LcgLane lc = lcg_lane_constants(lane);
    const int n = a.negative;
    const int d = a.d;
    const int64_t nchunks = (a.E + a.chunk - 1) / a.chunk;

    for (int64_t c = gw; c < nchunks; c += nwaves) {
        const int64_t e0 = c * a.chunk;
        const int64_t e1 = e0 + a.chunk < a.E ? e0 + a.chunk : a.E;
        int cu = -1;        // the held row (wave-uniform), -1 = none
        bool hot_cu = false;
        R hu, du;           // its value and this run's change
        auto flush = [&]() {
            if (cu < 0) return;
            if (hot_cu) du.atomic_add(a.node + (int64_t)cu * d, lane, d);
            else hu.store(a.node + (int64_t)cu * d, lane, d);
        };
        for (int64_t e = e0; e < e1; ++e) {
            const int u = uniform(a.edges[2 * e]);
            const int v = uniform(a.edges[2 * e + 1]);
            if (u < 0 || u >= a.V || v < 0 || v >= a.V) continue;  // reference: undefined
            if (u != cu) {
                flush();
                cu = u;
                hot_cu = is_hot(a, u);
                hu.load(a.node + (int64_t)u * d, lane, d);
#pragma unroll
                for (int q = 0; q < VEC; ++q) du.v[q] = 0.0f;
            }
            int t1[MAXN + 1], t2[MAXN + 1];
            bool v1[MAXN + 1], v2[MAXN + 1];
            o1_targets<MAXN>(a, lc, e, u, v, t1, t2, v1, v2);
            R in2;
            if (v != u) in2.load(a.node + (int64_t)v * d, lane, d);
            const bool hot_v = is_hot(a, v);
            R r1[MAXN + 1], r2[MAXN + 1];
#pragma unroll
            for (int k = 1; k <= MAXN; ++k) {
                if (v1[k]) {
                    if (t1[k] == u) r1[k] = hu;  // the held row (pair 1's input, pre-update)
                    else r1[k].load(a.node + (int64_t)t1[k] * d, lane, d);
                }
                if (v2[k] && t2[k] != v) r2[k].load(a.node + (int64_t)t2[k] * d, lane, d);
            }
            r1[0] = v != u ? in2 : hu;  // pair 1's positive node[v] (pre-update)
            // pair 1: input = the held u
            {
                R work;
                o1_pair<VEC, FULL, MAXN>(hu, r1, v1, n, a.lr, work);
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    hu.v[q] = hu.v[q] + work.v[q];  // pyx:247
                    du.v[q] = du.v[q] + work.v[q];
                }
            }
            // pair 2: input v, positive = the held u as pair 1 left it; a self-loop's input is
            // that row too; a negative equal to v reads v before pair 2's update
            r2[0] = hu;
            if (v == u) in2 = hu;
#pragma unroll
            for (int k = 1; k <= MAXN; ++k)
                if (v2[k] && t2[k] == v) r2[k] = in2;
            {
                R work;
                o1_pair<VEC, FULL, MAXN>(in2, r2, v2, n, a.lr, work);
                if (v == u) {  // self-loop: pair 2 updates the held row itself
                    // a contended row gets the self-loop's two changes as two atomics in order,
                    // as k_sgns_o1 sends them (a run of one edge writes what that kernel writes):
                    // the delta so far goes out now and pair 2's change starts the next one
                    if (hot_cu) flush();
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        hu.v[q] = hu.v[q] + work.v[q];
                        du.v[q] = hot_cu ? work.v[q] : du.v[q] + work.v[q];
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) in2.v[q] = in2.v[q] + work.v[q];
                    if (hot_v) work.atomic_add(a.node + (int64_t)v * d, lane, d);
                    else in2.store(a.node + (int64_t)v * d, lane, d);
                }
            }
        }
        flush();
    }
}

}  // namespace come
