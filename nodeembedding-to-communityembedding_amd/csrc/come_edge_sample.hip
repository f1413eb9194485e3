// come_edge_sample.hip -- edge sampling by weight on the device (gfx950), in front of the
// unchanged O1 kernels: the global edge CDF (k_edge_max, k_edge_tile_totals, k_edge_scan_totals,
// k_edge_tile_scan) and the sampler over it (k_edge_sample).
//
// The arithmetic is come_edge_sample.h's (cdf_units of come_walk_pq.h, edge_r64, edge_pick), shared
// with the CPU twins in come_cpu.cpp, so CDF words, sampled rows and indices are the host's bit for
// bit.
//
// come_edge_cdf.  ecdf[i] = the exact uint64 prefix sum of u_j = llrint(w_j / wmax * 2^32).  Four
// launches on the caller's stream, each reading only what an EARLIER launch wrote -- no workgroup
// ever waits on another (no look-back, no flags):
//   k_edge_max          grid-stride: validity and the largest weight (one atomicMax per wavefront
//                       on the weight's bits -- order-free; non-negative floats order as integers)
//   k_edge_tile_totals  one workgroup per tile of EDGE_TILE = 2048 edges: the tile's sum of units,
//                       stored in the tile's LAST slot of ecdf (its final value is written there
//                       by the next launch, so the output array is the only scratch)
//   k_edge_scan_totals  ONE workgroup: the inclusive scan of those slots, 256 tiles per round with
//                       the carry in a register; a tile's last slot then holds its final sum
//   k_edge_tile_scan    one workgroup per tile: rescan of the tile's units from the carry in the
//                       previous tile's last slot; writes every slot but the tile's last, so no
//                       slot is read and written in the same launch
// A one-off pass per graph (per pass with down-sampling): 3 reads of the weights, 8 B written per
// edge.
//
// k_edge_sample.  One lane per sample, 256-lane workgroups: one Philox block, one 64 x 64 -> high
// 64 multiply, about log2(E) dependent 8-byte reads of ecdf (the top levels of the search are the
// same few lines for every lane and stay in L2), one 8-byte gather of the edge row, one coalesced
// 8-byte store (plus 8 B of index when asked for).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "come_edge_sample.h"
#include "come_internal.h"

namespace come {

constexpr int EDGE_BLOCK = 256;
constexpr int EDGE_ITEMS = 8;  // consecutive edges per lane in the tile kernels
constexpr int EDGE_TILE = EDGE_BLOCK * EDGE_ITEMS;
constexpr int EDGE_MAX_BLOCKS = 2048;  // k_edge_max grid-strides beyond this

__device__ inline int64_t tile_last(int64_t t, int64_t E) {
    const int64_t end = (t + 1) * EDGE_TILE;
    return (end < E ? end : E) - 1;
}

// Inclusive scan of v over the workgroup's 256 lanes; *total: the workgroup's sum.  Every lane
// must call it; two barriers.
__device__ inline uint64_t block_scan_u64(uint64_t v, uint64_t *wsum, uint64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = __shfl_up((unsigned long long)v, off, 64);
        if (lane >= off) v += o;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (int i = 0; i < EDGE_BLOCK / 64; ++i) {
        const uint64_t s = wsum[i];
        before += i < wave ? s : 0u;
        all += s;
    }
    __syncthreads();  // wsum may be rewritten by the next call
    *total = all;
    return v + before;
}

__global__ void __launch_bounds__(EDGE_BLOCK) k_edge_max(const float *__restrict__ w, int64_t E,
                                                         uint32_t *__restrict__ wmax_bits,
                                                         int32_t *__restrict__ status) {
    float m = 0.0f;
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * EDGE_BLOCK + threadIdx.x; i < E;
         i += (int64_t)gridDim.x * EDGE_BLOCK) {
        const float x = w[i];
        bad |= !cdf_weight_ok(x);
        m = x > m ? x : m;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
        bad |= __shfl_xor(bad, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad) *status = 1;  // a plain (vector) store: every writer writes the same word
        if (m > 0.0f) atomicMax(wmax_bits, __float_as_uint(m));
    }
}

// The units of this lane's EDGE_ITEMS consecutive edges of tile t (0 past E); returns their sum.
__device__ inline uint64_t lane_units(const float *w, int64_t E, int64_t t, float wmax,
                                      uint64_t u[EDGE_ITEMS]) {
    const int64_t i0 = t * EDGE_TILE + (int64_t)threadIdx.x * EDGE_ITEMS;
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < EDGE_ITEMS; ++j) {
        u[j] = i0 + j < E ? cdf_units(w[i0 + j], wmax) : 0u;
        sum += u[j];
    }
    return sum;
}

__global__ void __launch_bounds__(EDGE_BLOCK)
    k_edge_tile_totals(const float *__restrict__ w, int64_t E,
                       const uint32_t *__restrict__ wmax_bits, int32_t *__restrict__ status,
                       uint64_t *__restrict__ ecdf) {
    __shared__ uint64_t wsum[EDGE_BLOCK / 64];
    const float wmax = __uint_as_float(*wmax_bits);
    if (!(wmax > 0.0f)) {  // only zeros (or nothing valid): every workgroup leaves
        if (blockIdx.x == 0 && threadIdx.x == 0) *status = 1;
        return;
    }
    if (*status) return;  // k_edge_max's verdict: uniform over the grid
    uint64_t u[EDGE_ITEMS], total;
    block_scan_u64(lane_units(w, E, blockIdx.x, wmax, u), wsum, &total);
    if (threadIdx.x == 0) ecdf[tile_last(blockIdx.x, E)] = total;
}

__global__ void __launch_bounds__(EDGE_BLOCK)
    k_edge_scan_totals(int64_t E, int64_t tiles, const int32_t *__restrict__ status,
                       uint64_t *__restrict__ ecdf) {
    __shared__ uint64_t wsum[EDGE_BLOCK / 64];
    if (*status) return;
    uint64_t carry = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += EDGE_BLOCK) {  // uniform trip count
        const int64_t t = t0 + threadIdx.x;
        const int64_t at = t < tiles ? tile_last(t, E) : 0;
        uint64_t total;
        const uint64_t incl = block_scan_u64(t < tiles ? ecdf[at] : 0u, wsum, &total);
        if (t < tiles) ecdf[at] = carry + incl;
        carry += total;
    }
}

__global__ void __launch_bounds__(EDGE_BLOCK)
    k_edge_tile_scan(const float *__restrict__ w, int64_t E,
                     const uint32_t *__restrict__ wmax_bits, const int32_t *__restrict__ status,
                     uint64_t *__restrict__ ecdf) {
    __shared__ uint64_t wsum[EDGE_BLOCK / 64];
    if (*status) return;
    const float wmax = __uint_as_float(*wmax_bits);
    const int64_t t = blockIdx.x;
    const int64_t last = tile_last(t, E);  // final since k_edge_scan_totals: not written here
    const uint64_t carry = t > 0 ? ecdf[t * EDGE_TILE - 1] : 0u;  // the previous tile's last slot
    uint64_t u[EDGE_ITEMS], total;
    const uint64_t mine = lane_units(w, E, t, wmax, u);
    uint64_t U = carry + block_scan_u64(mine, wsum, &total) - mine;
    const int64_t i0 = t * EDGE_TILE + (int64_t)threadIdx.x * EDGE_ITEMS;
#pragma unroll
    for (int j = 0; j < EDGE_ITEMS; ++j) {
        U += u[j];
        if (i0 + j < last) ecdf[i0 + j] = U;
    }
}

__global__ void __launch_bounds__(EDGE_BLOCK)
    k_edge_sample(const int2 *__restrict__ edges, const uint64_t *__restrict__ ecdf, int64_t E,
                  int64_t S, uint64_t seed, int64_t sample_offset, int2 *__restrict__ out,
                  int64_t *__restrict__ index_out) {
    const int64_t s = (int64_t)blockIdx.x * EDGE_BLOCK + threadIdx.x;
    if (s >= S) return;
    const uint64_t r64 = edge_r64((uint64_t)(sample_offset + s), (uint32_t)seed,
                                  (uint32_t)(seed >> 32));
    const int64_t pick = edge_pick(ecdf, E, r64);  // in [0, E)
    out[s] = edges[pick];
    if (index_out) index_out[s] = pick;
}

}  // namespace come

using namespace come;

extern "C" int come_edge_cdf(const float *weights, int64_t E, uint64_t *ecdf_out, int32_t *status,
                             void *stream) {
    if (E <= 0 || E > INT32_MAX) return set_error(COME_E_INVALID, "E must be in [1, 2^31)");
    if (!weights || !ecdf_out || !status) return set_error(COME_E_INVALID, "edge_cdf: null pointer");
    int dev = 0;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint32_t *wmax_bits = (uint32_t *)stream_scratch(dev, stream, kScratchEdgeWmax, sizeof(uint32_t));
    if (!wmax_bits) return scratch_failed();
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return hip_error(e, "edge_cdf status memset");
    e = hipMemsetAsync(wmax_bits, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return hip_error(e, "edge_cdf maximum memset");
    const int64_t tiles = (E + EDGE_TILE - 1) / EDGE_TILE;  // < 2^20
    const int64_t mblocks = (E + EDGE_BLOCK - 1) / EDGE_BLOCK;
    hipLaunchKernelGGL(k_edge_max,
                       dim3((unsigned)(mblocks < EDGE_MAX_BLOCKS ? mblocks : EDGE_MAX_BLOCKS)),
                       dim3(EDGE_BLOCK), 0, st, weights, E, wmax_bits, status);
    hipLaunchKernelGGL(k_edge_tile_totals, dim3((unsigned)tiles), dim3(EDGE_BLOCK), 0, st, weights,
                       E, (const uint32_t *)wmax_bits, status, ecdf_out);
    hipLaunchKernelGGL(k_edge_scan_totals, dim3(1), dim3(EDGE_BLOCK), 0, st, E, tiles,
                       (const int32_t *)status, ecdf_out);
    hipLaunchKernelGGL(k_edge_tile_scan, dim3((unsigned)tiles), dim3(EDGE_BLOCK), 0, st, weights, E,
                       (const uint32_t *)wmax_bits, (const int32_t *)status, ecdf_out);
    return hip_error(hipGetLastError(), "k_edge_cdf launches");
}

extern "C" int come_edge_sample(const int32_t *edges, const uint64_t *ecdf, int64_t E, int64_t S,
                                uint64_t seed, int64_t sample_offset, int32_t *out,
                                int64_t *index_out, void *stream) {
    if (E <= 0 || E > INT32_MAX) return set_error(COME_E_INVALID, "E must be in [1, 2^31)");
    if (S < 0 || sample_offset < 0)
        return set_error(COME_E_INVALID, "S and sample_offset must be >= 0");
    if (S == 0) return COME_OK;
    if (!edges || !ecdf || !out) return set_error(COME_E_INVALID, "edge_sample: null pointer");
    if (((uintptr_t)edges | (uintptr_t)out) & 7u)
        return set_error(COME_E_INVALID, "edge_sample: edges and out must be 8-byte aligned");
    int dev = 0;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    const int64_t blocks = (S + EDGE_BLOCK - 1) / EDGE_BLOCK;
    if (blocks > INT32_MAX) return set_error(COME_E_INVALID, "too many samples in one launch");
    hipLaunchKernelGGL(k_edge_sample, dim3((unsigned)blocks), dim3(EDGE_BLOCK), 0,
                       (hipStream_t)stream, (const int2 *)edges, ecdf, E, S, seed, sample_offset,
                       (int2 *)out, index_out);
    return hip_error(hipGetLastError(), "k_edge_sample launch");
}
