// come_c4.h -- what the C4 kernels share (gfx950): argument blocks, the bf16-part arithmetic,
// launch constants and the entry points' launch path (launch, with_width).  Included by
// come_community.hip (community step), come_gmm_estep.hip (GMM responsibilities),
// come_gmm_scatter.hip (M-step scatter matrices), come_gmm_params.hip (M-step parameters) and
// come_kmeans.hip (the launch path).  A tuning constant lives in the shape struct that uses it,
// beside the measurement that chose it; A/B builds go through scripts/build_ab.sh.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <math.h>
#include <mutex>
#include <set>
#include <stdint.h>
#include <type_traits>
#include <utility>

#include "come_internal.h"
#include "come_wave.h"

namespace come {

constexpr int kTR = 16;        // rows per workgroup tile
constexpr int kThreads = 256;

// ---- the entry points' launch path ------------------------------------------------------------
// Dynamic LDS of a launch and the limit its kernel is allowed (default: the CU's whole 160 KB).
struct Lds {
    size_t bytes;
    int limit = 160 * 1024;
};

// Raises kern's dynamic-LDS limit the first time it is asked to on `dev` (the entry points are
// re-entrant: the set of what is done is mutex-guarded).
inline int raise_lds_limit(int dev, const void *kern, int limit, const char *what) {
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (raised.count({kern, dev})) return COME_OK;
    const int rc = hip_error(
        hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, limit), what);
    if (rc == COME_OK) raised.insert({kern, dev});
    return rc;
}

// Launches kern(args...) on `stream` and returns the launch's status (`what` heads the error
// text).  A kernel launched with dynamic LDS gets its limit raised first (raise_lds_limit).
template <typename... P, typename... A>
inline int launch(int dev, void (*kern)(P...), const char *what, dim3 grid, dim3 block, Lds lds,
                  void *stream, const A &...args) {
    if (lds.bytes > 0) {
        const int rc = raise_lds_limit(dev, (const void *)kern, lds.limit, what);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(kern, grid, block, lds.bytes, (hipStream_t)stream, args...);
    return hip_error(hipGetLastError(), what);
}

// f(std::integral_constant<int, D>{}) for the MFMA kernels' runtime width d, D in {64, 128}
template <typename F>
inline int with_width(int d, F &&f) {
    if (d == 64) return f(std::integral_constant<int, 64>{});
    return f(std::integral_constant<int, 128>{});
}

// out[r][c] = sum_j A[r][j] * B(c, j) for the tile, where B(c, j) = Bm[c*d + j] (TRANS=false,
// i.e. B used as M @ a) or Bm[j*d + c] (TRANS=true, i.e. a @ B).  A and Bm live in LDS.
template <bool TRANS>
__device__ inline float tile_dot(const float *A, const float *Bm, int r, int c, int d) {
    float acc = 0.0f;
    if (TRANS) {
        for (int j = 0; j < d; ++j) acc = __builtin_fmaf(A[r * d + j], Bm[j * d + c], acc);
    } else {
        for (int j = 0; j < d; ++j) acc = __builtin_fmaf(A[r * d + j], Bm[c * d + j], acc);
    }
    return acc;
}

struct CommArgs {
    float *x;
    const float *pi;
    const float *mu;
    const float *inv_cov;
    int64_t V;
    int d;
    int K;
    float coef;  // (float)(beta / K), community_embeddings.py:77 (numpy weak-scalar cast)
    float lr;
    int iters;
    const void *img;  // k_community_b16: inv_cov as k_comm_split16's bf16 part images
};

struct RespArgs {
    const float *x;
    const float *prec_chol;
    const float *mu_prec;
    const float *log_norm;
    float *resp;
    float *lse;  // optional [V]: log sum_k exp(weighted log prob) per row (EM's log-likelihood)
    int64_t V;
    int d;
    int K;
    const int *lower;  // MFMA path: [K], 1 if prec_chol[k] has a non-zero below the diagonal
    const float *prec_t;  // MFMA path: the upper factors packed (k_pack_upper16 / k_pack_upper_b16)
    const float *prec_full;  // MFMA path: [K][d][d] prec_chol[k] transposed (k_transpose_sq), which
                             // k_gmm_resp16_full reads
};

// ---- fp32 operands as bf16 parts: the arithmetic of the C4 default kernels --------------------
//
// Every fp32 operand v is carried as three bf16 parts, v1 = bf16(v), v2 = bf16(v - v1), v3 =
// bf16(v - v1 - v2): each difference is exact in fp32 and |v - v1 - v2 - v3| <= 2^-27 |v|.  A
// product a b is taken as its six part products of order <= 2 (a3 b1 + a2 b2 + a1 b3 + a2 b1 +
// a1 b2 + a1 b1; the three dropped are below 2^-26 |a b|), each exact in fp32, summed by the MFMA
// in fp32: the result carries fp32-level error (tests hold it to the fp32 kernels' tolerances),
// not a reduced-precision one.  A 16x16x32 block costs six v_mfma_f32_16x16x32_bf16 (6 x 16
// cycles) instead of eight v_mfma_f32_16x16x4_f32 (8 x 32): 2.67x the fp32 MFMA rate.
// bf16 part arithmetic on packed pairs (element 0 in the low half)
__device__ __forceinline__ uint32_t bf16_pk(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ float bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
// (lo, hi) -> the packed first, second and third parts
__device__ __forceinline__ void bf16_split3(float lo, float hi, uint32_t &p1, uint32_t &p2,
                                            uint32_t &p3) {
    // (the empty asm hides where p1 and p2 came from: otherwise the compiler recomputes their
    // low halves with another v_cvt_pk_bf16_f32 instead of one shift)
    p1 = bf16_pk(lo, hi);
    asm("" : "+v"(p1));
    const float l2 = lo - bf16_lo(p1), h2 = hi - bf16_hi(p1);
    p2 = bf16_pk(l2, h2);
    asm("" : "+v"(p2));
    p3 = bf16_pk(l2 - bf16_lo(p2), h2 - bf16_hi(p2));
}

// ---- wide rows (128 < d <= 512): VALU forms with the d x d matrices streamed in row chunks ----
// The MFMA kernels above keep a whole d x d matrix (or a 128-row tile of inputs) in LDS, which
// stops at d = 128.  These forms cover every d up to kMaxDim: kTRW rows per workgroup, each
// component's matrix staged kChunkRows(d) rows at a time (<= 64 KiB, rows padded by one float
// against bank conflicts).  Same arithmetic as k_community_grad / k_gmm_resp (fmaf chains in j
// order), a fraction of the MFMA rate: they exist so that every embedding size the SGNS kernels
// accept also trains through the community step (community_embeddings.py:61-78) and the GMM.
constexpr int kTRW = 8;
__host__ __device__ inline int chunk_rows(int d) { return 16384 / (d + 1); }

}  // namespace come
