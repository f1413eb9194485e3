// come_community_loss.hip -- the community objective O3 (gfx950).
//
// Evaluates what Community2Vec.loss (community_embeddings.py:40-59) is meant to compute, the
// objective whose gradient come_community_grad follows:
//   row_i = sum_k pi[i][k] * (c_k - |x_i P_k - mu_k P_k|^2 / 2),   total = sum_i row_i
// with P_k the upper precision Cholesky factor and c_k = log det P_k - d/2 log(2 pi): the E-step's
// stream of log-densities (come_gmm_estep.hip) with a constant that carries no mixture weight, a
// pi-weighted running sum in place of the log-sum-exp, and no V x K output.
//   k_comm_loss_b16   d = 64, 128 with 16-byte aligned operands: k_gmm_resp_b16's MFMA stream over
//                     the same bf16-part images (come_resp_b16.h)
//   k_comm_loss_valu  any other d <= 512, or unaligned operands (rows of P_k streamed in chunks)
//   k_comm_loss_sum   the workgroups' partial sums into the total
// No float or double atomics: every workgroup adds its rows in a fixed order into one double,
// k_comm_loss_sum adds the doubles in a fixed order, so the total and the rows are bit-identical
// from run to run.

#include "come_c4.h"
#include "come_resp_b16.h"

namespace come {

struct LossArgs {
    const float *x;
    const float *pi;
    const float *prec_chol;
    const float *mu_prec;
    const float *log_norm;
    const char *img;  // MFMA path: prec_chol as k_pack_upper_b16's images
    float *row_out;   // optional [V]
    double *partial;  // [gridDim.x]
    int64_t V;
    int d;
    int K;
};

// k_gmm_resp_b16's body (one 16-row tile per wavefront, 8 wavefronts per 128-row workgroup, the
// row's bf16 parts formed once, a component staged in two units with global_load_lds) with the
// loss's epilogue: lane (row j, group kg) adds pi[row][k] * lp to its running fp32 sum for its
// components, the four sums of a row are added in a fixed order at the end.
template <int D>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4)))
    k_comm_loss_b16(LossArgs a) {
    using R = RespB16<D>;
    using f32x4 = __attribute__((ext_vector_type(4))) float;
    typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
    extern __shared__ __attribute__((aligned(16))) char smb[];
    constexpr R TB{};
    float *rowv = reinterpret_cast<float *>(smb + R::LDS_BYTES);  // [128] the workgroup's rows
    const int tid = threadIdx.x;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int j = lane & 15, kg = lane >> 4;
    const int64_t row = (int64_t)blockIdx.x * 128 + wid * 16 + j;
    const bool rowok = row < a.V;
    const int nt = a.K * R::NU;
    // unit t -> buffer b; a component's first unit also brings its mu_k P_k and c_k
    auto stage = [&](int64_t t, int b) {
        const char *src = a.img + t * R::UBYTES + 16 * lane;
#pragma unroll
        for (int q = 0; q < (R::PIECES + R::NW - 1) / R::NW; ++q) {
            const int i = wid + R::NW * q;
            if (R::PIECES % R::NW != 0 && i >= R::PIECES) break;  // wavefront-uniform
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const float *>(src + i * 1024),
                                             reinterpret_cast<float *>(smb + b * R::UBYTES + i * 1024),
                                             16, 0, 0);
        }
        if (t % R::NU == 0) {
            const int64_t k = t / R::NU;
            float *par = reinterpret_cast<float *>(smb + R::PAR) + (k & 1) * R::PARF;
            if (wid == 0) {
                const int s = lane * 4 < D ? lane * 4 : D - 4;
                __builtin_amdgcn_global_load_lds(a.mu_prec + k * D + s, par, 16, 0, 0);
            } else if (wid == 1) {
                __builtin_amdgcn_global_load_lds(a.log_norm + k, par + 256, 4, 0, 0);
            }
        }
    };
    stage(0, 0);
    if (nt > 1) stage(1, 1);
    // the row's parts, once: xp[s][P] = part P of features 32 s + 8 kg .. + 7
    bf16x8 xp[R::NS][3];
#pragma unroll
    for (int s = 0; s < R::NS; ++s) {
        uint32_t w[3][4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x4 v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (rowok) v = *reinterpret_cast<const f32x4 *>(a.x + row * D + 32 * s + 8 * kg + 4 * u);
            bf16_split3(v[0], v[1], w[0][2 * u], w[1][2 * u], w[2][2 * u]);
            bf16_split3(v[2], v[3], w[0][2 * u + 1], w[1][2 * u + 1], w[2][2 * u + 1]);
        }
#pragma unroll
        for (int P = 0; P < 3; ++P)
            xp[s][P] = __builtin_bit_cast(bf16x8, uint4{w[P][0], w[P][1], w[P][2], w[P][3]});
    }
    const int aoff = R::at(0, j, kg);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // A row's four lanes (group kg) take the components k with k % 4 == kg.  The lane's weight
    // for components 4 g .. 4 g + 3 is loaded while group g - 1 computes, four components (some
    // 480 MFMAs at d = 128) ahead of its use: no lane waits on a 4-byte strided load per component.
    // The loads take a wavefront-uniform base and a 32-bit lane offset clamped into the
    // workgroup's rows of pi: a clamped load is of a weight that is never used (a component
    // >= K, or a row >= V whose sum is dropped), so no load sits under a branch.
    const float *pib = a.pi + (int64_t)blockIdx.x * 128 * a.K;
    const int64_t left = (a.V - (int64_t)blockIdx.x * 128) * a.K;  // floats from pib to pi's end
    const int plast = (int)(left < (int64_t)128 * a.K ? left : (int64_t)128 * a.K) - 1;
    const int poff = (wid * 16 + j) * a.K + kg;
    float p_cur = 0.0f, p_nxt = pib[poff < plast ? poff : plast];
    float run = 0.0f;
    for (int k = 0; k < a.K; ++k) {
        if ((k & 3) == 0) {
            p_cur = p_nxt;
            p_nxt = pib[poff + k + 4 < plast ? poff + k + 4 : plast];
        }
        const float *par = reinterpret_cast<const float *>(smb + R::PAR) + (k & 1) * R::PARF;
        float sq = 0.0f;
        f32x4 acc[R::CT];
#pragma unroll
        for (int u = 0; u < R::NU; ++u) {
            const int t = k * R::NU + u;
            const char *ub = smb + (u & 1) * R::UBYTES;  // t & 1
#pragma unroll
            for (int bi = 0; bi < R::UB; ++bi) {
                const int b = u * R::UB + bi, ct = TB.ct[b], s = TB.s[b];
                const char *base = ub + bi * R::BLK + aoff;
                bf16x8 A[3];
#pragma unroll
                for (int P = 0; P < 3; ++P) A[P] = *reinterpret_cast<const bf16x8 *>(base + P * 1024);
                const f32x4 c0 = s == 0 ? f32x4{0.0f, 0.0f, 0.0f, 0.0f} : acc[ct];
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[2], xp[s][0], c0, 0, 0, 0);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[1], xp[s][1], acc[ct], 0, 0, 0);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], xp[s][2], acc[ct], 0, 0, 0);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[1], xp[s][0], acc[ct], 0, 0, 0);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], xp[s][1], acc[ct], 0, 0, 0);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], xp[s][0], acc[ct], 0, 0, 0);
                if (s == ct / 2) {  // tile ct complete: columns 16 ct + 4 kg + r
                    const f32x4 mp = *reinterpret_cast<const f32x4 *>(par + 16 * ct + 4 * kg);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float y = acc[ct][r] - mp[r];
                        sq = __builtin_fmaf(y, y, sq);
                    }
                }
            }
            if (t + 1 < nt) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();  // buffer t & 1 free; unit t + 1 (and its parameters) in LDS
                if (t + 2 < nt) stage(t + 2, u & 1);
            }
        }
        // the reduction leaves the row's sum of squares in all four of its lanes
        const float lp = par[256] - 0.5f * reduce_stage<5>(reduce_stage<4>(sq));
        if ((k & 3) == kg) run += p_cur * lp;
    }
    // (kg 0 + kg 1) + (kg 2 + kg 3), in every lane of the row
    const float rv = reduce_stage<5>(reduce_stage<4>(run));
    if (kg == 0) {
        rowv[wid * 16 + j] = rowok ? rv : 0.0f;
        if (rowok && a.row_out) a.row_out[row] = rv;
    }
    __syncthreads();
    if (wid == 0) {  // 128 rows -> one double: pairs (l, l + 64), then the xor butterfly
        double s = (double)rowv[lane] + (double)rowv[lane + 64];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) a.partial[blockIdx.x] = s;
    }
}

// VALU form: TR rows per workgroup, 256 / TR lanes per row, lane l of a row holding columns
// l, l + TPR, ... of y = x P_k in registers (d <= TPR * NACC) while the rows of P_k pass through
// LDS in chunks of chunk_rows(d) (k_gmm_resp_wide's staging; one chunk up to d = 127).  fmaf chains
// in j order as k_gmm_resp; a row's squares are summed per lane in column order and then over the
// row's lanes by the xor butterfly -- no LDS atomics, so the order is fixed.
template <int TR, int NACC>
__global__ void __launch_bounds__(kThreads) k_comm_loss_valu(LossArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int TPR = kThreads / TR;
    const int d = a.d, CH = chunk_rows(d), LDM = d + 1;
    float *X = smem;           // [TR][d]
    float *M = X + TR * d;     // [CH][d + 1] rows j0 .. j0 + CH of prec_chol[k]
    float *RV = M + CH * LDM;  // [TR]
    const int r = threadIdx.x / TPR, l = threadIdx.x % TPR;
    const int64_t r0 = (int64_t)blockIdx.x * TR;
    const int rows = (int)((a.V - r0) < TR ? (a.V - r0) : TR);
    for (int o = threadIdx.x; o < TR * d; o += kThreads)
        X[o] = o / d < rows ? a.x[(r0 + o / d) * d + (o % d)] : 0.0f;
    const bool rowok = r < rows;
    float run = 0.0f;
    for (int k = 0; k < a.K; ++k) {
        float y[NACC];
#pragma unroll
        for (int i = 0; i < NACC; ++i) y[i] = 0.0f;
        for (int j0 = 0; j0 < d; j0 += CH) {
            const int jn = d - j0 < CH ? d - j0 : CH;
            __syncthreads();
            for (int o = threadIdx.x; o < jn * d; o += kThreads)
                M[(o / d) * LDM + o % d] = a.prec_chol[(int64_t)k * d * d + (int64_t)j0 * d + o];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NACC; ++i) {
                const int c = l + TPR * i;
                if (c < d) {
                    float acc = y[i];
                    for (int j = 0; j < jn; ++j)
                        acc = __builtin_fmaf(X[r * d + j0 + j], M[j * LDM + c], acc);
                    y[i] = acc;
                }
            }
        }
        float sq = 0.0f;
#pragma unroll
        for (int i = 0; i < NACC; ++i) {
            const int c = l + TPR * i;
            if (c < d) {
                const float t = y[i] - a.mu_prec[(int64_t)k * d + c];
                sq = __builtin_fmaf(t, t, sq);
            }
        }
#pragma unroll
        for (int o = TPR / 2; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
        const float lp = a.log_norm[k] - 0.5f * sq;
        if (rowok) run += a.pi[(r0 + r) * a.K + k] * lp;
    }
    if (l == 0) {
        RV[r] = rowok ? run : 0.0f;
        if (rowok && a.row_out) a.row_out[r0 + r] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < TR; ++i) s += (double)RV[i];
        a.partial[blockIdx.x] = s;
    }
}

// total = the partials added in a fixed order: thread t takes t, t + 256, ... in order, then a tree
// over the 256 threads
__global__ void __launch_bounds__(256) k_comm_loss_sum(const double *__restrict__ partial,
                                                       int64_t n, double *__restrict__ out) {
    __shared__ double s[256];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) v += partial[i];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

}  // namespace come

using namespace come;

extern "C" int come_community_loss(const float *x, int64_t V, int d, const float *pi,
                                   const float *prec_chol, const float *mu_prec,
                                   const float *log_norm, int K, float *row_out, double *loss_out,
                                   void *stream) {
    if (V < 0 || d < 1 || d > kMaxDim || K < 1 || K > 4096)
        return set_error(COME_E_INVALID, "community_loss: need V>=0, 1<=d<=%d, 1<=K<=4096",
                         kMaxDim);
    if (V == 0) return COME_OK;
    if (!x || !pi || !prec_chol || !mu_prec || !log_norm || !loss_out)
        return set_error(COME_E_INVALID, "community_loss: null pointer");
    int dev;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    const bool mfma = (d == 64 || d == 128) && ((uintptr_t)x % 16) == 0 &&
                      ((uintptr_t)prec_chol % 16) == 0 && ((uintptr_t)mu_prec % 16) == 0;
    const int tile = mfma ? 128 : (d <= 128 ? 16 : kTRW);
    const int64_t blocks = (V + tile - 1) / tile;
    if (blocks > INT32_MAX) return set_error(COME_E_INVALID, "community_loss: V too large");
    double *partial = (double *)stream_scratch(dev, stream, kScratchLossPartial,
                                               sizeof(double) * (size_t)blocks);
    if (!partial) return scratch_failed();
    LossArgs a{x, pi, prec_chol, mu_prec, log_norm, nullptr, row_out, partial, V, d, K};
    if (mfma) {
        rc = with_width(d, [&](auto width) {
            constexpr int D = decltype(width)::value;
            using R = RespB16<D>;
            // the E-step's image slot: launches on one stream are ordered, so the two never overlap
            char *img = (char *)stream_scratch(dev, stream, kScratchRespSplit,
                                               (size_t)K * R::NB * R::BLK);
            if (!img) return scratch_failed();
            const int64_t work = (int64_t)K * R::NB * 64;
            int rc = launch(dev, k_pack_upper_b16<D>, "k_pack_upper_b16 launch",
                            dim3((unsigned)std::min<int64_t>((work + 255) / 256, 4096)), dim3(256),
                            {0}, stream, prec_chol, img, K);
            if (rc) return rc;
            a.img = img;
            return launch(dev, k_comm_loss_b16<D>, "k_comm_loss_b16 launch",
                          dim3((unsigned)blocks), dim3(512), {R::LDS_BYTES + 128 * sizeof(float)},
                          stream, a);
        });
    } else {
        const size_t floats = (size_t)tile * d + (size_t)chunk_rows(d) * (d + 1) + tile;
        rc = d <= 128 ? launch(dev, k_comm_loss_valu<16, 8>, "k_comm_loss_valu launch",
                               dim3((unsigned)blocks), dim3(kThreads), {sizeof(float) * floats},
                               stream, a)
                      : launch(dev, k_comm_loss_valu<kTRW, 16>, "k_comm_loss_valu launch",
                               dim3((unsigned)blocks), dim3(kThreads), {sizeof(float) * floats},
                               stream, a);
    }
    if (rc) return rc;
    return launch(dev, k_comm_loss_sum, "k_comm_loss_sum launch", dim3(1), dim3(256), {0}, stream,
                  (const double *)partial, blocks, loss_out);
}
