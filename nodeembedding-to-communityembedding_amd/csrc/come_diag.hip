// come_diag.hip -- diagonal-covariance communities (gfx950): the GMM E-step, the two M-step passes,
// the community step and the community loss for covariances diag(var_k).
//
// Per (row, component, feature) these are two or three fp32 VALU operations over one read of x: no
// d x d matrix and no LDS staging of the components.  Every 1 <= d <= 512 takes the same kernels.
//   k_diag_pack     prec_sqrt / mu_prec as one padded, interleaved image (the E-step's and the
//                   loss's wave-uniform operand: read with scalar loads, any operand alignment)
//   k_diag_dist     the shared body, one row per lane with 128 features of it in registers:
//                   sq[k] = sum_j (x_j ps_kj - mp_kj)^2 for eight components at a time, then the
//                   E-step's epilogue (log-probabilities parked in resp_out, running log-sum-exp,
//                   a second pass that normalises them) or the loss's (a pi-weighted running sum)
//   k_diag_moments  nk and resp^T X for one row chunk: a plain matrix product, on the exact fp32
//                   MFMA (two rows per instruction, 64 components x 128 features per wavefront)
//   k_diag_scatter  the centred sum_i r_ik (x_ij - mean_kj)^2 for one row chunk: lanes over 64
//                   features, KT components in registers, the weights broadcast from LDS
//   k_diag_reduce   the chunks' fp32 partials added in chunk order in float64
//   k_diag_grad     the community step: lanes over features, RB rows per wavefront sharing every
//                   read of mu_k / inv_var_k, all `iters` steps in registers
//   k_diag_loss_sum the workgroups' float64 partial sums into the total (k_comm_loss_sum's tree)
// No float or double atomics: every sum has a fixed order, so all outputs are bit-identical from
// run to run.

#include "come_c4.h"

namespace come {

constexpr int kDgFeat = 128;  // features of a row one lane holds
constexpr int kDgKB = 8;      // components per batch of k_diag_dist
constexpr int kDgPiece = 32;  // features per staging piece; the image's d is padded to it

__host__ __device__ inline int dg_dpad(int d) { return (d + kDgPiece - 1) / kDgPiece * kDgPiece; }

// img[k][j] = (prec_sqrt[k][j], -mu_prec[k][j]) for j < d, (0, -0) up to dpad: a padded feature
// adds (x * 0 - 0)^2 = 0.
__global__ void __launch_bounds__(256) k_diag_pack(const float *__restrict__ ps,
                                                   const float *__restrict__ mp,
                                                   float *__restrict__ img, int K, int d, int dpad) {
    const int64_t n = (int64_t)K * dpad;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (int64_t)gridDim.x * 256) {
        const int64_t k = o / dpad;
        const int j = (int)(o % dpad);
        float a = 0.0f, b = 0.0f;
        if (j < d) {
            a = ps[k * d + j];
            b = mp[k * d + j];
        }
        img[2 * o] = a;
        img[2 * o + 1] = -b;
    }
}

// A workgroup is four wavefronts; a row's features are split over NCH of them (128 each), so it
// holds 256 / NCH rows, one per lane.  The partial squares of a batch of components meet in LDS
// (two buffers, one barrier per batch) and are added in chunk order by the row's first wavefront,
// which runs the epilogue.
//   LOSS = false: out_a = resp_out [V x K] or NULL, out_b = lse_out [V]
//   LOSS = true:  out_a = row_out [V] or NULL, partial[blockIdx.x] = the workgroup's rows, float64
template <int NCH, bool LOSS>
__global__ void __launch_bounds__(256)
    k_diag_dist(const float *__restrict__ x, const float *__restrict__ img,
                const float *__restrict__ log_norm, const float *__restrict__ pi,
                float *__restrict__ out_a, float *__restrict__ out_b, double *__restrict__ partial,
                int64_t V, int d, int dpad, int K) {
    constexpr int RG = 4 / NCH;  // row groups (of 64 rows) per workgroup
    constexpr int LDST = kDgPiece + 1;
    __shared__ float stg[4][64 * LDST];
    __shared__ float ex[NCH > 1 ? 2 * 4 * kDgKB * 64 : 1];
    __shared__ float rowv[LOSS ? 64 * RG : 1];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rg = w / NCH, c = w % NCH;
    const int64_t r0 = ((int64_t)blockIdx.x * RG + rg) * 64;
    const int64_t row = r0 + lane;
    const bool rowok = row < V;
    const int fbase = c * kDgFeat;

    // the lane's 128 features, through LDS in pieces of 32 (coalesced reads of x, any alignment)
    float xr[kDgFeat];
    float *st = stg[w];
    const float *xb = x + r0 * d;  // (a wavefront whose rows are all past V stages nothing real)
#pragma unroll
    for (int p = 0; p < kDgFeat / kDgPiece; ++p) {
        const int f0 = fbase + kDgPiece * p;
        __syncthreads();
        if (f0 < d) {  // clamped addresses, no load under a branch: 16 loads in flight together
#pragma unroll
            for (int h = 0; h < kDgPiece; h += 16) {
                float v[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int idx = (h + i) * 64 + lane;
                    const int rr = idx >> 5, cc = idx & 31;
                    const int rw = r0 + rr < V ? rr : (int)(V - 1 - r0);
                    const int fc = f0 + cc < d ? f0 + cc : d - 1;
                    v[i] = xb[rw * d + fc];
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int idx = (h + i) * 64 + lane;
                    const int rr = idx >> 5, cc = idx & 31;
                    st[rr * LDST + cc] = (r0 + rr < V && f0 + cc < d) ? v[i] : 0.0f;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kDgPiece; ++j) xr[kDgPiece * p + j] = f0 < d ? st[lane * LDST + j] : 0.0f;
    }

    float m = -INFINITY, s = 0.0f, run = 0.0f;
    const int nb = (K + kDgKB - 1) / kDgKB;
    for (int kb = 0; kb < nb; ++kb) {
        float sq[kDgKB];
#pragma unroll
        for (int kk = 0; kk < kDgKB; ++kk) {
            const int k = kb * kDgKB + kk;
            const int kc = k < K ? k : K - 1;  // a component past K repeats the last one, unused
            const float *o = img + ((int64_t)kc * dpad + fbase) * 2;
            float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
            for (int p = 0; p < kDgFeat / kDgPiece; ++p) {
                if (fbase + kDgPiece * p < dpad) {  // wavefront-uniform
#pragma unroll
                    for (int j = 0; j < kDgPiece; j += 2) {
                        const int f = kDgPiece * p + j;
                        const float t0 = __builtin_fmaf(xr[f], o[2 * f], o[2 * f + 1]);
                        const float t1 = __builtin_fmaf(xr[f + 1], o[2 * f + 2], o[2 * f + 3]);
                        a0 = __builtin_fmaf(t0, t0, a0);
                        a1 = __builtin_fmaf(t1, t1, a1);
                    }
                }
            }
            sq[kk] = a0 + a1;
        }
        if (NCH > 1) {
            float *buf = ex + (kb & 1) * (4 * kDgKB * 64);
#pragma unroll
            for (int kk = 0; kk < kDgKB; ++kk) buf[(w * kDgKB + kk) * 64 + lane] = sq[kk];
            __syncthreads();
            if (c == 0) {
#pragma unroll
                for (int kk = 0; kk < kDgKB; ++kk) {
                    float t = buf[((rg * NCH) * kDgKB + kk) * 64 + lane];
#pragma unroll
                    for (int q = 1; q < NCH; ++q) t += buf[((rg * NCH + q) * kDgKB + kk) * 64 + lane];
                    sq[kk] = t;
                }
            }
        }
        if (c == 0 && rowok) {
#pragma unroll
            for (int kk = 0; kk < kDgKB; ++kk) {
                const int k = kb * kDgKB + kk;
                if (k < K) {
                    const float lp = log_norm[k] - 0.5f * sq[kk];
                    if (LOSS) {
                        run += pi[row * K + k] * lp;
                    } else {
                        if (out_a) out_a[row * K + k] = lp;
                        const float mn = fmaxf(m, lp);
                        if (mn > -INFINITY) {
                            s = s * __expf(m - mn) + __expf(lp - mn);
                            m = mn;
                        }
                    }
                }
            }
        }
    }
    if (LOSS) {
        if (c == 0) {
            rowv[rg * 64 + lane] = rowok ? run : 0.0f;
            if (rowok && out_a) out_a[row] = run;
        }
        __syncthreads();
        if (w == 0) {  // 64 RG rows -> one double: the groups in order, then the xor butterfly
            double t = 0.0;
#pragma unroll
            for (int g = 0; g < RG; ++g) t += (double)rowv[g * 64 + lane];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == 0) partial[blockIdx.x] = t;
        }
    } else if (c == 0 && rowok) {
        const float lse = s > 0.0f ? m + logf(s) : -INFINITY;
        out_b[row] = lse;
        if (out_a) {  // the lane's own log-probabilities, back from where it parked them
            for (int k = 0; k < K; ++k) {
                const float lp = out_a[row * K + k];
                out_a[row * K + k] = lse > -INFINITY ? __expf(lp - lse) : 0.0f;
            }
        }
    }
}

// One row chunk's centred scatter sum_i r_ik (x_ij - mean_kj)^2 for components k0 .. k0 + KT - 1
// and features 64 z .. 64 z + 63 (the centring is per component, so this is no matrix product).
// The chunk passes in tiles of 32 rows: the tile's weights [32][KT] go through LDS (coalesced
// loads one tile ahead, read back as broadcasts), wavefront w adds rows 8 w .. 8 w + 7 of every
// tile, in row order, into its lanes' KT fp32 sums (lane = feature); the four wavefronts' sums are
// added in wavefront order.  A row past the chunk has weight 0.  direct: the chunk is the whole
// input and the sums go to the float64 output itself.
template <int KT>
__global__ void __launch_bounds__(256)
    k_diag_scatter(const float *__restrict__ x, const float *__restrict__ resp,
                   const float *__restrict__ means, float *__restrict__ part,
                   double *__restrict__ out, int64_t V, int64_t per, int d, int K, int direct) {
    using f32x4 = __attribute__((ext_vector_type(4))) float;
    constexpr int TR = 32, WR = TR / 4;  // rows of a tile, of a wavefront's share of it
    constexpr int TILE = TR * KT;        // floats of one tile of weights
    constexpr int NQ = TILE / 256;       // weights a thread stages per tile
    __shared__ __attribute__((aligned(16))) float sm[4 * KT * 64];  // two tiles; then the sums
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = blockIdx.x;
    const int k0 = blockIdx.y * KT;
    const int kn = K - k0 < KT ? K - k0 : KT;
    const int j = blockIdx.z * 64 + lane;
    const int jc = j < d ? j : d - 1;
    const int64_t lo = (int64_t)chunk * per;
    const int64_t hi = lo + per < V ? lo + per : V;
    const int ntiles = (int)((hi - lo + TR - 1) / TR);
    float acc[KT], mk[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
        acc[kk] = 0.0f;
        mk[kk] = means[(int64_t)(k0 + (kk < kn ? kk : kn - 1)) * d + jc];
    }
    float rq[NQ], xq[WR];
    auto fetch = [&](int t) {  // tile t: the thread's weights and its wavefront's WR x values
        const int64_t t0 = lo + (int64_t)t * TR;
        const int left = (int)(hi - t0 < TR ? hi - t0 : TR);  // rows of the tile, >= 1
        const float *rb = resp + t0 * K + k0, *xb = x + t0 * d;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int idx = q * 256 + threadIdx.x;
            const int rr = idx / KT, kk = idx % KT;
            const float v = rb[(rr < left ? rr : left - 1) * K + (kk < kn ? kk : kn - 1)];
            rq[q] = (rr < left && kk < kn) ? v : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < WR; ++r) {
            const int rr = WR * w + r < left ? WR * w + r : left - 1;
            xq[r] = xb[rr * d + jc];
        }
    };
    auto stage = [&](int b) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) sm[b * TILE + q * 256 + threadIdx.x] = rq[q];
    };
    fetch(0);
    stage(0);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        float xc[WR];
#pragma unroll
        for (int r = 0; r < WR; ++r) xc[r] = xq[r];
        if (t + 1 < ntiles) fetch(t + 1);
        const float *tile = sm + (t & 1) * TILE + WR * w * KT;
#pragma unroll
        for (int r = 0; r < WR; ++r) {
            // (the sums are pinned after each row: otherwise the compiler issues the broadcast
            // reads of all rows first, holds 8 rows of weights in registers and, at KT = 32,
            // fills the register file)
            if (r > 0) {
#pragma unroll
                for (int kk = 0; kk < KT; ++kk) asm volatile("" : "+v"(acc[kk]));
            }
#pragma unroll
            for (int q = 0; q < KT / 4; ++q) {
                const f32x4 rr = *reinterpret_cast<const f32x4 *>(tile + r * KT + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kk = 4 * q + e;
                    const float u = xc[r] - mk[kk];
                    acc[kk] = __builtin_fmaf(rr[e], u * u, acc[kk]);
                }
            }
        }
        if (t + 1 < ntiles) stage((t + 1) & 1);
        __syncthreads();  // tile t + 1 is in LDS; every wavefront is done with tile t
    }
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) sm[(w * KT + kk) * 64 + lane] = acc[kk];
    __syncthreads();
    for (int o = threadIdx.x; o < KT * 64; o += 256) {
        const int kk = o >> 6, l = o & 63;
        const int jj = blockIdx.z * 64 + l;
        if (kk >= kn || jj >= d) continue;
        const float v = ((sm[(0 * KT + kk) * 64 + l] + sm[(1 * KT + kk) * 64 + l]) +
                         sm[(2 * KT + kk) * 64 + l]) + sm[(3 * KT + kk) * 64 + l];
        if (direct)
            out[(int64_t)(k0 + kk) * d + jj] = (double)v;
        else
            part[((int64_t)chunk * K + k0 + kk) * d + jj] = v;
    }
}

// One row chunk's moments, nk = sum_i r_ik and sx = sum_i r_ik x_ij, for components k0 .. k0 +
// 32 KT - 1 and features 128 z .. 128 z + 127: resp^T X is a matrix product, taken on
// v_mfma_f32_32x32x2_f32 (an exact fp32 fmaf chain in row order, no reduced precision).  A
// wavefront's instruction adds two rows: lane l = (h, c) holds resp[row + h][k0 + 32 kt + c] as
// the A operand of component tile kt and, as the B operands of the four feature tiles, the 16
// bytes x[row + h][j0 + 4 c .. + 3] -- one fully coalesced load of the row's 512 bytes, tile t's
// column c being feature j0 + 4 c + t (WIDE: x 16-byte aligned and d % 4 == 0; otherwise the same
// four values by 4-byte loads).  KT = 2 covers K <= 64 with one read of x.  The four wavefronts
// take the chunk's row pairs round robin; a wavefront keeps two sets of four pairs in flight, the
// loads of one set issued before the MFMAs of the other.  Their sums are added in wavefront order
// through LDS.  nk: every lane adds the weights it loads, the two halves of the wavefront and then
// the wavefronts are added in order.
template <int KT, bool WIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
    k_diag_moments(const float *__restrict__ x, const float *__restrict__ resp,
                   float *__restrict__ part, float *__restrict__ part_nk,
                   double *__restrict__ out, double *__restrict__ nk_out, int64_t V, int64_t per,
                   int d, int K, int direct) {
    using f32x16 = __attribute__((ext_vector_type(16))) float;
    using f32x4 = __attribute__((ext_vector_type(4))) float;
    __shared__ float red[KT * 4 * 16 * 64];
    __shared__ float rednk[KT * 32];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = blockIdx.x;
    const int k0 = blockIdx.y * 32 * KT, j0 = blockIdx.z * 128;
    const int c = lane & 31, h = lane >> 5;
    uint32_t kmask[KT];  // all ones for a component < K
    int kc[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        const bool kok = k0 + 32 * kt + c < K;
        kmask[kt] = kok ? 0xffffffffu : 0u;
        kc[kt] = kok ? k0 + 32 * kt + c : K - 1;
    }
    int jc[4];  // WIDE: jc[0] only, the start of a whole quad inside the row
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = j0 + 4 * c + t;
        jc[t] = WIDE ? (j0 + 4 * c < d ? j0 + 4 * c : d - 4) : (j < d ? j : d - 1);
    }
    const int64_t lo = (int64_t)chunk * per;
    const int64_t hi = lo + per < V ? lo + per : V;
    const int64_t npairs = (hi - lo + 1) / 2;
    f32x16 acc[KT][4];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kt][t][r] = 0.0f;
    float nkl[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) nkl[kt] = 0.0f;
    struct Set {
        uint32_t a[4][KT], m[4][KT];  // the weights as loaded, and their masks
        f32x4 b[4];
    };
    // pairs p, p + 4, p + 8, p + 12; a row past the chunk: weight 0 on the chunk's last row
    auto load = [&](Set &s, int64_t p) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t row = lo + 2 * (p + 4 * u) + h;
            const bool ok = row < hi;
            const int64_t rc = ok ? row : hi - 1;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                // (masked at its use, not selected here: a select puts the load under a branch
                // with its own wait, and a mask applied here waits for the load before the
                // other set's MFMAs: either way the pairs' loads complete one after the other)
                s.a[u][kt] = __float_as_uint(resp[rc * K + kc[kt]]);
                s.m[u][kt] = ok ? kmask[kt] : 0u;
            }
            if (WIDE) {
                s.b[u] = *reinterpret_cast<const f32x4 *>(x + rc * d + jc[0]);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) s.b[u][t] = x[rc * d + jc[t]];
            }
        }
    };
    auto mma = [&](const Set &s) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const float a = __uint_as_float(s.a[u][kt] & s.m[u][kt]);
                nkl[kt] += a;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[kt][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, s.b[u][t], acc[kt][t], 0,
                                                                      0, 0);
            }
    };
    Set s0, s1;
    load(s0, w);
    for (int64_t p = w; p < npairs; p += 32) {
        // (the fences keep a set's loads together and ahead of the other set's MFMAs: left to
        // itself the scheduler sinks each load to its use and waits for it there)
        load(s1, p + 16);  // (past the chunk's end: zero weights)
        __builtin_amdgcn_sched_barrier(0);
        mma(s0);
        __builtin_amdgcn_sched_barrier(0);
        load(s0, p + 32);
        __builtin_amdgcn_sched_barrier(0);
        mma(s1);
        __builtin_amdgcn_sched_barrier(0);
    }
    for (int ww = 0; ww < 4; ++ww) {
        if (w == ww) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int o = ((kt * 4 + t) * 16 + r) * 64 + lane;
                        red[o] = ww == 0 ? acc[kt][t][r] : red[o] + acc[kt][t][r];
                    }
                const float nkw = nkl[kt] + __shfl_xor(nkl[kt], 32);  // even rows, then odd rows
                if (lane < 32) {
                    const int o = kt * 32 + lane;
                    rednk[o] = ww == 0 ? nkw : rednk[o] + nkw;
                }
            }
        }
        __syncthreads();
    }
    // register r of lane (hh, cc) of tile (kt, t): component 32 kt + (r & 3) + 8 (r >> 2) + 4 hh,
    // feature 4 cc + t; the threads walk the features of a component in order
    for (int o = threadIdx.x; o < KT * 32 * 128; o += 256) {
        const int f = o & 127, kl = o >> 7;  // kl: component within the group
        const int kt = kl >> 5, kr = kl & 31;
        const int r = (kr & 3) + 4 * (kr >> 3), hh = (kr >> 2) & 1;
        const int kk = k0 + kl, jj = j0 + f;
        if (kk >= K || jj >= d) continue;
        const float v = red[((kt * 4 + (f & 3)) * 16 + r) * 64 + hh * 32 + (f >> 2)];
        if (direct)
            out[(int64_t)kk * d + jj] = (double)v;
        else
            part[((int64_t)chunk * K + kk) * d + jj] = v;
    }
    if (blockIdx.z == 0 && (int)threadIdx.x < KT * 32 && k0 + (int)threadIdx.x < K) {
        if (direct)
            nk_out[k0 + threadIdx.x] = (double)rednk[threadIdx.x];
        else
            part_nk[(int64_t)chunk * K + k0 + threadIdx.x] = rednk[threadIdx.x];
    }
}

// out[e] = sum over the chunks, in chunk order, of part[c][e], in float64; elements n .. n + n2 - 1
// are those of a second table, part2 [chunks][n2] into out2 (the moments' nk beside sx).  Sixteen
// chunks' loads are in flight per thread, the additions stay in chunk order.
__global__ void __launch_bounds__(64) k_diag_reduce(const float *__restrict__ part,
                                                    const float *__restrict__ part2, int chunks,
                                                    int64_t n, int64_t n2, double *__restrict__ out,
                                                    double *__restrict__ out2) {
    int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (e >= n + n2) return;
    const float *src = part;
    double *dst = out;
    int64_t stride = n;
    if (e >= n) {
        e -= n;
        src = part2;
        dst = out2;
        stride = n2;
    }
    double s = 0.0;
    int c = 0;
    for (; c + 16 <= chunks; c += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = src[(int64_t)(c + u) * stride + e];
#pragma unroll
        for (int u = 0; u < 16; ++u) s += (double)v[u];
    }
    for (; c < chunks; ++c) s += (double)src[(int64_t)c * stride + e];
    dst[e] = s;
}

// Lane l of a wavefront holds features l, l + 64, ... (NF of them) of RB rows; a component's mu
// and inv_var are read once per wavefront and serve the RB rows, pi[row][k] is wavefront-uniform.
// G += pi * (inv_var * (x - mu)) in the reference's order, the update as k_community_grad's.
template <int NF, int RB>
__global__ void __launch_bounds__(256)
    k_diag_grad(float *__restrict__ x, const float *__restrict__ pi, const float *__restrict__ mu,
                const float *__restrict__ iv, int64_t V, int d, int K, float coef, float lr,
                int iters) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + w) * RB;
    if (r0 >= V) return;
    float xr[RB][NF], g[RB][NF];
    int jc[NF];
#pragma unroll
    for (int s = 0; s < NF; ++s) jc[s] = lane + 64 * s < d ? lane + 64 * s : d - 1;
    const float *pr[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int64_t row = r0 + r < V ? r0 + r : V - 1;  // a row past V repeats the last, unstored
        pr[r] = pi + row * K;
#pragma unroll
        for (int s = 0; s < NF; ++s) xr[r][s] = x[row * d + jc[s]];
    }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int s = 0; s < NF; ++s) g[r][s] = 0.0f;
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            float m[NF], v[NF];
#pragma unroll
            for (int s = 0; s < NF; ++s) {
                m[s] = mu[(int64_t)k * d + jc[s]];
                v[s] = iv[(int64_t)k * d + jc[s]];
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const float p = pr[r][k];
#pragma unroll
                for (int s = 0; s < NF; ++s)
                    g[r][s] = __builtin_fmaf(p, v[s] * (xr[r][s] - m[s]), g[r][s]);
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int s = 0; s < NF; ++s) {
                float t = g[r][s] * coef;
                t = t < -5.0f ? -5.0f : (t > 5.0f ? 5.0f : t);
                xr[r][s] = xr[r][s] - t * lr;
            }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int s = 0; s < NF; ++s)
            if (r0 + r < V && lane + 64 * s < d) x[(r0 + r) * d + lane + 64 * s] = xr[r][s];
}

// k_comm_loss_sum's fixed tree: thread t takes t, t + 256, ... in order, then a tree over 256
__global__ void __launch_bounds__(256) k_diag_loss_sum(const double *__restrict__ partial,
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

static int dg_check(const char *what, int64_t V, int d, int K) {
    if (V < 0 || d < 1 || d > kMaxDim || K < 1 || K > 4096)
        return set_error(COME_E_INVALID, "%s: need V>=0, 1<=d<=%d, 1<=K<=4096", what, kMaxDim);
    return COME_OK;
}

// The image of (prec_sqrt, mu_prec) for launches on `stream`, or nullptr.
static const float *dg_image(int dev, void *stream, const float *ps, const float *mp, int K, int d,
                             int *rc) {
    const int dpad = dg_dpad(d);
    float *img = stream_scratch(dev, stream, kScratchDiagImage, sizeof(float) * 2 * (size_t)K * dpad);
    if (!img) {
        *rc = scratch_failed();
        return nullptr;
    }
    const int64_t n = (int64_t)K * dpad;
    *rc = launch(dev, k_diag_pack, "k_diag_pack launch",
                 dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), {0}, stream, ps,
                 mp, img, K, d, dpad);
    return *rc ? nullptr : img;
}

template <bool LOSS>
static int dg_dist(int dev, void *stream, const float *x, const float *img, const float *log_norm,
                   const float *pi, float *out_a, float *out_b, double *partial, int64_t V, int d,
                   int K, int nch) {
    const int dpad = dg_dpad(d);
    const dim3 grid((unsigned)((V + 256 / nch - 1) / (256 / nch)));
    if (nch == 1)
        return launch(dev, k_diag_dist<1, LOSS>, "k_diag_dist launch", grid, dim3(256), {0}, stream,
                      x, img, log_norm, pi, out_a, out_b, partial, V, d, dpad, K);
    if (nch == 2)
        return launch(dev, k_diag_dist<2, LOSS>, "k_diag_dist launch", grid, dim3(256), {0}, stream,
                      x, img, log_norm, pi, out_a, out_b, partial, V, d, dpad, K);
    return launch(dev, k_diag_dist<4, LOSS>, "k_diag_dist launch", grid, dim3(256), {0}, stream, x,
                  img, log_norm, pi, out_a, out_b, partial, V, d, dpad, K);
}

static int dg_nch(int d) { return d <= kDgFeat ? 1 : (d <= 2 * kDgFeat ? 2 : 4); }

constexpr int kDgKT = 32;       // components per workgroup of k_diag_scatter (8 when K <= 8)
constexpr int kDgKTSmall = 8;
static int dg_kt(int K) { return K <= kDgKTSmall ? kDgKTSmall : kDgKT; }

static void dg_plan(int64_t V, int d, int K, int cus, int *chunks, int64_t *rows) {
    if (cus <= 0) cus = 256;
    const int kt = dg_kt(K);
    const int64_t groups = (int64_t)((K + kt - 1) / kt) * ((d + 63) / 64);
    // eight workgroups per CU over the chunks; partials (K d + K floats per chunk) <= 128 MB; a
    // chunk has at least 64 rows
    const int64_t cap = std::max<int64_t>(
        1, std::min<int64_t>((int64_t(128) << 20) / (4 * ((int64_t)K * d + K)), (V + 63) / 64));
    int64_t c = std::max<int64_t>(1, std::min<int64_t>((8 * (int64_t)cus + groups - 1) / groups, cap));
    *chunks = (int)c;
    *rows = std::max<int64_t>(1, (V + c - 1) / c);
}

template <bool SCATTER>
static int dg_mstep(const char *what, const float *x, int64_t V, int d, const float *resp,
                    const float *means, int K, int chunks, void *scratch, double *nk_out,
                    double *out, void *stream) {
    int rc = dg_check(what, V, d, K);
    if (rc) return rc;
    if (chunks < 1 || (int64_t)chunks * ((int64_t)K * d + K) * 4 > (int64_t(128) << 20))
        return set_error(COME_E_INVALID, "%s: chunks must be >= 1 with chunks * (K d + K) * 4 <= "
                                         "128 MB (got %d; see come_gmm_diag_scratch)", what, chunks);
    if (!out || (!SCATTER && !nk_out) || (SCATTER && !means))
        return set_error(COME_E_INVALID, "%s: null pointer", what);
    if (V > 0 && (!x || !resp)) return set_error(COME_E_INVALID, "%s: null pointer", what);
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    const int64_t n = (int64_t)K * d;
    if (V == 0) {
        rc = hip_error(hipMemsetAsync(out, 0, sizeof(double) * n, (hipStream_t)stream), what);
        if (!rc && !SCATTER)
            rc = hip_error(hipMemsetAsync(nk_out, 0, sizeof(double) * K, (hipStream_t)stream), what);
        return rc;
    }
    const int64_t per = (V + chunks - 1) / chunks;
    const int used = (int)((V + per - 1) / per);
    if (used > 1 && !scratch) return set_error(COME_E_INVALID, "%s: null scratch", what);
    const int direct = used == 1;
    float *part = (float *)scratch;
    float *part_nk = direct ? nullptr : part + (int64_t)used * n;
    if (SCATTER) {
        const int kt = dg_kt(K);
        const dim3 grid((unsigned)used, (unsigned)((K + kt - 1) / kt), (unsigned)((d + 63) / 64));
        rc = kt == kDgKTSmall
                 ? launch(dev, k_diag_scatter<kDgKTSmall>, "k_diag_scatter launch", grid, dim3(256),
                          {0}, stream, x, resp, means, part, out, V, per, d, K, direct)
                 : launch(dev, k_diag_scatter<kDgKT>, "k_diag_scatter launch", grid, dim3(256), {0},
                          stream, x, resp, means, part, out, V, per, d, K, direct);
    } else {
        const bool wide = ((uintptr_t)x % 16) == 0 && d % 4 == 0;
        const int kt = K <= 32 ? 1 : 2;
        const dim3 grid((unsigned)used, (unsigned)((K + 32 * kt - 1) / (32 * kt)),
                        (unsigned)((d + 127) / 128));
        auto go = [&](auto kern) {
            return launch(dev, kern, "k_diag_moments launch", grid, dim3(256), {0}, stream, x, resp,
                          part, part_nk, out, nk_out, V, per, d, K, direct);
        };
        rc = kt == 1 ? (wide ? go(k_diag_moments<1, true>) : go(k_diag_moments<1, false>))
                     : (wide ? go(k_diag_moments<2, true>) : go(k_diag_moments<2, false>));
    }
    if (rc || direct) return rc;
    const int64_t n2 = SCATTER ? 0 : K;
    return launch(dev, k_diag_reduce, "k_diag_reduce launch", dim3((unsigned)((n + n2 + 63) / 64)),
                  dim3(64), {0}, stream, (const float *)part, (const float *)part_nk, used, n, n2,
                  out, nk_out);
}

}  // namespace come

using namespace come;

extern "C" int come_gmm_estep_diag(const float *x, int64_t V, int d, const float *prec_sqrt,
                                   const float *mu_prec, const float *log_norm, int K,
                                   float *resp_out, float *lse_out, void *stream) {
    int rc = dg_check("gmm_estep_diag", V, d, K);
    if (rc) return rc;
    if (V == 0) return COME_OK;
    if (!x || !prec_sqrt || !mu_prec || !log_norm || !lse_out)
        return set_error(COME_E_INVALID, "gmm_estep_diag: null pointer");
    const int nch = dg_nch(d);
    if ((V + 256 / nch - 1) / (256 / nch) > INT32_MAX)
        return set_error(COME_E_INVALID, "gmm_estep_diag: V too large");
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    const float *img = dg_image(dev, stream, prec_sqrt, mu_prec, K, d, &rc);
    if (!img) return rc;
    return dg_dist<false>(dev, stream, x, img, log_norm, nullptr, resp_out, lse_out, nullptr, V, d,
                          K, nch);
}

extern "C" int come_community_loss_diag(const float *x, int64_t V, int d, const float *pi,
                                        const float *prec_sqrt, const float *mu_prec,
                                        const float *log_norm, int K, float *row_out,
                                        double *loss_out, void *stream) {
    int rc = dg_check("community_loss_diag", V, d, K);
    if (rc) return rc;
    if (V == 0) return COME_OK;
    if (!x || !pi || !prec_sqrt || !mu_prec || !log_norm || !loss_out)
        return set_error(COME_E_INVALID, "community_loss_diag: null pointer");
    const int nch = dg_nch(d);
    const int64_t blocks = (V + 256 / nch - 1) / (256 / nch);
    if (blocks > INT32_MAX) return set_error(COME_E_INVALID, "community_loss_diag: V too large");
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    double *partial = (double *)stream_scratch(dev, stream, kScratchLossPartial,
                                               sizeof(double) * (size_t)blocks);
    if (!partial) return scratch_failed();
    const float *img = dg_image(dev, stream, prec_sqrt, mu_prec, K, d, &rc);
    if (!img) return rc;
    rc = dg_dist<true>(dev, stream, x, img, log_norm, pi, row_out, nullptr, partial, V, d, K, nch);
    if (rc) return rc;
    return launch(dev, k_diag_loss_sum, "k_diag_loss_sum launch", dim3(1), dim3(256), {0}, stream,
                  (const double *)partial, blocks, loss_out);
}

extern "C" int come_gmm_diag_scratch(int64_t V, int d, int K, int cus, int *chunks_out,
                                     int *rows_per_chunk_out) {
    int rc = dg_check("gmm_diag_scratch", V, d, K);
    if (rc) return rc;
    if (!chunks_out || !rows_per_chunk_out)
        return set_error(COME_E_INVALID, "gmm_diag_scratch: null pointer");
    int chunks;
    int64_t rows;
    dg_plan(V, d, K, cus, &chunks, &rows);
    if (rows > INT32_MAX)
        return set_error(COME_E_INVALID, "gmm_diag_scratch: V must be < 2^31 rows per chunk");
    *chunks_out = chunks;
    *rows_per_chunk_out = (int)rows;
    return COME_OK;
}

extern "C" int come_gmm_diag_moments(const float *x, int64_t V, int d, const float *resp, int K,
                                     int chunks, void *scratch, double *nk_out, double *sx_out,
                                     void *stream) {
    return dg_mstep<false>("gmm_diag_moments", x, V, d, resp, nullptr, K, chunks, scratch, nk_out,
                           sx_out, stream);
}

extern "C" int come_gmm_diag_scatter(const float *x, int64_t V, int d, const float *resp,
                                     const float *means, int K, int chunks, void *scratch,
                                     double *ssq_out, void *stream) {
    return dg_mstep<true>("gmm_diag_scatter", x, V, d, resp, means, K, chunks, scratch, nullptr,
                          ssq_out, stream);
}

extern "C" int come_community_grad_diag(float *x, int64_t V, int d, const float *pi,
                                        const float *mu, const float *inv_var, int K, float beta,
                                        float lr, int iters, void *stream) {
    int rc = dg_check("community_grad_diag", V, d, K);
    if (rc) return rc;
    if (iters < 0) return set_error(COME_E_INVALID, "community_grad_diag: need iters>=0");
    if (V == 0 || iters == 0) return COME_OK;
    if (!x || !pi || !mu || !inv_var)
        return set_error(COME_E_INVALID, "community_grad_diag: null pointer");
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    const float coef = (float)((double)beta / (double)K);
    const int nf = (d + 63) / 64;
    const int rb = nf <= 2 ? 8 : 4;
    const int64_t blocks = (V + 4 * rb - 1) / (4 * rb);
    if (blocks > INT32_MAX) return set_error(COME_E_INVALID, "community_grad_diag: V too large");
    const dim3 grid((unsigned)blocks);
    if (nf == 1)
        return launch(dev, k_diag_grad<1, 8>, "k_diag_grad launch", grid, dim3(256), {0}, stream, x,
                      pi, mu, inv_var, V, d, K, coef, lr, iters);
    if (nf == 2)
        return launch(dev, k_diag_grad<2, 8>, "k_diag_grad launch", grid, dim3(256), {0}, stream, x,
                      pi, mu, inv_var, V, d, K, coef, lr, iters);
    if (nf <= 4)
        return launch(dev, k_diag_grad<4, 4>, "k_diag_grad launch", grid, dim3(256), {0}, stream, x,
                      pi, mu, inv_var, V, d, K, coef, lr, iters);
    return launch(dev, k_diag_grad<8, 4>, "k_diag_grad launch", grid, dim3(256), {0}, stream, x, pi,
                  mu, inv_var, V, d, K, coef, lr, iters);
}
