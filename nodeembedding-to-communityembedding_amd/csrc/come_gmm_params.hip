// come_gmm_params.hip -- GMM M-step parameters + E-step constants in one launch (gfx950):
// come_gmm_params -> k_gmm_params, on the scatter matrices of come_gmm_scatter.hip.
//
// One workgroup per component, float64 in LDS (d <= 128: 128 x 129 doubles = 129 KB): cov =
// S / nk + reg I (sklearn _estimate_gaussian_covariances_full), the right-looking Cholesky
// factorisation in place (U = L^T in the upper triangle), then prec_chol = L^-T = U^-1 bottom-up by
// rows with two lanes of one wavefront per column (sklearn _compute_precision_cholesky:
// solve_triangular(L, I).T): a column's values are written and read by its own wavefront only, so
// the inverse needs no barrier.  Then the E-step's fp32 inputs.  Replaces ~30 small launches (torch
// cholesky_ex / solve_triangular / einsum) and a host sync per EM iteration.

#include "come_c4.h"

namespace come {

struct ParamsArgs {
    const double *__restrict__ S, *__restrict__ nk, *__restrict__ means, *__restrict__ weights;
    int K, d;
    double reg;
    double *cov, *pc;
    float *e_pc, *e_mp, *e_ln;
    int *info;
};

// Right-looking Cholesky steps j .. j + NB - 1 in one phase (no barrier inside).  Step m turns
// A^(m) into A^(m+1)[i][c] = A^(m)[i][c] - t_m(i) A^(m)[c][j + m], t_m(i) = A^(m)[i][j + m] / pivot_m.
// Each thread recomputes, in registers and in exactly that order, the panel values A^(m)[i][j + m]
// it needs (the same expressions as one step per barrier, so the factor is bit-identical), writes
// rows j + m of U = L^T to the upper triangle and the NB steps' trailing update to the lower --
// disjoint from every read of the phase.
template <int NB>
__device__ __forceinline__ void chol_panel(double *A, int LD, int d, int j, int tid, double *ld,
                                           int *bad) {
    const int tx = tid & 15, ty = tid >> 4;
    double P[NB][NB], ra[NB], lk[NB];  // P[k][m] = A^(m)[j + k][j + m], m < k
    bool okv[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        double t[NB];
#pragma unroll
        for (int m = 0; m <= k; ++m) {
            double x = A[(j + k) * LD + j + m];
#pragma unroll
            for (int q = 0; q < m; ++q) x = x - t[q] * P[m][q];
            if (m < k) {
                P[k][m] = x;
                t[m] = x * ra[m];
            } else {
                okv[k] = x > 0.0;
                lk[k] = sqrt(okv[k] ? x : 1.0);
                ra[k] = 1.0 / (okv[k] ? x : 1.0);
            }
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            ld[j + k] = lk[k];
            if (!okv[k] && *bad == 0) *bad = j + k + 1;
        }
    }
    // U rows j + m: U[j + m][i] = A^(m)[i][j + m] / L[j + m][j + m] for i > j + m
    for (int i = j + 1 + tid; i < d; i += 256) {
        double t[NB];
#pragma unroll
        for (int m = 0; m < NB; ++m) {
            if (j + m >= i) break;
            double x = A[i * LD + j + m];
#pragma unroll
            for (int q = 0; q < m; ++q) x = x - t[q] * P[m][q];
            t[m] = x * ra[m];
            A[(j + m) * LD + i] = x / lk[m];
        }
    }
    // trailing rows / columns from j + NB: the thread's columns cc = j + NB + tx + 16 n with their
    // panel values in registers, then each row's elements loaded, updated by the NB steps, stored
    double c[NB][8];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        const int cc = j + NB + tx + 16 * n;
        double t[NB];
#pragma unroll
        for (int m = 0; m < NB; ++m) {
            double x = cc < d ? A[cc * LD + j + m] : 0.0;
#pragma unroll
            for (int q = 0; q < m; ++q) x = x - t[q] * P[m][q];
            t[m] = x * ra[m];
            c[m][n] = x;
        }
    }
    for (int ii = j + NB + ty; ii < d; ii += 16) {
        double t[NB];
#pragma unroll
        for (int m = 0; m < NB; ++m) {
            double x = A[ii * LD + j + m];
#pragma unroll
            for (int q = 0; q < m; ++q) x = x - t[q] * P[m][q];
            t[m] = x * ra[m];
        }
        double v[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int cc = j + NB + tx + 16 * n;
            v[n] = cc <= ii ? A[ii * LD + cc] : 0.0;
        }
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int cc = j + NB + tx + 16 * n;
            double y = v[n];
#pragma unroll
            for (int m = 0; m < NB; ++m) y = y - t[m] * c[m][n];
            if (cc <= ii) A[ii * LD + cc] = y;
        }
    }
}

// Rows r, r - 1, .., r - R + 1 of P = U^-1 for the lane pair of column c (h: the parity of q it
// sums): the R dots over q > r share the loads of P[q][c]; then row r - k adds U[r - k][q] P[q][c]
// for q = r, r - 1, .., r - k + 1 from registers before its dot.  P[q][c] (q < c) sits at A[c][q],
// the diagonal in pd.  Written by the h = 0 lane; read back only by this wavefront.
template <int R>
__device__ __forceinline__ void inv_rows(double *A, int LD, int d, int r, int c, int h,
                                         double pdc, const double *pd) {
    double S[R];
#pragma unroll
    for (int k = 0; k < R; ++k) S[k] = 0.0;
    if (c < d && c > r) {
        double s[R][4];
#pragma unroll
        for (int k = 0; k < R; ++k) s[k][0] = s[k][1] = s[k][2] = s[k][3] = 0.0;
        int q = r + 1 + h;
        for (; q + 6 < c; q += 8) {
            const double p0 = A[c * LD + q], p1 = A[c * LD + q + 2];
            const double p2 = A[c * LD + q + 4], p3 = A[c * LD + q + 6];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const double *u = A + (r - k) * LD + q;
                s[k][0] += u[0] * p0;
                s[k][1] += u[2] * p1;
                s[k][2] += u[4] * p2;
                s[k][3] += u[6] * p3;
            }
        }
        for (; q <= c; q += 2) {
            const double pq = q == c ? pdc : A[c * LD + q];
#pragma unroll
            for (int k = 0; k < R; ++k) s[k][0] += A[(r - k) * LD + q] * pq;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) S[k] = (s[k][0] + s[k][1]) + (s[k][2] + s[k][3]);
    }
    double O[R];
#pragma unroll
    for (int k = 0; k < R; ++k) O[k] = __shfl_xor(S[k], 1);
    if (h == 0 && c < d && c >= r - R + 1) {
        double Pv[R];  // P[r - k][c]
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int rk = r - k;
            if (c <= rk) {
                Pv[k] = c == rk ? pd[rk] : 0.0;
                continue;
            }
            double acc;
            if (k == 0) {
                acc = S[0] + O[0];
            } else {
                acc = A[rk * LD + r] * Pv[0];
#pragma unroll
                for (int m = 1; m < k; ++m) acc = acc + A[rk * LD + r - m] * Pv[m];
                acc = acc + (S[k] + O[k]);
            }
            Pv[k] = -acc * pd[rk];
            A[c * LD + rk] = Pv[k];
        }
    }
}

// Cholesky columns per barrier and inverse rows per round (scripts/params_ab.py at K = 50, d = 128:
// 8 / 4 -> 0.190 ms, 4 / 4 0.198, 8 / 2 0.215, 4 / 2 0.223; profiles/r07_ab_gmm_params6.txt)
constexpr int kParamsNB = 8, kParamsInvR = 4;

__global__ void __launch_bounds__(256) k_gmm_params(ParamsArgs p) {
    extern __shared__ __attribute__((aligned(16))) double A[];  // [d][d + 1]
    __shared__ double ld[128], pd[128], mus[128], red[256];
    __shared__ int bad;
    const int k = blockIdx.x, d = p.d, LD = d + 1, tid = threadIdx.x, dd = d * d;
    const int tx = tid & 15, ty = tid >> 4;
    const double *__restrict__ S = p.S + (int64_t)k * dd;
    double *__restrict__ cov = p.cov + (int64_t)k * dd;
    const double nkk = p.nk[k];
    // S / nk[:, None, None] + reg I (the torch path's order), 16 coalesced loads in flight per lane
    for (int base = tid; base < dd; base += 256 * 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = base + 256 * u < dd ? S[base + 256 * u] : 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = base + 256 * u;
            if (e >= dd) break;
            const int i = e / d, j = e - i * d;
            const double c = i == j ? v[u] / nkk + p.reg : v[u] / nkk;
            cov[e] = c;
            A[i * LD + j] = c;
        }
    }
    if (tid < d) mus[tid] = p.means[(int64_t)k * d + tid];
    if (tid == 0) bad = 0;
    __syncthreads();
    // Cholesky, right-looking, kParamsNB columns per barrier (chol_panel), then the 4 / 2 / 1 left
    int j = 0;
    for (; j + kParamsNB <= d; j += kParamsNB) {
        chol_panel<kParamsNB>(A, LD, d, j, tid, ld, &bad);
        __syncthreads();
    }
    if (kParamsNB > 4 && j + 4 <= d) {
        chol_panel<4>(A, LD, d, j, tid, ld, &bad);
        __syncthreads();
        j += 4;
    }
    if (j + 2 <= d) {
        chol_panel<2>(A, LD, d, j, tid, ld, &bad);
        __syncthreads();
        j += 2;
    }
    if (j < d) {
        chol_panel<1>(A, LD, d, j, tid, ld, &bad);
        __syncthreads();
    }
    // P = U^-1 = L^-T (upper), bottom-up by rows: P[r][c] = -(sum_{r<q<=c} U[r][q] P[q][c]) /
    // U[r][r]; P[q][c] (q < c) kept in the lower triangle at A[c][q], its diagonal in pd.  Column
    // c = tid / 2 belongs to lanes 2c, 2c + 1 of one wavefront, which split the dot by the parity
    // of q (four partial sums each) and combine by a lane exchange: every P value a lane reads was
    // written by its own wavefront at an earlier row (LDS accesses of a wavefront are ordered), so
    // the rows need no barrier.
    for (int r = tid; r < d; r += 256) pd[r] = 1.0 / ld[r];
    __syncthreads();
    {
        const int c = tid >> 1, h = tid & 1;
        const double pdc = c < d ? pd[c] : 0.0;
        int r = d - 2;
        for (; r >= kParamsInvR - 1; r -= kParamsInvR)
            inv_rows<kParamsInvR>(A, LD, d, r, c, h, pdc, pd);
        if (kParamsInvR > 2 && r >= 1) {
            inv_rows<2>(A, LD, d, r, c, h, pdc, pd);
            r -= 2;
        }
        if (r == 0) inv_rows<1>(A, LD, d, r, c, h, pdc, pd);
    }
    __syncthreads();
    // prec_chol (upper): row r, column c > r at A[c][r], pd on the diagonal
    double *pc = p.pc + (int64_t)k * d * d;
    float *epc = p.e_pc + (int64_t)k * d * d;
    for (int r = ty; r < d; r += 16)
        for (int c = tx; c < d; c += 16) {
            const double v = c < r ? 0.0 : (c == r ? pd[r] : A[c * LD + r]);
            pc[r * d + c] = v;
            epc[r * d + c] = (float)v;
        }
    // mu_k prec_chol_k (column j: rows i <= j) and log det = sum log diag(prec_chol)
    if (tid < d) {
        const int j = tid;
        double s = mus[j] * pd[j];
        for (int i = 0; i < j; ++i) s += mus[i] * A[j * LD + i];
        p.e_mp[(int64_t)k * d + j] = (float)s;
    }
    red[tid] = tid < d ? log(pd[tid]) : 0.0;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        p.e_ln[k] = (float)(log(p.weights[k]) + red[0] - 0.5 * d * log(2.0 * 3.14159265358979323846));
        p.info[k] = bad;
    }
}

}  // namespace come

using namespace come;

extern "C" int come_gmm_params(const double *scatter, const double *nk, const double *means,
                               const double *weights, int K, int d, double reg_covar,
                               double *cov_out, double *prec_chol_out, float *e_prec_chol,
                               float *e_mu_prec, float *e_log_norm, int *info, void *stream) {
    if (K < 1 || d < 1 || d > 128)
        return set_error(COME_E_INVALID, "gmm_params: need K >= 1 and 1 <= d <= 128");
    if (!scatter || !nk || !means || !weights || !cov_out || !prec_chol_out || !e_prec_chol ||
        !e_mu_prec || !e_log_norm || !info)
        return set_error(COME_E_INVALID, "null pointer");
    int dev;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    ParamsArgs p{scatter, nk, means, weights, K, d, reg_covar, cov_out, prec_chol_out,
                 e_prec_chol, e_mu_prec, e_log_norm, info};
    // (the kernel's static LDS, ~3 KB, counts against the 160 KB too: the limit asked for is what
    // d = 128 needs, 129 KB, not the whole of it)
    return launch(dev, k_gmm_params, "k_gmm_params launch", dim3(K), dim3(256),
                  {sizeof(double) * (size_t)d * (d + 1), (int)(sizeof(double) * 128 * 129)}, stream,
                  p);
}
