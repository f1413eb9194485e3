// come_kmeans.hip -- k-means (Lloyd) assignment, accumulation and centre update (gfx950).
//
// Replaces the torch chain of GaussianMixture._kmeans_labels (a [V, K] distance matrix, argmin,
// bincount, index_add_) and gives come_amd.kmeans.KMeans its hot path: come_kmeans_lloyd ->
// k_kmeans_lloyd16 (d = 64, 128, K <= 64: fp32 MFMA scores and one-hot x X MFMA sums, X read
// once from HBM) or k_kmeans_lloyd_valu (any d, K), then k_kmeans_reduce (chunk partials in a
// fixed order, float64); come_kmeans_assign (labels only); come_kmeans_update -> k_kmeans_update.

#include "come_c4.h"

namespace come {

// ---- chunks -----------------------------------------------------------------------------------
// A chunk is a run of consecutive rows whose cluster sums one wavefront (MFMA kernel) or one
// workgroup (VALU kernel) accumulates in fp32, in row order; the chunks' partials are then summed
// in chunk order in float64.  Rows per chunk is a multiple of 16 (the MFMA row tile).  The MFMA
// kernel runs 4 chunks per workgroup and two workgroups per CU: 8 chunks per CU; the partials
// [chunks][K][d] stay <= 128 MB.
static void km_plan(int64_t V, int d, int K, int cus, int *chunks, int64_t *rows) {
    if (cus <= 0) cus = 256;
    const bool mfma = (d == 64 || d == 128) && K <= 64;
    int64_t n = (int64_t)(mfma ? 8 : 2) * cus;
    const int64_t cap = std::max<int64_t>(1, (int64_t(128) << 20) / ((int64_t)K * d * 4));
    n = std::min(n, cap);
    n = std::min(n, (V + 15) / 16);
    n = std::max<int64_t>(n, 1);
    int64_t per = (V + n - 1) / n;
    per = std::max<int64_t>(16, (per + 15) / 16 * 16);
    *rows = per;
    *chunks = (int)std::max<int64_t>(1, (V + per - 1) / per);
}

struct KmArgs {
    const float *x;
    const float *centers;
    int32_t *labels;
    float *mindist;     // optional [V]
    float *psums;       // [chunks][K][d] partial sums (accumulating launches)
    int32_t *pcounts;   // [chunks][K]
    double *pinertia;   // [chunks]
    int64_t V;
    int64_t rows_per_chunk;
    int d;
    int K;
    int chunks;         // chunks in use: ceil(V / rows_per_chunk)
};

// ---- d = 64, 128, K <= 64: scores and sums on v_mfma_f32_16x16x4_f32 -------------------------
//
// The workgroup stages the centres once (rows padded by 4 floats: the 16 lanes of a ds_read_b128
// group cover 64 distinct banks; rows K .. 63 zero) with h_k = 0.5 |c_k|^2 beside them, +inf for
// k >= K, so a padded column scores 0 - inf = -inf and never wins.  Wavefront w of workgroup b owns
// chunk 4 b + w and walks it in tiles of 16 rows.
//   scores   s[i][k] = x_i . c_k - h_k: lane (i = l % 16, g = l / 16) loads features 16 t + 4 g ..
//            + 3 of row i (one dwordx4 per t) as the A operand of k-slot g; lane (j, g) reads the
//            same features of centre 16 ct + j from LDS as B.  Four column tiles ct: the tile's
//            scores for row 4 g + r, column 16 ct + j land in register r of accumulator ct.
//   argmax   over the lane's 4 columns in ascending order (strict >), then over the 16 lanes of the
//            group by xor exchanges on (score, index) with ties to the lower index: the lowest
//            cluster index among equal scores wins.
//   sums     S[k][j] += sum_i onehot[i][k] x[i][j] as MFMAs with the tile's rows as the reduction
//            index: A = the one-hot (0 or 1: every product exact, adding a 0 changes nothing), B =
//            X read again with the lane's low bits on the feature (L1 hits).  Per cluster and
//            feature this is an fp32 sum of the chunk's member rows in row order: deterministic.
// Rows past the chunk's end are loaded clamped and carry label -1 (no one-hot, no store).
template <int D>
struct Km16 {
    static constexpr int LD = D + 4;
    static constexpr int KP = 64;      // padded cluster count
    static constexpr int NT = D / 16;  // feature tiles
};

template <int D, bool ACC>
__global__ void __launch_bounds__(256) k_kmeans_lloyd16(KmArgs a) {
    using C = Km16<D>;
    using f32x4 = __attribute__((ext_vector_type(4))) float;
    __shared__ __attribute__((aligned(16))) float Cs[C::KP * C::LD];
    __shared__ float hn[C::KP];
    const int tid = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int j = lane & 15, g = lane >> 4;
    const int K = a.K;
    for (int o = tid; o < C::KP * (D / 4); o += 256) {
        const int row = o / (D / 4), q = o % (D / 4);
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (row < K) v = *reinterpret_cast<const f32x4 *>(a.centers + (int64_t)row * D + 4 * q);
        *reinterpret_cast<f32x4 *>(Cs + row * C::LD + 4 * q) = v;
    }
    __syncthreads();
    if (tid < C::KP) {
        float s = 0.0f;
        for (int c = 0; c < D; ++c) s = __builtin_fmaf(Cs[tid * C::LD + c], Cs[tid * C::LD + c], s);
        hn[tid] = tid < K ? 0.5f * s : INFINITY;
    }
    __syncthreads();
    const int64_t chunk = (int64_t)blockIdx.x * 4 + wid;
    if (chunk >= a.chunks) return;
    const int64_t c0 = chunk * a.rows_per_chunk;
    int64_t c1 = c0 + a.rows_per_chunk;
    if (c1 > a.V) c1 = a.V;
    float hl[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) hl[ct] = hn[16 * ct + j];
    f32x4 sacc[ACC ? 4 : 1][ACC ? C::NT : 1];
#pragma unroll
    for (int kt = 0; kt < (ACC ? 4 : 1); ++kt)
#pragma unroll
        for (int jt = 0; jt < (ACC ? C::NT : 1); ++jt) sacc[kt][jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    int cnt = 0;
    double inert = 0.0;
    // the next tile's rows are loaded while this tile is multiplied (one wavefront per SIMD at
    // d = 128: nothing else hides the HBM latency)
    f32x4 xn[C::NT];
    {
        const int64_t arow = c0 + j < c1 ? c0 + j : c1 - 1;
        const float *xr = a.x + arow * D + 4 * g;
#pragma unroll
        for (int t = 0; t < C::NT; ++t) xn[t] = *reinterpret_cast<const f32x4 *>(xr + 16 * t);
    }
    for (int64_t r0 = c0; r0 < c1; r0 += 16) {
        f32x4 xv[C::NT];
#pragma unroll
        for (int t = 0; t < C::NT; ++t) xv[t] = xn[t];
        {
            const int64_t nrow = r0 + 16 + j < c1 ? r0 + 16 + j : c1 - 1;
            const float *xr = a.x + nrow * D + 4 * g;
#pragma unroll
            for (int t = 0; t < C::NT; ++t) xn[t] = *reinterpret_cast<const f32x4 *>(xr + 16 * t);
        }
        float xx = 0.0f;
#pragma unroll
        for (int t = 0; t < C::NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) xx = __builtin_fmaf(xv[t][e], xv[t][e], xx);
        xx += __shfl_xor(xx, 16);
        xx += __shfl_xor(xx, 32);
        f32x4 sc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) sc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < C::NT; ++t)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const f32x4 b =
                    *reinterpret_cast<const f32x4 *>(Cs + (16 * ct + j) * C::LD + 16 * t + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    sc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[t][e], b[e], sc[ct], 0, 0, 0);
            }
        int lab[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float best = sc[0][r] - hl[0];
            int bi = j;
#pragma unroll
            for (int ct = 1; ct < 4; ++ct) {
                const float s = sc[ct][r] - hl[ct];
                if (s > best) {
                    best = s;
                    bi = 16 * ct + j;
                }
            }
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {
                const float ob = __shfl_xor(best, m);
                const int oi = __shfl_xor(bi, m);
                if (ob > best || (ob == best && oi < bi)) {
                    best = ob;
                    bi = oi;
                }
            }
            bi = bi < K ? bi : K - 1;
            const float xr2 = __shfl(xx, 4 * g + r);
            const float md = fmaxf(0.0f, xr2 - 2.0f * best);
            const int64_t row = r0 + 4 * g + r;
            const bool live = row < c1;
            if (live && j == 0) {
                a.labels[row] = bi;
                if (a.mindist) a.mindist[row] = md;
                inert += (double)md;
            }
            lab[r] = live ? bi : -1;
        }
        if (ACC) {
            int L[16];  // the tile's labels, row by row
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) L[4 * s + r] = __shfl(lab[r], 16 * s);
#pragma unroll
            for (int r = 0; r < 16; ++r) cnt += L[r] == lane;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                // k-slot g of step s is row 4 s + g
                const int ml = g == 0 ? L[4 * s] : g == 1 ? L[4 * s + 1] : g == 2 ? L[4 * s + 2]
                                                                                  : L[4 * s + 3];
                const int64_t brow = r0 + 4 * s + g < c1 ? r0 + 4 * s + g : c1 - 1;
                const float *xb = a.x + brow * D + j;
                float bv[C::NT];
#pragma unroll
                for (int jt = 0; jt < C::NT; ++jt) bv[jt] = xb[16 * jt];
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const float oh = ml == 16 * kt + j ? 1.0f : 0.0f;
#pragma unroll
                    for (int jt = 0; jt < C::NT; ++jt)
                        sacc[ACC ? kt : 0][ACC ? jt : 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            oh, bv[jt], sacc[ACC ? kt : 0][ACC ? jt : 0], 0, 0, 0);
                }
            }
        }
    }
    if (!ACC) return;
    float *ps = a.psums + chunk * K * D;
#pragma unroll
    for (int kt = 0; kt < (ACC ? 4 : 1); ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 16 * kt + 4 * g + r;
            if (k < K) {
#pragma unroll
                for (int jt = 0; jt < (ACC ? C::NT : 1); ++jt)
                    ps[(int64_t)k * D + 16 * jt + j] = sacc[kt][jt][r];
            }
        }
    if (lane < K) a.pcounts[chunk * K + lane] = cnt;
    // rows 4 g + r were summed by lane 16 g: the four groups' sums in group order
    const double i0 = __shfl(inert, 0), i1 = __shfl(inert, 16), i2 = __shfl(inert, 32),
                 i3 = __shfl(inert, 48);
    if (lane == 0) a.pinertia[chunk] = ((i0 + i1) + i2) + i3;
}

// ---- any d <= kMaxDim, any K <= 4096 on the VALU ---------------------------------------------
// Workgroup = chunk.  Assignment: thread t takes rows c0 + t, c0 + t + 256, ..., scores four
// centres at a time (fmaf chains in j order), ascending k with a strict >, so ties go to the lowest
// index.  Accumulation (acc != 0): the chunk's partial slice is zeroed by the workgroup, then thread
// t owns feature columns t, t + 256 and walks the chunk's rows in order (labels re-read after the
// barrier): an fp32 sum in row order, no atomics on floats (the counts use integer LDS atomics).
__global__ void __launch_bounds__(256) k_kmeans_lloyd_valu(KmArgs a, int acc) {
    extern __shared__ __attribute__((aligned(16))) double smd[];
    const int d = a.d, K = a.K, tid = threadIdx.x;
    double *red = smd;                                  // [256]
    float *hn = reinterpret_cast<float *>(smd + 256);   // [K]
    int *cnt = reinterpret_cast<int *>(hn + K);         // [K]
    const int64_t chunk = blockIdx.x;
    const int64_t c0 = chunk * a.rows_per_chunk;
    int64_t c1 = c0 + a.rows_per_chunk;
    if (c1 > a.V) c1 = a.V;
    float *ps = acc ? a.psums + chunk * K * d : nullptr;
    for (int k = tid; k < K; k += 256) {
        float s = 0.0f;
        for (int c = 0; c < d; ++c) {
            const float v = a.centers[(int64_t)k * d + c];
            s = __builtin_fmaf(v, v, s);
        }
        hn[k] = 0.5f * s;
        cnt[k] = 0;
    }
    if (acc)
        for (int64_t o = tid; o < (int64_t)K * d; o += 256) ps[o] = 0.0f;
    __syncthreads();
    double inert = 0.0;
    for (int64_t r = c0 + tid; r < c1; r += 256) {
        const float *xr = a.x + r * d;
        float xx = 0.0f;
        for (int c = 0; c < d; ++c) xx = __builtin_fmaf(xr[c], xr[c], xx);
        float best = -INFINITY;
        int bi = 0;
        for (int k0 = 0; k0 < K; k0 += 4) {
            float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const float *cp[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cp[u] = a.centers + (int64_t)(k0 + u < K ? k0 + u : K - 1) * d;
            for (int c = 0; c < d; ++c) {
                const float xc = xr[c];
#pragma unroll
                for (int u = 0; u < 4; ++u) s4[u] = __builtin_fmaf(xc, cp[u][c], s4[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (k0 + u < K) {
                    const float s = s4[u] - hn[k0 + u];
                    if (s > best) {
                        best = s;
                        bi = k0 + u;
                    }
                }
            }
        }
        const float md = fmaxf(0.0f, xx - 2.0f * best);
        a.labels[r] = bi;
        if (a.mindist) a.mindist[r] = md;
        inert += (double)md;
        if (acc) atomicAdd(&cnt[bi], 1);
    }
    if (!acc) return;
    red[tid] = inert;
    __syncthreads();  // (also: the labels above are visible to the whole workgroup)
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) a.pinertia[chunk] = red[0];
    for (int k = tid; k < K; k += 256) a.pcounts[chunk * K + k] = cnt[k];
    for (int c = tid; c < d; c += 256)
        for (int64_t r = c0; r < c1; ++r) {
            float *p = ps + (int64_t)a.labels[r] * d + c;
            *p = *p + a.x[r * d + c];
        }
}

// ---- chunk reduction ---------------------------------------------------------------------------
// sums[e] = sum_c psums[c][e], counts[k] = sum_c pcounts[c][k], inertia = sum_c pinertia[c] in
// float64 / int64.  Entry e of a workgroup's 32 is summed by 8 threads over the chunks p, p + 8,
// ..., the 8 results added in p order: a fixed order whatever the grid.
constexpr int kKmRedE = 32, kKmRedP = 8;
__global__ void __launch_bounds__(256)
    k_kmeans_reduce(const float *psums, const int32_t *pcounts, const double *pinertia, int chunks,
                    int64_t nsum, int K, double *sums, int64_t *counts, double *inertia) {
    __shared__ double red[kKmRedP][kKmRedE];
    __shared__ long long redc[kKmRedP][kKmRedE];
    const int t = threadIdx.x % kKmRedE, p = threadIdx.x / kKmRedE;
    const int64_t e = (int64_t)blockIdx.x * kKmRedE + t;
    double s = 0.0;
    long long n = 0;
    if (e < nsum) {
        for (int c = p; c < chunks; c += kKmRedP) s += (double)psums[(int64_t)c * nsum + e];
    } else if (e < nsum + K) {
        for (int c = p; c < chunks; c += kKmRedP) n += pcounts[(int64_t)c * K + (e - nsum)];
    } else if (e == nsum + K) {
        for (int c = p; c < chunks; c += kKmRedP) s += pinertia[c];
    }
    red[p][t] = s;
    redc[p][t] = n;
    __syncthreads();
    if (p != 0) return;
    for (int q = 1; q < kKmRedP; ++q) {
        s += red[q][t];
        n += redc[q][t];
    }
    if (e < nsum) sums[e] = s;
    else if (e < nsum + K) counts[e - nsum] = n;
    else if (e == nsum + K) *inertia = s;
}

// ---- centre update -------------------------------------------------------------------------------
// c_k = (float)(sums_k / counts_k); a cluster without rows keeps its centre bit for bit.
// stats2[0] = sum (new - old)^2 in float64: one workgroup, per-thread partials then a tree.
__global__ void __launch_bounds__(1024)
    k_kmeans_update(float *centers, const double *sums, const int64_t *counts, int K, int d,
                    double *stats2) {
    __shared__ double red[1024];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t o = tid; o < (int64_t)K * d; o += 1024) {
        const int64_t n = counts[o / d];
        if (n > 0) {
            const float old = centers[o];
            const float nw = (float)(sums[o] / (double)n);
            centers[o] = nw;
            const double df = (double)nw - (double)old;
            s += df * df;
        }
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) stats2[0] = red[0];
}

static int km_check(const char *who, int64_t V, int64_t vmin, int d, int K) {
    if (V < vmin)
        return set_error(COME_E_INVALID, "%s: V must be >= %d (got %lld)", who, (int)vmin,
                         (long long)V);
    if (d < 1 || d > kMaxDim)
        return set_error(COME_E_INVALID, "%s: d must be in [1, %d] (got %d)", who, kMaxDim, d);
    const int kmax = (d == 64 || d == 128 || d > 128) ? 4096 : 64;
    if (K < 1 || K > kmax)
        return set_error(COME_E_INVALID, "%s: K must be in [1, %d] for d = %d (got %d)", who, kmax,
                         d, K);
    return COME_OK;
}

// the Lloyd pass over `used` chunks of `per` rows (accumulating into `a`'s partials when acc)
static int km_launch(int dev, KmArgs a, bool acc, void *stream) {
    const bool mfma = (a.d == 64 || a.d == 128) && a.K <= 64 && ((uintptr_t)a.x % 16) == 0 &&
                      ((uintptr_t)a.centers % 16) == 0;
    if (!mfma)
        return launch(dev, k_kmeans_lloyd_valu, "k_kmeans_lloyd_valu launch", dim3(a.chunks),
                      dim3(256), {sizeof(double) * 256 + (size_t)a.K * 8}, stream, a,
                      acc ? 1 : 0);
    const dim3 grid((unsigned)((a.chunks + 3) / 4));
    return with_width(a.d, [&](auto width) {
        constexpr int D = decltype(width)::value;
        if (acc)
            return launch(dev, k_kmeans_lloyd16<D, true>, "k_kmeans_lloyd16 launch", grid, dim3(256),
                          {0}, stream, a);
        return launch(dev, k_kmeans_lloyd16<D, false>, "k_kmeans_assign16 launch", grid, dim3(256),
                      {0}, stream, a);
    });
}

}  // namespace come

using namespace come;

extern "C" int come_kmeans_scratch(int64_t V, int d, int K, int cus, int *chunks_out,
                                   int *rows_per_chunk_out) {
    int rc = km_check("kmeans_scratch", V, 1, d, K);
    if (rc) return rc;
    if (!chunks_out || !rows_per_chunk_out) return set_error(COME_E_INVALID, "null pointer");
    int chunks;
    int64_t rows;
    km_plan(V, d, K, cus, &chunks, &rows);
    if (rows > INT32_MAX)
        return set_error(COME_E_INVALID, "kmeans_scratch: V must be < 2^31 rows per chunk");
    *chunks_out = chunks;
    *rows_per_chunk_out = (int)rows;
    return COME_OK;
}

extern "C" int come_kmeans_lloyd(const float *x, int64_t V, int d, const float *centers, int K,
                                 int chunks, void *scratch, int32_t *labels_out,
                                 float *mindist_out, double *sums_out, int64_t *counts_out,
                                 double *inertia_out, void *stream) {
    int rc = km_check("kmeans_lloyd", V, 1, d, K);
    if (rc) return rc;
    if (chunks < 1 || (int64_t)chunks * K * d * 4 > (int64_t(128) << 20))
        return set_error(COME_E_INVALID, "kmeans_lloyd: chunks must be >= 1 with chunks * K * d * 4 "
                                         "<= 128 MB (got %d; see come_kmeans_scratch)", chunks);
    if (!x || !centers || !scratch || !labels_out || !sums_out || !counts_out || !inertia_out)
        return set_error(COME_E_INVALID, "null pointer");
    if ((uintptr_t)scratch % 8)
        return set_error(COME_E_INVALID, "kmeans_lloyd: scratch must be 8-byte aligned");
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    int64_t per = (V + chunks - 1) / chunks;
    per = std::max<int64_t>(16, (per + 15) / 16 * 16);
    const int used = (int)((V + per - 1) / per);
    // scratch: double inertia [chunks], float sums [chunks][K][d], int32 counts [chunks][K]
    double *pin = reinterpret_cast<double *>(scratch);
    float *ps = reinterpret_cast<float *>(pin + chunks);
    int32_t *pc = reinterpret_cast<int32_t *>(ps + (int64_t)chunks * K * d);
    KmArgs a{x, centers, labels_out, mindist_out, ps, pc, pin, V, per, d, K, used};
    rc = km_launch(dev, a, true, stream);
    if (rc) return rc;
    const int64_t nsum = (int64_t)K * d;
    return launch(dev, k_kmeans_reduce, "k_kmeans_reduce launch",
                  dim3((unsigned)((nsum + K + 1 + kKmRedE - 1) / kKmRedE)), dim3(256), {0}, stream,
                  (const float *)ps, (const int32_t *)pc, (const double *)pin, used, nsum, K,
                  sums_out, counts_out, inertia_out);
}

extern "C" int come_kmeans_assign(const float *x, int64_t V, int d, const float *centers, int K,
                                  int32_t *labels_out, float *mindist_out, void *stream) {
    int rc = km_check("kmeans_assign", V, 0, d, K);
    if (rc) return rc;
    if (V == 0) return COME_OK;
    if (!x || !centers || !labels_out) return set_error(COME_E_INVALID, "null pointer");
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    int chunks;
    int64_t per;
    km_plan(V, d, K, num_cus(dev), &chunks, &per);
    KmArgs a{x, centers, labels_out, mindist_out, nullptr, nullptr, nullptr, V, per, d, K, chunks};
    return km_launch(dev, a, false, stream);
}

extern "C" int come_kmeans_update(float *centers, const double *sums, const int64_t *counts, int K,
                                  int d, double *stats2, void *stream) {
    int rc = km_check("kmeans_update", 1, 1, d, K);
    if (rc) return rc;
    if (!centers || !sums || !counts || !stats2) return set_error(COME_E_INVALID, "null pointer");
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    return launch(dev, k_kmeans_update, "k_kmeans_update launch", dim3(1), dim3(1024), {0}, stream,
                  centers, sums, counts, K, d, stats2);
}
