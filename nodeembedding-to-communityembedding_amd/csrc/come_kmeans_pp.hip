// come_kmeans_pp.hip -- greedy k-means++ seeding (gfx950): the candidates' distances in one pass
// over X, the choice of the best candidate, and the draw of the next candidates.
//
// Replaces the torch chain of come_amd.kmeans.kmeans_plusplus (float64 cumsum, searchsorted, a
// skinny GEMM, a [V, T] distance matrix in several elementwise passes, argmin / index_select)
// with three entry points whose results never leave the device:
//   come_kmeans_pp_step   -> k_pp_step (dist, per-chunk column sums) + k_pp_pots (their total)
//   come_kmeans_pp_pick   -> k_pp_pick (argmin of the potentials, its column and chunk sums)
//   come_kmeans_pp_sample -> k_pp_sample (the searchsorted of T draws on the float64 cumulative sum)
// The work per row is T <= 16 candidates x d subtractions and fmafs on the VALU against one read of
// the row: bound by the read of X.  No float atomics: every sum is taken in a fixed order.

#include "come_c4.h"

namespace come {

constexpr int kPpMaxT = 16;
constexpr int kPpRowStep = 32;                // rows per chunk: a multiple of the widest block step
constexpr int64_t kPpPartialBytes = 2 << 20;  // chunks * T * 8 stays within this
constexpr int kPpSegs = 256;                  // threads of the fixed-order chunk sum
constexpr int kPpGroups = 16;                 // its second level: 16 groups of 16 segments

// ---- chunks -----------------------------------------------------------------------------------
// A chunk is the run of consecutive rows of one workgroup of k_pp_step: 32 per CU.  Between 4
// (T = 16) and 8 (T <= 2) workgroups are resident per CU, by their registers, so the chunks are
// kept several times as many as that: the last, partly filled round of workgroups is short.
static int64_t pp_rows_per_chunk(int64_t V, int chunks) {
    const int64_t per = (V + chunks - 1) / chunks;
    return (per + kPpRowStep - 1) / kPpRowStep * kPpRowStep;
}

static void pp_plan(int64_t V, int T, int cus, int *chunks, int64_t *rows) {
    if (cus <= 0) cus = 256;
    int64_t n = (int64_t)32 * cus;
    n = std::min(n, kPpPartialBytes / ((int64_t)T * 8));
    n = std::min(n, (V + kPpRowStep - 1) / kPpRowStep);
    n = std::max<int64_t>(n, 1);
    const int64_t per = pp_rows_per_chunk(V, (int)n);
    *chunks = (int)((V + per - 1) / per);
    *rows = per;  // == pp_rows_per_chunk(V, *chunks): what come_kmeans_pp_step derives
}

// ---- a fixed-order sum of n doubles p[0], p[stride], ... -----------------------------------------
// Thread j of the 256 sums segment j (seg = ceil(n / 256) consecutive entries, in order) into
// sh[j], and the first 16 threads each 16 consecutive segments, in order, into sh[256 + j / 16].
// seg_base(sh, j) is then the sum of the entries before segment j: the groups before j's, in order,
// plus the segments before j in its group, in order (at most 30 adds; non-decreasing in j for
// entries >= 0), and seg_base(sh, 256) the total.  k_pp_pots and k_pp_sample share it, so a
// potential and the cumulative sum searched for it agree bit for bit.
// (Entries are loaded eight at a time, ahead of the adds that take them in order: a loop of one
// load and one dependent add pays the whole memory latency per entry.)
__device__ inline void seg_store(double *sh, int tid, double s) {  // segment tid's sum is s
    sh[tid] = s;
    __syncthreads();
    if (tid < kPpGroups) {
        double g = 0.0;
        for (int q = 0; q < kPpGroups; ++q) g += sh[kPpGroups * tid + q];
        sh[kPpSegs + tid] = g;
    }
    __syncthreads();
}
__device__ inline void seg_sums(const double *p, int64_t stride, int n, int tid, double *sh) {
    const int seg = (n + kPpSegs - 1) / kPpSegs;
    const int lo = tid * seg < n ? tid * seg : n, hi = lo + seg < n ? lo + seg : n;
    double s = 0.0;
    int c = lo;
    for (; c + 8 <= hi; c += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = p[(c + q) * stride];
#pragma unroll
        for (int q = 0; q < 8; ++q) s += v[q];
    }
    for (; c < hi; ++c) s += p[c * stride];
    seg_store(sh, tid, s);
}
__device__ inline double seg_base(const double *sh, int j) {
    double s = 0.0, w = 0.0;
    for (int q = 0; q < j / kPpGroups; ++q) s += sh[kPpSegs + q];
    for (int q = j / kPpGroups * kPpGroups; q < j; ++q) w += sh[q];
    return s + w;
}

struct PpArgs {
    const float *x;
    const float *closest;  // optional [V]
    const int32_t *cand;   // [T]
    float *dist;           // [V][T]
    double *ppot;          // [chunks][T]
    int64_t V;
    int64_t rows_per_chunk;
    int d;
};

// ---- the pass over X ----------------------------------------------------------------------------
// G lanes share a row, lane g of them the features (p G + g) VEC .. + VEC - 1 of pass p; a
// wavefront walks 64 / G rows at a time.  <4, 8>: dwordx4 loads, 128 contiguous bytes per row and
// instruction, for 16-byte aligned rows (x aligned, d % 4 == 0); <1, 64>: dword loads, anything
// else.  The candidates' rows are staged in LDS once per workgroup, negated (x + (-c) is x - c bit
// for bit, and an add of two floats packs into v_pk_add_f32 where a subtraction does not) and zero
// beyond d, like the row loads, so a padded feature adds (0 - 0)^2; they are read back as one
// ds_read per pass and candidate, all row groups the same address.  A distance is the lane's fmaf
// chain over its features in pass order (two chains at VEC = 4, added at the end), then the xor
// butterfly over the group's lanes: a fixed order.  The group's first lane stores the row's T
// distances and adds them to its float64 column sums; the workgroup's sums are added in lane-group
// order.
template <int VEC, int G, int T>
__global__ void __launch_bounds__(256) k_pp_step(PpArgs a) {
    constexpr int LD = kMaxDim;     // staged row stride
    constexpr int RW = 64 / G;      // rows per wavefront step
    constexpr int NL = 256 / G;     // row groups per workgroup
    typedef float vec __attribute__((ext_vector_type(VEC)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    using acc_t = std::conditional_t<VEC == 4, f32x2, float>;
    __shared__ __attribute__((aligned(16))) float cs[T * LD];
    __shared__ double red[NL][T];
    __shared__ int bad[T];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane % G;
    const int d = a.d;
    const int64_t chunk = blockIdx.x;
    const int64_t c0 = chunk * a.rows_per_chunk;
    if (c0 >= a.V) {  // a chunk past the rows (a caller's own chunk count): empty sums
        if (tid < T) a.ppot[chunk * T + tid] = 0.0;
        return;
    }
    const int64_t c1 = c0 + a.rows_per_chunk < a.V ? c0 + a.rows_per_chunk : a.V;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int64_t r = a.cand[t];
        const bool ok = r >= 0 && r < a.V;
        for (int j = tid; j < LD; j += 256)
            cs[t * LD + j] = (ok && j < d) ? -a.x[r * d + j] : 0.0f;
        if (tid == 0) bad[t] = !ok;
    }
    __syncthreads();
    unsigned badmask = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) badmask |= bad[t] ? 1u << t : 0u;
    const int P = (d + VEC * G - 1) / (VEC * G);
    double ps[T];
#pragma unroll
    for (int t = 0; t < T; ++t) ps[t] = 0.0;
    for (int64_t r0 = c0 + wid * RW; r0 < c1; r0 += 4 * RW) {
        const int64_t row = r0 + lane / G;
        const bool live = row < c1;
        const float *xr = a.x + (live ? row : c1 - 1) * d;
        // VEC = 4: features 0, 2 and 1, 3 of a load go down two fmaf chains as one packed add
        // and one packed fma each (v_pk_add_f32, v_pk_fma_f32: half the VALU issue)
        acc_t acc2[T];
#pragma unroll
        for (int t = 0; t < T; ++t) acc2[t] = acc_t(0.0f);
        for (int p0 = 0; p0 < P; p0 += 4) {
            vec xv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int off = ((p0 + q) * G + g) * VEC;
                if (off < d) {
                    xv[q] = *reinterpret_cast<const vec *>(xr + off);
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) xv[q][e] = 0.0f;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (p0 + q < P) {  // (the same in every lane)
                    const int off = ((p0 + q) * G + g) * VEC;
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const vec c = *reinterpret_cast<const vec *>(cs + t * LD + off);
                        if constexpr (VEC == 4) {
                            const acc_t lo = __builtin_shufflevector(xv[q], xv[q], 0, 1) +
                                             __builtin_shufflevector(c, c, 0, 1);
                            const acc_t hi = __builtin_shufflevector(xv[q], xv[q], 2, 3) +
                                             __builtin_shufflevector(c, c, 2, 3);
                            acc2[t] = __builtin_elementwise_fma(lo, lo, acc2[t]);
                            acc2[t] = __builtin_elementwise_fma(hi, hi, acc2[t]);
                        } else {
                            const float df = xv[q][0] + c[0];
                            acc2[t] = __builtin_fmaf(df, df, acc2[t]);
                        }
                    }
                }
            }
        }
        float acc[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if constexpr (VEC == 4) acc[t] = acc2[t][0] + acc2[t][1];
            else acc[t] = acc2[t];
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            acc[t] = reduce_stage<0>(acc[t]);
            acc[t] = reduce_stage<1>(acc[t]);
            acc[t] = reduce_stage<2>(acc[t]);
            if constexpr (G == 64) {
                acc[t] = reduce_stage<3>(acc[t]);
                acc[t] = reduce_stage<4>(acc[t]);
                acc[t] = reduce_stage<5>(acc[t]);
            }
        }
        if (live && g == 0) {
            const float cl = a.closest ? a.closest[row] : INFINITY;
            float *out = a.dist + row * T;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float v = (badmask >> t & 1u) ? INFINITY : fminf(cl, acc[t]);
                out[t] = v;
                ps[t] += (double)v;
            }
        }
    }
    if (g == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) red[tid / G][t] = ps[t];
    }
    __syncthreads();
    if (tid < T) {
        double s = 0.0;
        for (int l = 0; l < NL; ++l) s += red[l][tid];
        a.ppot[chunk * T + tid] = s;
    }
}

// pots[t] = the sum of ppot[.][t] in chunk order (seg_sums): workgroup t
__global__ void __launch_bounds__(kPpSegs)
    k_pp_pots(const double *ppot, int chunks, int T, double *pots) {
    __shared__ double sh[kPpSegs + kPpGroups];
    seg_sums(ppot + blockIdx.x, T, chunks, threadIdx.x, sh);
    if (threadIdx.x == 0) pots[blockIdx.x] = seg_base(sh, kPpSegs);
}

// ---- the best candidate ---------------------------------------------------------------------------
// best = argmin_t pots[t] (strict <: ties to the lowest t), taken by every thread; its column of
// dist and of ppot copied out.
__global__ void __launch_bounds__(256)
    k_pp_pick(const float *dist, int64_t V, int T, const double *ppot, const double *pots,
              int chunks, float *closest_out, double *cpot_out, int32_t *best_out,
              double *pot_out) {
    int best = 0;
    double pb = pots[0];
    for (int t = 1; t < T; ++t) {
        const double p = pots[t];
        if (p < pb) {
            pb = p;
            best = t;
        }
    }
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t i = i0; i < V; i += step) closest_out[i] = dist[i * T + best];
    for (int64_t c = i0; c < chunks; c += step) cpot_out[c] = ppot[c * T + best];
    if (i0 == 0) {
        *best_out = best;
        *pot_out = pb;
    }
}

// ---- the next candidates --------------------------------------------------------------------------
// Workgroup t draws r = u[t] * pot and returns the first row with closest > 0 whose cumulative sum
// reaches r (row 0 for r = 0: nothing to search).
//   cum(row) = prefix(chunk) + (base(thread) + running sum of the thread's rows): prefix is the
// seg_sums / seg_base order over cpot; inside the chunk thread j sums the rows j * sub .. + sub - 1
// in order and base is seg_base over the threads' totals.  First the first chunk with cpot > 0
// whose prefix, cpot included, reaches r, then the first such row in it.  Only entries with a
// positive increment are taken, so a row without mass is never returned, whatever the rounding of
// the sums' different orders.  Should the chunk's rows, summed this way, stop short of its cpot
// (summed in k_pp_step's order) by a rounding, the chunk's last row with closest > 0 is returned.
__global__ void __launch_bounds__(kPpSegs)
    k_pp_sample(const float *closest, int64_t V, const double *cpot, int chunks,
                int64_t rows_per_chunk, const double *u, int32_t *cand_out) {
    __shared__ double sh[kPpSegs + kPpGroups], sh2[kPpSegs + kPpGroups];
    __shared__ double pre;
    __shared__ int found;
    __shared__ long long hit, lastpos;
    const int tid = threadIdx.x;
    if (tid == 0) {
        found = INT32_MAX;
        hit = INT64_MAX;
        lastpos = -1;
    }
    seg_sums(cpot, 1, chunks, tid, sh);
    const double r = u[blockIdx.x] * seg_base(sh, kPpSegs);
    if (r <= 0.0) {  // u = 0 or no mass at all (the same in every thread)
        if (tid == 0) cand_out[blockIdx.x] = 0;
        return;
    }
    const int seg = (chunks + kPpSegs - 1) / kPpSegs;
    const double base = seg_base(sh, tid);
    double run = 0.0, mypre = 0.0;
    int mine = INT32_MAX;
    const int lo = tid * seg < chunks ? tid * seg : chunks;
    const int hi = lo + seg < chunks ? lo + seg : chunks;
    for (int c = lo; c < hi; c += 8) {  // (loads ahead of the adds, as in seg_sums)
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = c + q < hi ? cpot[c + q] : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double before = base + run;
            run += v[q];
            if (mine == INT32_MAX && v[q] > 0.0 && base + run >= r) {
                mine = c + q;
                mypre = before;
            }
        }
    }
    if (mine != INT32_MAX) atomicMin(&found, mine);
    __syncthreads();
    const int c = found;
    if (c == INT32_MAX) {  // (r is a NaN or beyond the total by a rounding: searchsorted's clamp)
        if (tid == 0) cand_out[blockIdx.x] = (int32_t)(V - 1);
        return;
    }
    if (mine == c) pre = mypre;
    const int64_t c0 = (int64_t)c * rows_per_chunk;
    const int64_t c1 = c0 + rows_per_chunk < V ? c0 + rows_per_chunk : V;
    const int64_t sub = (rows_per_chunk + kPpSegs - 1) / kPpSegs;
    int64_t b0 = c0 + tid * sub, b1 = b0 + sub;
    if (b0 > c1) b0 = c1;
    if (b1 > c1) b1 = c1;
    double s = 0.0;
    long long lp = -1;
    for (int64_t i = b0; i < b1; ++i) {
        const float v = closest[i];
        s += (double)v;
        if (v > 0.0f) lp = i;
    }
    seg_store(sh2, tid, s);  // (its barriers publish pre too)
    const double rbase = seg_base(sh2, tid), cp = pre;
    run = 0.0;
    long long h = INT64_MAX;
    for (int64_t i = b0; i < b1; ++i) {
        const float v = closest[i];
        run += (double)v;
        if (v > 0.0f && cp + (rbase + run) >= r) {
            h = i;
            break;
        }
    }
    if (h != INT64_MAX) atomicMin(&hit, h);
    if (lp >= 0) atomicMax(&lastpos, lp);
    __syncthreads();
    if (tid == 0) {
        long long row = hit != INT64_MAX ? hit : lastpos >= 0 ? lastpos : c0;
        if (row > V - 1) row = V - 1;
        cand_out[blockIdx.x] = (int32_t)row;
    }
}

static int pp_check(const char *who, int64_t V, int d, int T) {
    if (V < 1 || V > INT32_MAX)
        return set_error(COME_E_INVALID, "%s: V must be in [1, 2^31) (got %lld)", who,
                         (long long)V);
    if (d < 1 || d > kMaxDim)
        return set_error(COME_E_INVALID, "%s: d must be in [1, %d] (got %d)", who, kMaxDim, d);
    if (T < 1 || T > kPpMaxT)
        return set_error(COME_E_INVALID, "%s: T must be in [1, %d] (got %d)", who, kPpMaxT, T);
    return COME_OK;
}

static int pp_check_chunks(const char *who, int chunks, int T) {
    if (chunks < 1 || (int64_t)chunks * T * 8 > kPpPartialBytes)
        return set_error(COME_E_INVALID, "%s: chunks must be >= 1 with chunks * T * 8 <= 2 MB "
                                         "(got %d; see come_kmeans_pp_scratch)", who, chunks);
    return COME_OK;
}

template <int VEC, int G, int T>
static int pp_launch_t(int dev, const PpArgs &a, int t, int chunks, void *stream) {
    if (t == T)
        return launch(dev, k_pp_step<VEC, G, T>, "k_pp_step launch", dim3((unsigned)chunks),
                      dim3(256), {0}, stream, a);
    if constexpr (T > 1) return pp_launch_t<VEC, G, T - 1>(dev, a, t, chunks, stream);
    return set_error(COME_E_INVALID, "kmeans_pp_step: T must be in [1, %d]", kPpMaxT);
}

}  // namespace come

using namespace come;

extern "C" int come_kmeans_pp_scratch(int64_t V, int d, int T, int cus, int *chunks_out,
                                      int *rows_per_chunk_out) {
    int rc = pp_check("kmeans_pp_scratch", V, d, T);
    if (rc) return rc;
    if (!chunks_out || !rows_per_chunk_out) return set_error(COME_E_INVALID, "null pointer");
    int chunks;
    int64_t rows;
    pp_plan(V, T, cus, &chunks, &rows);
    *chunks_out = chunks;
    *rows_per_chunk_out = (int)rows;
    return COME_OK;
}

extern "C" int come_kmeans_pp_step(const float *x, int64_t V, int d, const float *closest,
                                   const int32_t *cand, int T, int chunks, float *dist_out,
                                   double *ppot, double *pots_out, void *stream) {
    int rc = pp_check("kmeans_pp_step", V, d, T);
    if (rc) return rc;
    rc = pp_check_chunks("kmeans_pp_step", chunks, T);
    if (rc) return rc;
    if (!x || !cand || !dist_out || !ppot || !pots_out)
        return set_error(COME_E_INVALID, "null pointer");
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    const PpArgs a{x, closest, cand, dist_out, ppot, V, pp_rows_per_chunk(V, chunks), d};
    if (d % 4 == 0 && (uintptr_t)x % 16 == 0)
        rc = pp_launch_t<4, 8, kPpMaxT>(dev, a, T, chunks, stream);
    else
        rc = pp_launch_t<1, 64, kPpMaxT>(dev, a, T, chunks, stream);
    if (rc) return rc;
    return launch(dev, k_pp_pots, "k_pp_pots launch", dim3((unsigned)T), dim3(kPpSegs), {0}, stream,
                  (const double *)ppot, chunks, T, pots_out);
}

extern "C" int come_kmeans_pp_pick(const float *dist, int64_t V, int T, const double *ppot,
                                   const double *pots, int chunks, float *closest_out,
                                   double *cpot_out, int32_t *best_out, double *pot_out,
                                   void *stream) {
    int rc = pp_check("kmeans_pp_pick", V, 1, T);
    if (rc) return rc;
    rc = pp_check_chunks("kmeans_pp_pick", chunks, T);
    if (rc) return rc;
    if (!dist || !ppot || !pots || !closest_out || !cpot_out || !best_out || !pot_out)
        return set_error(COME_E_INVALID, "null pointer");
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    const int64_t blocks = std::min<int64_t>((V + 255) / 256, (int64_t)8 * num_cus(dev));
    return launch(dev, k_pp_pick, "k_pp_pick launch", dim3((unsigned)blocks), dim3(256), {0},
                  stream, dist, V, T, ppot, pots, chunks, closest_out, cpot_out, best_out, pot_out);
}

extern "C" int come_kmeans_pp_sample(const float *closest, int64_t V, const double *cpot,
                                     int chunks, int rows_per_chunk, const double *u, int T,
                                     int32_t *cand_out, void *stream) {
    int rc = pp_check("kmeans_pp_sample", V, 1, T);
    if (rc) return rc;
    if (chunks < 1 || rows_per_chunk < 1 || (int64_t)chunks * rows_per_chunk < V)
        return set_error(COME_E_INVALID, "kmeans_pp_sample: chunks must be >= 1 with chunks * "
                                         "rows_per_chunk >= V (got %d x %d; see "
                                         "come_kmeans_pp_scratch)", chunks, rows_per_chunk);
    if (!closest || !cpot || !u || !cand_out) return set_error(COME_E_INVALID, "null pointer");
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    return launch(dev, k_pp_sample, "k_pp_sample launch", dim3((unsigned)T), dim3(kPpSegs), {0},
                  stream, closest, V, cpot, chunks, (int64_t)rows_per_chunk, u, cand_out);
}
