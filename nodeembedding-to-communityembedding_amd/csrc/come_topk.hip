// come_topk.hip -- exact top-k neighbour search over an embedding table (gfx950).
//
// come_topk: for every query row the k best base rows under dot, cosine or squared-L2, without the
// [Q, V] score matrix of topk(Q @ B.T): the grid is query tiles x base chunks, every (tile, chunk)
// keeps one k-entry list per query, the chunks' lists go to scratch ([chunks][Q][k] keys and
// indices) and k_topk_merge reduces them.  k_topk16 (d = 64, 128, 16-byte aligned operands: fp32
// MFMA scores, base tiles streamed through LDS) or k_topk_valu (any d <= kMaxDim: fmaf chains in
// feature order), then k_topk_merge; k_row_sqnorms gives the base rows' squared norms.
//
// Keys.  Inside a chunk a candidate is ranked by a key that leaves the query's own factor out, so
// that a score costs one VALU op on top of the dot product: key = fmaf(dot, mul_j, add_j) with
// (mul, add) = (1, 0) for dot, (1 / |b_j|, 0) for cosine (0 for a zero row) and (2, -|b_j|^2) for
// L2 -- larger is better for all three.  The merge turns a key into the reported score (cosine:
// key / |q|; L2: max(0, |q|^2 - key)) and orders by (score, index).
//
// Order.  Equal keys go to the lower base index; a NaN key passes no comparison and is never kept;
// an empty list entry is (-inf, INT32_MAX), the worst there is.  No float atomics, every list is
// owned by one wavefront: the result is bit-identical from run to run.

#include "come_c4.h"

namespace come {

constexpr int kTopkMaxK = 64;
constexpr int kTopkMaxChunks = 64;
constexpr int kTopkBT = 32;    // base rows per staged tile (two 16-column MFMA tiles)
constexpr int kTopkQT = 128;   // queries per workgroup of k_topk16: 4 wavefronts x 2 x 16 rows
constexpr int kTopkEmpty = 0x7fffffff;

struct TopkArgs {
    const float *q;
    const float *base;
    const float *bsq;        // [V] squared base norms (unused for dot)
    const int32_t *exclude;  // optional [Q]
    float *pkey;             // [chunks][Q][k]
    int32_t *pidx;           // [chunks][Q][k]
    int64_t Q;
    int64_t V;
    int64_t rows_per_chunk;
    int d;
    int k;
    int metric;
};

// chunks so that tiles x chunks is about `fill` workgroups per compute unit
static void tp_plan(int64_t Q, int64_t V, int d, int cus, int *chunks, int64_t *rows) {
    if (cus <= 0) cus = 256;
    const bool mfma = d == 64 || d == 128;
    const int64_t tiles = mfma ? (Q + kTopkQT - 1) / kTopkQT : Q;
    const int64_t want = (int64_t)(mfma ? 2 : 8) * cus;
    int64_t n = (want + tiles - 1) / tiles;
    n = std::min<int64_t>(n, kTopkMaxChunks);
    n = std::min<int64_t>(n, (V + kTopkBT - 1) / kTopkBT);
    n = std::max<int64_t>(n, 1);
    int64_t per = (V + n - 1) / n;
    per = (per + kTopkBT - 1) / kTopkBT * kTopkBT;
    *rows = per;
    *chunks = (int)((V + per - 1) / per);
}

// (mul, add) of base row j's key; a row past the chunk's end gets (0, -inf): its key is -inf (or
// NaN), which passes no threshold
__device__ __forceinline__ void key_terms(int metric, float bsq, bool live, float &mul, float &add) {
    mul = 1.0f;
    add = 0.0f;
    if (metric == COME_TOPK_COSINE) mul = bsq > 0.0f ? 1.0f / sqrtf(bsq) : (bsq == 0.0f ? 0.0f : bsq);
    if (metric == COME_TOPK_L2) {
        mul = 2.0f;
        add = -bsq;
    }
    if (!live) {
        mul = 0.0f;
        add = -INFINITY;
    }
}

// ---- a k-entry list held by the wavefront, entry e in lane e ------------------------------------
// An entry is ranked by one 64-bit word: the key as an order-preserving unsigned (high half) and
// INT32_MAX - index (low half), so the smallest word is the worst entry -- lowest key, among equal
// keys the highest index -- and an empty entry (-inf, INT32_MAX) is below every real one.  Lanes
// >= k hold the all-ones word.
__device__ __forceinline__ uint32_t key_bits(float s) {
    const uint32_t u = __float_as_uint(s + 0.0f);  // (-0 -> +0: equal keys, equal words)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bits_key(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ unsigned long long entry_word(float s, int i) {
    return ((unsigned long long)key_bits(s) << 32) | (uint32_t)(kTopkEmpty - i);
}

// x of this lane and of its partner of butterfly stage S, in either order (come_wave.h's partners:
// DPP quad_perm / row mirrors, then gfx950's permlane swaps; all VALU).  Valid for a reduction whose
// stages leave every lane of a group with the same value, as a minimum does.
template <int S>
__device__ __forceinline__ void stage_pair(uint32_t x, uint32_t &a, uint32_t &b) {
    constexpr int ctrl = S == 0 ? 0xB1 : S == 1 ? 0x4E : S == 2 ? 0x141 : 0x140;
    if constexpr (S < 4) {
        a = x;
        b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, 0xF, 0xF, false);
    } else if constexpr (S == 4) {
        const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
        a = r[0];
        b = r[1];
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
        a = r[0];
        b = r[1];
    }
}
template <int S>
__device__ __forceinline__ void stage_pair64(unsigned long long x, unsigned long long &a,
                                             unsigned long long &b) {
    uint32_t al, bl, ah, bh;
    stage_pair<S>((uint32_t)x, al, bl);
    stage_pair<S>((uint32_t)(x >> 32), ah, bh);
    a = ((unsigned long long)ah << 32) | al;
    b = ((unsigned long long)bh << 32) | bl;
}
// the smallest (m1) and second smallest (m2) of the 64 lanes' words, in every lane
template <int S>
__device__ __forceinline__ void two_min_stage(unsigned long long &m1, unsigned long long &m2) {
    unsigned long long a1, b1, a2, b2;
    stage_pair64<S>(m1, a1, b1);
    stage_pair64<S>(m2, a2, b2);
    m1 = a1 < b1 ? a1 : b1;
    const unsigned long long hi = a1 < b1 ? b1 : a1, lo2 = a2 < b2 ? a2 : b2;
    m2 = hi < lo2 ? hi : lo2;
}

// Inserts candidate (cs, ci) if it beats the worst entry; returns the key of the worst entry
// afterwards: the list's threshold.  One reduction: with the worst entry replaced, the worst is the
// smaller of the candidate and the old second worst.
__device__ __forceinline__ float list_insert(float &es, int &ei, float cs, int ci, int k) {
    const int lane = (int)(threadIdx.x & 63);
    const unsigned long long w = lane < k ? entry_word(es, ei) : ~0ULL;
    unsigned long long m1 = w, m2 = ~0ULL;
    two_min_stage<0>(m1, m2);
    two_min_stage<1>(m1, m2);
    two_min_stage<2>(m1, m2);
    two_min_stage<3>(m1, m2);
    two_min_stage<4>(m1, m2);
    two_min_stage<5>(m1, m2);
    const unsigned long long cw = entry_word(cs, ci);
    if (!(cw > m1)) return bits_key((uint32_t)(m1 >> 32));
    const int wl = __builtin_ctzll(__ballot(w == m1));  // (empty entries are equal: the first)
    if (lane == wl) {
        es = cs;
        ei = ci;
    }
    return bits_key((uint32_t)((cw < m2 ? cw : m2) >> 32));
}

// ---- d = 64, 128: scores on v_mfma_f32_16x16x4_f32 -------------------------------------------
//
// Workgroup (bx, by) = queries 128 bx .. + 127 against chunk by.  Wavefront w owns query rows 32 w
// .. + 31 as two 16-row sub-tiles, held for the whole chunk as A operands in k_kmeans_lloyd16's
// layout (lane (i = l % 16, g = l / 16) has features 16 t + 4 g .. + 3 of row i).  The workgroup
// stages 32 base rows at a time into LDS (rows padded by 4 floats, double-buffered: the next tile's
// global loads are in flight while this one is multiplied, one barrier per tile) with the rows'
// (mul, add) beside them.  The scores of sub-tile s, query row 4 g + r against base row 16 ct + j
// land in register r of accumulator [s][ct] of lane (j, g); the row's threshold -- the key of the
// worst entry of its list, -inf while the list is short -- sits in thr[s][r] of the 16 lanes of
// group g.  Only if some key of the wavefront passes its threshold does anything else happen: each
// passing candidate is inserted into its row's list in LDS ([128][k] keys, [128][k] indices; the
// wavefront reads the k entries one per lane) and the row's threshold is refreshed.  The filter
// is strict: an equal key met later in the chunk has a higher index and loses; inside one tile the
// insertion compares (key, index) in full, whatever the order candidates are taken in.
template <int D>
__global__ void __launch_bounds__(256) k_topk16(TopkArgs a) {
    using f32x4 = __attribute__((ext_vector_type(4))) float;
    constexpr int LD = D + 4, NT = D / 16, BT = kTopkBT;
    constexpr int NLD = BT * (D / 4) / 256;  // float4 loads per thread per tile
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *Bs = smem;                              // [2][BT][LD]
    float *bmul = Bs + 2 * BT * LD;                // [2][BT]
    float *badd = bmul + 2 * BT;                   // [2][BT]
    int *excl = reinterpret_cast<int *>(badd + 2 * BT);  // [128]
    float *lkey = reinterpret_cast<float *>(excl + kTopkQT);  // [128][k]
    int *lidx = reinterpret_cast<int *>(lkey + kTopkQT * a.k);  // [128][k]
    const int tid = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int j = lane & 15, g = lane >> 4;
    const int k = a.k, metric = a.metric;
    const int64_t q0 = (int64_t)blockIdx.x * kTopkQT;
    const int64_t chunk = blockIdx.y;
    const int64_t c0 = chunk * a.rows_per_chunk;
    int64_t c1 = c0 + a.rows_per_chunk;
    if (c1 > a.V) c1 = a.V;

    for (int o = tid; o < kTopkQT * k; o += 256) {
        lkey[o] = -INFINITY;
        lidx[o] = kTopkEmpty;
    }
    if (tid < kTopkQT) {
        const int64_t qr = q0 + tid;
        excl[tid] = (a.exclude && qr < a.Q) ? a.exclude[qr] : -1;
    }
    f32x4 xv[2][NT];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        int64_t qr = q0 + 32 * wid + 16 * s + j;
        if (qr >= a.Q) qr = a.Q - 1;
        const float *xr = a.q + qr * D + 4 * g;
#pragma unroll
        for (int t = 0; t < NT; ++t) xv[s][t] = *reinterpret_cast<const f32x4 *>(xr + 16 * t);
    }
    float thr[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r)  // (a row past Q: +inf, nothing passes)
            thr[s][r] = q0 + 32 * wid + 16 * s + 4 * g + r < a.Q ? -INFINITY : INFINITY;
    const bool wave_live = q0 + 32 * wid < a.Q;  // a wavefront without queries only stages

    // staging: thread tid moves float4 slots tid, tid + 256, ... of the tile; threads < BT also
    // the row's key terms
    f32x4 st[NLD];
    float sm = 0.0f, sa = 0.0f;
    auto fetch = [&](int64_t r0) {
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int o = tid + 256 * u, row = o / (D / 4), c4 = o % (D / 4);
            const int64_t br = r0 + row < c1 ? r0 + row : c1 - 1;
            st[u] = *reinterpret_cast<const f32x4 *>(a.base + br * D + 4 * c4);
        }
        if (tid < BT) {
            const bool live = r0 + tid < c1;
            const float bsq = (metric != COME_TOPK_DOT && live) ? a.bsq[r0 + tid] : 0.0f;
            key_terms(metric, bsq, live, sm, sa);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int o = tid + 256 * u, row = o / (D / 4), c4 = o % (D / 4);
            *reinterpret_cast<f32x4 *>(Bs + (buf * BT + row) * LD + 4 * c4) = st[u];
        }
        if (tid < BT) {
            bmul[buf * BT + tid] = sm;
            badd[buf * BT + tid] = sa;
        }
    };
    // one staged tile: scores, keys, filter, and the insertions of what passed
    auto multiply = [&](int64_t r0, int buf) {
        f32x4 acc[2][2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[s][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const float *bt = Bs + buf * BT * LD;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const f32x4 b =
                    *reinterpret_cast<const f32x4 *>(bt + (16 * ct + j) * LD + 16 * t + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        acc[s][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s][t][e], b[e],
                                                                         acc[s][ct], 0, 0, 0);
            }
        bool any = false;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const float m = bmul[buf * BT + 16 * ct + j], ad = badd[buf * BT + 16 * ct + j];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc[s][ct][r] = __builtin_fmaf(acc[s][ct][r], m, ad);
                    any |= acc[s][ct][r] > thr[s][r];
                }
        }
        if (__ballot(any) != 0) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const float key = acc[s][ct][r];
                        unsigned long long mask = __ballot(key > thr[s][r]);
                        while (mask) {
                            const int src = __builtin_ctzll(mask);
                            mask &= mask - 1;
                            const int sj = src & 15, sg = src >> 4;
                            const int row = 32 * wid + 16 * s + 4 * sg + r;
                            const float cs = __shfl(key, src);
                            const int ci = (int)(r0 + 16 * ct + sj);
                            if (ci == excl[row]) continue;
                            float es = INFINITY;
                            int ei = -1;
                            if (lane < k) {
                                es = lkey[row * k + lane];
                                ei = lidx[row * k + lane];
                            }
                            const float nt = list_insert(es, ei, cs, ci, k);
                            if (lane < k) {
                                lkey[row * k + lane] = es;
                                lidx[row * k + lane] = ei;
                            }
                            if (g == sg) thr[s][r] = nt;
                        }
                    }
        }
    };
    fetch(c0);
    stash(0);
    __syncthreads();
    int buf = 0;
    for (int64_t r0 = c0; r0 < c1; r0 += BT, buf ^= 1) {
        const bool more = r0 + BT < c1;
        if (more) fetch(r0 + BT);
        if (wave_live) multiply(r0, buf);
        if (more) stash(buf ^ 1);
        __syncthreads();
    }
    // the wavefront's 32 lists -> the chunk's slice (rows past Q are not stored)
    for (int rr = 0; rr < 32; ++rr) {
        const int row = 32 * wid + rr;
        const int64_t qr = q0 + row;
        if (qr >= a.Q) break;
        if (lane < k) {
            const int64_t o = (chunk * a.Q + qr) * k + lane;
            a.pkey[o] = lkey[row * k + lane];
            a.pidx[o] = lidx[row * k + lane];
        }
    }
}

// ---- any d <= kMaxDim, any alignment, on the VALU ---------------------------------------------
// One wavefront = (query, chunk): the query sits in LDS, lane l scores base rows c0 + l, c0 + l +
// 64, ... by an fmaf chain in feature order, and the list lives in registers, entry e in lane e.
// Passing candidates are inserted in ascending index order.
__global__ void __launch_bounds__(64) k_topk_valu(TopkArgs a) {
    __shared__ float qs[kMaxDim];
    const int lane = threadIdx.x, d = a.d, k = a.k, metric = a.metric;
    const int64_t qr = blockIdx.x, chunk = blockIdx.y;
    const int64_t c0 = chunk * a.rows_per_chunk;
    int64_t c1 = c0 + a.rows_per_chunk;
    if (c1 > a.V) c1 = a.V;
    for (int c = lane; c < d; c += 64) qs[c] = a.q[qr * d + c];
    __syncthreads();
    const int ex = a.exclude ? a.exclude[qr] : -1;
    float es = lane < k ? -INFINITY : INFINITY;
    int ei = lane < k ? kTopkEmpty : -1;
    float thr = -INFINITY;
    for (int64_t r0 = c0; r0 < c1; r0 += 64) {
        const int64_t br = r0 + lane;
        const bool live = br < c1;
        const float *b = a.base + (live ? br : c1 - 1) * d;
        float dot = 0.0f;
        for (int c = 0; c < d; ++c) dot = __builtin_fmaf(qs[c], b[c], dot);
        const float bsq = (metric != COME_TOPK_DOT && live) ? a.bsq[br] : 0.0f;
        float m, ad;
        key_terms(metric, bsq, live, m, ad);
        const float key = __builtin_fmaf(dot, m, ad);
        unsigned long long mask = __ballot(key > thr);
        while (mask) {
            const int src = __builtin_ctzll(mask);
            mask &= mask - 1;
            const float cs = __shfl(key, src);
            const int ci = (int)(r0 + src);
            if (ci == ex) continue;
            thr = list_insert(es, ei, cs, ci, k);
        }
    }
    if (lane < k) {
        const int64_t o = (chunk * a.Q + qr) * k + lane;
        a.pkey[o] = es;
        a.pidx[o] = ei;
    }
}

// ---- merge --------------------------------------------------------------------------------------
// One wavefront per query: the chunks' chunks * k candidates become reported scores (the query's
// factor applied: cosine key / |q|, L2 max(0, |q|^2 - key)), and k rounds each take the best
// candidate after the one taken before, in the order (score best first, index ascending): every
// lane scans candidates lane, lane + 64, ..., then the wavefront reduces.  Rounds that find nothing
// write the tail: index -1, score -inf (+inf for L2).
__global__ void __launch_bounds__(64)
    k_topk_merge(const float *q, const float *pkey, const int32_t *pidx, int64_t Q, int d, int k,
                 int chunks, int metric, int32_t *idx_out, float *score_out) {
    const int lane = threadIdx.x;
    const int64_t qr = blockIdx.x;
    float qf = 0.0f;
    if (metric != COME_TOPK_DOT) {
        // |q|^2 by one fmaf chain in feature order (every lane the same chain)
        float s = 0.0f;
        for (int c = 0; c < d; ++c) s = __builtin_fmaf(q[qr * d + c], q[qr * d + c], s);
        qf = s;
        if (metric == COME_TOPK_COSINE) qf = s > 0.0f ? 1.0f / sqrtf(s) : (s == 0.0f ? 0.0f : s);
    }
    const bool l2 = metric == COME_TOPK_L2;
    const int n = chunks * k;
    // rank value: larger is better (L2: the negated distance)
    float ps = INFINITY;
    int pi = -1;
    for (int round = 0; round < k; ++round) {
        float bs = -INFINITY;
        int bi = kTopkEmpty;
        for (int c = lane; c < n; c += 64) {
            const int64_t o = ((int64_t)(c / k) * Q + qr) * k + (c % k);
            const int ci = pidx[o];
            if (ci == kTopkEmpty) continue;
            const float key = pkey[o];
            float v = key;
            if (metric == COME_TOPK_COSINE) v = key * qf;
            if (l2) v = -fmaxf(0.0f, qf - key);
            if (!(v < ps || (v == ps && ci > pi))) continue;  // taken already (or NaN)
            if (v > bs || (v == bs && ci < bi)) {
                bs = v;
                bi = ci;
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const float os = __shfl_xor(bs, m);
            const int oi = __shfl_xor(bi, m);
            if (os > bs || (os == bs && oi < bi)) {
                bs = os;
                bi = oi;
            }
        }
        const bool found = bi != kTopkEmpty;
        if (lane == 0) {
            idx_out[qr * k + round] = found ? bi : -1;
            score_out[qr * k + round] = found ? (l2 ? -bs : bs) : (l2 ? INFINITY : -INFINITY);
        }
        if (found) {
            ps = bs;
            pi = bi;
        } else {
            ps = -INFINITY;
            pi = kTopkEmpty;  // nothing is after this: the remaining rounds write the tail
        }
    }
}

// ---- squared row norms -----------------------------------------------------------------------
// out[r] = sum_c x[r][c]^2 as one fp32 fmaf chain in feature order, one thread per row.
__global__ void __launch_bounds__(256) k_row_sqnorms(const float *x, int64_t V, int d, float *out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= V) return;
    const float *xr = x + r * d;
    float s = 0.0f;
    for (int c = 0; c < d; ++c) s = __builtin_fmaf(xr[c], xr[c], s);
    out[r] = s;
}

static int tp_check(const char *who, int64_t Q, int64_t V, int d, int k) {
    if (Q < 1) return set_error(COME_E_INVALID, "%s: Q must be >= 1 (got %lld)", who, (long long)Q);
    if (V < 1 || V > INT32_MAX)
        return set_error(COME_E_INVALID, "%s: V must be in [1, 2^31) (got %lld)", who, (long long)V);
    if (d < 1 || d > kMaxDim)
        return set_error(COME_E_INVALID, "%s: d must be in [1, %d] (got %d)", who, kMaxDim, d);
    if (k < 1 || k > kTopkMaxK)
        return set_error(COME_E_INVALID, "%s: k must be in [1, %d] (got %d)", who, kTopkMaxK, k);
    return COME_OK;
}

static int sqnorms_launch(int dev, const float *x, int64_t V, int d, float *out, void *stream) {
    return launch(dev, k_row_sqnorms, "k_row_sqnorms launch", dim3((unsigned)((V + 255) / 256)),
                  dim3(256), {0}, stream, x, V, d, out);
}

}  // namespace come

using namespace come;

extern "C" int come_topk_scratch(int64_t Q, int64_t V, int d, int k, int cus, int *chunks_out,
                                 int64_t *rows_per_chunk_out) {
    int rc = tp_check("topk_scratch", Q, V, d, k);
    if (rc) return rc;
    if (!chunks_out || !rows_per_chunk_out)
        return set_error(COME_E_INVALID, "topk_scratch: null pointer");
    tp_plan(Q, V, d, cus, chunks_out, rows_per_chunk_out);
    return COME_OK;
}

extern "C" int come_row_sqnorms(const float *x, int64_t V, int d, float *out, void *stream) {
    if (V < 1 || V > INT32_MAX)
        return set_error(COME_E_INVALID, "row_sqnorms: V must be in [1, 2^31) (got %lld)",
                         (long long)V);
    if (d < 1 || d > kMaxDim)
        return set_error(COME_E_INVALID, "row_sqnorms: d must be in [1, %d] (got %d)", kMaxDim, d);
    if (!x || !out) return set_error(COME_E_INVALID, "row_sqnorms: null pointer");
    int dev;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    return sqnorms_launch(dev, x, V, d, out, stream);
}

extern "C" int come_topk(const float *q, int64_t Q, const float *base, int64_t V, int d, int k,
                         int metric, const int32_t *exclude, const float *base_sq, int chunks,
                         void *scratch, int32_t *idx_out, float *score_out, void *stream) {
    int rc = tp_check("topk", Q, V, d, k);
    if (rc) return rc;
    if (metric != COME_TOPK_DOT && metric != COME_TOPK_COSINE && metric != COME_TOPK_L2)
        return set_error(COME_E_INVALID, "topk: unknown metric %d", metric);
    if (chunks < 1 || chunks > kTopkMaxChunks)
        return set_error(COME_E_INVALID, "topk: chunks must be in [1, %d] (got %d; see "
                                         "come_topk_scratch)", kTopkMaxChunks, chunks);
    if (!q || !base || !scratch || !idx_out || !score_out)
        return set_error(COME_E_INVALID, "topk: null pointer");
    if ((uintptr_t)scratch % 4)
        return set_error(COME_E_INVALID, "topk: scratch must be 4-byte aligned");
    int dev;
    rc = ensure_init(&dev);
    if (rc) return rc;
    int64_t per = (V + chunks - 1) / chunks;
    per = (per + kTopkBT - 1) / kTopkBT * kTopkBT;
    const int used = (int)((V + per - 1) / per);
    // scratch: float keys [chunks][Q][k], int32 indices [chunks][Q][k], then float |b|^2 [V] when
    // the caller gave none
    float *pkey = reinterpret_cast<float *>(scratch);
    int32_t *pidx = reinterpret_cast<int32_t *>(pkey + (int64_t)chunks * Q * k);
    if (!base_sq && metric != COME_TOPK_DOT) {
        float *own = reinterpret_cast<float *>(pidx + (int64_t)chunks * Q * k);
        rc = sqnorms_launch(dev, base, V, d, own, stream);
        if (rc) return rc;
        base_sq = own;
    }
    const TopkArgs a{q, base, base_sq, exclude, pkey, pidx, Q, V, per, d, k, metric};
    const bool mfma = (d == 64 || d == 128) && ((uintptr_t)q % 16) == 0 &&
                      ((uintptr_t)base % 16) == 0;
    if (mfma) {
        const dim3 grid((unsigned)((Q + kTopkQT - 1) / kTopkQT), (unsigned)used);
        const size_t lds = sizeof(float) * (2 * kTopkBT * (d + 4) + 4 * kTopkBT + kTopkQT +
                                            2 * (size_t)kTopkQT * k);
        rc = with_width(d, [&](auto width) {
            constexpr int D = decltype(width)::value;
            return launch(dev, k_topk16<D>, "k_topk16 launch", grid, dim3(256), {lds}, stream, a);
        });
    } else {
        rc = launch(dev, k_topk_valu, "k_topk_valu launch", dim3((unsigned)Q, (unsigned)used),
                    dim3(64), {0}, stream, a);
    }
    if (rc) return rc;
    return launch(dev, k_topk_merge, "k_topk_merge launch", dim3((unsigned)Q), dim3(64), {0}, stream,
                  q, (const float *)pkey, (const int32_t *)pidx, Q, d, k, used, metric, idx_out,
                  score_out);
}
