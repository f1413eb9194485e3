// come_sgns_loss.hip -- the SGNS objectives O1 / O2 as losses (gfx950).
//
// A loss pass is the training launch without its write half: the same pair enumeration
// (pyx:494-508), the same LCG negative draws (pyx:133-135) and the same row gathers as
// come_sgns_o2, and no store to either table.  For an input row a, a positive row b and negative
// rows t_1..t_n:
//   pair = softplus(-f(a, b)) + sum_k softplus(f(a, t_k)),   softplus(z) = log(1 + e^z)
// the exact objective (no +-6 skip, no sigmoid table).  f is the trainer's fp32 dot (lane_partial
// + the xor butterfly of come_sgns_common.h), softplus is float64 on that fp32 value.
//   k_sgns_o2_loss     one wavefront per walk: the centre's ctx row stays in registers over its
//                      window partners, the window's walk entries sit one per lane (spans of at
//                      most 64 positions), negatives come from the trainer's DrawBatch
//   k_sgns_pairs_loss  one wavefront per explicit (input, positive, negatives) pair, grid-stride
//   k_loss_partial / k_loss_total   the per-walk (per-pair) doubles and counts summed by a fixed
//                      two-level tree
// Lane k of a pair holds f_k (k = 0 the positive), so the 1 + n softplus evaluations run at once;
// the pair's terms are then added in k order, a walk's pairs in the trainer's order.  No float or
// double atomics: every output is bit-identical from run to run, and the total is the same whether
// the per-walk output goes to the caller's buffer or to library scratch.

#include <math.h>

#include "come_c4.h"
#include "come_sgns_common.h"

namespace come {

constexpr int kLossChunk = 5;       // target rows gathered together (n = 5: one chunk per pair)
constexpr int kLossSumBlock = 4096;  // values per first-level workgroup of the total

struct O2LossArgs {
    const float *node;
    const float *ctx;
    const int32_t *walks;
    const uint64_t *seeds;
    const uint32_t *table;
    int V;
    int P;
    int L;
    int d;
    int window;
    int negative;
    FastMod fm;
    int packed;
    int64_t *counter;  // work queue (nullptr = grid-stride)
    double *vals;      // [P] the walks' sums
    int32_t *cnt;      // [P] the walks' pair counts
};

struct PairsLossArgs {
    const float *inp;
    const float *out;
    const int32_t *rows_in;
    const int32_t *rows_pos;
    const int32_t *rows_neg;
    int V;
    int M;
    int d;
    int negative;
    double *vals;  // [M]
    int32_t *cnt;  // [M] 1 for a counted pair
};

// Row loads of the loss kernels, without a lane mask per register (Row::load keeps VEC of them in
// scalar registers, which these kernels do not have to spare).  The widths of a VEC (with_row, as
// the trainer's kernel_set) are 64 (VEC / 2) < d <= 64 VEC (VEC = 1: 1 <= d <= 64), so a register
// below VEC / 2 lies wholly inside the row.  In the others a lane whose element is past d reads
// element d - 1 instead (in bounds; a stray value), and zero_tail() then clears those lanes of the
// pair's INPUT row: every dot of a pair has the input row as a factor, so a stray element of a
// positive or negative row meets a zero and adds +-0 to its lane's fmaf chain, as Row::load's
// zeros do.
template <int VEC, bool FULL>
__device__ inline void load_row(Row<VEC, FULL> &r, const float *__restrict__ row, int lane,
                                int d) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const int e = lane + 64 * i;
        r.v[i] = row[(FULL || i < VEC / 2) ? e : (e < d - 1 ? e : d - 1)];
    }
}

// r.v[i] *= 1 where the lane's element is below d, 0 where it is not (x * 1.0f is x)
template <int VEC, bool FULL>
__device__ inline void zero_tail(Row<VEC, FULL> &r, int lane, int d) {
    if (FULL) return;
#pragma unroll
    for (int i = VEC / 2; i < VEC; ++i) {
        const int left = d - (lane + 64 * i);  // > 0 inside the row
        r.v[i] *= (float)(left < 0 ? 0 : (left > 1 ? 1 : left));
    }
}

__device__ inline double readlane_f64(double v, int lane) {
    return __builtin_bit_cast(double, readlane_u64(__builtin_bit_cast(uint64_t, v), lane));
}

// The dots of up to 64 targets, one per lane, waiting for their softplus: a pair takes 1 + n
// consecutive slots (slot 0 of a pair is its positive), so at n = 5 ten pairs share one float64
// evaluation in which 60 lanes work, instead of ten evaluations with 6 lanes each.
struct TermBatch {
    float f;    // lane l: the dot of slot l
    float sign; // lane l: -1 for a positive's slot (l % (1 + n) == 0), else +1
    int live;   // lane l: slot l takes part (0 for a skipped negative)
    int fill;   // slots in use (wave-uniform)
};

// One pair with its input row `in` and positive row `pos` in registers, into the next 1 + n slots
// of `tb` (the caller has made room).  Negative k (1..n) is row readlane(tv, toff + k - 1) of
// `out`; it is skipped when it equals `skip` or lies outside [0, V) (a skipped target's gather
// reads row 0 and is discarded: the loads stay unconditional).
template <int VEC, bool FULL>
__device__ inline void pair_dots(TermBatch &tb, const Row<VEC, FULL> &in,
                                 const Row<VEC, FULL> &pos, const float *__restrict__ out,
                                 int V, int d, uint32_t tv, int toff, int n, int skip,
                                 int lane) {
    using R = Row<VEC, FULL>;
    const int s0 = tb.fill;
    const float f0 = wave_sum(lane_partial(in, pos));
    if (lane == s0) {
        tb.f = f0;
        tb.live = 1;
    }
    for (int k0 = 0; k0 < n; k0 += kLossChunk) {
        R r[kLossChunk];
        float part[kLossChunk];
        uint32_t okm = 0;  // bit c: target k0 + c + 1 takes part
#pragma unroll
        for (int c = 0; c < kLossChunk; ++c) {
            part[c] = 0.0f;
            if (k0 + c < n) {
                const int t = (int)readlane_u32(tv, toff + k0 + c);
                const bool ok = t != skip && t >= 0 && t < V;
                okm |= (ok ? 1u : 0u) << c;
                load_row(r[c], out + (int64_t)(ok ? t : 0) * d, lane, d);
            }
        }
#pragma unroll
        for (int c = 0; c < kLossChunk; ++c)
            if (k0 + c < n) part[c] = lane_partial(in, r[c]);
        wave_sum_all(part);
#pragma unroll
        for (int c = 0; c < kLossChunk; ++c)
            if (lane == s0 + 1 + k0 + c) {
                tb.f = part[c];
                tb.live = (int)((okm >> c) & 1u);
            }
    }
    tb.fill = s0 + 1 + n;
}

// softplus of every live slot in float64 (max(z, 0) + log1p(exp(-|z|)), z = -f for a positive),
// then each pair's terms added in slot order from 0.0 (a skipped slot adds +0.0) and handed to
// done(q, value) in pair order.  Leaves the batch empty.
template <class F>
__device__ inline void batch_flush(TermBatch &tb, int n, int lane, F &&done) {
    double term = 0.0;
    if (lane < tb.fill && tb.live) {
        const double z = (double)(tb.sign * tb.f);
        term = fmax(z, 0.0) + log1p(exp(-fabs(z)));
    }
    int q = 0;
    for (int s0 = 0; s0 < tb.fill; s0 += n + 1, ++q) {
        double s = 0.0;
        for (int k = 0; k <= n; ++k) s += readlane_f64(term, s0 + k);
        done(q, s);
    }
    tb.fill = 0;
}

template <int VEC, bool FULL>
__global__ void __launch_bounds__(256) k_sgns_o2_loss(O2LossArgs a) {
    using R = Row<VEC, FULL>;
    const int lane = threadIdx.x & 63;
    // (the grid is at most 8 four-wave workgroups per CU: 32-bit wave numbers)
    const int gw = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    const int nwaves = (int)(gridDim.x * (blockDim.x >> 6));
    const LcgLane lc = lcg_lane_constants(lane);
    const int d = a.d, n = a.negative;
    const int path_len = a.L < kMaxSentenceLen ? a.L : kMaxSentenceLen;  // pyx:480
    TermBatch tb{0.0f, lane % (n + 1) == 0 ? -1.0f : 1.0f, 0, 0};

    for (int64_t p = a.counter ? next_unit(a.counter, 0, 0, lane) : gw; p < a.P;
         p = next_unit(a.counter, p, nwaves, lane)) {
        const int32_t *__restrict__ idx = a.walks + p * (int64_t)a.L;
        DrawBatch db;
        db.used = 0;
        db.base = uniform64(a.seeds[p]);
        db.target = 0;
        if (n > 0) draws_fill(db, db.base, lc, a);
        double wsum = 0.0;  // the walk's pairs, added in the trainer's order
        int pairs = 0;
        auto add = [&](int, double v) { wsum += v; };
        for (int i = 0; i < path_len; ++i) {
            const int j0 = i - a.window < 0 ? 0 : i - a.window;
            const int j1 = (int64_t)i + a.window + 1 > path_len ? path_len : i + a.window + 1;
            // the window's entries one per lane when they fit (window <= 31, or a short walk)
            const bool inreg = j1 - j0 <= 64;
            int wv = -1;
            if (inreg && lane < j1 - j0) wv = idx[j0 + lane];
            const int ci = inreg ? (int)readlane_u32((uint32_t)wv, i - j0) : uniform(idx[i]);
            if (ci < 0 || ci >= a.V) continue;  // codelens[i] == 0 (pyx:495)
            R pos;
            load_row(pos, a.ctx + (int64_t)ci * d, lane, d);
            for (int j = j0; j < j1; ++j) {
                if (j == i) continue;
                const int cj = inreg ? (int)readlane_u32((uint32_t)wv, j - j0) : uniform(idx[j]);
                if (cj < 0 || cj >= a.V) continue;  // pyx:504
                R in;
                load_row(in, a.node + (int64_t)cj * d, lane, d);
                zero_tail(in, lane, d);
                if (n > 0 && db.used + n > 64) draws_fill(db, draws_state_at_used(db, lc), lc, a);
                if (tb.fill + n + 1 > 64) batch_flush(tb, n, lane, add);
                pair_dots<VEC, FULL>(tb, in, pos, a.ctx, a.V, d, db.target, db.used, n, ci, lane);
                db.used += n;
                ++pairs;
            }
        }
        batch_flush(tb, n, lane, add);
        if (lane == 0) {
            a.vals[p] = wsum;
            a.cnt[p] = pairs;
        }
    }
}

template <int VEC, bool FULL>
__global__ void __launch_bounds__(256) k_sgns_pairs_loss(PairsLossArgs a) {
    using R = Row<VEC, FULL>;
    const int lane = threadIdx.x & 63;
    // (the grid is at most 8 four-wave workgroups per CU: 32-bit wave numbers)
    const int gw = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    const int nwaves = (int)(gridDim.x * (blockDim.x >> 6));
    const int d = a.d, n = a.negative;
    TermBatch tb{0.0f, lane % (n + 1) == 0 ? -1.0f : 1.0f, 0, 0};
    int64_t mq = 0;  // lane q: the pair index of the batch's q-th pair
    auto put = [&](int q, double v) {
        const int64_t m = (int64_t)readlane_u64((uint64_t)mq, q);
        if (lane == 0) a.vals[m] = v;
    };
    for (int64_t m = gw; m < a.M; m += nwaves) {
        const int ri = uniform(a.rows_in[m]), rp = uniform(a.rows_pos[m]);
        uint32_t tv = 0xFFFFFFFFu;
        if (lane < n) tv = (uint32_t)a.rows_neg[m * (int64_t)n + lane];
        const bool counted = ri >= 0 && ri < a.V && rp >= 0 && rp < a.V;
        if (lane == 0) {
            a.cnt[m] = counted ? 1 : 0;
            if (!counted) a.vals[m] = 0.0;
        }
        if (!counted) continue;
        R in, pos;
        load_row(in, a.inp + (int64_t)ri * d, lane, d);
        zero_tail(in, lane, d);
        load_row(pos, a.out + (int64_t)rp * d, lane, d);
        if (tb.fill + n + 1 > 64) batch_flush(tb, n, lane, put);
        if (lane == tb.fill / (n + 1)) mq = m;
        pair_dots<VEC, FULL>(tb, in, pos, a.out, a.V, d, tv, 0, n, -1, lane);
    }
    batch_flush(tb, n, lane, put);
}

// 256 values per thread-strided pass, then a tree over the 256 threads: the order depends on the
// number of values alone.
__device__ inline void block_sum(double v, int64_t c, double *outv, int64_t *outc) {
    __shared__ double sv[256];
    __shared__ int64_t sc[256];
    sv[threadIdx.x] = v;
    sc[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sv[threadIdx.x] += sv[threadIdx.x + o];
            sc[threadIdx.x] += sc[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *outv = sv[0];
        *outc = sc[0];
    }
}

// first level: workgroup b adds values [b * kLossSumBlock, (b + 1) * kLossSumBlock)
__global__ void __launch_bounds__(256) k_loss_partial(const double *__restrict__ vals,
                                                      const int32_t *__restrict__ cnt, int64_t n,
                                                      double *__restrict__ psum,
                                                      int64_t *__restrict__ pcnt) {
    const int64_t lo = (int64_t)blockIdx.x * kLossSumBlock;
    const int64_t hi = lo + kLossSumBlock < n ? lo + kLossSumBlock : n;
    double v = 0.0;
    int64_t c = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        v += vals[i];
        c += cnt[i];
    }
    block_sum(v, c, psum + blockIdx.x, pcnt + blockIdx.x);
}

// second level: one workgroup adds the partials (k_comm_loss_sum's order)
__global__ void __launch_bounds__(256) k_loss_total(const double *__restrict__ psum,
                                                    const int64_t *__restrict__ pcnt, int64_t n,
                                                    double *__restrict__ loss_out,
                                                    int64_t *__restrict__ pairs_out) {
    double v = 0.0;
    int64_t c = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        v += psum[i];
        c += pcnt[i];
    }
    __shared__ int64_t total_c;
    block_sum(v, c, loss_out, &total_c);
    __syncthreads();
    if (threadIdx.x == 0 && pairs_out) *pairs_out = total_c;
}

// f(std::integral_constant<int, VEC>{}, std::integral_constant<bool, FULL>{}) for row width d
template <typename F>
static int with_row(int d, F &&f) {
    const int vec = d <= 64 ? 1 : d <= 128 ? 2 : d <= 256 ? 4 : 8;
    const bool full = vec > 1 && d == 64 * vec;
#define COME_ROW(V)                                                            \
    case V:                                                                    \
        return full ? f(std::integral_constant<int, V>{}, std::true_type{})    \
                    : f(std::integral_constant<int, V>{}, std::false_type{});
    switch (vec) {
        case 1:  // d <= 64 is never FULL (as the trainer's kernel_set)
            return f(std::integral_constant<int, 1>{}, std::false_type{});
        COME_ROW(2)
        COME_ROW(4)
        default:
            COME_ROW(8)
    }
#undef COME_ROW
}

static int check_tables(const char *who, int64_t V, int d, int negative) {
    if (V <= 0) return set_error(COME_E_INVALID, "%s: V must be > 0 (got %lld)", who, (long long)V);
    if (V > INT32_MAX)
        return set_error(COME_E_INVALID, "%s: V must fit int32 row indices (got %lld)", who,
                         (long long)V);
    if (d < 1 || d > kMaxDim)
        return set_error(COME_E_INVALID, "%s: d must be in [1, %d] (got %d)", who, kMaxDim, d);
    if (negative < 0 || negative > kMaxNegative)
        return set_error(COME_E_INVALID, "%s: negative must be in [0, %d] (got %d)", who,
                         kMaxNegative, negative);
    return COME_OK;
}

// The per-unit doubles (the caller's buffer or scratch) and counts, then the two-level total.
struct LossBuffers {
    double *vals;
    int32_t *cnt;
    double *psum;
    int64_t *pcnt;
    int64_t blocks;
};

static int loss_buffers(int dev, void *stream, int64_t units, double *unit_out, LossBuffers *b) {
    b->blocks = (units + kLossSumBlock - 1) / kLossSumBlock;
    b->vals = unit_out;
    if (!b->vals) {
        b->vals = (double *)stream_scratch(dev, stream, kScratchSgnsLossVals,
                                           sizeof(double) * (size_t)units);
        if (!b->vals) return scratch_failed();
    }
    b->cnt = (int32_t *)stream_scratch(dev, stream, kScratchSgnsLossCnt,
                                       sizeof(int32_t) * (size_t)units);
    if (!b->cnt) return scratch_failed();
    b->psum = (double *)stream_scratch(dev, stream, kScratchSgnsLossPart,
                                       (sizeof(double) + sizeof(int64_t)) * (size_t)b->blocks);
    if (!b->psum) return scratch_failed();
    b->pcnt = (int64_t *)(b->psum + b->blocks);
    return COME_OK;
}

static int loss_total(int dev, void *stream, int64_t units, const LossBuffers &b,
                      double *loss_out, int64_t *pairs_out) {
    int rc = launch(dev, k_loss_partial, "k_loss_partial launch", dim3((unsigned)b.blocks),
                    dim3(256), {0}, stream, (const double *)b.vals, (const int32_t *)b.cnt, units,
                    b.psum, b.pcnt);
    if (rc) return rc;
    return launch(dev, k_loss_total, "k_loss_total launch", dim3(1), dim3(256), {0}, stream,
                  (const double *)b.psum, (const int64_t *)b.pcnt, b.blocks, loss_out, pairs_out);
}

// One wavefront per unit in 4-wave workgroups, at most 8 workgroups per CU.  The kernels run 4 to
// 6 waves per SIMD, so 4 to 6 of a CU's 8 workgroups are resident at once; the others start as
// those finish and take what is left in the work queue (the pairs kernel: their grid-stride share).
static unsigned loss_grid(int dev, int64_t units) {
    int64_t blocks = (units + 3) / 4;
    const int64_t cap = (int64_t)num_cus(dev) * 8;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks > 0 ? blocks : 1);
}

}  // namespace come

using namespace come;

extern "C" int come_sgns_o2_loss(const float *node, const float *ctx, int64_t V, int d,
                                 const int32_t *walks, int64_t P, int L, const uint64_t *seeds,
                                 int window, int negative, const uint32_t *table, uint64_t T,
                                 int flags, double *walk_out, double *loss_out,
                                 int64_t *pairs_out, void *stream) {
    if (flags != 0 && flags != COME_TABLE_PACKED)
        return set_error(COME_E_INVALID, "sgns_o2_loss: flags must be 0 or COME_TABLE_PACKED");
    const int packed = flags == COME_TABLE_PACKED;
    if (packed && ((uintptr_t)table % 16) != 0)
        return set_error(COME_E_INVALID, "sgns_o2_loss: packed table must be 16-byte aligned");
    int rc = check_tables("sgns_o2_loss", V, d, negative);
    if (rc) return rc;
    if (negative > 0 && (table == nullptr || T == 0))
        return set_error(COME_E_INVALID, "sgns_o2_loss: negative sampling needs a non-empty table");
    if (P < 0 || L < 0 || window < 0)
        return set_error(COME_E_INVALID, "sgns_o2_loss: P, L and window must be >= 0");
    if (L > kMaxSentenceLen)
        return set_error(COME_E_INVALID, "sgns_o2_loss: L must be <= %d (got %d)", kMaxSentenceLen,
                         L);
    if (P > INT32_MAX) return set_error(COME_E_INVALID, "sgns_o2_loss: P too large");
    if (P == 0) return COME_OK;
    if (!node || !ctx || (!walks && L > 0) || !seeds || !loss_out)
        return set_error(COME_E_INVALID, "sgns_o2_loss: null node/ctx/walks/seeds/loss_out pointer");
    int dev = 0;
    rc = ensure_init(&dev);
    if (rc) return rc;
    LossBuffers b;
    rc = loss_buffers(dev, stream, P, walk_out, &b);
    if (rc) return rc;
    const O2LossArgs a{node,     ctx, walks,  seeds,    table,  (int)V,
                       (int)P,   L,   d,      window,   negative, make_fastmod(T ? T : 1),
                       packed,   launch_counter(dev, stream), b.vals,   b.cnt};
    rc = with_row(d, [&](auto vec, auto full) {
        return launch(dev, k_sgns_o2_loss<decltype(vec)::value, decltype(full)::value>,
                      "k_sgns_o2_loss launch", dim3(loss_grid(dev, P)), dim3(256), {0}, stream, a);
    });
    if (rc) return rc;
    return loss_total(dev, stream, P, b, loss_out, pairs_out);
}

extern "C" int come_sgns_pairs_loss(const float *inp, const float *out, int64_t V, int d,
                                    const int32_t *rows_in, const int32_t *rows_pos,
                                    const int32_t *rows_neg, int64_t M, int negative,
                                    double *pair_out, double *loss_out, int64_t *pairs_out,
                                    void *stream) {
    int rc = check_tables("sgns_pairs_loss", V, d, negative);
    if (rc) return rc;
    if (M < 0) return set_error(COME_E_INVALID, "sgns_pairs_loss: M must be >= 0");
    if (M > INT32_MAX) return set_error(COME_E_INVALID, "sgns_pairs_loss: M too large");
    if (M == 0) return COME_OK;
    if (!inp || !out || !rows_in || !rows_pos || (!rows_neg && negative > 0) || !loss_out)
        return set_error(COME_E_INVALID,
                         "sgns_pairs_loss: null inp/out/rows_in/rows_pos/rows_neg/loss_out pointer");
    int dev = 0;
    rc = ensure_init(&dev);
    if (rc) return rc;
    LossBuffers b;
    rc = loss_buffers(dev, stream, M, pair_out, &b);
    if (rc) return rc;
    const PairsLossArgs a{inp, out, rows_in, rows_pos, rows_neg, (int)V, (int)M, d, negative,
                          b.vals, b.cnt};
    rc = with_row(d, [&](auto vec, auto full) {
        return launch(dev, k_sgns_pairs_loss<decltype(vec)::value, decltype(full)::value>,
                      "k_sgns_pairs_loss launch", dim3(loss_grid(dev, M)), dim3(256), {0}, stream,
                      a);
    });
    if (rc) return rc;
    return loss_total(dev, stream, M, b, loss_out, pairs_out);
}
