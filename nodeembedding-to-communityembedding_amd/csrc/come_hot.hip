// come_hot.hip -- "hot" rows of a negative-sampling table: the rows so frequent that several
// Hogwild wavefronts update them at the same time.
//
// Why: the reference's Hogwild has `workers` CPU threads, each reading a row fresh from coherent
// memory right before its saxpy (pyx:140-149), so a hub row is seldom updated by two threads at
// once.  On MI355X thousands of wavefronts are in flight and the per-XCD L2s are not coherent, so
// a plain read-modify-write of a hub row (drawn as a negative every few hundred draws, visited by
// a large share of walks) loses most concurrent updates, and a row cached in a wavefront for a
// whole window collects updates computed from a stale copy.  The O2 kernel therefore treats hot
// rows differently from the rest: read right before each pair and updated with float atomics at
// the memory side (no update lost, no stale cache); cold rows keep the cached / plain form.
//
// Hotness is measured on the table itself: a row's draw probability is its number of slots / T
// (model.py:97-122 gives each row count^0.75 / Z of the slots), and the walk-visit frequency of a
// node grows with the same count (its degree), so the rows with the most slots are the contended
// ones in both roles.  come_hot_rows counts each row's slots and marks rows with >= min_count.
#include "come_internal.h"

namespace come {

// counts[v] += occurrences of v in table[0, T); a wavefront whose 64 slots hold one value (the
// common case: make_table's runs are ~T/V slots long) adds once.
__global__ void __launch_bounds__(256) k_table_counts(const uint32_t *__restrict__ table,
                                                      uint64_t T, int64_t V,
                                                      uint32_t *__restrict__ counts) {
    const uint64_t n = (uint64_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < T;
         base += n) {
        const uint64_t s = base + lane;
        const bool in = s < T;
        const uint32_t v = in ? table[s] : 0xFFFFFFFFu;
        const uint32_t first = (uint32_t)__shfl((int)v, 0);
        const bool uniform_wave = __all(!in || v == first) && first < (uint64_t)V;
        if (uniform_wave) {
            const int cnt = __popcll(__ballot(in));
            if (lane == 0) atomicAdd(counts + first, (uint32_t)cnt);
        } else if (in && (int64_t)v < V) {
            atomicAdd(counts + v, 1u);
        }
    }
}

// The same over come_pack_table's words: slot s = 64 w + i holds base_w + popcount(bits_w & (2^(i+1)
// - 1)) (one 16-B word per 64 slots, read by every lane of the wavefront: one line).
__global__ void __launch_bounds__(256) k_table_counts_packed(const uint4 *__restrict__ words,
                                                             uint64_t T, int64_t V,
                                                             uint32_t *__restrict__ counts) {
    const uint64_t n = (uint64_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < T;
         base += n) {
        const uint64_t s = base + lane;
        const bool in = s < T;
        const uint4 wd = words[base >> 6];
        const uint64_t bits = ((uint64_t)wd.w << 32) | wd.z;
        const uint64_t mask = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
        const uint32_t v = in ? wd.x + (uint32_t)__popcll(bits & mask) : 0xFFFFFFFFu;
        const uint32_t first = (uint32_t)__shfl((int)v, 0);
        const bool uniform_wave = __all(!in || v == first) && first < (uint64_t)V;
        if (uniform_wave) {
            const int cnt = __popcll(__ballot(in));
            if (lane == 0) atomicAdd(counts + first, (uint32_t)cnt);
        } else if (in && (int64_t)v < V) {
            atomicAdd(counts + v, 1u);
        }
    }
}

// hot_bits[w] bit b = counts[32 w + b] >= min_count
__global__ void __launch_bounds__(256) k_hot_bits(const uint32_t *__restrict__ counts, int64_t V,
                                                  uint64_t min_count,
                                                  uint32_t *__restrict__ hot_bits) {
    const int64_t words = (V + 31) / 32;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words;
         w += (int64_t)gridDim.x * blockDim.x) {
        uint32_t bits = 0;
        for (int b = 0; b < 32; ++b) {
            const int64_t r = 32 * w + b;
            if (r < V && counts[r] >= min_count) bits |= 1u << b;
        }
        hot_bits[w] = bits;
    }
}

// ---- "quiet" rows: the node-table rows so rarely visited that a wavefront may hold one for a
// walk window (the windowed stream kernel's LDS ring).  What makes a hold harmful is another
// wavefront visiting the row meanwhile, so the rule is on the expected number of such visitors:
//     visitors x (the row's share of walk visits) <= eps,
// visitors = wavefronts in flight x (2w + 1) positions each.  The visit share is the degree share,
// recovered from the table: node id v + id_shift (row v) got count^power / Z of the slots, and the
// slots hold the *id*, which the kernels use as a row (model.py:97-122) -- so row v's own count
// sizes the slots of row v + id_shift, and share_v = counts[v + id_shift]^(1/power) / sum_u
// counts[u]^(1/power).  A row whose count the table does not hold (v + id_shift >= V: the table's
// clamp folds it into its last value) is not quiet, and neither is a hot row.

// sum[0] += sum_v counts[v]^(1/power)
__global__ void __launch_bounds__(256) k_quiet_sum(const uint32_t *__restrict__ counts, int64_t V,
                                                   double inv_power, double *__restrict__ sum) {
    double s = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V;
         v += (int64_t)gridDim.x * blockDim.x)
        s += pow((double)counts[v], inv_power);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0 && s != 0.0) atomicAdd(sum, s);
}

// quiet_bits[w] bit b = row 32 w + b is quiet
__global__ void __launch_bounds__(256) k_quiet_bits(const uint32_t *__restrict__ counts, int64_t V,
                                                    int id_shift, double inv_power,
                                                    double visitors, double eps,
                                                    uint64_t hot_min_count,
                                                    const double *__restrict__ sum,
                                                    uint32_t *__restrict__ quiet_bits) {
    const int64_t words = (V + 31) / 32;
    const double bound = eps * sum[0] / visitors;  // on counts[.]^(1/power)
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words;
         w += (int64_t)gridDim.x * blockDim.x) {
        uint32_t bits = 0;
        for (int b = 0; b < 32; ++b) {
            const int64_t r = 32 * w + b, own = r + id_shift;
            if (r < V && own >= 0 && own < V && counts[r] < hot_min_count &&
                pow((double)counts[own], inv_power) <= bound)
                bits |= 1u << b;
        }
        quiet_bits[w] = bits;
    }
}

static int hot_rows_impl(int dev, const uint32_t *table, uint64_t T, int packed, int64_t V,
                         uint64_t min_count, uint32_t *counts, uint32_t *hot_bits, void *stream) {
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(uint32_t) * (size_t)V, (hipStream_t)stream);
    if (e != hipSuccess) return hip_error(e, "hipMemsetAsync(counts)");
    uint64_t blocks = (T + 255) / 256;
    const uint64_t cap = (uint64_t)num_cus(dev) * 16;
    if (blocks > cap) blocks = cap;
    if (packed)
        hipLaunchKernelGGL(k_table_counts_packed, dim3((unsigned)blocks), dim3(256), 0,
                           (hipStream_t)stream, (const uint4 *)table, T, V, counts);
    else
        hipLaunchKernelGGL(k_table_counts, dim3((unsigned)blocks), dim3(256), 0,
                           (hipStream_t)stream, table, T, V, counts);
    int rc = hip_error(hipGetLastError(), "k_table_counts launch");
    if (rc) return rc;
    const int64_t words = (V + 31) / 32;
    int64_t wb = (words + 255) / 256;
    if (wb > 4096) wb = 4096;
    hipLaunchKernelGGL(k_hot_bits, dim3((unsigned)wb), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t *)counts, V, min_count, hot_bits);
    return hip_error(hipGetLastError(), "k_hot_bits launch");
}

int derive_hot_rows(int dev, const uint32_t *table, uint64_t T, int packed, int64_t V, int d,
                    void *stream, const uint32_t **bits_out) {
    uint32_t *counts = (uint32_t *)stream_scratch(dev, stream, kScratchHotCounts,
                                                  sizeof(uint32_t) * (size_t)V);
    uint32_t *bits = (uint32_t *)stream_scratch(dev, stream, kScratchHotBits,
                                                sizeof(uint32_t) * (size_t)((V + 31) / 32));
    if (!counts || !bits) return scratch_failed();
    const double share = d <= 128 ? COME_DEFAULT_HOT_SHARE : COME_DEFAULT_HOT_SHARE_WIDE;
    uint64_t min_count = (uint64_t)(share * (double)T);
    if (min_count < 1) min_count = 1;
    *bits_out = bits;
    return hot_rows_impl(dev, table, T, packed, V, min_count, counts, bits, stream);
}

}  // namespace come

using namespace come;

extern "C" int come_hot_rows(const uint32_t *table, uint64_t T, int64_t V, uint64_t min_count,
                             uint32_t *counts, uint32_t *hot_bits, void *stream) {
    if (V <= 0 || V > INT32_MAX) return set_error(COME_E_INVALID, "hot_rows: V out of range");
    if (!table || !counts || !hot_bits || T == 0)
        return set_error(COME_E_INVALID, "hot_rows: null pointer or empty table");
    int dev = 0;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    return hot_rows_impl(dev, table, T, 0, V, min_count, counts, hot_bits, stream);
}

extern "C" int come_quiet_rows(const uint32_t *table, uint64_t T, int64_t V, double power,
                               int id_shift, double visitors, double eps, uint64_t hot_min_count,
                               uint32_t *counts, double *sum, uint32_t *quiet_bits, void *stream) {
    if (V <= 0 || V > INT32_MAX) return set_error(COME_E_INVALID, "quiet_rows: V out of range");
    if (!table || !counts || !sum || !quiet_bits || T == 0)
        return set_error(COME_E_INVALID, "quiet_rows: null pointer or empty table");
    if (!(power > 0.0) || !(visitors > 0.0) || !(eps >= 0.0))
        return set_error(COME_E_INVALID, "quiet_rows: power and visitors must be > 0, eps >= 0");
    int dev = 0;
    int rc = ensure_init(&dev);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(uint32_t) * (size_t)V, (hipStream_t)stream);
    if (e != hipSuccess) return hip_error(e, "hipMemsetAsync(counts)");
    e = hipMemsetAsync(sum, 0, sizeof(double), (hipStream_t)stream);
    if (e != hipSuccess) return hip_error(e, "hipMemsetAsync(sum)");
    uint64_t blocks = (T + 255) / 256;
    const uint64_t cap = (uint64_t)num_cus(dev) * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_table_counts, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       table, T, V, counts);
    rc = hip_error(hipGetLastError(), "k_table_counts launch");
    if (rc) return rc;
    int64_t vb = (V + 255) / 256;
    if (vb > 4096) vb = 4096;
    hipLaunchKernelGGL(k_quiet_sum, dim3((unsigned)vb), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t *)counts, V, 1.0 / power, sum);
    rc = hip_error(hipGetLastError(), "k_quiet_sum launch");
    if (rc) return rc;
    const int64_t words = (V + 31) / 32;
    int64_t wb = (words + 255) / 256;
    if (wb > 4096) wb = 4096;
    hipLaunchKernelGGL(k_quiet_bits, dim3((unsigned)wb), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t *)counts, V, id_shift, 1.0 / power, visitors, eps,
                       hot_min_count, (const double *)sum, quiet_bits);
    return hip_error(hipGetLastError(), "k_quiet_bits launch");
}
