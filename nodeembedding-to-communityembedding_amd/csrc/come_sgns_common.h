// come_sgns_common.h -- skip-gram negative-sampling updates for gfx950 (MI355X, CDNA4): what every
// SGNS kernel shares (rows in registers, dot products, the sigmoid lookup, the negative draws).
// The trainer kernels are in come_sgns_o2.h and come_sgns_o1.h, the loss kernels in
// come_sgns_loss.hip.
//
// Replaces the reference's Cython hot loop, /root/reference/utils/training_sdg_inner.pyx:
//   fast0_o2/fast1_o2 (pyx:105-201) + train_o2 (pyx:454-509)   -> k_sgns_o2
//   fast0_o1/fast1_o1 (pyx:205-296) + train_o1 (pyx:407-450)   -> k_sgns_o1
//
// Execution model:
//  * One 64-lane wavefront owns one walk (O2) or one edge (O1) and processes its positive pairs in
//    the reference's order, one pair at a time -- exactly the work one reference thread does per
//    nogil call (pyx:493).  All walks/edges of a batch are in flight at once (Hogwild across
//    wavefronts, as the reference's worker threads are Hogwild across walks).
//  * A d-dim fp32 row is spread over the wave: lane l holds elements l, l+64, ... (VEC =
//    ceil(d/64) of them); every row access is VEC wave instructions of 256 contiguous bytes.
//  * The (1 + negative) target rows of a pair are gathered together, their dot products reduced
//    with interleaved xor butterflies, then resolved in reference order (a negative that repeats an
//    earlier target sees that target's updated row, pyx:147, via register forwarding).
//  * Negatives never touch the host: lane k of the wave computes LCG draw (base + k) by jump-ahead
//    (the LCG is affine mod 2^48, pyx:134) and gathers table[(s >> 16) % T] for 64 draws at once;
//    each pair then reads its n draws with v_readlane (wave-uniform, scalar registers).
//  * Dot product order is fixed: per-lane fmaf chain, then xor butterfly 1,2,4,8,16,32.  The CPU
//    oracle's WAVE64 mode restates this order, so COME_MODE_SEQUENTIAL is bit-exact with it.
//  * Compiled with -ffp-contract=off: every fused multiply-add is an explicit fmaf, matching the
//    reference's saxpy (pyx:146-149) element for element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "come_internal.h"
#include "come_wave.h"

namespace come {

// One copy per translation unit (each .hip file is its own code object); come_init uploads the
// table into every copy (upload_exp_table_vec*).
static __constant__ float c_exp_table[kExpTableSize];

struct LcgLane {  // this lane's jump-ahead (A^k, C_k): s_{b+k} = A^k s_b + C_k  (mod 2^48)
    uint64_t a, c;
};

__device__ inline LcgLane lcg_lane_constants(int k) {
    uint64_t a = 1, c = 0;
    for (int i = 0; i < k; ++i) {
        a = (a * kLcgMul) & kLcgMask;
        c = (c * kLcgMul + kLcgAdd) & kLcgMask;
    }
    return {a, c};
}

__device__ inline uint64_t lcg_next(uint64_t s) { return (s * kLcgMul + kLcgAdd) & kLcgMask; }

// The 64 lanes' jump-ahead constants as a table in constant memory: a kernel short of registers
// reads its lane's pair when it refills a batch of draws (every 64 draws) instead of holding
// four VGPRs for the whole kernel.
struct LcgTable {
    uint64_t a[64], c[64];
};
constexpr LcgTable make_lcg_table() {
    LcgTable t{};
    uint64_t a = 1, c = 0;
    for (int k = 0; k < 64; ++k) {
        t.a[k] = a;
        t.c[k] = c;
        a = (a * kLcgMul) & kLcgMask;
        c = (c * kLcgMul + kLcgAdd) & kLcgMask;
    }
    return t;
}
static __constant__ LcgTable c_lcg = make_lcg_table();
constexpr LcgTable kLcgHost = make_lcg_table();
// state 64 draws after s, for any lane: A^64 s + C_64 (wave-uniform, scalar)
constexpr uint64_t kLcgA64 = (kLcgHost.a[63] * kLcgMul) & kLcgMask;
constexpr uint64_t kLcgC64 = (kLcgHost.c[63] * kLcgMul + kLcgAdd) & kLcgMask;

struct LcgFromTable {  // same interface as LcgLane, constants read at use
    int lane;
};
__device__ inline uint64_t lcg_state_of(uint64_t base, const LcgLane &lc) {
    return (lc.a * base + lc.c) & kLcgMask;
}
__device__ inline uint64_t lcg_state_of(uint64_t base, const LcgFromTable &lt) {
    return (c_lcg.a[lt.lane] * base + c_lcg.c[lt.lane]) & kLcgMask;
}

__device__ inline uint32_t table_slot(uint64_t s, uint64_t m, uint32_t d) {
    const uint32_t x = (uint32_t)(s >> 16);  // < 2^32 because s < 2^48 (pyx:133)
    if (d == 0) return x;                     // T >= 2^32: x % T == x
    return (uint32_t)__umul64hi(m * (uint64_t)x, (uint64_t)d);
}

// Packed negative table (come_pack_table): word w = {base, unused, bits} covers slots
// [64w, 64w + 64); table[64w + i] = base + popcount(bits & ((2 << i) - 1)), bit i (i >= 1) set iff
// slot i holds one more than slot i - 1.  Exact for every table whose values step by 0 or 1
// inside each 64-slot word -- make_table's are (model.py:107-121 advances widx by at most one per
// slot).  One 16-B load per draw from a T/4-byte structure (25 MB at T = 1e8, Infinity-Cache
// resident) instead of a 4-B load from the 400 MB table.
template <class Args>
__device__ inline uint32_t table_value(const Args &a, uint32_t slot) {
    if (a.packed) {
        const uint4 w = reinterpret_cast<const uint4 *>(a.table)[slot >> 6];
        const uint64_t bits = ((uint64_t)w.w << 32) | w.z;
        const uint64_t mask = (2ull << (slot & 63)) - 1ull;  // slot & 63 == 63: all ones
        return w.x + (uint32_t)__popcll(bits & mask);
    }
    return a.table[slot];
}

__device__ inline int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline float uniformf(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ inline uint64_t uniform64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint32_t readlane_u32(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ inline uint64_t readlane_u64(uint64_t v, int lane) {
    const uint32_t lo = readlane_u32((uint32_t)v, lane);
    const uint32_t hi = readlane_u32((uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// ---- row <-> registers -------------------------------------------------------------------------
template <int VEC, bool FULL>
struct Row {
    float v[VEC];  // lane l holds elements l, l + 64, ..., l + 64 (VEC - 1)

    // Every wave instruction touches 256 contiguous bytes (two 128-B lines): full-rate loads,
    // stores and -- what fixes this layout -- full-rate float atomics (MI355X_MICROARCH.md
    // "Global float atomics": 256 contiguous bytes per wave instruction).
    __device__ inline void load(const float *__restrict__ row, int lane, int d) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int e = lane + 64 * i;
            v[i] = (FULL || e < d) ? row[e] : 0.0f;
        }
    }

    // Non-temporal loads (global_load ... nt): rows with little reuse, so the L2 / Infinity Cache
    // keep the small structures every wavefront reads (hot bitmap, packed negative table)
    __device__ inline void load_nt(const float *__restrict__ row, int lane, int d) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int e = lane + 64 * i;
            v[i] = (FULL || e < d) ? __builtin_nontemporal_load(row + e) : 0.0f;
        }
    }

    // Agent-scope relaxed loads (global_load ... sc1): bypass this CU's L1, which other CUs'
    // stores never refresh (MI355X_MICROARCH.md: inter-workgroup visibility), so a row several
    // wavefronts update is read as last written to L2 / memory.
    __device__ inline void load_fresh(const float *__restrict__ row, int lane, int d) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int e = lane + 64 * i;
            v[i] = (FULL || e < d) ? __hip_atomic_load(row + e, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT)
                                   : 0.0f;
        }
    }

    __device__ inline void load_as(const float *__restrict__ row, int lane, int d, bool fresh) {
        if (fresh) load_fresh(row, lane, d);
        else load(row, lane, d);
    }

    __device__ inline void store(float *__restrict__ row, int lane, int d) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int e = lane + 64 * i;
            if (FULL || e < d) row[e] = v[i];
        }
    }

    // row += v with no-return float atomics (Hogwild write-back: no update is lost)
    __device__ inline void atomic_add(float *__restrict__ row, int lane, int d) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int e = lane + 64 * i;
            if (FULL || e < d) atomicAdd(row + e, v[i]);
        }
    }
};

template <int VEC, bool FULL>
__device__ inline float lane_partial(const Row<VEC, FULL> &a, const Row<VEC, FULL> &b) {
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) p = __builtin_fmaf(a.v[i], b.v[i], p);
    return p;
}

__device__ inline float wave_sum(float p) {
    p = reduce_stage<0>(p);
    p = reduce_stage<1>(p);
    p = reduce_stage<2>(p);
    p = reduce_stage<3>(p);
    p = reduce_stage<4>(p);
    return reduce_stage<5>(p);
}

// Sum the first `count` of `part[]` across the wave, the six stages interleaved over the targets
// so their latencies overlap.
template <int N>
__device__ inline void wave_sum_n(float (&part)[N], int count) {
#define COME_STAGE(S)                                          \
    _Pragma("unroll") for (int k = 0; k < N; ++k) if (k < count) part[k] = reduce_stage<S>(part[k]);
    COME_STAGE(0) COME_STAGE(1) COME_STAGE(2) COME_STAGE(3) COME_STAGE(4) COME_STAGE(5)
#undef COME_STAGE
}

// All N of `part[]`, with no branch per add: for a caller whose unused entries are initialised and
// never read (the stream kernel: a lane past n holds a dot nobody looks at).
template <int N>
__device__ inline void wave_sum_all(float (&part)[N]) {
#define COME_STAGE(S) \
    _Pragma("unroll") for (int k = 0; k < N; ++k) part[k] = reduce_stage<S>(part[k]);
    COME_STAGE(0) COME_STAGE(1) COME_STAGE(2) COME_STAGE(3) COME_STAGE(4) COME_STAGE(5)
#undef COME_STAGE
}

// sigma lookup exactly as generated from pyx:141-143: skip if f <= -6 or f >= 6, else
// EXP_TABLE[(int)(((double)f + 6.0) * 83.0)].  Returns false for a skipped target.  `tab` is
// c_exp_table or a copy of it (the stream kernel's LDS copy: no scalar-memory round trip per
// target).
__device__ inline bool sigmoid_tab(const float *tab, float f, float *sig) {
    if (f <= -(float)kMaxExp || f >= (float)kMaxExp) return false;
    const int b = (int)(((double)f + 6.0) * 83.0);
    *sig = tab[b];
    return true;
}

// ---- batch of 64 negative draws held one per lane ------------------------------------------
struct DrawBatch {
    uint32_t target;  // this lane's table value for draw (base + lane)
    uint64_t base;    // LCG state of draw `base`'s index 0 (wave-uniform)
    int used;         // draws of the batch already consumed (wave-uniform)
};

// Lanes < count gather their draw's table value (the others hold 0 and must not be consumed).
template <class Args>
__device__ inline void draws_fill(DrawBatch &b, uint64_t state0, const LcgLane &lc,
                                  const Args &a, int count = 64) {
    b.base = state0;
    b.used = 0;
    b.target = 0;
    if ((int)(threadIdx.x & 63) < count) {
        const uint64_t s = (lc.a * state0 + lc.c) & kLcgMask;
        b.target = table_value(a, table_slot(s, a.fm.m, a.fm.d));
    }
}

// State of the draw `b.used` positions after the batch base (0 < used <= 64).
__device__ inline uint64_t draws_state_at_used(const DrawBatch &b, const LcgLane &lc) {
    const uint64_t s = (lc.a * b.base + lc.c) & kLcgMask;  // this lane's state
    if (b.used < 64) return uniform64(readlane_u64(s, b.used));
    return lcg_next(uniform64(readlane_u64(s, 63)));
}

// Double-buffered draws: lanes of t0 hold draws base0 + lane, lanes of t1 the next 64.  The ring
// kernel holds both batches in registers and issues the next batch's table gather as soon as the
// current one starts, so its pairs never wait for the table; take(k) = target of draw `used + k`
// (used + k < 128).  The stream kernel keeps the batches in LDS and uses gather_hot() alone: its
// refill, every 64 draws, is synchronous -- the pair that triggers it waits for the gather's
// dependent loads (LCG constants, table word, bitmap word) before the batch is written.
struct DrawPipe {
    uint32_t t0, t1;
    uint64_t base0, base1;
    int used;

    template <class Args, class Lcg>
    __device__ inline uint32_t gather(uint64_t base, const Lcg &lc, const Args &a) {
        const uint64_t s = lcg_state_of(base, lc);  // draw base + lane
        return table_value(a, table_slot(s, a.fm.m, a.fm.d));
    }

    // gather() plus the drawn row's hot bit (a.hot) in bit 31 (rows are < 2^31); a table value
    // outside [0, V) gets no bit and stays out of range.  The bitmap word is one more dependent
    // per-lane load, 64 draws ahead of use.
    template <class Args, class Lcg>
    __device__ inline uint32_t gather_hot(uint64_t base, const Lcg &lc, const Args &a) {
        const uint32_t v = gather(base, lc, a);
        if (a.hot == nullptr || (int64_t)v >= a.V) return v;
        return v | (((a.hot[v >> 5] >> (v & 31)) & 1u) << 31);
    }
};

// ---- small helpers of the trainer and loss kernels ---------------------------------------------
// Row r is in the hot bitmap (wave-uniform r: one scalar load).
template <class Args>
__device__ inline bool is_hot(const Args &a, int r) {
    return a.hot != nullptr && ((a.hot[(uint32_t)r >> 5] >> (r & 31)) & 1u);
}

// Next unit of a wavefront: from the launch's work queue (one atomic per unit; a wavefront that
// starts late -- e.g. its CU was busy with a concurrent RCCL kernel -- simply claims fewer
// walks) or, without a queue, the static grid-stride sequence.
__device__ inline int64_t next_unit(int64_t *counter, int64_t cur, int64_t stride, int lane) {
    if (!counter) return cur + stride;
    int64_t v = 0;
    if (lane == 0) v = (int64_t)atomicAdd((unsigned long long *)counter, 1ull);
    return (int64_t)uniform64((uint64_t)v);  // lane 0 is the first active lane here
}

// State 64 draws after `base` (lane 63's state advanced once).
__device__ inline uint64_t advance64_uniform(uint64_t base) {
    return (kLcgA64 * base + kLcgC64) & kLcgMask;
}
__device__ inline uint64_t advance64(uint64_t base, const LcgLane &lc) {
    const uint64_t s = (lc.a * base + lc.c) & kLcgMask;
    return lcg_next(uniform64(readlane_u64(s, 63)));
}

template <int VEC, bool FULL>
__device__ inline void atomic_add_delta(float *__restrict__ row, const Row<VEC, FULL> &cur,
                                        const Row<VEC, FULL> &orig, int lane, int d) {
    Row<VEC, FULL> delta;
#pragma unroll
    for (int e = 0; e < VEC; ++e) delta.v[e] = cur.v[e] - orig.v[e];
    delta.atomic_add(row, lane, d);
}

}  // namespace come
