// come_sgns_o2.h -- the O2 (walk) trainer kernels: k_sgns_o2 (direct), k_sgns_o2_ring (sequential
// mode) and k_sgns_o2_stream (Hogwild mode).  Execution model: come_sgns_common.h.
#pragma once
#include "come_sgns_common.h"

namespace come {

// ---- O2: one wavefront per walk ------------------------------------------------------------

struct O2Args {
    float *node;
    float *ctx;
    const int32_t *walks;
    const uint64_t *seeds;
    const uint32_t *table;
    int64_t V;
    int64_t P;
    int L;
    int d;
    int window;
    int negative;
    float lr;
    float alpha;
    FastMod fm;
    int packed;        // table points to come_pack_table's words
    int64_t *counter;  // work queue: walks are claimed with atomicAdd (nullptr = grid-stride)
    unsigned long long *upd_count;  // optional: += target row updates applied (come.h
                                    // o2_update_count); one atomic per walk
    int fresh;       // direct kernel: rows read with agent-scope loads (bypass the CU's L1)
    int wb_atomic;   // direct kernel: row updates written as float-atomic deltas (none lost)
    const uint32_t *hot;  // HOG, optional: bitmap of contended rows (come_hot_rows); their
                          // updates are float-atomic deltas, their reads are per pair
    const uint32_t *quiet;  // windowed stream kernel, optional: bitmap of rows few other wavefronts
                            // visit (come_quiet_rows); as input rows they stay in the wavefront's
                            // LDS ring while a position holding them is inside the walk window
};

// The serial resolution of one O2 pair (pyx:141-149), shared by the direct and the ring kernel:
// the positive `pos`, then the negatives r[1..MAXN] (rows t[k], entries with !valid[k] skipped) in
// reference order.  part[k] holds the targets' dots against the input row `in` as it was before
// the pair, reduced over the wave.  On return `work` is the pair's change of the input row (the
// caller applies in += work, pyx:149), r[k] and `pos` hold the updated rows, upd[k] / pos_upd say
// which changed, and nupd has grown by their number.  Forced inline: the rows are registers of the
// calling kernel (left to its own judgement the compiler makes <8, *, 20> a call).
template <int VEC, bool FULL, int MAXN>
__device__ __forceinline__ void o2_resolve(float lr, float alpha, const Row<VEC, FULL> &in,
                                           Row<VEC, FULL> &pos, bool &pos_upd,
                                           Row<VEC, FULL> (&r)[MAXN + 1], const int (&t)[MAXN + 1],
                                           const bool (&valid)[MAXN + 1], float (&part)[MAXN + 1],
                                           Row<VEC, FULL> &work, bool (&upd)[MAXN + 1],
                                           int &nupd) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) work.v[e] = 0.0f;
    // positive (d == 0, label 1)
    {
        float sig;
        if (sigmoid_tab(c_exp_table, uniformf(part[0]), &sig)) {
            const float g = ((1.0f - sig) * lr) * alpha;  // pyx:144
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                work.v[e] = __builtin_fmaf(g, pos.v[e], work.v[e]);  // pyx:146
                pos.v[e] = __builtin_fmaf(g, in.v[e], pos.v[e]);     // pyx:147
            }
            pos_upd = true;
            ++nupd;
        }
    }
    upd[0] = false;
#pragma unroll
    for (int k = 1; k <= MAXN; ++k) {
        upd[k] = false;
        if (!valid[k]) continue;
        float f = part[k];
        // A repeated negative sees the row as left by its latest earlier occurrence.
        int prev = -1;
#pragma unroll
        for (int q = 1; q < k; ++q)
            if (valid[q] && t[q] == t[k]) prev = q;
        if (prev >= 0) {
#pragma unroll
            for (int q = 1; q < k; ++q) {
                if (q == prev) {
                    r[k] = r[q];
                    f = upd[q] ? wave_sum(lane_partial(in, r[k])) : part[q];
                }
            }
        }
        f = uniformf(f);
        part[k] = f;  // effective dot of this occurrence (a later repeat may reuse it)
        float sig;
        if (!sigmoid_tab(c_exp_table, f, &sig)) continue;  // pyx:141-142
        const float g = ((0.0f - sig) * lr) * alpha;  // pyx:144, label 0
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            work.v[e] = __builtin_fmaf(g, r[k].v[e], work.v[e]);  // pyx:146
            r[k].v[e] = __builtin_fmaf(g, in.v[e], r[k].v[e]);    // pyx:147
        }
        upd[k] = true;
        ++nupd;
    }
}

// One O2 pair (pyx:105-151) with the input row `in` and the positive row `pos` already in
// registers.  Draws the pair's n negatives (pyx:133-135), gathers their rows, reduces every dot
// product, resolves the targets in reference order, stores the updated negative rows, updates
// `pos` in registers (pos_upd |= updated) and finally applies `in += work` (pyx:149).
template <int VEC, bool FULL, int MAXN>
__device__ inline void o2_pair(const O2Args &a, DrawBatch &db, const LcgLane &lc, int lane, int ci,
                               Row<VEC, FULL> &pos, bool &pos_upd, Row<VEC, FULL> &in,
                               Row<VEC, FULL> &work, int &nupd) {
    using R = Row<VEC, FULL>;
    const int n = a.negative;
    const int d = a.d;
    if (n > 0 && db.used + n > 64) draws_fill(db, draws_state_at_used(db, lc), lc, a);
    int t[MAXN + 1];
    bool valid[MAXN + 1];
    t[0] = ci;
    valid[0] = true;
#pragma unroll
    for (int k = 1; k <= MAXN; ++k) {
        if (k <= n) {
            const int tk = (int)readlane_u32(db.target, db.used + k - 1);
            t[k] = tk;
            // pyx:135 skip == positive; out-of-range table values skipped (no OOB)
            valid[k] = tk != ci && tk >= 0 && tk < a.V;
        } else {
            t[k] = -1;
            valid[k] = false;
        }
    }
    if (n > 0) db.used += n;

    R r[MAXN + 1], o[MAXN + 1];
#pragma unroll
    for (int k = 1; k <= MAXN; ++k)
        if (valid[k]) {
            r[k].load_as(a.ctx + (int64_t)t[k] * d, lane, d, a.fresh);
            o[k] = r[k];
        }

    // dots of every target against the (fixed) input row, butterflies interleaved
    float part[MAXN + 1];
    part[0] = lane_partial(in, pos);
#pragma unroll
    for (int k = 1; k <= MAXN; ++k) part[k] = valid[k] ? lane_partial(in, r[k]) : 0.0f;
    wave_sum_n(part, n + 1);

    bool upd[MAXN + 1];
    o2_resolve<VEC, FULL, MAXN>(a.lr, a.alpha, in, pos, pos_upd, r, t, valid, part, work, upd, nupd);
    // write back in order, so a repeated row ends with its last version; atomic mode adds the
    // row's change over the pair once (last updated occurrence minus the value loaded)
#pragma unroll
    for (int k = 1; k <= MAXN; ++k) {
        if (!upd[k]) continue;
        if (!a.wb_atomic && !is_hot(a, t[k])) {
            r[k].store(a.ctx + (int64_t)t[k] * d, lane, d);
            continue;
        }
        bool last = true;
#pragma unroll
        for (int q = k + 1; q <= MAXN; ++q)
            if (upd[q] && t[q] == t[k]) last = false;
        if (last) atomic_add_delta(a.ctx + (int64_t)t[k] * d, r[k], o[k], lane, d);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) in.v[e] = in.v[e] + work.v[e];  // pyx:149
}

// Direct variant: every pair reads and writes its input and positive rows in HBM.  Used when the
// LDS ring of the cached variant would not fit (large window x d).
template <int VEC, bool FULL, int MAXN>
__global__ void __launch_bounds__(256) k_sgns_o2(O2Args a) {
    using R = Row<VEC, FULL>;
    const int lane = threadIdx.x & 63;
    const int64_t waves_per_block = blockDim.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * waves_per_block;
    const LcgLane lc = lcg_lane_constants(lane);
    const int d = a.d;
    const int path_len = a.L < kMaxSentenceLen ? a.L : kMaxSentenceLen;  // pyx:480

    for (int64_t p = gw; p < a.P; p += nwaves) {
        const int32_t *__restrict__ idx = a.walks + p * (int64_t)a.L;
        DrawBatch db;
        db.used = 0;
        db.base = uniform64(a.seeds[p]);
        db.target = 0;
        if (a.negative > 0) draws_fill(db, db.base, lc, a);
        int nupd = 0;
        for (int i = 0; i < path_len; ++i) {
            const int ci = uniform(idx[i]);
            if (ci < 0 || ci >= a.V) continue;  // codelens[i] == 0 (pyx:495)
            const int j0 = i - a.window < 0 ? 0 : i - a.window;
            const int j1 = i + a.window + 1 > path_len ? path_len : i + a.window + 1;
            for (int j = j0; j < j1; ++j) {
                if (j == i) continue;
                const int cj = uniform(idx[j]);
                if (cj < 0 || cj >= a.V) continue;  // pyx:504
                R in, pos;
                in.load_as(a.node + (int64_t)cj * d, lane, d, a.fresh);
                pos.load_as(a.ctx + (int64_t)ci * d, lane, d, a.fresh);
                const R pos0 = pos;
                bool pos_upd = false;
                R work;
                o2_pair<VEC, FULL, MAXN>(a, db, lc, lane, ci, pos, pos_upd, in, work, nupd);
                // in += work and pos's change: at the memory side (float atomics) for contended
                // rows, plain stores otherwise
                if (pos_upd) {
                    if (a.wb_atomic || is_hot(a, ci))
                        atomic_add_delta(a.ctx + (int64_t)ci * d, pos, pos0, lane, d);
                    else
                        pos.store(a.ctx + (int64_t)ci * d, lane, d);
                }
                if (a.wb_atomic || is_hot(a, cj)) work.atomic_add(a.node + (int64_t)cj * d, lane, d);
                else in.store(a.node + (int64_t)cj * d, lane, d);
            }
        }
        if (a.upd_count && lane == 0 && nupd) atomicAdd(a.upd_count, (unsigned long long)nupd);
    }
}

// Cached, software-pipelined variant (the hot kernel).
//
// Traffic cuts, exact in sequential order:
//  * the center's positive row ctx[idx[i]] stays in registers across its 2w pairs (no negative of
//    those pairs can be that row: pyx:135 skips it) and is written back once per center;
//  * the input rows of the window [i-w, i+w] live in a per-wavefront LDS ring of 2w+1 rows: a
//    walk position's node row is read from HBM once, when it enters the window, instead of once
//    per pair.  Positions holding the same node id alias: entering copies the live LDS row, every
//    update is applied to all aliases.
// Latency hiding (one wavefront walks its pairs strictly in order, so memory-level parallelism
// has to come from running ahead):
//  * the walk's row indices sit in two VGPR chunks of 64 positions (v_readlane), refilled 64
//    positions ahead -- no dependent index loads;
//  * the next pair's negative rows are loaded while the current pair computes, the next center's
//    positive row and entering node row while the current center runs, the next 64 table draws
//    while the current 64 are consumed.  Every prefetched row that the current work writes before
//    it is used is replaced by the register copy (forwarding), so sequential order is preserved
//    bit for bit.  Prefetch loads are unconditional (out-of-range targets read row 0 and are
//    discarded) so the compiler's vmcnt waits stay counted, never vmcnt(0).
// Write-back: plain stores -- the positive once per center, a node row when its last alias leaves
// the window, negative rows per pair.
// This is the SEQUENTIAL-mode kernel (one wavefront, the parity anchor).  Its caching is exact
// only when no other wavefront touches the cached rows: for Hogwild, caching node rows for a
// window trains measurably worse on graphs with hubs (tests/test_gpu_tierc.py), so Hogwild runs
// k_sgns_o2_stream.
template <int VEC, bool FULL, int MAXN>
__global__ void __launch_bounds__(128) k_sgns_o2_ring(O2Args a) {
    using R = Row<VEC, FULL>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const int64_t waves_per_block = blockDim.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * waves_per_block + wib;
    const int64_t nwaves = (int64_t)gridDim.x * waves_per_block;
    const LcgLane lc = lcg_lane_constants(lane);
    const int d = a.d;
    const int w = a.window;
    const int n = a.negative;
    const int RS = 2 * w + 1;  // ring slots (<= 64: ids live one per lane)
    const int path_len = a.L < kMaxSentenceLen ? a.L : kMaxSentenceLen;  // pyx:480
    const int wave_floats = (RS * d + 3) & ~3;
    float *ring = lds + wib * wave_floats;
    auto valid_row = [&](int r) { return r >= 0 && r < a.V; };
    auto slot_add = [&](int s, int delta) {  // (s + delta) mod RS for |delta| <= RS
        s += delta;
        if (s < 0) s += RS;
        if (s >= RS) s -= RS;
        return s;
    };

    for (int64_t p = a.counter ? next_unit(a.counter, 0, 0, lane) : gw; p < a.P;
         p = next_unit(a.counter, p, nwaves, lane)) {
        const int32_t *__restrict__ walk = a.walks + p * (int64_t)a.L;
        // ---- walk indices: positions [wbase, wbase + 128) in two VGPR chunks ----
        int wbase = 0;
        int c0 = lane < path_len ? walk[lane] : -1;
        int c1 = 64 + lane < path_len ? walk[64 + lane] : -1;
        auto idx_at = [&](int q) {  // validated row of walk position q (-1 = None / past the end)
            if (q >= path_len) return -1;
            const int off = q - wbase;
            const int r = off < 64 ? __builtin_amdgcn_readlane(c0, off)
                                   : __builtin_amdgcn_readlane(c1, off - 64);
            return valid_row(r) ? r : -1;
        };
        // ---- draws ----
        DrawPipe dp;
        dp.used = 0;
        dp.base0 = uniform64(a.seeds[p]);
        dp.t0 = dp.t1 = 0;
        if (n > 0) {
            dp.t0 = dp.gather(dp.base0, lc, a);
            dp.base1 = advance64(dp.base0, lc);
            dp.t1 = dp.gather(dp.base1, lc, a);
        }
        auto take = [&](int k) -> int {
            const int q = dp.used + k;
            return (int)(q < 64 ? readlane_u32(dp.t0, q) : readlane_u32(dp.t1, q - 64));
        };
        auto advance = [&]() {
            if (n == 0) return;
            dp.used += n;
            if (dp.used >= 64) {
                dp.used -= 64;
                dp.t0 = dp.t1;
                dp.base0 = dp.base1;
                dp.base1 = advance64(dp.base1, lc);
                dp.t1 = dp.gather(dp.base1, lc, a);
            }
        };
        // next pair's negatives: raw targets and their rows (row 0 stands in for bad targets)
        int tn[MAXN + 1];
        R rn[MAXN + 1];
        auto fetch_next = [&]() {
#pragma unroll
            for (int k = 1; k <= MAXN; ++k) {
                const int tk = k <= n ? take(k - 1) : -1;
                tn[k] = tk;
                rn[k].load(a.ctx + (int64_t)(valid_row(tk) ? tk : 0) * d, lane, d);
            }
        };
        fetch_next();

        int nupd = 0;  // target row updates of this walk (wave-uniform)
        // ---- ring (LDS rows) + ids (one per lane) ----
        int ids = -1;  // lane s: node row held by ring slot s
        auto id_of = [&](int s) { return __builtin_amdgcn_readlane(ids, s); };
        auto alias_mask = [&](int id, int except) -> uint64_t {
            return __ballot(lane < RS && lane != except && ids == id);
        };
        auto set_id = [&](int s, int id) { ids = lane == s ? id : ids; };
        auto write_back = [&](int s, int id) {  // the last holder of a node row stores it
            if (alias_mask(id, s) != 0) return;
            R row;
            row.load(ring + s * d, lane, d);
            row.store(a.node + (int64_t)id * d, lane, d);
        };
        auto enter_row = [&](int s, int id, const R &fetched) {  // fetched: node[id] loaded earlier
            const uint64_t m = alias_mask(id, s);
            if (m) {
                R row;
                row.load(ring + __builtin_ctzll(m) * d, lane, d);
                row.store(ring + s * d, lane, d);
            } else {
                fetched.store(ring + s * d, lane, d);
            }
            set_id(s, id);
        };
        for (int q = 0; q < w && q < path_len; ++q) {  // positions [0, w) before center 0
            const int id = idx_at(q);
            if (id >= 0) {
                R row;
                row.load(a.node + (int64_t)id * d, lane, d);
                enter_row(q, id, row);
            }
        }
        // center-level prefetch: the positive of the next center, the row entering with it
        R pos_n, ent_n;
        int pos_n_id = idx_at(0), ent_n_id = idx_at(w);
        pos_n.load(a.ctx + (int64_t)(pos_n_id >= 0 ? pos_n_id : 0) * d, lane, d);
        ent_n.load(a.node + (int64_t)(ent_n_id >= 0 ? ent_n_id : 0) * d, lane, d);

        int si = 0;  // slot of position i
        for (int i = 0; i < path_len; ++i) {
            // this center's prefetched rows, then prefetch for center i+1
            if (i + 1 + w >= wbase + 128) {  // keep [i, i + 1 + w] inside the two chunks
                wbase += 64;
                c0 = c1;
                c1 = wbase + 64 + lane < path_len ? walk[wbase + 64 + lane] : -1;
            }
            const int ci = pos_n_id;
            R pos = pos_n;
            // ring: position i-w-1 leaves, position i+w enters (same slot)
            const int se = slot_add(si, w);
            if (i + w < path_len || i - w - 1 >= 0) {
                const int old_id = i - w - 1 >= 0 ? id_of(se) : -1;
                if (old_id >= 0 && old_id == ent_n_id) {
                    // the same node leaves and enters: keep the live LDS row (no store, no load)
                } else {
                    if (old_id >= 0) write_back(se, old_id);
                    set_id(se, -1);
                    if (i + w < path_len && ent_n_id >= 0) enter_row(se, ent_n_id, ent_n);
                }
            }
            // prefetch for center i+1, after this boundary's write-back (a node that just left
            // may be the one entering next; its prefetched copy must not predate the store)
            pos_n_id = idx_at(i + 1);
            ent_n_id = idx_at(i + 1 + w);
            pos_n.load(a.ctx + (int64_t)(pos_n_id >= 0 ? pos_n_id : 0) * d, lane, d);
            ent_n.load(a.node + (int64_t)(ent_n_id >= 0 ? ent_n_id : 0) * d, lane, d);

            if (ci >= 0) {  // codelens[i] != 0 (pyx:495)
                bool pos_upd = false;
                const int j0 = i - w < 0 ? 0 : i - w;
                const int j1 = i + w + 1 > path_len ? path_len : i + w + 1;
                for (int j = j0; j < j1; ++j) {
                    if (j == i) continue;
                    const int sj = slot_add(si, j - i);
                    const int cj = id_of(sj);
                    if (cj < 0) continue;  // pyx:504
                    R in;
                    in.load(ring + sj * d, lane, d);
                    // this pair's negatives were prefetched; put the next pair's in flight
                    int t[MAXN + 1];
                    R r[MAXN + 1];
#pragma unroll
                    for (int k = 1; k <= MAXN; ++k) {
                        t[k] = tn[k];
                        r[k] = rn[k];
                    }
                    advance();
                    fetch_next();

                    // ---- the pair (pyx:128-149) ----
                    bool valid[MAXN + 1];
#pragma unroll
                    for (int k = 1; k <= MAXN; ++k)
                        valid[k] = k <= n && t[k] != ci && valid_row(t[k]);  // pyx:135
                    float part[MAXN + 1];
                    part[0] = lane_partial(in, pos);
#pragma unroll
                    for (int k = 1; k <= MAXN; ++k) part[k] = lane_partial(in, r[k]);
                    wave_sum_n(part, n + 1);
                    R work;
                    bool upd[MAXN + 1];
                    o2_resolve<VEC, FULL, MAXN>(a.lr, a.alpha, in, pos, pos_upd, r, t, valid, part,
                                                work, upd, nupd);
#pragma unroll
                    for (int k = 1; k <= MAXN; ++k) {
                        if (!upd[k]) continue;
                        r[k].store(a.ctx + (int64_t)t[k] * d, lane, d);
                        // prefetched copies of this row are now stale: forward the new value
#pragma unroll
                        for (int q = 1; q <= MAXN; ++q)
                            if (tn[q] == t[k]) rn[q] = r[k];
                        if (pos_n_id == t[k]) pos_n = r[k];
                    }
#pragma unroll
                    for (int e = 0; e < VEC; ++e) in.v[e] = in.v[e] + work.v[e];  // pyx:149
                    uint64_t m = alias_mask(cj, -1);  // the slot and every alias of it
                    while (m) {
                        const int rr = __builtin_ctzll(m);
                        m &= m - 1;
                        in.store(ring + rr * d, lane, d);
                    }
                }
                if (pos_upd) {
                    pos.store(a.ctx + (int64_t)ci * d, lane, d);
#pragma unroll
                    for (int q = 1; q <= MAXN; ++q)
                        if (tn[q] == ci) rn[q] = pos;  // prefetched before this write-back
                    if (pos_n_id == ci) pos_n = pos;
                }
            }
            si = slot_add(si, 1);
        }
        // positions still in the ring leave in order
        const int first = path_len - w - 1 > 0 ? path_len - w - 1 : 0;
        for (int q = first; q < path_len; ++q) {
            const int s = q % RS;
            const int id = id_of(s);
            if (id >= 0) write_back(s, id);
            set_id(s, -1);
        }
        if (a.upd_count && lane == 0 && nupd) atomicAdd(a.upd_count, (unsigned long long)nupd);
    }
}

// Streaming Hogwild variant (COME_MODE_HOGWILD; the product's Hogwild mode).
//
// Semantics per pair are the reference thread's (pyx:128-149): the input row, the positive row and
// the negative rows are read from memory for the pair and written back after it -- nothing is
// cached across pairs except a cold center's positive row, held for that center's 2w pairs (no
// negative of those pairs can be that row, pyx:135).  Rows are split by contention (a.hot,
// come_hot_rows): cold rows are written back with plain stores (few other wavefronts touch them
// while the pair runs), hot rows (hubs) with float-atomic deltas at the memory side (none of the
// many concurrent updates lost).  Measured against the sequential oracle on a power-law graph
// (tests/test_gpu_tierc.py): caching node rows for a window (the ring kernel's traffic cut) and
// writing them back later trains 3.6-6% worse, plain stores for hubs 1.8% worse, this form within
// 1% (the 1% bar of SURVEY.md §8c tier C).
// Latency hiding as in the ring kernel, one pair ahead: the next pair's input row, its positive
// (when the center changes or is hot), its negative rows and the hot bits of its rows are in
// flight while the current pair computes.  A prefetched copy of a row the current pair then
// updates must not stay as it was read.  At d <= 128 the pair that updates such a row (a general
// pair, below) waits for its write-backs and reads the next pair's rows again: a cold row's copy
// then holds the stored value (on walks that share no row the launch is bit-identical to the
// sequential order, tests/test_gpu_stream.py), a hot row's the memory after this wavefront's
// atomic.  The one exception is a hot center's own change, added when the next pair of that
// center takes the copy over (copy + delta: the copy keeps the other wavefronts' atomics it was
// read with).  Wider rows patch the copies in registers.
// The waits (d <= 128): vmcnt counts loads, stores and atomics in issue order, so a plain pair has
// exactly one wait on it -- for the next pair's rows, placed before the pair's first store -- and
// waits for no store or atomic; a general pair does, and so does the pair that refills the draws
// or the walk positions (every 64 draws / positions).  profiles/r08_ab_straight_path.txt has the
// loop's waits as compiled, before and after.
// Two paths per pair.  On large tables nearly every pair is *plain*: its
// context-table rows (center, n draws) are distinct rows of the table, none of them is a row of the
// next pair (whose center may be the same), and the next pair has another input row.  One vector
// test over `ids` (the two pairs' rows, one per lane) decides it; a plain pair then skips the
// per-target bookkeeping that exists for aliases -- the range and == center tests, the scan for a
// repeated negative, the compares that patch prefetched copies -- and takes its (1 + n) sigmoids in
// one step across lanes from the LDS copy of the exp table.  Every other pair runs the serial
// resolution.  The arithmetic (loads, fma order, stores, atomics) is the same on both paths.
// What is wave-uniform per target lives in lanes, not in scalar registers: the dots / g_k (`fv`),
// the rows and hot bits (`ids`); the draw batches and the walk's positions sit in LDS, read by
// lane or by uniform address.
// Wavefronts per SIMD the stream kernel is compiled for: at d <= 128, n <= 5 it is held to 64
// VGPRs for 8 waves per SIMD (a 20-byte spill, none of it inside the pair loop).  That was worth
// 108 vs 119 ms per C3 launch against the 7 waves its natural 70 VGPRs give while every pair
// waited for its stores (profiles/r02_ab_stream_occupancy.txt); with one wait per pair the two
// are level, 724.7 vs 722.6 ms (profiles/r08_ab_straight_path.txt: 0.3%, less than three times
// the spread, so the cap stays as it was).  Wider rows / more negatives keep their natural size:
// C5's <4, true, 10> held to 4 waves per SIMD ran 3.57 vs 2.10 s per 1M-walk launch
// (profiles/r05_ab_c5_waves.txt).
// WINDOW (VEC <= 2, w <= kWinMaxW, V < 2^30): input rows marked quiet (a.quiet) are read once per
// stay in the walk window and written back once when they leave it.  Each wavefront keeps a ring
// of 2 kWinMaxW + 1 rows in LDS (5,632 B at d = 128: five 4-wave workgroups per CU, so it is
// compiled for 5 waves per SIMD); lane s of `ring_ids` names the row slot s holds.  A position's
// row enters the ring with its first pair (read by the usual prefetch, stored to the slot instead
// of memory after `in += work`), later prefetches of it are skipped, and the same row at two
// positions of the window shares one slot.  When the center moves, every slot whose row is at no
// position of the new window is stored to memory; the rest at the walk's end.  Hot and ordinary
// rows take the path above unchanged, and one wavefront computes bit for bit what the kernel
// without the ring does (the ring holds the stored value).
constexpr int kWinMaxW = 5;
constexpr int kWinSlots = 2 * kWinMaxW + 1;

template <int VEC, int MAXN, bool WINDOW>
constexpr int stream_waves_per_eu() {
    return WINDOW ? 5 : (VEC <= 2 && MAXN <= 5) ? 8 : 1;
}

template <int VEC, bool FULL, int MAXN, bool WINDOW = false>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(stream_waves_per_eu<VEC, MAXN, WINDOW>())))
    k_sgns_o2_stream(O2Args a) {
    static_assert(!WINDOW || VEC <= 2, "the window ring holds rows of d <= 128");
    using R = Row<VEC, FULL>;
    const int lane = threadIdx.x & 63;
    const int64_t waves_per_block = blockDim.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * waves_per_block;
    const LcgFromTable lc{lane};
    const int d = a.d;
    const int w = a.window;  // <= 31 (launcher): lookups never fall behind the index window
    const int n = a.negative;
    const int path_len = a.L < kMaxSentenceLen ? a.L : kMaxSentenceLen;  // pyx:480
    // V < 2^31 (launcher): one unsigned compare covers r >= 0 && r < V
    const uint32_t Vu = (uint32_t)a.V;
    auto valid_row = [&](int r) { return (uint32_t)r < Vu; };
    // d <= 128: a general pair re-reads the next pair's rows after its write-backs instead of
    // patching the prefetched registers (see the write-back below)
    constexpr bool kReread = VEC <= 2;
    constexpr uint32_t kHotBit = 0x80000000u;
    constexpr uint32_t kQuietBit = WINDOW ? 0x40000000u : 0u;  // walk positions only
    constexpr uint32_t kFlagBits = kHotBit | kQuietBit;
    constexpr int kWaitVm0 = 0x0F70;  // s_waitcnt vmcnt(0), no other counter (gfx9 encoding)
    // the exp table in LDS, staged once per workgroup (4,000 bytes): a lookup is one ds_read
    // instead of two dependent scalar-memory loads, and the plain body does all (1 + n) at once
    __shared__ float s_exp[kExpTableSize];
    for (int i = threadIdx.x; i < kExpTableSize; i += blockDim.x) s_exp[i] = c_exp_table[i];
    __syncthreads();
    // this wavefront's 128 draws in flight (two batches of 64, hot bit in bit 31), in LDS: the
    // next pair's n draws go to lanes of `ids` with one ds_read, and no register holds the batches
    // between refills (a wavefront's LDS accesses execute in order)
    __shared__ uint32_t s_draws[4][128];
    uint32_t *draws = s_draws[threadIdx.x >> 6];
    // and its window of 128 walk positions (encoded rows, see chunk() below), for the same reason
    __shared__ int s_walk[4][128];
    int *wpos = s_walk[threadIdx.x >> 6];
    // WINDOW: this wavefront's ring of quiet input rows, slot s at [s][i][lane] (element
    // lane + 64 i, the registers' layout)
    float *ring = nullptr;
    if constexpr (WINDOW) {
        __shared__ float s_ring[4][kWinSlots * 64 * VEC];
        ring = s_ring[threadIdx.x >> 6];
    }

    for (int64_t p = a.counter ? next_unit(a.counter, 0, 0, lane) : gw; p < a.P;
         p = next_unit(a.counter, p, nwaves, lane)) {
        const int32_t *__restrict__ walk = a.walks + p * (int64_t)a.L;
        // ---- walk indices: positions [wbase, wbase + 128) in two chunks of 64, slid forward.
        // Each entry holds one position's row with its hot bit in bit 31 (gathered when the chunk
        // is loaded, 64 positions ahead of use); -1 = None / past the end.
        auto chunk = [&](int q0) {
            const int q = q0 + lane;
            int v = q < path_len ? walk[q] : -1;
            if (!valid_row(v)) return -1;
            if (a.hot != nullptr && ((a.hot[(uint32_t)v >> 5] >> (v & 31)) & 1u))
                v = (int)((uint32_t)v | kHotBit);
            else if (WINDOW && a.quiet != nullptr &&
                     ((a.quiet[(uint32_t)v >> 5] >> (v & 31)) & 1u))
                v = (int)((uint32_t)v | kQuietBit);
            return v;
        };
        int wbase = 0;
        wpos[lane] = chunk(0);
        wpos[64 + lane] = chunk(64);
        __builtin_amdgcn_wave_barrier();
        auto raw_at = [&](int q) {  // encoded row of walk position q
            if (q >= path_len) return -1;
            while (q - wbase >= 128) {  // positions behind q - 2w are never asked for again
                wbase += 64;
                wpos[lane] = wpos[64 + lane];
                wpos[64 + lane] = chunk(wbase + 64);
                __builtin_amdgcn_wave_barrier();
            }
            return uniform(wpos[q - wbase]);
        };
        // ---- pairs in the reference order (pyx:494-508): center i ascending, j ascending ----
        int it_i = 0, it_j = -1;
        bool nqj = false;  // WINDOW: the pair next_pair() produced has a quiet input row
        auto next_pair = [&](int &ci, int &cj, int &pi, bool &hi, bool &hj) -> bool {
            for (;;) {
                if (it_i >= path_len) return false;
                const int i = it_i;
                const int j0 = i - w < 0 ? 0 : i - w;
                const int j1 = i + w + 1 > path_len ? path_len : i + w + 1;
                if (it_j < j0) it_j = j0;
                const int rci = raw_at(i);
                if (rci == -1 || it_j >= j1) {  // codelens[i] == 0, or the center is done
                    ++it_i;
                    it_j = -1;
                    continue;
                }
                const int j = it_j++;
                if (j == i) continue;
                const int rcj = raw_at(j);
                if (rcj == -1) continue;  // pyx:504
                ci = (int)((uint32_t)rci & ~kFlagBits);
                cj = (int)((uint32_t)rcj & ~kFlagBits);
                if constexpr (WINDOW) nqj = ((uint32_t)rcj & kQuietBit) != 0;
                hi = ((uint32_t)rci & kHotBit) != 0;
                hj = ((uint32_t)rcj & kHotBit) != 0;
                pi = i;
                return true;
            }
        };
        // ---- draws (hot bit in bit 31) ----
        DrawPipe dp;
        dp.used = 0;
        dp.base0 = uniform64(a.seeds[p]);
        if (n > 0) {
            draws[lane] = dp.gather_hot(dp.base0, lc, a);
            dp.base1 = advance64_uniform(dp.base0);
            draws[64 + lane] = dp.gather_hot(dp.base1, lc, a);
            __builtin_amdgcn_wave_barrier();
        }
        auto advance = [&]() {
            if (n == 0) return;
            dp.used += n;
            if (dp.used >= 64) {
                dp.used -= 64;
                draws[lane] = draws[64 + lane];
                dp.base0 = dp.base1;
                dp.base1 = advance64_uniform(dp.base1);
                draws[64 + lane] = dp.gather_hot(dp.base1, lc, a);
                __builtin_amdgcn_wave_barrier();
            }
        };
        // ---- the next pair: ids, hot bits, rows in flight ----
        int nci = -1, ncj = -1, npi = -1;
        bool nhi = false, nhj = false;
        R in_n, pos_n, rn[MAXN + 1];
        R padd;  // kReread: a hot center's change by this pair, owed to the next pair's copy
        bool padd_on = false;
        int prev_i = -1;  // center of the pair just done
        // The context-table rows of two consecutive pairs, one per lane, for the alias test: lanes
        // [0, MAXN] hold the current pair's (ci, t[1..MAXN]), lanes [32, 32 + MAXN] the next
        // pair's (nci, tn[1..MAXN]); draws carry their hot bit, a target past n is 0xFFFFFFFF.
        static_assert(MAXN < 32, "the alias test keeps a pair's rows in half a wavefront");
        uint32_t ids = 0xFFFFFFFFu;
        // rows of the pair next_pair() just produced.  Negative rows are read non-temporally:
        // random rows with little reuse, so the caches keep the packed negative table's words
        // and the hot bitmap instead (with the packed table: 105.7-106.0 vs 108.1 ms per C3
        // launch; no gain with the plain table, profiles/r03_ab_nt_sites.txt)
        // the next pair's k-th negative row, from lane 32 + k of `ids` (past n: no row)
        auto next_target = [&](int k) {
            return k <= n ? (int)(readlane_u32(ids, 32 + k) & ~kHotBit) : -1;
        };
        // WINDOW: the row each ring slot holds, slot s in lane s (-1 = free)
        int ring_ids = -1;
        auto ring_find = [&](int id) {  // the slot holding row id, or -1
            const uint64_t m = __ballot(ring_ids == id);
            return m ? (int)__builtin_ctzll(m) : -1;
        };
        auto ring_write_back = [&](int s) {  // slot s -> memory, and free
            const int id = (int)readlane_u32((uint32_t)ring_ids, s);
            R out;
#pragma unroll
            for (int e = 0; e < VEC; ++e) out.v[e] = ring[(s * VEC + e) * 64 + lane];
            out.store(a.node + (int64_t)id * d, lane, d);
            ring_ids = lane == s ? -1 : ring_ids;
        };
        auto prefetch = [&](bool need_pos) {
            bool held = false;  // a quiet row already in the ring is not read again
            if constexpr (WINDOW) held = nqj && ring_find(ncj) >= 0;
            if (!held) in_n.load(a.node + (int64_t)ncj * d, lane, d);
            if (need_pos) pos_n.load(a.ctx + (int64_t)nci * d, lane, d);
            // lane 32 + k <- draw used + k - 1 (k <= n; used + n <= 127)
            const bool drawn = lane > 32 && lane <= 32 + n;
            const uint32_t nx = drawn ? draws[drawn ? dp.used + lane - 33 : 0] : 0xFFFFFFFFu;
            ids = lane < 32 ? ids : lane == 32 ? (uint32_t)nci : nx;
#pragma unroll
            for (int k = 1; k <= MAXN; ++k) {
                const int tk = next_target(k);
                rn[k].load_nt(a.ctx + (int64_t)(valid_row(tk) ? tk : 0) * d, lane, d);
            }
        };
        // The same rows again, past this CU's L1, once a general pair's write-backs are complete:
        // every load then returns what its row holds after them.
        auto reread = [&](bool need_pos) {
            in_n.load_fresh(a.node + (int64_t)ncj * d, lane, d);
            if (need_pos) pos_n.load_fresh(a.ctx + (int64_t)nci * d, lane, d);
#pragma unroll
            for (int k = 1; k <= MAXN; ++k) {
                const int tk = next_target(k);
                rn[k].load_fresh(a.ctx + (int64_t)(valid_row(tk) ? tk : 0) * d, lane, d);
            }
        };
        bool have = next_pair(nci, ncj, npi, nhi, nhj);
        if (have) prefetch(true);
        if (kReread) __builtin_amdgcn_s_waitcnt(kWaitVm0);  // as after reread() below
        int nupd = 0;
        R pos;  // the current center's positive (carried across the center's pairs while cold)
        bool pos_upd = false;

        while (have) {
            // ---- the next pair becomes the current one ----
            const int ci = nci, cj = ncj, ic = npi;
            const bool hot_ci = nhi, hot_cj = nhj;
            const bool quiet_cj = WINDOW && nqj;
            R in = in_n;
            int t[MAXN + 1];
            R r[MAXN + 1];
#pragma unroll
            for (int k = 1; k <= MAXN; ++k) {
                t[k] = next_target(k);
                r[k] = rn[k];
            }
            const bool new_center = ic != prev_i;
            if (new_center || hot_ci) {  // a hot positive is re-read for every pair
                pos = pos_n;
                if (kReread && padd_on)  // read before the last pair's atomic: copy + change
#pragma unroll
                    for (int e = 0; e < VEC; ++e) pos.v[e] += padd.v[e];
            }
            if (new_center) pos_upd = false;
            prev_i = ic;
            int slot = -1;  // WINDOW: the ring slot of this pair's input row
            if constexpr (WINDOW) {
                uint64_t occ = new_center ? __ballot(ring_ids >= 0) : 0;
                if (occ) {
                    // rows at the new window's positions, one per lane; a slot whose row is at
                    // none of them has left the window
                    // slide the index window up to the last of them first
                    (void)raw_at(ic + w < path_len ? ic + w : path_len - 1);
                    const int q = ic - w + lane;
                    int wid = -1;
                    if (lane <= 2 * w && q >= 0 && q < path_len) {
                        const int v = wpos[q - wbase];
                        wid = v == -1 ? -1 : (int)((uint32_t)v & ~kFlagBits);
                    }
                    while (occ) {
                        const int s = __builtin_ctzll(occ);
                        occ &= occ - 1;
                        const int id = (int)readlane_u32((uint32_t)ring_ids, s);
                        if (__ballot(wid == id) == 0) ring_write_back(s);
                    }
                }
                if (quiet_cj) {
                    slot = ring_find(cj);
                    if (slot >= 0)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) in.v[e] = ring[(slot * VEC + e) * 64 + lane];
                }
            }
            // the next pair's ids move to lanes [0, 32) (v_permlane32_swap: {lower, upper} halves
            // broadcast); prefetch() then writes the pair after it into lanes [32, 32 + MAXN]
            ids = (uint32_t)__builtin_amdgcn_permlane32_swap((int)ids, (int)ids, false, false)[1];
            const uint32_t thm = (uint32_t)__ballot((ids & kHotBit) != 0);  // bit k: t[k] is hot
            // ---- put the pair after it in flight ----
            advance();
            have = next_pair(nci, ncj, npi, nhi, nhj);
            if (have) prefetch(npi != ic || nhi);

            // ---- plain pair?  One test, as vector compares over `ids`: every draw of the pair
            // is a row of the table (pyx:135's range), and no context-table row of this pair
            // equals another row of it or a row of the next pair -- except the center, which the
            // next pair usually shares (the carried positive; handled below for both paths).
            // Then no target is skipped for its id, no negative repeats, and no prefetched copy
            // needs a patch: the pair takes the straight-line body.  Node-table rows alias only
            // as ncj == cj. ----
            const uint32_t idv = ids & ~kHotBit;
            uint64_t alias = __ballot(idv == (uint32_t)ci) & ~(1ull | (1ull << 32));
#pragma unroll
            for (int k = 1; k <= MAXN; ++k)  // t[k] == -1 past n: matches no lane of idv
                alias |= __ballot(idv == (uint32_t)t[k]) & ~(1ull << k);
            const uint64_t negs = (2ull << n) - 2ull;  // lanes 1..n
            // (kReread: nor is the next center, at another position, this center's row)
            const bool plain = have && ncj != cj && alias == 0 &&
                               (__ballot(idv < Vu) & negs) == negs &&
                               !(kReread && nci == ci && npi != ic);

            // ---- the pair (pyx:128-149) ----
            bool valid[MAXN + 1];  // general pairs only; a plain pair's n targets are all valid
#pragma unroll
            for (int k = 1; k <= MAXN; ++k)
                valid[k] = !plain && k <= n && t[k] != ci && valid_row(t[k]);  // pyx:135
            float part[MAXN + 1];
            part[0] = lane_partial(in, pos);
#pragma unroll
            for (int k = 1; k <= MAXN; ++k) part[k] = lane_partial(in, r[k]);
            wave_sum_all(part);  // past n: the dot of row 0, never read
            // every lane holds every sum: keep target k's in lane k of one register
            float fv = 0.0f;
#pragma unroll
            for (int k = 0; k <= MAXN; ++k) fv = lane == k ? part[k] : fv;
            auto f_of = [&](int k) {
                return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fv), k));
            };
            R work;
#pragma unroll
            for (int e = 0; e < VEC; ++e) work.v[e] = 0.0f;
            // A plain pair's (1 + n) sigmoids at once: its dots are final (no target repeats), so
            // skip test, bucket (the same f64 operations, pyx:141-143) and g (pyx:144) run across
            // lanes, the table entry comes from LDS.  g_k replaces the dot in lane k and returns to
            // a scalar by v_readlane; the targets to update are one bit mask.
            uint64_t act = 0;
            if (plain) {
                const bool skip = fv <= -(float)kMaxExp || fv >= (float)kMaxExp;
                int b = (int)(((double)fv + 6.0) * 83.0);
                b = (uint32_t)b < (uint32_t)kExpTableSize ? b : 0;  // skipped lanes: any entry
                act = __ballot(!skip) & ((2ull << n) - 1ull);  // targets 0..n
                fv = (((lane == 0 ? 1.0f : 0.0f) - s_exp[b]) * a.lr) * a.alpha;  // now g_k
            }
            auto g_of = f_of;  // a plain pair's fv holds g_k
            float gpos = 0.0f;  // this pair's g of the positive (0 = skipped)
            {
                float sig = 0.0f;
                if (plain ? (act & 1ull) != 0 : sigmoid_tab(s_exp, f_of(0), &sig)) {
                    const float g = plain ? g_of(0) : ((1.0f - sig) * a.lr) * a.alpha;  // pyx:144
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        work.v[e] = __builtin_fmaf(g, pos.v[e], work.v[e]);  // pyx:146
                        pos.v[e] = __builtin_fmaf(g, in.v[e], pos.v[e]);     // pyx:147
                    }
                    pos_upd = true;
                    gpos = g;
                    ++nupd;
                }
            }
            bool upd[MAXN + 1];
            float gk[MAXN + 1];
#pragma unroll
            for (int k = 1; k <= MAXN; ++k) {
                upd[k] = false;
                gk[k] = 0.0f;
                float g;
                if (plain) {
                    if (!((act >> k) & 1ull)) continue;  // pyx:141-142, or k > n
                    g = g_of(k);
                } else {
                    if (!valid[k]) continue;
                    float f = f_of(k);
                    int prev = -1;  // latest earlier occurrence of the same negative row
#pragma unroll
                    for (int q = 1; q < k; ++q)
                        if (valid[q] && t[q] == t[k]) prev = q;
                    if (prev >= 0) {
#pragma unroll
                        for (int q = 1; q < k; ++q) {
                            if (q == prev) {
                                r[k] = r[q];
                                f = upd[q] ? uniformf(wave_sum(lane_partial(in, r[k]))) : f_of(q);
                            }
                        }
                        fv = lane == k ? f : fv;  // a later repeat may reuse this occurrence's dot
                    }
                    float sig;
                    if (!sigmoid_tab(s_exp, f, &sig)) continue;  // pyx:141-142
                    g = ((0.0f - sig) * a.lr) * a.alpha;  // pyx:144, label 0
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    work.v[e] = __builtin_fmaf(g, r[k].v[e], work.v[e]);  // pyx:146
                    r[k].v[e] = __builtin_fmaf(g, in.v[e], r[k].v[e]);    // pyx:147
                }
                upd[k] = true;
                gk[k] = g;
                ++nupd;
            }
            // ---- write-back: negatives (in order; a repeated row ends with its last version): a
            // hot row receives this occurrence's change (g * in) as a float atomic at the memory
            // side, a cold row is stored.  The next pair's rows were read before these writes.  A
            // plain pair shares none of them.  After a general pair, d <= 128 (kReread): nothing
            // is patched in registers -- the pair waits for its write-backs and reads the next
            // pair's rows again (below), which returns the stored value of a cold row (with walks
            // that share no row the launch stays bit-identical to the sequential order) and, for
            // a hot row, the memory after this wavefront's atomic (the other wavefronts' included).
            // Any assignment to the prefetched registers other than a load, even one skipped at
            // run time, made the compiler copy them after every store and wait for the store
            // (profiles/r08_ab_straight_path.txt).  Wide rows keep one patch for hot and cold
            // copies, the row update's own fma (pyx:147) -- exact for a cold copy read after the
            // previous store (it holds the row this pair updated), and without r[k] live past
            // its store: 149 instead of 181 VGPRs at d = 256, n = 10 (3 waves per SIMD instead of
            // 2: 2137 vs 2741 ms per C5 launch, profiles/r04_ab_stream_patch.txt) ----
            // The pair's one wait for the next pair's rows stands here, before the first store:
            // vmcnt counts loads, stores and atomics in issue order and how many targets a pair
            // writes varies, so a wait placed after them (where the rows rotate next -> current)
            // can only be vmcnt(0), a store round trip per pair.  Here the loads have had the
            // whole pair to land, and the stores get the whole next pair.
            if (kReread) __builtin_amdgcn_s_waitcnt(kWaitVm0);
#pragma unroll
            for (int k = 1; k <= MAXN; ++k) {
                if (!upd[k]) continue;
                if ((thm >> k) & 1u) {
                    R dlt;  // this occurrence's change, g * in
#pragma unroll
                    for (int e = 0; e < VEC; ++e) dlt.v[e] = gk[k] * in.v[e];
                    dlt.atomic_add(a.ctx + (int64_t)t[k] * d, lane, d);
                } else {
                    r[k].store(a.ctx + (int64_t)t[k] * d, lane, d);
                }
                if (!kReread && !plain) {
#pragma unroll
                    for (int q = 1; q <= MAXN; ++q)
                        if (next_target(q) == t[k])
#pragma unroll
                            for (int e = 0; e < VEC; ++e)
                                rn[q].v[e] = __builtin_fmaf(gk[k], in.v[e], rn[q].v[e]);
                    if (have && nci == t[k] && (npi != ic || nhi))
#pragma unroll
                        for (int e = 0; e < VEC; ++e)
                            pos_n.v[e] = __builtin_fmaf(gk[k], in.v[e], pos_n.v[e]);
                }
            }
            // ---- the positive: hot -> this pair's change, g * in, now (memory side); the copy the
            // next pair of this center has in flight predates it and receives it when that pair
            // takes the copy over (padd).  Cold -> stored once when the center ends.
            padd_on = false;
            if (hot_ci && gpos != 0.0f) {
                R pdl;
#pragma unroll
                for (int e = 0; e < VEC; ++e) pdl.v[e] = gpos * in.v[e];
                pdl.atomic_add(a.ctx + (int64_t)ci * d, lane, d);
                if (kReread) {
                    padd = pdl;
                    padd_on = plain && nci == ci;
                } else {
                    if (!plain)
#pragma unroll
                        for (int q = 1; q <= MAXN; ++q)
                            if (next_target(q) == ci)
#pragma unroll
                                for (int e = 0; e < VEC; ++e) rn[q].v[e] += pdl.v[e];
                    if (have && nci == ci)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) pos_n.v[e] += pdl.v[e];
                }
            } else if (!hot_ci && pos_upd && (!have || npi != ic)) {
                pos.store(a.ctx + (int64_t)ci * d, lane, d);
                if (!kReread) {
                    if (!plain)
#pragma unroll
                        for (int q = 1; q <= MAXN; ++q)
                            if (next_target(q) == ci) rn[q] = pos;
                    if (have && nci == ci) pos_n = pos;
                }
            }
            // ---- the input row: in += work (pyx:149) ----
            if (hot_cj) {
                work.atomic_add(a.node + (int64_t)cj * d, lane, d);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) in.v[e] = in.v[e] + work.v[e];
                bool to_ring = false;
                if constexpr (WINDOW) {
                    if (quiet_cj && slot < 0) {  // first pair of its stay: take a free slot
                        const uint64_t free_slots =
                            ~__ballot(ring_ids >= 0) & ((1ull << kWinSlots) - 1ull);
                        if (free_slots) {  // always: at most 2w rows of the window are held
                            slot = __builtin_ctzll(free_slots);
                            ring_ids = lane == slot ? cj : ring_ids;
                        }
                    }
                    to_ring = quiet_cj && slot >= 0;
                    if (to_ring)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) ring[(slot * VEC + e) * 64 + lane] = in.v[e];
                }
                if (!to_ring) in.store(a.node + (int64_t)cj * d, lane, d);
            }
            if (kReread) {
                if (!plain && have) {
                    // every store and atomic of this pair acknowledged (vmcnt counts them with
                    // the loads), then the next pair's rows again
                    __builtin_amdgcn_s_waitcnt(kWaitVm0);
                    reread(npi != ic || nhi);
                    // and landed: with a load pending on any way into the loop's header, the
                    // compiler guards the header's uses with waits that also cover the stores
                    // of a plain pair
                    __builtin_amdgcn_s_waitcnt(kWaitVm0);
                }
            } else if (have && ncj == cj) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) in_n.v[e] += work.v[e];
            }
        }
        if constexpr (WINDOW) {  // rows still in the ring at the walk's end
            uint64_t occ = __ballot(ring_ids >= 0);
            while (occ) {
                const int s = __builtin_ctzll(occ);
                occ &= occ - 1;
                ring_write_back(s);
            }
        }
        if (a.upd_count && lane == 0 && nupd) atomicAdd(a.upd_count, (unsigned long long)nupd);
    }
}

}  // namespace come
