// counter_scan.hpp -- the counter_pn per-key scan shared by the dense
// counter kernel (mat_counter_dense.hip, the batched materialize/4) and the
// fused cached read (read6.hip, read/6 from the snapshot cache): wave
// reductions, row loads, scalar side loads, per-key metadata and the
// newest-to-oldest filter + fold over a key's ops (one wave per key), with
// row-per-lane loads (scan_key) or, for D = 8, lane-contiguous quad rows
// (scan_key_q8).
#pragma once
#include "common.hpp"

namespace agn {
namespace {

__device__ __forceinline__ uint64_t dpp_u64(uint64_t v, int ctrl_id) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    switch (ctrl_id) {
        case 0:
            lo = __builtin_amdgcn_update_dpp(0u, lo, 0xB1, 0xF, 0xF, false);  // quad_perm 1,0,3,2
            hi = __builtin_amdgcn_update_dpp(0u, hi, 0xB1, 0xF, 0xF, false);
            break;
        case 1:
            lo = __builtin_amdgcn_update_dpp(0u, lo, 0x4E, 0xF, 0xF, false);  // quad_perm 2,3,0,1
            hi = __builtin_amdgcn_update_dpp(0u, hi, 0x4E, 0xF, 0xF, false);
            break;
        case 2:
            lo = __builtin_amdgcn_update_dpp(0u, lo, 0x141, 0xF, 0xF, false);  // row_half_mirror
            hi = __builtin_amdgcn_update_dpp(0u, hi, 0x141, 0xF, 0xF, false);
            break;
        default:
            lo = __builtin_amdgcn_update_dpp(0u, lo, 0x140, 0xF, 0xF, false);  // row_mirror
            hi = __builtin_amdgcn_update_dpp(0u, hi, 0x140, 0xF, 0xF, false);
            break;
    }
    return ((uint64_t)hi << 32) | lo;
}

// Full-wave i64 sum: 4 DPP steps make every 16-lane row uniform, then the 4
// row totals are read into SGPRs.
__device__ __forceinline__ int64_t wave_sum_dpp(int64_t x) {
    uint64_t v = (uint64_t)x;
    v += dpp_u64(v, 0);
    v += dpp_u64(v, 1);
    v += dpp_u64(v, 2);
    v += dpp_u64(v, 3);
    uint64_t t = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, r * 16);
        const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), r * 16);
        t += ((uint64_t)hi << 32) | lo;
    }
    return (int64_t)t;
}

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

template <bool NT, class T>
__device__ __forceinline__ T ld(const T *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// One OpSSCommit row; 16-byte loads when the row is 16-byte aligned (D even).
// NT: non-temporal (streamed once; keeps the log from thrashing L2/MALL).
template <int D, bool NT>
__device__ __forceinline__ void load_row(const uint64_t *__restrict__ p, uint64_t (&o)[D]) {
    if constexpr (D % 2 == 0) {
        const u64x2 *q = reinterpret_cast<const u64x2 *>(p);
#pragma unroll
        for (int j = 0; j < D / 2; ++j) {
            const u64x2 x = ld<NT>(q + j);
            o[2 * j] = x.x;
            o[2 * j + 1] = x.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < D; ++j) o[j] = ld<NT>(p + j);
    }
}

// Wave-uniform byte (key_type, sct_ignore) through the scalar cache: an s_load
// of the aligned dword (byte arrays are read in 4-byte units; allocations are
// rounded up far beyond that), so the check never waits on the vector-memory
// queue, where it would drain the cross-key prefetch.
// (ldc: the read-only per-key / per-request arrays load through the scalar
// cache also where the kernel's pointers carry no __restrict__ -- read6.hip,
// k_counter_q8e2's parameter block -- instead of as vector loads each waited
// for before its readfirstlane)
__device__ __forceinline__ uint32_t byte_of(const uint8_t *__restrict__ p, uint64_t idx) {
    const uint32_t w = ldc(reinterpret_cast<const uint32_t *>(p) + (idx >> 2));
    return (w >> ((uint32_t)(idx & 3u) * 8u)) & 0xffu;
}

// Per-key metadata as branch-free scalar loads, so key_off, the segment
// length and the id base share one round trip (a conditional load would be
// scheduled after the previous one's wait): absent arrays are replaced by an
// in-bounds dummy address whose value is discarded.
struct KeyMeta {
    uint64_t off, n;
    uint32_t id0;
};
__device__ __forceinline__ KeyMeta key_meta(uint64_t key, const uint64_t *__restrict__ key_off,
                                            const uint64_t *__restrict__ key_len,
                                            const uint32_t *__restrict__ key_id0) {
    const uint64_t *lp = key_len ? key_len + key : key_off + key + 1;
    const uint32_t *ip = key_id0 ? key_id0 + key : reinterpret_cast<const uint32_t *>(key_off + key);
    const uint64_t off = uniform_u64(ldc(key_off + key));
    const uint64_t l = uniform_u64(ldc(lp));
    const uint32_t id = __builtin_amdgcn_readfirstlane(ldc(ip));
    return KeyMeta{off, key_len ? l : l - off, key_id0 ? id : AGN_ID0_NONE};
}

// Process the key's ops in chunks of 64 (lane = op), rows by 16-byte VGPR
// loads.  The op id that defines NewLastOp is one scalar load after the scan:
// loading every lane's op id with its row instead (+4 B per op, no dependent
// load) measured 2.7 % slower (profiles/r01/ab_counter_ids_wpb.log).
//
// PAIR (small D only, where the registers are free): a key longer than one
// chunk is walked two chunks per step with both chunks' loads issued before
// either is compared (unconditional loads, idle lanes clamped to the key's
// first entry), so a 65..128-op key costs one row round trip instead of two --
// the latency of a small batch (cfg1: 10k keys x 100 ops, one wave per key,
// ~1.2 waves per wave slot) is a few such round trips.
template <int D, bool WARM>
__device__ __forceinline__ void scan_chunk(const uint64_t (&o)[D], int64_t ev, bool valid,
                                           uint64_t b, const uint64_t *__restrict__ txid,
                                           uint64_t txr, uint64_t e, const uint64_t (&r)[D],
                                           const uint64_t (&s)[D], uint64_t (&ct)[D], int64_t &sum,
                                           uint32_t &cnt, int64_t &first_excl,
                                           int64_t &first_err) {
    bool okR = true, leS = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        okR = okR && (o[j] <= r[j]);
        if (WARM) leS = leS && (o[j] <= s[j]);
    }
    bool nip = WARM ? !leS : true;  // belongs_to_snapshot_op (ignore -> true)
    if (txid != nullptr) nip = nip || (txid[e] == txr);
    const bool incl = valid && nip && okR;
    const bool excl = valid && nip && !okR;
    if (first_excl < 0) {
        const uint64_t bx = ballot(excl);
        if (bx) first_excl = (int64_t)b + (int64_t)__builtin_ctzll(bx);
    }
#pragma unroll
    for (int j = 0; j < D; ++j) ct[j] = (incl && o[j] > ct[j]) ? o[j] : ct[j];
    const bool bad = incl && ev == AGN_EFFECT_INVALID;
    cnt += (uint32_t)__builtin_popcountll(ballot(incl));
    if (first_err < 0) {
        const uint64_t be = ballot(bad);
        if (be) first_err = (int64_t)b + (int64_t)__builtin_ctzll(be);
    }
    sum += (incl && !bad) ? ev : 0;
}

template <int D, bool WARM, bool PAIR = false>
__device__ __forceinline__ void scan_key(const uint64_t *__restrict__ oc,
                                         const int64_t *__restrict__ eff,
                                         const uint64_t *__restrict__ txid, uint64_t txr,
                                         uint64_t off, uint64_t n, const uint64_t (&r)[D],
                                         const uint64_t (&s)[D], uint64_t (&ct)[D], int64_t &sum,
                                         uint32_t &cnt, int64_t &first_excl, int64_t &first_err) {
    const int lane = lane_id();
    if constexpr (PAIR) {
        if (n > (uint64_t)AGN_WAVE) {
            for (uint64_t b = 0; b < n; b += 2 * AGN_WAVE) {
                const uint64_t p0 = b + (uint64_t)lane, p1 = p0 + AGN_WAVE;
                const bool v0 = p0 < n, v1 = p1 < n;
                const uint64_t e0 = off + (v0 ? p0 : 0ull), e1 = off + (v1 ? p1 : 0ull);
                uint64_t o0[D], o1[D];
                load_row<D, false>(oc + e0 * D, o0);
                load_row<D, false>(oc + e1 * D, o1);
                const int64_t ev0 = eff[e0], ev1 = eff[e1];
                scan_chunk<D, WARM>(o0, ev0, v0, b, txid, txr, e0, r, s, ct, sum, cnt,
                                    first_excl, first_err);
                scan_chunk<D, WARM>(o1, ev1, v1, b + AGN_WAVE, txid, txr, e1, r, s, ct, sum, cnt,
                                    first_excl, first_err);
            }
            return;
        }
    }
    for (uint64_t b = 0; b < n; b += AGN_WAVE) {
        const uint64_t pos = b + (uint64_t)lane;
        const bool valid = pos < n;
        const uint64_t e = off + (valid ? pos : 0ull);  // in-bounds for idle lanes
        uint64_t o[D];
        load_row<D, false>(oc + e * D, o);
        const int64_t ev = eff[e];
        bool okR = true, leS = true;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            okR = okR && (o[j] <= r[j]);
            if (WARM) leS = leS && (o[j] <= s[j]);
        }
        bool nip = WARM ? !leS : true;  // belongs_to_snapshot_op (ignore -> true)
        if (txid != nullptr) nip = nip || (txid[e] == txr);
        const bool incl = valid && nip && okR;
        const bool excl = valid && nip && !okR;
        if (first_excl < 0) {
            const uint64_t bx = ballot(excl);
            if (bx) first_excl = (int64_t)b + (int64_t)__builtin_ctzll(bx);
        }
#pragma unroll
        for (int j = 0; j < D; ++j) ct[j] = (incl && o[j] > ct[j]) ? o[j] : ct[j];
        const bool bad = incl && ev == AGN_EFFECT_INVALID;
        cnt += (uint32_t)__builtin_popcountll(ballot(incl));
        if (first_err < 0) {
            const uint64_t be = ballot(bad);
            if (be) first_err = (int64_t)b + (int64_t)__builtin_ctzll(be);
        }
        sum += (incl && !bad) ? ev : 0;
    }
}

// ---- presence masks (D <= 8, one mask word per clock) ---------------------
// A sparse log's key whose entries do not all carry the same DC set, or whose
// DCs are not all in R (agn_log.key_mask), is scanned with its per-entry
// masks: lane = op, the row and its mask word loaded together, and the dict
// fold of is_op_in_snapshot (src/clocksi_materializer.erl:236-258): a DC of
// the op missing from R excludes the op (:245-247), a DC missing from SCT
// reads 0 (vectorclock:le), LastOpCt takes the max over each included op's
// own DCs and unites their DC sets (um, per lane).  s[] is SCT with its
// missing DCs already 0.  Same outputs as scan_key otherwise.
template <int D, bool WARM>
__device__ __forceinline__ void scan_key_msk(const uint64_t *__restrict__ oc,
                                             const uint64_t *__restrict__ oc_mask,
                                             const int64_t *__restrict__ eff,
                                             const uint64_t *__restrict__ txid, uint64_t txr,
                                             uint64_t off, uint64_t n, const uint64_t (&r)[D],
                                             const uint64_t (&s)[D], uint64_t rm, uint64_t (&ct)[D],
                                             uint64_t &um, int64_t &sum, uint32_t &cnt,
                                             int64_t &first_excl, int64_t &first_err) {
    constexpr uint64_t FULL = (1ull << D) - 1ull;
    const int lane = lane_id();
    for (uint64_t b = 0; b < n; b += AGN_WAVE) {
        const uint64_t pos = b + (uint64_t)lane;
        const bool valid = pos < n;
        const uint64_t e = off + (valid ? pos : 0ull);
        uint64_t o[D];
        load_row<D, false>(oc + e * D, o);
        const uint64_t m = (oc_mask ? oc_mask[e] : FULL) & FULL;
        const int64_t ev = eff[e];
        bool okR = (m & ~rm) == 0ull, leS = true;  // a DC of the op missing from R: false
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const bool p = ((m >> j) & 1ull) != 0ull;
            okR = okR && (!p || o[j] <= r[j]);
            if (WARM) leS = leS && (!p || o[j] <= s[j]);
        }
        bool nip = WARM ? !leS : true;
        if (txid != nullptr) nip = nip || (txid[e] == txr);
        const bool incl = valid && nip && okR;
        const bool excl = valid && nip && !okR;
        if (first_excl < 0) {
            const uint64_t bx = ballot(excl);
            if (bx) first_excl = (int64_t)b + (int64_t)__builtin_ctzll(bx);
        }
#pragma unroll
        for (int j = 0; j < D; ++j)
            ct[j] = (incl && ((m >> j) & 1ull) && o[j] > ct[j]) ? o[j] : ct[j];
        um |= incl ? m : 0ull;
        const bool bad = incl && ev == AGN_EFFECT_INVALID;
        cnt += (uint32_t)__builtin_popcountll(ballot(incl));
        if (first_err < 0) {
            const uint64_t be = ballot(bad);
            if (be) first_err = (int64_t)b + (int64_t)__builtin_ctzll(be);
        }
        sum += (incl && !bad) ? ev : 0;
    }
}

// OR of a per-lane DC set over the wave (D <= 8 bits), as a scalar.
template <int D>
__device__ __forceinline__ uint64_t wave_or_bits(uint64_t um) {
    uint64_t r = 0;
#pragma unroll
    for (int j = 0; j < D; ++j) r |= (ballot(((um >> j) & 1ull) != 0ull) != 0ull) ? (1ull << j) : 0ull;
    return r;
}

// scan_key for D = 8 with lane-CONTIGUOUS row loads ("quad rows"): load j of a
// 64-op chunk reads bytes [1 KiB j, 1 KiB (j+1)) of the chunk's rows, so
// every instruction covers 8 whole 128-byte lines -- the row-per-lane loads
// of scan_key touch 32 lines per instruction, 32 bytes of each, and request
// every line four times.  Lane l holds DCs 2p, 2p+1 (p = l & 3) of op
// 16 j + (l >> 2): the per-op verdicts are nibbles of wave ballots folded on
// the scalar unit into 64-bit op masks (incl / excl), and the LastOpCt maxima
// stay per part (ctA, ctB) until one xor-shuffle fold at the end of the key.
// The effect (and TxId) loads stay lane = op.  Same results as scan_key.
// One 64-op chunk of quad rows (load j: lane l holds DCs 2p, 2p+1 of op
// 16 j + (l >> 2)) and its effects (lane = op).
struct Q8Chunk {
    u64x2 x[4];
    int64_t ev;
};

template <bool NT, bool EFF_NT>
__device__ __forceinline__ Q8Chunk q8_load(const uint64_t *__restrict__ oc,
                                           const int64_t *__restrict__ eff, uint64_t off,
                                           uint64_t b, uint64_t n_entries) {
    const int lane = lane_id();
    const u64x2 *rows = reinterpret_cast<const u64x2 *>(oc);
    const uint64_t lim = n_entries * 4u - 1u, lim_e = n_entries - 1u;
    Q8Chunk c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint64_t u = (off + b) * 4u + (uint64_t)(j * AGN_WAVE + lane);
        u = u < lim ? u : lim;  // past the log's end: clamped, masked in q8_fold
        c.x[j] = ld<NT>(rows + u);
    }
    uint64_t e = off + b + (uint64_t)lane;
    e = e < lim_e ? e : lim_e;
    c.ev = ld<NT && EFF_NT>(eff + e);
    return c;
}

// noR: R lacks one of the DCs every op of the key carries -- every op is
// excluded (is_op_in_snapshot's missing-DC branch, :245-247); the SCT compare
// (notInPrev) still decides which exclusions count.
template <bool WARM>
__device__ __forceinline__ void q8_fold(const Q8Chunk &c, const uint64_t *__restrict__ txid,
                                        uint64_t txr, uint64_t off, uint64_t b, uint64_t n,
                                        uint64_t n_entries, uint64_t rA, uint64_t rB, uint64_t sA,
                                        uint64_t sB, uint64_t &ctA, uint64_t &ctB, int64_t &sum,
                                        uint32_t &cnt, int64_t &first_excl, int64_t &first_err,
                                        bool noR = false) {
    const int lane = lane_id();
    const int q = lane >> 2;
    const uint64_t valid = (n - b >= (uint64_t)AGN_WAVE) ? ~0ull : ((1ull << (n - b)) - 1ull);
    uint64_t bad = 0, gt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bad |= nib_any16(ballot(c.x[j].x > rA || c.x[j].y > rB)) << (16 * j);
        if (WARM) gt |= nib_any16(ballot(c.x[j].x > sA || c.x[j].y > sB)) << (16 * j);
    }
    uint64_t nip = WARM ? gt : ~0ull;  // belongs_to_snapshot_op: not covered by SCT
    if (txid != nullptr) {
        uint64_t e = off + b + (uint64_t)lane;
        e = e < n_entries - 1u ? e : n_entries - 1u;
        nip |= ballot(txid[e] == txr);
    }
    if (noR) bad = ~0ull;
    const uint64_t incl = valid & nip & ~bad, excl = valid & nip & bad;
    if (first_excl < 0 && excl) first_excl = (int64_t)b + (int64_t)__builtin_ctzll(excl);
    cnt += (uint32_t)__builtin_popcountll(incl);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = ((incl >> (16 * j + q)) & 1ull) != 0ull;
        ctA = (in && c.x[j].x > ctA) ? c.x[j].x : ctA;
        ctB = (in && c.x[j].y > ctB) ? c.x[j].y : ctB;
    }
    const bool mine = ((incl >> lane) & 1ull) != 0ull;
    const bool badv = mine && c.ev == AGN_EFFECT_INVALID;
    if (first_err < 0) {
        const uint64_t be = ballot(badv);
        if (be) first_err = (int64_t)b + (int64_t)__builtin_ctzll(be);
    }
    sum += (mine && !badv) ? c.ev : 0;
}

// q8_load / q8_fold in three steps, for a caller that fetches a chunk's
// effects only once it knows which ops are included (k_counter_quad2): an
// excluded or snapshot-covered op's effect is never read (q8_fold uses c.ev
// under `mine` only), and it is 8 of the 72 bytes an op costs.
// q8_load_rows: the chunk's quad rows alone.
struct Q8Rows {
    u64x2 x[4];
};

template <bool NT>
__device__ __forceinline__ Q8Rows q8_load_rows(const uint64_t *__restrict__ oc, uint64_t off,
                                               uint64_t b, uint64_t n_entries) {
    const int lane = lane_id();
    const u64x2 *rows = reinterpret_cast<const u64x2 *>(oc);
    const uint64_t lim = n_entries * 4u - 1u;
    Q8Rows c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint64_t u = (off + b) * 4u + (uint64_t)(j * AGN_WAVE + lane);
        u = u < lim ? u : lim;  // past the log's end: clamped, masked in q8_verdict
        c.x[j] = ld<NT>(rows + u);
    }
    return c;
}

// q8_verdict: everything q8_fold derives from the rows -- first_excl, cnt and
// the ctA / ctB maxima -- and the chunk's 64-bit mask of included ops.
template <bool WARM>
__device__ __forceinline__ uint64_t q8_verdict(const Q8Rows &c, const uint64_t *__restrict__ txid,
                                               uint64_t txr, uint64_t off, uint64_t b, uint64_t n,
                                               uint64_t n_entries, uint64_t rA, uint64_t rB,
                                               uint64_t sA, uint64_t sB, uint64_t &ctA,
                                               uint64_t &ctB, uint32_t &cnt, int64_t &first_excl,
                                               bool noR = false) {
    const int lane = lane_id();
    const int q = lane >> 2;
    const uint64_t valid = (n - b >= (uint64_t)AGN_WAVE) ? ~0ull : ((1ull << (n - b)) - 1ull);
    uint64_t bad = 0, gt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bad |= nib_any16(ballot(c.x[j].x > rA || c.x[j].y > rB)) << (16 * j);
        if (WARM) gt |= nib_any16(ballot(c.x[j].x > sA || c.x[j].y > sB)) << (16 * j);
    }
    uint64_t nip = WARM ? gt : ~0ull;  // belongs_to_snapshot_op: not covered by SCT
    if (txid != nullptr) {
        uint64_t e = off + b + (uint64_t)lane;
        e = e < n_entries - 1u ? e : n_entries - 1u;
        nip |= ballot(txid[e] == txr);
    }
    if (noR) bad = ~0ull;
    const uint64_t incl = valid & nip & ~bad, excl = valid & nip & bad;
    if (first_excl < 0 && excl) first_excl = (int64_t)b + (int64_t)__builtin_ctzll(excl);
    cnt += (uint32_t)__builtin_popcountll(incl);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = ((incl >> (16 * j + q)) & 1ull) != 0ull;
        ctA = (in && c.x[j].x > ctA) ? c.x[j].x : ctA;
        ctB = (in && c.x[j].y > ctB) ? c.x[j].y : ctB;
    }
    return incl;
}

// q8_load_eff: lane l's effect when op b + l is included (an included op lies
// inside the key, so its address needs no clamp).  Every other lane reads
// `dummy`, one in-bounds address the wave has fetched already: an address
// select, not a branch (a branch around the load is waited for on the spot).
// A chunk without an included op fetches no effect line.
__device__ __forceinline__ int64_t q8_load_eff(const int64_t *__restrict__ eff, uint64_t off,
                                               uint64_t b, uint64_t incl,
                                               const int64_t *__restrict__ dummy) {
    const int lane = lane_id();
    const bool mine = ((incl >> lane) & 1ull) != 0ull;
    const int64_t *p = mine ? eff + (off + b + (uint64_t)lane) : dummy;
    return *p;
}

// q8_fold_eff: first_err and sum from the included ops' effects.
__device__ __forceinline__ void q8_fold_eff(uint64_t incl, int64_t ev, uint64_t b, int64_t &sum,
                                            int64_t &first_err) {
    const bool mine = ((incl >> lane_id()) & 1ull) != 0ull;
    const bool badv = mine && ev == AGN_EFFECT_INVALID;
    if (first_err < 0) {
        const uint64_t be = ballot(badv);
        if (be) first_err = (int64_t)b + (int64_t)__builtin_ctzll(be);
    }
    sum += (mine && !badv) ? ev : 0;
}

// ---- packed rows (agn_log_index_pack; D = 8, cold dense reads) -------------
// A key's OpSSCommit rows as u32 deltas against the key's column minima
// (pack_base[key][d]): 32 bytes per op instead of 64.  A 64-op chunk is 2 KiB,
// two lane-contiguous 16-byte loads: lane l of load j holds DCs 4p .. 4p+3
// (p = l & 1) of op 32 j + (l >> 1).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct P8Rows {
    u32x4 x[2];
};

template <bool NT>
__device__ __forceinline__ P8Rows p8_load_rows(const uint32_t *__restrict__ rows, uint64_t off,
                                               uint64_t b, uint64_t n_entries) {
    const int lane = lane_id();
    const u32x4 *r = reinterpret_cast<const u32x4 *>(rows);
    const uint64_t lim = n_entries * 2u - 1u;
    P8Rows c;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        uint64_t u = (off + b) * 2u + (uint64_t)(j * AGN_WAVE + lane);
        u = u < lim ? u : lim;  // past the log's end: clamped, masked in p8_verdict
        c.x[j] = ld<NT>(r + u);
    }
    return c;
}

// Bit q of the result = some bit of pair q of b (q = 0..31), on the scalar
// unit: nib_any16 for a ballot whose 2 lanes per op are its 2 parts.
__device__ __forceinline__ uint64_t pair_any32(uint64_t b) {
    b = (b | (b >> 1)) & 0x5555555555555555ull;
    b = (b | (b >> 1)) & 0x3333333333333333ull;
    b = (b | (b >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    b = (b | (b >> 4)) & 0x00FF00FF00FF00FFull;
    b = (b | (b >> 8)) & 0x0000FFFF0000FFFFull;
    return (b | (b >> 16)) & 0xFFFFFFFFull;
}

// q8_verdict<false> over packed rows.  thr: this lane's four columns of
// R - pack_base, saturated to 2^32 - 1 -- oc = base + delta <= R iff
// delta <= R - base; noR: R is below the base in some column, so every op is
// excluded.  mx: the lane's running maxima of the included ops' deltas (the
// LastOpCt of the cold read is base + max delta, folded after the key).
__device__ __forceinline__ uint64_t p8_verdict(const P8Rows &c, uint64_t b, uint64_t n,
                                               const u32x4 &thr, bool noR, u32x4 &mx,
                                               uint32_t &cnt, int64_t &first_excl) {
    const int q = lane_id() >> 1;
    const uint64_t valid = (n - b >= (uint64_t)AGN_WAVE) ? ~0ull : ((1ull << (n - b)) - 1ull);
    uint64_t bad = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const u32x4 d = c.x[j];
        bad |= pair_any32(ballot(d.x > thr.x || d.y > thr.y || d.z > thr.z || d.w > thr.w))
               << (32 * j);
    }
    if (noR) bad = ~0ull;
    const uint64_t incl = valid & ~bad, excl = valid & bad;
    if (first_excl < 0 && excl) first_excl = (int64_t)b + (int64_t)__builtin_ctzll(excl);
    cnt += (uint32_t)__builtin_popcountll(incl);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const bool in = ((incl >> (32 * j + q)) & 1ull) != 0ull;
        const u32x4 d = c.x[j];
        mx.x = (in && d.x > mx.x) ? d.x : mx.x;
        mx.y = (in && d.y > mx.y) ? d.y : mx.y;
        mx.z = (in && d.z > mx.z) ? d.z : mx.z;
        mx.w = (in && d.w > mx.w) ? d.w : mx.w;
    }
    return incl;
}

// ---- four packed keys per wave (k_counter_pack4) ---------------------------
// The wave's per-(key, DC) values -- R, pack_base, the thresholds, LastOpCt --
// live one per lane in the "slot" layout the transposed fold below ends in:
// lane l holds key g = l >> 4 and DC d = 4 (l & 1) + 2 ((l >> 3) & 1) +
// ((l >> 2) & 1); bit 1 of the lane does not count (lanes l and l ^ 2 hold the
// same slot).  p4_slot is the slot's index 8 g + d in a [4][8] row group.
__device__ __forceinline__ int p4_slot(int lane) {
    return ((lane >> 4) << 3) + ((lane & 1) << 2) + (((lane >> 3) & 1) << 1) + ((lane >> 2) & 1);
}

// p8_verdict's thresholds of key g from the slot layout: lane l compares DCs
// 4p .. 4p+3 (p = l & 1), held by lanes 16 g + p + {0, 4, 8, 12}.
__device__ __forceinline__ u32x4 p4_thr(uint32_t t, int g) {
    const int src = 16 * g + (lane_id() & 1);
    u32x4 th;
    th.x = (uint32_t)__shfl((int)t, src, AGN_WAVE);
    th.y = (uint32_t)__shfl((int)t, src + 4, AGN_WAVE);
    th.z = (uint32_t)__shfl((int)t, src + 8, AGN_WAVE);
    th.w = (uint32_t)__shfl((int)t, src + 12, AGN_WAVE);
    return th;
}

// The max over the wave of four keys' p8_verdict maxima (16 values per lane),
// as one transposed reduction: at strides 32, 16, 8 and 4 a lane keeps the
// half of its values its lane bit selects (the key pair, the key, the
// component pair, the component) and sends the other half to its partner, the
// stride-2 step folds the one value left -- 8 + 4 + 2 + 1 + 1 shuffles where
// four per-key folds take 4 x 20.  Returns the slot layout: the maximum of key
// g = l >> 4 at DC 4 (l & 1) + 2 ((l >> 3) & 1) + ((l >> 2) & 1).
__device__ __forceinline__ uint32_t p4_maxfold(const u32x4 (&mx)[4]) {
    const int lane = lane_id();
    auto xch = [](uint32_t keep, uint32_t send, int stride) {
        const uint32_t got = (uint32_t)__shfl_xor((int)send, stride, AGN_WAVE);
        return got > keep ? got : keep;
    };
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0,
               b2 = (lane & 4) != 0;
    uint32_t v8[8], v4[4], v2[2];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            v8[4 * k + c] = xch(b5 ? mx[2 + k][c] : mx[k][c], b5 ? mx[k][c] : mx[2 + k][c], 32);
#pragma unroll
    for (int c = 0; c < 4; ++c) v4[c] = xch(b4 ? v8[4 + c] : v8[c], b4 ? v8[c] : v8[4 + c], 16);
#pragma unroll
    for (int j = 0; j < 2; ++j) v2[j] = xch(b3 ? v4[2 + j] : v4[j], b3 ? v4[j] : v4[2 + j], 8);
    const uint32_t v1 = xch(b2 ? v2[1] : v2[0], b2 ? v2[0] : v2[1], 4);
    return xch(v1, v1, 2);
}

// ---- eight narrow keys per wave (k_counter_pack8) --------------------------
// The narrow tier's rows (agn_log_index_pack16): u16 deltas, 16 bytes per op,
// so lane l holds all eight DCs of op l of a key -- dword j its DCs 2j (low
// half) and 2j + 1 -- and a key's verdict is one ballot.  The wave's
// per-(key, DC) values live one per lane: lane l holds key l >> 3, DC l & 7.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// The maxima of the two u16 halves, each on its own.
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
    const u16x2 m = __builtin_elementwise_max(__builtin_bit_cast(u16x2, a),
                                              __builtin_bit_cast(u16x2, b));
    return __builtin_bit_cast(uint32_t, m);
}

__device__ __forceinline__ uint64_t n8_readlane_u64(uint64_t v, int l) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// The 16-byte unit of entry off + lane, clamped at the log's end (the caller
// masks the lanes past the key's length).
template <bool NT>
__device__ __forceinline__ u32x4 n8_load_rows(const uint16_t *__restrict__ rows16, uint64_t off,
                                              uint64_t n_entries) {
    uint64_t e = off + (uint64_t)lane_id();
    e = e < n_entries - 1u ? e : n_entries - 1u;
    return ld<NT>(reinterpret_cast<const u32x4 *>(rows16) + e);
}

// The thresholds min(R - base, 2^16 - 1) of the per-(key, DC) layout, two per
// dword: an even lane 8g + 2j gets DCs 2j (low half) and 2j + 1 of key g, the
// halves of row dword j.
__device__ __forceinline__ uint32_t n8_thr_pack(uint32_t t) {
    const uint32_t nx = __builtin_amdgcn_update_dpp(0u, t, 0xF5, 0xF, 0xF, false);  // quad_perm 1,1,3,3
    return t | (nx << 16);
}

// Nonzero iff this lane's op is excluded by some column: a u16 delta above its
// threshold (th[j]: the thresholds of DCs 2j, 2j + 1, wave-uniform).
// max(d, th) != th per half, so neither half of a dword reaches into the
// other; no short circuit (a branch between the row loads' waits).
__device__ __forceinline__ uint32_t n8_excl(const u32x4 &d, uint32_t th0, uint32_t th1,
                                            uint32_t th2, uint32_t th3) {
    return (pk_max_u16(d.x, th0) ^ th0) | (pk_max_u16(d.y, th1) ^ th1) |
           (pk_max_u16(d.z, th2) ^ th2) | (pk_max_u16(d.w, th3) ^ th3);
}

// q8_load_eff for a lane that knows its own verdict.
__device__ __forceinline__ int64_t n8_load_eff(const int64_t *__restrict__ eff, uint64_t off,
                                               bool mine, const int64_t *__restrict__ dummy) {
    const int64_t *p = mine ? eff + (off + (uint64_t)lane_id()) : dummy;
    return *p;
}

// The max over the wave (lane = op) of eight keys' included deltas (4 dwords
// of 2 halves per key and lane), as one transposed reduction: at strides 32,
// 16 and 8 a lane keeps the keys its lane bit selects and sends the others to
// its partner, at strides 4 and 2 the dwords, at stride 1 one half-word --
// 16 + 8 + 4 + 2 + 1 + 1 exchanges.  Returns the per-(key, DC) layout: lane l
// holds the maximum of key l >> 3 at DC l & 7.
__device__ __forceinline__ uint32_t n8_maxfold(const u32x4 (&mx)[8]) {
    const int lane = lane_id();
    auto xch = [](uint32_t keep, uint32_t send, int stride) {
        return pk_max_u16((uint32_t)__shfl_xor((int)send, stride, AGN_WAVE), keep);
    };
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0,
               b2 = (lane & 4) != 0, b1 = (lane & 2) != 0, b0 = (lane & 1) != 0;
    uint32_t v16[16], v8[8], v4[4], v2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            v16[4 * k + c] = xch(b5 ? mx[4 + k][c] : mx[k][c], b5 ? mx[k][c] : mx[4 + k][c], 32);
#pragma unroll
    for (int c = 0; c < 8; ++c) v8[c] = xch(b4 ? v16[8 + c] : v16[c], b4 ? v16[c] : v16[8 + c], 16);
#pragma unroll
    for (int c = 0; c < 4; ++c) v4[c] = xch(b3 ? v8[4 + c] : v8[c], b3 ? v8[c] : v8[4 + c], 8);
#pragma unroll
    for (int j = 0; j < 2; ++j) v2[j] = xch(b2 ? v4[2 + j] : v4[j], b2 ? v4[j] : v4[2 + j], 4);
    const uint32_t v1 = xch(b1 ? v2[1] : v2[0], b1 ? v2[0] : v2[1], 2);
    const uint32_t m = xch(v1, v1, 1);
    return b0 ? m >> 16 : m & 0xFFFFu;
}

// The i64 sums over the wave of eight keys' per-lane terms, transposed the
// same way: strides 32, 16 and 8 halve the keys, three DPP steps then sum each
// aligned group of eight lanes.  Lane l holds the sum of key l >> 3.
__device__ __forceinline__ uint64_t n8_sumfold(const uint64_t (&s)[8]) {
    const int lane = lane_id();
    auto xch = [](uint64_t keep, uint64_t send, int stride) {
        return keep + shfl_xor_u64(send, stride);
    };
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
    uint64_t v4[4], v2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) v4[k] = xch(b5 ? s[4 + k] : s[k], b5 ? s[k] : s[4 + k], 32);
#pragma unroll
    for (int k = 0; k < 2; ++k) v2[k] = xch(b4 ? v4[2 + k] : v4[k], b4 ? v4[k] : v4[2 + k], 16);
    uint64_t v = xch(b3 ? v2[1] : v2[0], b3 ? v2[0] : v2[1], 8);
    v += dpp_u64(v, 0);
    v += dpp_u64(v, 1);
    v += dpp_u64(v, 2);
    return v;
}

// The effect tier's i16 of entry off + lane (agn_log_index_eff16), as its 16
// bits, under n8_load_rows' clamp: a 64-op key is one 128-byte line.
__device__ __forceinline__ uint32_t n8_load_eff16(const int16_t *__restrict__ eff16, uint64_t off,
                                                  uint64_t n_entries) {
    // min(off + lane, n_entries - 1) as a wave-uniform base plus a 32-bit lane
    // offset: one address VGPR per load
    const uint64_t last = n_entries - 1u;
    const uint64_t o = off < last ? off : last;
    const uint32_t room = last - o < 63u ? (uint32_t)(last - o) : 63u;
    const uint32_t l = (uint32_t)lane_id() < room ? (uint32_t)lane_id() : room;
    return (uint32_t)ld<true>(reinterpret_cast<const uint16_t *>(eff16) + o + l);
}

// n8_sumfold for u32 terms (the effect tier's: 64 terms of magnitude at most
// 32 767 fit an i32): half the registers and half the shuffles.  Lane l holds
// the sum of key l >> 3 mod 2^32.
__device__ __forceinline__ uint32_t n8_sumfold32(const uint32_t (&s)[8]) {
    const int lane = lane_id();
    auto xch = [](uint32_t keep, uint32_t send, int stride) {
        return keep + (uint32_t)__shfl_xor((int)send, stride, AGN_WAVE);
    };
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
    uint32_t v4[4], v2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) v4[k] = xch(b5 ? s[4 + k] : s[k], b5 ? s[k] : s[4 + k], 32);
#pragma unroll
    for (int k = 0; k < 2; ++k) v2[k] = xch(b4 ? v4[2 + k] : v4[k], b4 ? v4[k] : v4[2 + k], 16);
    uint32_t v = xch(b3 ? v2[1] : v2[0], b3 ? v2[0] : v2[1], 8);
    v += __builtin_amdgcn_update_dpp(0u, v, 0xB1, 0xF, 0xF, false);   // quad_perm 1,0,3,2
    v += __builtin_amdgcn_update_dpp(0u, v, 0x4E, 0xF, 0xF, false);   // quad_perm 2,3,0,1
    v += __builtin_amdgcn_update_dpp(0u, v, 0x141, 0xF, 0xF, false);  // row_half_mirror
    return v;
}

// Wave-uniform groups of per-key metadata as one scalar load each: the arrays
// are aligned to their elements only.
typedef unsigned long long u64x4 __attribute__((ext_vector_type(4)));
typedef u64x4 u64x4_a8 __attribute__((aligned(8)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));
__device__ __forceinline__ u64x4 ldc_u64x4(const uint64_t *p) {
    return *(const __attribute__((address_space(4))) u64x4_a8 *)p;
}
__device__ __forceinline__ u32x4 ldc_u32x4(const uint32_t *p) {
    return *(const __attribute__((address_space(4))) u32x4_a4 *)p;
}

// scan_key for D = 8 with lane-CONTIGUOUS row loads ("quad rows"): load j of a
// 64-op chunk reads bytes [1 KiB j, 1 KiB (j+1)) of the chunk's rows, so
// every instruction covers 8 whole 128-byte lines -- the row-per-lane loads
// of scan_key touch 32 lines per instruction, 32 bytes of each, and request
// every line four times.  Lane l holds DCs 2p, 2p+1 (p = l & 3) of op
// 16 j + (l >> 2): the per-op verdicts are nibbles of wave ballots folded on
// the scalar unit into 64-bit op masks (incl / excl), and the LastOpCt maxima
// stay per part (ctA, ctB) until one xor-shuffle fold at the end of the key.
// The effect (and TxId) loads stay lane = op.  Same results as scan_key.
// FROM1: the caller has loaded and folded chunk 0 (read6.hip issues it
// before its cache lookup) and the walk starts at op 64.
template <bool WARM, bool NT, bool EFF_NT = false, bool FROM1 = false>
__device__ __forceinline__ void scan_key_q8(
    const uint64_t *__restrict__ oc, const int64_t *__restrict__ eff,
    const uint64_t *__restrict__ txid, uint64_t txr, uint64_t off, uint64_t n,
    uint64_t n_entries, uint64_t rA, uint64_t rB, uint64_t sA, uint64_t sB, uint64_t &ctA,
    uint64_t &ctB, int64_t &sum, uint32_t &cnt, int64_t &first_excl, int64_t &first_err,
    bool noR = false) {
    for (uint64_t b = FROM1 ? AGN_WAVE : 0; b < n; b += AGN_WAVE) {
        const Q8Chunk c = q8_load<NT, EFF_NT>(oc, eff, off, b, n_entries);
        // every load of the chunk is in flight before the first verdict (left
        // alone, the scheduler interleaves the ballots with the loads and
        // waits for each row load in turn)
        __builtin_amdgcn_sched_barrier(0);
        q8_fold<WARM>(c, txid, txr, off, b, n, n_entries, rA, rB, sA, sB, ctA, ctB, sum, cnt,
                      first_excl, first_err, noR);
    }
}

// scan_key_q8 for a key whose entries carry different DC sets (presence
// masks, D = 8): the quad rows as above plus each op's mask word (lane = op,
// loaded with the effects), which the lanes holding its parts read with one
// shuffle per load.  The dict fold of is_op_in_snapshot (:236-258) per part:
// a DC of the op missing from R (rm) excludes it, absent DCs are not
// compared, SCT's absent DCs are 0 in sA / sB; LastOpCt takes each included
// op's present DCs only, and um (lane = op) collects the included ops' sets.
template <bool WARM>
__device__ __forceinline__ void scan_key_q8_msk(
    const uint64_t *__restrict__ oc, const uint64_t *__restrict__ oc_mask,
    const int64_t *__restrict__ eff, const uint64_t *__restrict__ txid, uint64_t txr,
    uint64_t off, uint64_t n, uint64_t n_entries, uint64_t rA, uint64_t rB, uint64_t sA,
    uint64_t sB, uint64_t rm, uint64_t &ctA, uint64_t &ctB, uint64_t &um, int64_t &sum,
    uint32_t &cnt, int64_t &first_excl, int64_t &first_err) {
    const int lane = lane_id();
    const int q = lane >> 2, p = lane & 3;
    const uint64_t lim_e = n_entries - 1u;
    for (uint64_t b = 0; b < n; b += AGN_WAVE) {
        const Q8Chunk c = q8_load<true, false>(oc, eff, off, b, n_entries);
        uint64_t e = off + b + (uint64_t)lane;
        e = e < lim_e ? e : lim_e;
        const uint32_t m = (uint32_t)(oc_mask ? oc_mask[e] : 0xFFull) & 0xFFu;
        __builtin_amdgcn_sched_barrier(0);
        const uint64_t valid = (n - b >= (uint64_t)AGN_WAVE) ? ~0ull : ((1ull << (n - b)) - 1ull);
        // ops with a DC missing from R
        const uint64_t noR = ballot((m & ~(uint32_t)rm) != 0u);
        uint64_t bad = noR, gt = 0, pres[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t mq = (uint32_t)__shfl((int)m, 16 * j + q, AGN_WAVE);
            pres[j] = mq;
            const bool pa = (mq >> (2 * p)) & 1u, pb = (mq >> (2 * p + 1)) & 1u;
            bad |= nib_any16(ballot((pa && c.x[j].x > rA) || (pb && c.x[j].y > rB))) << (16 * j);
            if (WARM)
                gt |= nib_any16(ballot((pa && c.x[j].x > sA) || (pb && c.x[j].y > sB))) << (16 * j);
        }
        uint64_t nip = WARM ? gt : ~0ull;
        if (txid != nullptr) nip |= ballot(txid[e] == txr);
        const uint64_t incl = valid & nip & ~bad, excl = valid & nip & bad;
        if (first_excl < 0 && excl) first_excl = (int64_t)b + (int64_t)__builtin_ctzll(excl);
        cnt += (uint32_t)__builtin_popcountll(incl);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = ((incl >> (16 * j + q)) & 1ull) != 0ull;
            const bool pa = (pres[j] >> (2 * p)) & 1u, pb = (pres[j] >> (2 * p + 1)) & 1u;
            ctA = (in && pa && c.x[j].x > ctA) ? c.x[j].x : ctA;
            ctB = (in && pb && c.x[j].y > ctB) ? c.x[j].y : ctB;
        }
        const bool mine = ((incl >> lane) & 1ull) != 0ull;
        um |= mine ? (uint64_t)m : 0ull;
        const bool badv = mine && c.ev == AGN_EFFECT_INVALID;
        if (first_err < 0) {
            const uint64_t be = ballot(badv);
            if (be) first_err = (int64_t)b + (int64_t)__builtin_ctzll(be);
        }
        sum += (mine && !badv) ? c.ev : 0;
    }
}

}  // namespace
}  // namespace agn
