// mat_counter_dense.hip — the counter_pn fast path for dense clocks, D <= 8
// (BASELINE cfg1/cfg2 shapes): the same semantics as k_counter (filter.hpp +
// mat_counter.hip), specialised where the general kernel pays for
// generality:
//   * the read clock R and SCT are wave-uniform: explicit noalias kernel
//     arguments + readfirstlane keep them in SGPRs (s_load, no VGPRs);
//   * no presence masks (every DC present), so "+1 encoding" and per-DC
//     branches disappear;
//   * rows are 16-byte VGPR loads (scan_key); for D = 8 a lane-contiguous
//     "quad rows" variant (scan_key_q8, non-temporal); for even D
//     (scan_key_glds) each chunk of 64 entries is streamed
//     (OpSSCommit rows, effects, op ids) into LDS by non-temporal LDS-DMA
//     (global_load_lds), the fastest pure-read idiom measured (7.1-7.2 TB/s
//     against 6.0 for 16-byte VGPR loads, profiles/r01/ab_read_probe.log),
//     and reads the NewLastOp op id from LDS instead of a dependent load --
//     faster on some boxes, slower on others (counter_variant below);
//   * cold (SCT = ignore) and warm reads run separate loop bodies, so the
//     cold body does one D-wide compare per op, exactly the reference's
//     VC compare count;
//   * the i64 effect sum is reduced with DPP row ops + 4 readlanes;
//   * one wave per request and no loop: the grid is the whole batch, so the
//     wave dispatcher overlaps the dependent round trips of different keys
//     (measured against cross-key software pipelines and grouped streams:
//     profiles/r01/ab_counter_key_per_wave.log, ab_grid_oversubscription.log),
//     in XCD-aware block order (xcd_block: consecutive requests share the
//     lines of the per-request arrays inside one L2);
//   * per-key side values (key_type, sct_ignore, base value) are scalar
//     loads, never vector loads + vmcnt(0).
// HBM bytes per op: 8*D + 8; per key: 8 + 16*D + 32;
// the LDS-DMA path also reads the chunk's 4-byte op ids (+4 per op).
#include <atomic>
#include <cstdlib>
#include <vector>

#include "counter_scan.hpp"

namespace agn {
namespace {

// k_counter_q8e's hand-on sub-lists: count, and the stride of their counters
// (uint32 words: one 128-byte line each)
constexpr uint32_t QL_S = 1024, QL_STRIDE = 32;

// The counter launchers' block order (block_order's mode): the XCD-aware
// order for small batches, else runs of `bulk` blocks per XCD (order_or:
// AGN_XCD_REMAP / AGN_XCD_CHUNK override).  Same-box A/Bs
// (profiles/r06/ab_xcd_chunk.log): dense cfg2 runs of 64 7.57 ms against
// 7.83 identity and 7.92 XCD-aware, warm 7.43 against 7.69; the masked
// q8e in one process 8.02 against 8.18 identity and 8.37 XCD-aware (with
// the bench's hints), its warm two-per-wave form level in every order.
inline uint32_t counter_order(uint64_t n_req, uint32_t bulk) {
    return order_or(n_req < (1ull << 20) ? 1u : bulk);
}
constexpr uint32_t BULK_CHUNK = 64;
// k_counter_pack4 (four requests per block): the run per XCD -- cold cfg2 in
// one process 4.176 ms in runs of 64, 4.217 of 32, 4.170 of 128
// (profiles/r10/ab_q2_four.log) -- and whether the launcher takes the kernel
// without AGN_Q2_FOUR set (4.176 against 4.752 ms there).
constexpr uint32_t BULK_CHUNK4 = 64;
constexpr bool Q2_FOUR_DEFAULT = true;
// k_counter_pack8 (eight requests per block over the narrow tier): the run per
// XCD -- cold cfg2 in one process 2.549 ms in runs of 64, 2.615 of 32, 2.547 of
// 128 (profiles/r11/ab_q2_narrow.log) -- and the launcher's bound on the log's
// wide keys: at most one key in NARROW_WIDE_DIV may lack the narrow form (a
// group holding one runs its eight requests one after the other through oc).
// At the bound, 1M keys x 64 ops with one key in 1024 wide, the kernel ran
// 0.331 against 0.469 ms for k_counter_pack4 (1.42x; one in 256: 1.32x;
// profiles/r11/ab_narrow_bound.log), so the bound stands as estimated.
constexpr uint32_t BULK_CHUNK8 = 64;
constexpr uint64_t NARROW_WIDE_DIV = 1024;
// k_counter_pack8<true> (the effect tier, agn_log_index_eff16): whether the
// launcher takes it without AGN_Q2_EFF16 set, and its bound on the log's
// escaped entries: at most one entry in EFF16_ESC_DIV may hold the escape (a
// group whose included ops hold one takes the kernel's branch to `eff`).
// Cold cfg2 in one process 2.373 ms with the tier against 2.707 without
// (profiles/r12/ab_q2_eff16.log).  At the bound, 1M keys x 64 ops with one
// entry in 1024 escaped, evenly spread, 0.257 against 0.289 ms (1.12x; one in
// 256: 1.16x; one in 64, an escape in every key: 1.12x;
// profiles/r12/ab_eff_bound.log): the tier did not lose at any density
// measured, and the bound stands as estimated.
constexpr bool EFF16_DEFAULT = true;
constexpr uint64_t EFF16_ESC_DIV = 1024;

struct DenseArgs {
    uint64_t n_req;
    uint64_t n_entries;
    uint32_t req_type;
    uint32_t xcd;  // block_order mode: 0 identity, 1 xcd_block, g >= 2 runs of g per XCD
    uint32_t pair; // 1: D <= 4 keys longer than a chunk walk two chunks per step
    uint32_t qnt;  // quad rows, non-temporal loads: bit 0 rows, bit 1 effects (AGN_COUNTER_QUAD_NT)
    uint32_t hints;  // agn_read.hints (k_counter_q8e / k_counter_quad2)
    uint32_t ql_cap; // k_counter_q8e / q8m: entries per hand-on sub-list
};

// Presence masks of a sparse batch (the MSK instantiations; one word per
// clock, D <= 8): agn_log.key_mask / oc_mask, agn_read.R_mask / sct_mask and
// agn_result.lastct_mask.  Any may be null (= every DC present).
struct MaskArgs {
    const uint64_t *key_mask, *oc_mask, *R_mask, *sct_mask;
    uint64_t *o_mask;
};

// A request of a sparse batch: the DC set U every op of its key carries (0 =
// the entries differ or it is unknown), R's and SCT's DC sets, and whether
// the dense scan serves it exactly (uni: no ops, or U is known and inside R:
// then every compare of is_op_in_snapshot's dict fold is a compare of U's
// columns, src/clocksi_materializer.erl:236-258, and the columns outside U
// are neutralised -- R and SCT read as +inf there, so they never exclude an
// op nor keep it out of the snapshot; LastOpCt keeps SCT's value there).
template <int D>
struct Presence {
    uint64_t U, Rm, Sm;
    bool uni;
};

template <int D, bool MSK>
__device__ __forceinline__ Presence<D> presence(const MaskArgs &m, uint64_t kmw, uint64_t rmw,
                                                uint64_t smw, uint64_t n) {
    constexpr uint64_t FULL = (1ull << D) - 1ull;
    Presence<D> p;
    if constexpr (!MSK) {
        p.U = p.Rm = p.Sm = FULL;
        p.uni = true;
    } else {
        // a log without masks: every entry carries every DC
        p.U = m.oc_mask ? (m.key_mask ? (kmw & FULL) : 0ull) : FULL;
        p.Rm = m.R_mask ? (rmw & FULL) : FULL;
        p.Sm = m.sct_mask ? (smw & FULL) : FULL;
        p.uni = n == 0 || (p.U != 0ull && (p.U & ~p.Rm) == 0ull);
    }
    return p;
}

typedef __attribute__((address_space(3))) void *lds_ptr;

// LDS words per wave of the LDS-DMA path: rows (DCP*64 u64, reused as the
// LastOpCt stage), effects (64 u64), op ids (64 u32).
template <int D>
struct GldsLds {
    static constexpr int DCP = D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : 8;
    static constexpr int ROWS = DCP * AGN_WAVE, EFF = ROWS, OPID = EFF + AGN_WAVE,
                         WORDS = OPID + AGN_WAVE / 2;
};

// scan_key for even D through LDS-DMA: each chunk of 64 log entries is
// fetched by global_load_lds (non-temporal) into the wave's LDS slice --
// D/2 x 1 KiB of OpSSCommit rows (image linear: row of lane l at 8*D*l
// bytes), the effects and the op ids as 4-byte pieces -- then every lane
// reads its row back with ds_read_b128.  Addresses past the end of the log
// are clamped (those lanes are idle).  Returns the op id that defines
// NewLastOp, read from LDS: fetching the chunk's 256 B of op ids with the
// rows (+5.4 % bytes) removes the dependent round trip a scalar load of the
// one id costs after the scan (measured 8.09 -> 7.29 ms on cfg2,
// profiles/r01/ab_counter_glds.log).  Only DMA loads are in flight, so the
// one vmcnt(0) per chunk drains nothing else.
template <int D, bool WARM>
__device__ __forceinline__ int64_t scan_key_glds(
    const uint64_t *__restrict__ oc, const int64_t *__restrict__ eff,
    const uint32_t *__restrict__ op_id, const uint64_t *__restrict__ txid, uint64_t txr,
    uint64_t off, uint64_t n, uint64_t n_entries, const uint64_t (&r)[D],
    const uint64_t (&s)[D], uint64_t (&ct)[D], int64_t &sum, uint32_t &cnt,
    int64_t &first_excl, int64_t &first_err, uint64_t *lds) {
    using L = GldsLds<D>;
    const int lane = lane_id();
    const uint64_t lim_oc = n_entries * D - 2u, lim_e = n_entries * 2u - 1u,
                   lim_id = n_entries - 1u;
    const uint32_t *ids = reinterpret_cast<const uint32_t *>(lds + L::OPID);
    int64_t hid = -1;
    for (uint64_t b = 0; b < n; b += AGN_WAVE) {
        const uint64_t pos = b + (uint64_t)lane;
        const bool valid = pos < n;
        const uint64_t e = off + (valid ? pos : 0ull);
        const uint64_t cb = (off + b) * D;
#pragma unroll
        for (int j = 0; j < D / 2; ++j) {
            uint64_t q = cb + (uint64_t)(j * AGN_WAVE + lane) * 2u;
            q = q < lim_oc ? q : lim_oc;
            __builtin_amdgcn_global_load_lds((const void *)(oc + q), (lds_ptr)(lds + j * 2 * AGN_WAVE),
                                             16, 0, 2 /* nt */);
        }
        const uint32_t *e32 = reinterpret_cast<const uint32_t *>(eff);
#pragma unroll
        for (int j = 0; j < 2; ++j) {  // i64 effects as 2 x 64 dwords
            uint64_t q = (off + b) * 2u + (uint64_t)(j * AGN_WAVE + lane);
            q = q < lim_e ? q : lim_e;
            __builtin_amdgcn_global_load_lds((const void *)(e32 + q),
                                             (lds_ptr)(lds + L::EFF + j * AGN_WAVE / 2), 4, 0, 2);
        }
        {
            uint64_t q = off + b + (uint64_t)lane;
            q = q < lim_id ? q : lim_id;
            __builtin_amdgcn_global_load_lds((const void *)(op_id + q), (lds_ptr)(lds + L::OPID), 4,
                                             0, 2);
        }
        __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) lgkmcnt(0): the DMA has landed
        __builtin_amdgcn_wave_barrier();
        uint64_t o[D];
        const u64x2 *lr = reinterpret_cast<const u64x2 *>(lds + (uint64_t)lane * D);
#pragma unroll
        for (int j = 0; j < D / 2; ++j) {
            const u64x2 x = lr[j];
            o[2 * j] = x.x;
            o[2 * j + 1] = x.y;
        }
        const int64_t ev = (int64_t)lds[L::EFF + lane];
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
            if (bx) {
                first_excl = (int64_t)b + (int64_t)__builtin_ctzll(bx);
                hid = (int64_t)ids[__builtin_ctzll(bx)];
            }
        }
        if (first_excl < 0 && b + AGN_WAVE >= n) hid = (int64_t)ids[(n - 1) - b];  // get_first_id
#pragma unroll
        for (int j = 0; j < D; ++j) ct[j] = (incl && o[j] > ct[j]) ? o[j] : ct[j];
        const bool bad = incl && ev == AGN_EFFECT_INVALID;
        cnt += (uint32_t)__builtin_popcountll(ballot(incl));
        if (first_err < 0) {
            const uint64_t be = ballot(bad);
            if (be) first_err = (int64_t)b + (int64_t)__builtin_ctzll(be);
        }
        sum += (incl && !bad) ? ev : 0;
        __builtin_amdgcn_wave_barrier();  // LDS reads done before the next chunk's DMA
    }
    return hid;
}

// Row-load variants of k_counter_key (bit-identical results; agn_tune picks
// per device): VGPR rows (scan_key), LDS-DMA rows (scan_key_glds, even D),
// quad rows (scan_key_q8, D = 8, non-temporal).
enum { ROWS_VGPR = 0, ROWS_GLDS = 1, ROWS_QUAD = 2, ROWS_QUAD2 = 3 };

// One wave = one request, no loop: the grid is the batch (ceil(n_req / WPB)
// blocks).  Measured on cfg2 this beats every software-pipelined variant
// above: with ~10M short-lived waves the dispatcher keeps every CU's wave
// slots full and the HBM queue deep, while each wave's dependent round trips
// (metadata -> rows -> NewLastOp id) overlap with other waves' instead of
// serialising inside one.  Side values are scalar loads (no vmcnt drains).
// R, key_off, the segment length and the consecutive-id base (key_id0) are
// issued as one group of scalar loads, and with key_id0 the NewLastOp id
// needs no load after the scan: +0.9 % against the previous prologue
// (profiles/r01/ab_counter_prologue.log).  Where the rest of the gap to the
// read ceiling goes (diagnostic builds, scripts/build_diag.sh,
// profiles/r01/ab_counter_attribution.log): not latency -- two requests per
// wave with both keys' rows in flight (2x bytes per wave slot) measured
// +0.2 %, dropping the metadata loads 0.3 % -- but the per-key result
// writes: 92 B per key (1.9 % of the bytes) cost 9 % of the kernel time
// (writing 16 B instead: 8.33 -> 7.57 ms), full 128 B record lines 1 %,
// non-temporal stores +7 % worse.  The HBM read/write turnaround, not the
// instruction stream, is the remaining bound.
template <int D, bool ANY_WARM, int WPB, int VAR, bool KEYS, bool MSK>
__global__ __launch_bounds__(64 * WPB) void k_counter_key(
    DenseArgs a, MaskArgs mk, const uint64_t *__restrict__ keys,
    const uint64_t *__restrict__ key_off, const uint64_t *__restrict__ key_len,
    const uint8_t *__restrict__ key_type, const uint32_t *__restrict__ key_id0,
    const uint64_t *__restrict__ oc, const uint32_t *__restrict__ op_id,
    const int64_t *__restrict__ eff, const uint64_t *__restrict__ log_txid,
    const uint64_t *__restrict__ R, const uint64_t *__restrict__ sct,
    const uint8_t *__restrict__ sct_ignore, const uint64_t *__restrict__ req_txid,
    const int64_t *__restrict__ base_value, int64_t *__restrict__ o_value,
    int64_t *__restrict__ o_hole, uint64_t *__restrict__ o_lastct,
    uint32_t *__restrict__ o_count, uint32_t *__restrict__ o_flags,
    uint32_t *__restrict__ o_err) {
    constexpr int DCP = D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : 8;  // pow2 >= D
    constexpr int V = DCP;                                          // op slots per lane
    constexpr bool GLDS = VAR == ROWS_GLDS;
    constexpr bool QUAD = VAR == ROWS_QUAD && D == 8;
    static_assert(!(MSK && GLDS), "sparse batches use VGPR or quad rows");
    constexpr int LW = GLDS ? GldsLds<D>::WORDS : QUAD ? 1 : DCP * AGN_WAVE;
    __shared__ uint64_t lds_all[WPB][LW];  // GLDS: chunk rows/effects/ids; then the ct stage

    const int lane = lane_id();
    const int w = WPB == 1 ? 0 : (int)(threadIdx.x >> 6);
    // unconditional (as the side loads below): a conditional scalar load is
    // waited for on its own
    const uint32_t blk = block_order(a.xcd, blockIdx.x, gridDim.x);
    const uint64_t i = uniform_u64((uint64_t)blk * WPB + (uint64_t)w);
    if (i >= a.n_req) return;
    uint64_t r[D], s[D], e[D], ct[D];
#pragma unroll
    for (int j = 0; j < D; ++j) r[j] = uniform_u64(R[i * D + j]);  // issued with the key's metadata
    // KEYS = false (identity key map): R and the key's metadata in one round trip
    const uint64_t key = KEYS ? uniform_u64(keys[i]) : i;
    const KeyMeta km = key_meta(key, key_off, key_len, key_id0);
    const uint64_t off = km.off, n = km.n;
    const uint32_t id0 = km.id0;  // consecutive-id base (agn_log_index_ids)
    // The side bytes and rows (key_type, sct_ignore, SCT, TxId) load
    // unconditionally -- from an in-bounds dummy when the column is absent --
    // so they share the metadata's round trip: a conditional scalar load is
    // waited for on its own before the row loads issue.
    const uint32_t kty =
        byte_of(key_type ? key_type : reinterpret_cast<const uint8_t *>(key_off), key);
    const uint64_t *sct_p = (ANY_WARM && sct) ? sct : R;
    const uint32_t sib =
        ANY_WARM ? byte_of(sct_ignore ? sct_ignore : reinterpret_cast<const uint8_t *>(R), i) : 0u;
    const uint64_t txv = uniform_u64((req_txid ? req_txid : R)[i]);
    uint64_t sv[D];
#pragma unroll
    for (int j = 0; j < D; ++j) sv[j] = ANY_WARM ? uniform_u64(sct_p[i * D + j]) : 0ull;
    // sparse batch: the key's DC set and R's / SCT's mask words, same round trip
    uint64_t kmw = 0, rmw = 0, smw = 0;
    if constexpr (MSK) {
        kmw = uniform_u64(*(mk.key_mask ? mk.key_mask + key : R));
        rmw = uniform_u64(*(mk.R_mask ? mk.R_mask + i : R));
        smw = uniform_u64(*((ANY_WARM && mk.sct_mask) ? mk.sct_mask + i : R));
    }
    if (n != 0 && key_type != nullptr && kty != (a.req_type & 0xffu)) {
        if (lane == 0) {  // erlang:error(corrupted_ops_cache) (:190-191)
            o_flags[i] = AGN_F_ERR_CORRUPTED;
            o_err[i] = 0xffffffffu;
        }
        return;
    }
    const bool sct_ign = !ANY_WARM || sct == nullptr || (sct_ignore && sib != 0u);
    const Presence<D> pr = presence<D, MSK>(mk, kmw, rmw, smw, n);
#pragma unroll
    for (int j = 0; j < D; ++j) {
        // e = SCT as a dict read (missing DC = 0); LastOpCt starts as it
        // (materialize/4 :94-95).  s = the compare value: +inf outside U on
        // the dense scan of a sparse key.
        const bool inU = ((pr.U >> j) & 1ull) != 0ull;
        e[j] = (sct_ign || !((pr.Sm >> j) & 1ull)) ? 0ull : sv[j];
        s[j] = (MSK && pr.uni && !inU) ? ~0ull : e[j];
        r[j] = (MSK && pr.uni && !inU) ? ~0ull : r[j];
        ct[j] = e[j];
    }
    const uint64_t txr = req_txid ? txv : 0ull;
    const uint64_t *tx = (txr != 0ull) ? log_txid : nullptr;
    int64_t sum = 0, first_excl = -1, first_err = -1;
    uint32_t cnt = 0;
    int64_t hid = -1;
    uint64_t um = 0;            // MSK, mixed key: DCs of the included ops (per lane)
    uint64_t ctA = 0, ctB = 0;  // QUAD: LastOpCt of DCs 2p, 2p+1 (p = lane & 3)
    const bool warm = ANY_WARM && !sct_ign;
#define AGN_MSK_SCAN()                                                                         \
    do {                                                                                       \
        if (!warm)                                                                             \
            scan_key_msk<D, false>(oc, mk.oc_mask, eff, tx, txr, off, n, r, s, pr.Rm, ct, um,  \
                                   sum, cnt, first_excl, first_err);                           \
        else                                                                                   \
            scan_key_msk<D, ANY_WARM>(oc, mk.oc_mask, eff, tx, txr, off, n, r, s, pr.Rm, ct,   \
                                      um, sum, cnt, first_excl, first_err);                    \
    } while (0)
    if constexpr (QUAD) {
        const int p = lane & 3;
        const uint64_t rA = p == 0 ? r[0] : p == 1 ? r[2 % D] : p == 2 ? r[4 % D] : r[6 % D];
        const uint64_t rB = p == 0 ? r[1 % D] : p == 1 ? r[3 % D] : p == 2 ? r[5 % D] : r[7 % D];
        const uint64_t sA = p == 0 ? s[0] : p == 1 ? s[2 % D] : p == 2 ? s[4 % D] : s[6 % D];
        const uint64_t sB = p == 0 ? s[1 % D] : p == 1 ? s[3 % D] : p == 2 ? s[5 % D] : s[7 % D];
        const uint64_t eA = p == 0 ? e[0] : p == 1 ? e[2 % D] : p == 2 ? e[4 % D] : e[6 % D];
        const uint64_t eB = p == 0 ? e[1 % D] : p == 1 ? e[3 % D] : p == 2 ? e[5 % D] : e[7 % D];
        ctA = eA;
        ctB = eB;
#define AGN_Q8(W, NT, ENT)                                                                     \
    scan_key_q8<W, NT, ENT>(oc, eff, tx, txr, off, n, a.n_entries, rA, rB, sA, sB, ctA, ctB, sum, \
                            cnt, first_excl, first_err)
        if (!MSK || pr.uni) {
            if (!warm) {
                if (a.qnt & 2u) AGN_Q8(false, true, true);
                else if (a.qnt & 1u) AGN_Q8(false, true, false);
                else AGN_Q8(false, false, false);
            } else {
                if (a.qnt & 2u) AGN_Q8(ANY_WARM, true, true);
                else if (a.qnt & 1u) AGN_Q8(ANY_WARM, true, false);
                else AGN_Q8(ANY_WARM, false, false);
            }
            if (MSK) {  // outside U: SCT's value (an op's row there is not in its dict)
                ctA = ((pr.U >> (2 * p)) & 1ull) ? ctA : eA;
                ctB = ((pr.U >> (2 * p + 1)) & 1ull) ? ctB : eB;
            }
        } else if constexpr (MSK) {
            // a mixed key: the quad rows with each op's mask word
            if (!warm)
                scan_key_q8_msk<false>(oc, mk.oc_mask, eff, tx, txr, off, n, a.n_entries, rA, rB,
                                       sA, sB, pr.Rm, ctA, ctB, um, sum, cnt, first_excl,
                                       first_err);
            else
                scan_key_q8_msk<ANY_WARM>(oc, mk.oc_mask, eff, tx, txr, off, n, a.n_entries, rA,
                                          rB, sA, sB, pr.Rm, ctA, ctB, um, sum, cnt, first_excl,
                                          first_err);
        }
#undef AGN_Q8
    } else if constexpr (GLDS && D % 2 == 0) {
        if (!ANY_WARM || sct_ign)
            hid = scan_key_glds<D, false>(oc, eff, op_id, tx, txr, off, n, a.n_entries, r, s, ct,
                                          sum, cnt, first_excl, first_err, lds_all[w]);
        else
            hid = scan_key_glds<D, ANY_WARM>(oc, eff, op_id, tx, txr, off, n, a.n_entries, r, s,
                                             ct, sum, cnt, first_excl, first_err, lds_all[w]);
    } else {
        if (MSK && !pr.uni) {
            if constexpr (MSK) AGN_MSK_SCAN();
        } else if (D <= 4 && a.pair) {
            if (!warm)
                scan_key<D, false, true>(oc, eff, tx, txr, off, n, r, s, ct, sum, cnt, first_excl,
                                         first_err);
            else
                scan_key<D, ANY_WARM, true>(oc, eff, tx, txr, off, n, r, s, ct, sum, cnt,
                                            first_excl, first_err);
        } else {
            if (!warm)
                scan_key<D, false>(oc, eff, tx, txr, off, n, r, s, ct, sum, cnt, first_excl,
                                   first_err);
            else
                scan_key<D, ANY_WARM>(oc, eff, tx, txr, off, n, r, s, ct, sum, cnt, first_excl,
                                      first_err);
        }
        if (MSK && pr.uni) {
#pragma unroll
            for (int j = 0; j < D; ++j) ct[j] = ((pr.U >> j) & 1ull) ? ct[j] : e[j];
        }
    }
#undef AGN_MSK_SCAN
    // NewLastOp id and base value: scalar loads, issued before the reductions
    if (hid < 0) {
        const uint64_t pos = first_excl >= 0 ? (uint64_t)first_excl : n - 1;
        if (id0 != AGN_ID0_NONE)  // op_id[off + pos] == id0 + pos (agn_log_index_ids)
            hid = n ? (int64_t)((uint64_t)id0 + pos) : 0;
        else
            hid = n ? (int64_t)op_id[uniform_u64(off + pos)] : 0;
    }
    const int64_t base = base_value ? (int64_t)uniform_u64((uint64_t)base_value[i]) : 0;

    const int64_t total = wave_sum_dpp(sum);
    const bool ct_ign = sct_ign && cnt == 0u;
    if constexpr (QUAD) {
        // LastOpCt: the 16 lanes of each part fold by xor-shuffles; lanes 0..3
        // write the row's 4 x 16 bytes
#pragma unroll
        for (int x = 4; x < AGN_WAVE; x <<= 1) {
            ctA = umax64(ctA, shfl_xor_u64(ctA, x));
            ctB = umax64(ctB, shfl_xor_u64(ctB, x));
        }
        if (lane < 4) {
            u64x2 v;
            v.x = ct_ign ? 0ull : ctA;
            v.y = ct_ign ? 0ull : ctB;
            reinterpret_cast<u64x2 *>(o_lastct + i * D)[lane] = v;
        }
    } else {
        // LastOpCt: per-lane maxima -> LDS [DCP][64] -> each lane folds V slots
        // of one DC -> xor-shuffle across the 64/DCP lanes that share it
        uint64_t(*stage)[AGN_WAVE] = reinterpret_cast<uint64_t(*)[AGN_WAVE]>(lds_all[w]);
#pragma unroll
        for (int j = 0; j < D; ++j) stage[j][lane] = ct[j];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int c = lane % DCP, g = lane / DCP;
        uint64_t m = 0;
        if (c < D) {
#pragma unroll
            for (int v = 0; v < V; ++v) m = umax64(m, stage[c][g * V + v]);
        }
#pragma unroll
        for (int x = DCP; x < AGN_WAVE; x <<= 1) m = umax64(m, shfl_xor_u64(m, x));
        if (g == 0 && c < D) o_lastct[i * D + (uint64_t)c] = ct_ign ? 0ull : m;
    }
    // LastOpCt's DC set: SCT's united with the included ops' (U, or the
    // per-lane sets of a mixed key)
    uint64_t mo = 0;
    if constexpr (MSK) {
        const uint64_t un = pr.uni ? (cnt ? pr.U : 0ull) : wave_or_bits<D>(um);
        mo = ct_ign ? 0ull : ((sct_ign ? 0ull : pr.Sm) | un);
    }
    if (lane == 0) {
        // NewLastOp = id(oldest excluded) - 1, else get_first_id (:49-63)
        const int64_t hole = first_excl >= 0 ? hid - 1 : hid;
        uint32_t fl = 0;
        if (cnt) fl |= AGN_F_NEWSS;
        if (ct_ign) fl |= AGN_F_CT_IGNORE;
        if (first_err >= 0) fl |= AGN_F_ERR_UNEXPECTED;
        o_value[i] = (int64_t)((uint64_t)base + (uint64_t)total);
        o_hole[i] = hole;
        o_count[i] = cnt;
        o_flags[i] = fl;
        o_err[i] = first_err >= 0 ? (uint32_t)(off + (uint64_t)first_err) : 0xffffffffu;
        if (MSK && mk.o_mask) mk.o_mask[i] = mo;
    }
}

// agn_log.key_id0, unless AGN_COUNTER_ID0=0 (A/B knob: always load the op id)
inline const uint32_t *id0_index(const agn_log &log) {
    const char *v = AGN_KNOB("AGN_COUNTER_ID0");
    return (v && v[0] == '0') ? nullptr : log.key_id0;
}

// ROWS_QUAD2 (D = 8): quad rows, TWO requests per wave with both keys'
// first chunks in flight at once (9 KiB of rows per wave slot instead of 4.5).
// Same results as k_counter_key.  The default for warm batches (the SCT
// rows and flags lengthen each request's prologue, which the second key's
// loads cover); cold batches measured no change (56 VGPRs, 8 waves).
// AGN_COUNTER_VARIANT=3 forces it, =2 the one-request form.
struct Q2Key {
    uint64_t i, key, off, n, txr;
    uint32_t id0;
    bool corrupt, sct_ign;
    bool uni;  // the dense scan serves the key: its DC set U is known (MSK) or the batch is dense
    bool noR;  // MSK: U is known but R lacks one of its DCs -- every op excluded (:245-247)
    uint64_t rA, rB, sA, sB, eA, eB;  // per lane: DCs 2p, 2p+1 (p = lane & 3)
    uint64_t U, Sm, Rm;               // MSK (Presence)
};

// agn_log.key_mask of a key (an in-bounds dummy when the log has none).
__device__ __forceinline__ uint64_t key_word(const MaskArgs &mk, uint64_t key,
                                             const uint64_t *__restrict__ key_off) {
    return uniform_u64(ldc(mk.key_mask ? mk.key_mask + key : key_off));
}

// The key's segment (the metadata the row loads depend on).
__device__ __forceinline__ void q2_meta(Q2Key &k, uint64_t i, const uint64_t *__restrict__ keys,
                                        const uint64_t *__restrict__ key_off,
                                        const uint64_t *__restrict__ key_len,
                                        const uint32_t *__restrict__ key_id0) {
    k.i = i;
    k.key = keys ? uniform_u64(ldc(keys + i)) : i;
    const KeyMeta km = key_meta(k.key, key_off, key_len, key_id0);
    k.off = km.off;
    k.n = km.n;
    k.id0 = km.id0;
}

// The rest of a request's prologue: key_type, SCT and its ignore byte, TxId,
// R, the presence words of a sparse batch -- as raw scalar loads (q2_load:
// every address depends only on the request and the key's segment), then the
// values derived from them (q2_apply).  Scalar loads return out of order, so
// the first use of any of them waits for all (lgkmcnt(0)): k_counter_q8e
// issues the whole group under chunk 0's rows and puts a scheduling barrier
// before the first use -- left alone, the scheduler interleaved uses with the
// loads and the warm masked prologue became three dependent scalar round
// trips after the rows (warm masked cfg2 1.23x the dense warm kernel).
// R's and SCT's DCs 2p, 2p+1 (p = lane & 3) -- the pair this lane compares
// -- come as one 16-byte vector load each: as 16 uniform words apiece they
// sat in SGPRs next to the kernel's pointer arguments, and the warm masked
// kernel spilled 17 SGPRs to VGPR lanes (v_writelane / v_readlane, issue
// stalls: SQ_WAIT_INST_ANY 1662 vs 990 quad-cycles per wave, warm masked cfg2
// 1.26x the dense warm kernel).
struct Q2Raw {
    uint64_t kmw, txv, rmw, smw;
    u64x2 rq, sq;        // per lane: R / SCT at DCs 2p, 2p+1
    uint32_t ktw, sibw;  // the dwords holding key_type[key] / sct_ignore[i]
};

template <bool ANY_WARM, bool MSK>
__device__ __forceinline__ Q2Raw q2_load(const Q2Key &k, const DenseArgs &a, const MaskArgs &mk,
                                         bool with_km, const uint64_t *__restrict__ key_off,
                                         const uint8_t *__restrict__ key_type,
                                         const uint64_t *__restrict__ R,
                                         const uint64_t *__restrict__ sct,
                                         const uint8_t *__restrict__ sct_ignore,
                                         const uint64_t *__restrict__ req_txid) {
    constexpr int D = 8;
    const uint64_t i = k.i;
    Q2Raw x;
    const uint8_t *ktp = key_type ? key_type : reinterpret_cast<const uint8_t *>(key_off);
    x.ktw = __builtin_amdgcn_readfirstlane(ldc(reinterpret_cast<const uint32_t *>(ktp) + (k.key >> 2)));
    const uint8_t *sip = sct_ignore ? sct_ignore : reinterpret_cast<const uint8_t *>(R);
    x.sibw = ANY_WARM ? __builtin_amdgcn_readfirstlane(ldc(reinterpret_cast<const uint32_t *>(sip) + (i >> 2)))
                      : 0u;
    x.txv = uniform_u64(ldc((req_txid ? req_txid : R) + i));
    x.kmw = (MSK && with_km) ? key_word(mk, k.key, key_off) : 0ull;
    x.rmw = x.smw = 0ull;
    if constexpr (MSK) {
        // AGN_HINT_R_FULL: every R mask carries all D DCs (not read)
        const bool rfull = (a.hints & AGN_HINT_R_FULL) != 0u;
        x.rmw = uniform_u64(ldc((mk.R_mask && !rfull) ? mk.R_mask + i : R));
        x.smw = uniform_u64(ldc((ANY_WARM && mk.sct_mask) ? mk.sct_mask + i : R));
    }
    const uint64_t *sct_p = (ANY_WARM && sct) ? sct : R;
    const uint64_t pp = 2u * (uint64_t)(lane_id() & 3);
    x.rq = *reinterpret_cast<const u64x2 *>(R + i * D + pp);
    if constexpr (ANY_WARM) x.sq = *reinterpret_cast<const u64x2 *>(sct_p + i * D + pp);
    else x.sq = u64x2{0ull, 0ull};
    return x;
}

// Pins the raw side values behind the scheduling barrier: the IR passes hoist
// a use (kmw & 0xFF) next to its load, where its wait would precede the other
// loads' issue; a use of an asm output cannot move above the asm.
__device__ __forceinline__ void q2_pin(Q2Raw &x) {
    asm volatile("" : "+s"(x.kmw), "+s"(x.txv), "+s"(x.rmw), "+s"(x.smw), "+s"(x.ktw), "+s"(x.sibw));
}

template <bool ANY_WARM, bool MSK>
__device__ __forceinline__ void q2_apply(Q2Key &k, const DenseArgs &a, const MaskArgs &mk,
                                         const Q2Raw &x, uint64_t kmw,
                                         const uint8_t *__restrict__ key_type,
                                         const uint64_t *__restrict__ sct,
                                         const uint8_t *__restrict__ sct_ignore,
                                         const uint64_t *__restrict__ req_txid) {
    constexpr int D = 8;
    const uint32_t kty = (x.ktw >> ((uint32_t)(k.key & 3u) * 8u)) & 0xffu;
    k.corrupt = k.n != 0 && key_type != nullptr && kty != (a.req_type & 0xffu);
    const uint32_t sib = ANY_WARM ? (x.sibw >> ((uint32_t)(k.i & 3u) * 8u)) & 0xffu : 0u;
    k.sct_ign = !ANY_WARM || sct == nullptr || (sct_ignore && sib != 0u);
    k.txr = req_txid ? x.txv : 0ull;
    const uint64_t rmw = (a.hints & AGN_HINT_R_FULL) ? ~0ull : x.rmw;
    const Presence<D> pr = presence<D, MSK>(mk, kmw, rmw, x.smw, k.n);
    k.U = pr.U;
    k.Rm = pr.Rm;
    k.Sm = pr.Sm;
    // a known DC set U is served by the dense scan whether or not R covers it:
    // when R lacks one of U's DCs, every op (all carry U) is excluded
    const bool known = !MSK || pr.uni || pr.U != 0ull;
    k.uni = known;
    k.noR = MSK && known && !pr.uni;
    // this lane's DCs dA = 2p, dB = 2p + 1
    const uint32_t dA = 2u * (uint32_t)(lane_id() & 3), dB = dA + 1u;
    const bool inA = ((pr.U >> dA) & 1ull) != 0ull, inB = ((pr.U >> dB) & 1ull) != 0ull;
    // e = SCT as a dict read (a DC missing from it = 0); s = the compare
    // value, r = R: +inf outside U on the dense scan of a masked key
    k.eA = (k.sct_ign || !((pr.Sm >> dA) & 1ull)) ? 0ull : x.sq.x;
    k.eB = (k.sct_ign || !((pr.Sm >> dB) & 1ull)) ? 0ull : x.sq.y;
    k.sA = (MSK && known && !inA) ? ~0ull : k.eA;
    k.sB = (MSK && known && !inB) ? ~0ull : k.eB;
    k.rA = (MSK && known && !inA) ? ~0ull : x.rq.x;
    k.rB = (MSK && known && !inB) ? ~0ull : x.rq.y;
}

template <bool ANY_WARM, bool MSK>
__device__ __forceinline__ void q2_side(Q2Key &k, const DenseArgs &a, const MaskArgs &mk,
                                        uint64_t kmw, const uint64_t *__restrict__ key_off,
                                        const uint8_t *__restrict__ key_type,
                                        const uint64_t *__restrict__ R,
                                        const uint64_t *__restrict__ sct,
                                        const uint8_t *__restrict__ sct_ignore,
                                        const uint64_t *__restrict__ req_txid) {
    const Q2Raw x = q2_load<ANY_WARM, MSK>(k, a, mk, false, key_off, key_type, R, sct, sct_ignore,
                                           req_txid);
    q2_apply<ANY_WARM, MSK>(k, a, mk, x, kmw, key_type, sct, sct_ignore, req_txid);
}

// A request's share of the packed index: the key's pack_ok byte (scalar
// cache) and pack_base at this lane's DCs 2p, 2p+1 (p = lane & 3), the
// layout of R in Q2Key -- one 16-byte vector load, as q2_load's of R and for
// its reason: as 8 uniform words per key next to the kernel's pointer
// arguments the base rows would push scalar state out to VGPR lanes.  Both
// addresses need only the key id: they share R's round trip.  bq stays in
// registers to the LastOpCt fold (the packed rows take 8 VGPRs per key where
// the quad rows take 16).
struct Q2Pack {
    u64x2 bq;
    uint32_t ok;  // the pack_ok byte
};

__device__ __forceinline__ Q2Pack q2_pack_load(const Q2Key &k, const uint64_t *__restrict__ base,
                                               const uint8_t *__restrict__ ok) {
    Q2Pack p;
    p.ok = ldc_byte(ok, k.key);
    p.bq = *reinterpret_cast<const u64x2 *>(base + k.key * 8u + 2u * (uint64_t)(lane_id() & 3));
    return p;
}

// PACK: the request's share of the packed index loads with the rest (pk).
template <bool ANY_WARM, bool MSK, bool PACK = false>
__device__ __forceinline__ Q2Key q2_prologue(const DenseArgs &a, const MaskArgs &mk, uint64_t i,
                                             const uint64_t *__restrict__ keys,
                                             const uint64_t *__restrict__ key_off,
                                             const uint64_t *__restrict__ key_len,
                                             const uint8_t *__restrict__ key_type,
                                             const uint32_t *__restrict__ key_id0,
                                             const uint64_t *__restrict__ R,
                                             const uint64_t *__restrict__ sct,
                                             const uint8_t *__restrict__ sct_ignore,
                                             const uint64_t *__restrict__ req_txid,
                                             const uint64_t *__restrict__ pack_base = nullptr,
                                             const uint8_t *__restrict__ pack_ok = nullptr,
                                             Q2Pack *pk = nullptr) {
    Q2Key k;
    q2_meta(k, i, keys, key_off, key_len, key_id0);
    if constexpr (PACK) *pk = q2_pack_load(k, pack_base, pack_ok);
    const uint64_t kmw = MSK ? key_word(mk, k.key, key_off) : 0ull;
    q2_side<ANY_WARM, MSK>(k, a, mk, kmw, key_off, key_type, R, sct, sct_ignore, req_txid);
    return k;
}

struct Q2Acc {
    int64_t sum = 0, first_excl = -1, first_err = -1;
    uint32_t cnt = 0;
    uint64_t ctA, ctB;
    uint64_t um = 0;  // MSK, mixed key: the included ops' DC set
};

template <bool ANY_WARM>
__device__ __forceinline__ void q2_fold(const Q2Key &k, const Q8Chunk &c, uint64_t b,
                                        const uint64_t *__restrict__ log_txid, uint64_t n_entries,
                                        Q2Acc &s) {
    const uint64_t *tx = k.txr ? log_txid : nullptr;
    if (ANY_WARM && !k.sct_ign)
        q8_fold<true>(c, tx, k.txr, k.off, b, k.n, n_entries, k.rA, k.rB, k.sA, k.sB, s.ctA, s.ctB,
                      s.sum, s.cnt, s.first_excl, s.first_err, k.noR);
    else
        q8_fold<false>(c, tx, k.txr, k.off, b, k.n, n_entries, k.rA, k.rB, k.sA, k.sB, s.ctA,
                       s.ctB, s.sum, s.cnt, s.first_excl, s.first_err, k.noR);
}

template <bool ANY_WARM>
__device__ __forceinline__ void q2_rest(const Q2Key &k, const uint64_t *__restrict__ oc,
                                        const int64_t *__restrict__ eff,
                                        const uint64_t *__restrict__ log_txid, uint64_t n_entries,
                                        Q2Acc &s) {
    if (k.n <= (uint64_t)AGN_WAVE) return;
    const uint64_t *tx = k.txr ? log_txid : nullptr;
    if (ANY_WARM && !k.sct_ign)
        scan_key_q8<true, true, false, true>(oc, eff, tx, k.txr, k.off, k.n, n_entries, k.rA, k.rB,
                                             k.sA, k.sB, s.ctA, s.ctB, s.sum, s.cnt, s.first_excl,
                                             s.first_err, k.noR);
    else
        scan_key_q8<false, true, false, true>(oc, eff, tx, k.txr, k.off, k.n, n_entries, k.rA,
                                              k.rB, k.sA, k.sB, s.ctA, s.ctB, s.sum, s.cnt,
                                              s.first_excl, s.first_err, k.noR);
}

// A mixed key of a sparse batch (MSK, !uni): the per-entry-mask scan, lane =
// op, with R / SCT / the LastOpCt seed gathered back from the quad lanes
// (lane p < 4 holds DCs 2p, 2p+1).
template <bool ANY_WARM>
__device__ __forceinline__ void q2_msk(const Q2Key &k, const uint64_t *__restrict__ oc,
                                       const uint64_t *__restrict__ oc_mask,
                                       const int64_t *__restrict__ eff,
                                       const uint64_t *__restrict__ log_txid, uint64_t n_entries,
                                       Q2Acc &s) {
    const uint64_t *tx = k.txr ? log_txid : nullptr;
    if (ANY_WARM && !k.sct_ign)
        scan_key_q8_msk<true>(oc, oc_mask, eff, tx, k.txr, k.off, k.n, n_entries, k.rA, k.rB,
                              k.sA, k.sB, k.Rm, s.ctA, s.ctB, s.um, s.sum, s.cnt, s.first_excl,
                              s.first_err);
    else
        scan_key_q8_msk<false>(oc, oc_mask, eff, tx, k.txr, k.off, k.n, n_entries, k.rA, k.rB,
                               k.sA, k.sB, k.Rm, s.ctA, s.ctB, s.um, s.sum, s.cnt, s.first_excl,
                               s.first_err);
}

template <bool MSK>
__device__ __forceinline__ void q2_epilogue(const Q2Key &k, Q2Acc &s, uint32_t hints,
                                            const uint32_t *__restrict__ op_id,
                                            const int64_t *__restrict__ base_value,
                                            int64_t *__restrict__ o_value,
                                            int64_t *__restrict__ o_hole,
                                            uint64_t *__restrict__ o_lastct,
                                            uint32_t *__restrict__ o_count,
                                            uint32_t *__restrict__ o_flags,
                                            uint32_t *__restrict__ o_err,
                                            uint64_t *__restrict__ o_mask) {
    constexpr int D = 8;
    const int lane = lane_id();
    const uint64_t i = k.i;
    if (k.corrupt) {
        if (lane == 0) {  // erlang:error(corrupted_ops_cache) (:190-191)
            o_flags[i] = AGN_F_ERR_CORRUPTED;
            o_err[i] = 0xffffffffu;
        }
        return;
    }
    int64_t hid;
    const uint64_t pos = s.first_excl >= 0 ? (uint64_t)s.first_excl : k.n - 1;
    if (k.id0 != AGN_ID0_NONE)
        hid = k.n ? (int64_t)((uint64_t)k.id0 + pos) : 0;
    else
        // readfirstlane returns int: an id with bit 31 set must not sign-extend into the hole
        hid = k.n ? (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane(
                        (int)ldc(op_id + uniform_u64(k.off + pos))) : 0;
    const int64_t base = base_value ? (int64_t)uniform_u64((uint64_t)ldc(base_value + i)) : 0;
    const int64_t total = wave_sum_dpp(s.sum);
    const bool ct_ign = k.sct_ign && s.cnt == 0u;
    uint64_t mo = 0;
    if constexpr (MSK) {
        if (k.uni) {  // outside U: SCT's value (an op's row there is not in its dict)
            const int p = lane & 3;
            s.ctA = ((k.U >> (2 * p)) & 1ull) ? s.ctA : k.eA;
            s.ctB = ((k.U >> (2 * p + 1)) & 1ull) ? s.ctB : k.eB;
        }
        const uint64_t un = k.uni ? (s.cnt ? k.U : 0ull) : wave_or_bits<D>(s.um);
        mo = ct_ign ? 0ull : ((k.sct_ign ? 0ull : k.Sm) | un);
    }
#pragma unroll
    for (int x = 4; x < AGN_WAVE; x <<= 1) {
        s.ctA = umax64(s.ctA, shfl_xor_u64(s.ctA, x));
        s.ctB = umax64(s.ctB, shfl_xor_u64(s.ctB, x));
    }
    if (lane < 4) {
        u64x2 v;
        v.x = ct_ign ? 0ull : s.ctA;
        v.y = ct_ign ? 0ull : s.ctB;
        reinterpret_cast<u64x2 *>(o_lastct + i * D)[lane] = v;
    }
    if (lane == 0) {
        const int64_t hole = s.first_excl >= 0 ? hid - 1 : hid;
        uint32_t fl = 0;
        if (s.cnt) fl |= AGN_F_NEWSS;
        if (ct_ign) fl |= AGN_F_CT_IGNORE;
        if (s.first_err >= 0) fl |= AGN_F_ERR_UNEXPECTED;
        o_value[i] = (int64_t)((uint64_t)base + (uint64_t)total);
        o_hole[i] = hole;
        o_count[i] = s.cnt;
        o_err[i] = s.first_err >= 0 ? (uint32_t)(k.off + (uint64_t)s.first_err) : 0xffffffffu;
        // AGN_HINT_CT_FLAG: a LastOpCt over every column is a flag bit, not a
        // mask word (one store stream less per request)
        const bool full = MSK && (hints & AGN_HINT_CT_FLAG) && mo == 0xFFull;
        if (full) fl |= AGN_F_CT_FULL;
        o_flags[i] = fl;
        if (MSK && o_mask && !full) o_mask[i] = mo;
    }
}

// q2_epilogue in steps, for k_counter_quad2's forms that run the two keys'
// steps side by side (Q2_EFF, Q2_STORE below): the verdict of chunk 0 (q2_fold
// without the effects), the LastOpCt fold, the request's result as values,
// and the stores -- per key as q2_epilogue's, or one set for the pair.
template <bool ANY_WARM>
__device__ __forceinline__ uint64_t q2_verdict(const Q2Key &k, const Q8Rows &c,
                                               const uint64_t *__restrict__ log_txid,
                                               uint64_t n_entries, Q2Acc &s) {
    const uint64_t *tx = k.txr ? log_txid : nullptr;
    if (ANY_WARM && !k.sct_ign)
        return q8_verdict<true>(c, tx, k.txr, k.off, 0, k.n, n_entries, k.rA, k.rB, k.sA, k.sB,
                                s.ctA, s.ctB, s.cnt, s.first_excl, k.noR);
    return q8_verdict<false>(c, tx, k.txr, k.off, 0, k.n, n_entries, k.rA, k.rB, k.sA, k.sB, s.ctA,
                             s.ctB, s.cnt, s.first_excl, k.noR);
}

// LastOpCt: the 16 lanes of each part fold by xor-shuffles (no effect needed)
template <bool MSK>
__device__ __forceinline__ void q2_ctfold(const Q2Key &k, Q2Acc &s) {
    if constexpr (MSK) {
        if (k.uni) {  // outside U: SCT's value (an op's row there is not in its dict)
            const int p = lane_id() & 3;
            s.ctA = ((k.U >> (2 * p)) & 1ull) ? s.ctA : k.eA;
            s.ctB = ((k.U >> (2 * p + 1)) & 1ull) ? s.ctB : k.eB;
        }
    }
#pragma unroll
    for (int x = 4; x < AGN_WAVE; x <<= 1) {
        s.ctA = umax64(s.ctA, shfl_xor_u64(s.ctA, x));
        s.ctB = umax64(s.ctB, shfl_xor_u64(s.ctB, x));
    }
}

struct Q2Out {
    int64_t value, hole;
    uint32_t cnt, fl, err;
    uint64_t mo;
    bool ct_ign;
    bool wm;  // MSK: the request writes its lastct_mask word
};

// A served (not corrupt) request's result, after the scan and q2_ctfold.
template <bool MSK>
__device__ __forceinline__ Q2Out q2_result(const Q2Key &k, const Q2Acc &s, uint32_t hints,
                                           const uint32_t *__restrict__ op_id,
                                           const int64_t *__restrict__ base_value, bool has_mask) {
    constexpr int D = 8;
    int64_t hid;
    const uint64_t pos = s.first_excl >= 0 ? (uint64_t)s.first_excl : k.n - 1;
    if (k.id0 != AGN_ID0_NONE)
        hid = k.n ? (int64_t)((uint64_t)k.id0 + pos) : 0;
    else
        hid = k.n ? (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane(
                        (int)ldc(op_id + uniform_u64(k.off + pos))) : 0;
    const int64_t base = base_value ? (int64_t)uniform_u64((uint64_t)ldc(base_value + k.i)) : 0;
    const int64_t total = wave_sum_dpp(s.sum);
    Q2Out r;
    r.ct_ign = k.sct_ign && s.cnt == 0u;
    r.mo = 0;
    if constexpr (MSK) {
        const uint64_t un = k.uni ? (s.cnt ? k.U : 0ull) : wave_or_bits<D>(s.um);
        r.mo = r.ct_ign ? 0ull : ((k.sct_ign ? 0ull : k.Sm) | un);
    }
    r.value = (int64_t)((uint64_t)base + (uint64_t)total);
    r.hole = s.first_excl >= 0 ? hid - 1 : hid;
    r.cnt = s.cnt;
    r.fl = 0;
    if (s.cnt) r.fl |= AGN_F_NEWSS;
    if (r.ct_ign) r.fl |= AGN_F_CT_IGNORE;
    if (s.first_err >= 0) r.fl |= AGN_F_ERR_UNEXPECTED;
    r.err = s.first_err >= 0 ? (uint32_t)(k.off + (uint64_t)s.first_err) : 0xffffffffu;
    const bool full = MSK && (hints & AGN_HINT_CT_FLAG) && r.mo == 0xFFull;  // q2_epilogue
    if (full) r.fl |= AGN_F_CT_FULL;
    r.wm = MSK && has_mask && !full;
    return r;
}

// One request's stores (q2_epilogue's).
__device__ __forceinline__ void q2_store(const Q2Key &k, const Q2Acc &s, const Q2Out &r,
                                         int64_t *__restrict__ o_value,
                                         int64_t *__restrict__ o_hole,
                                         uint64_t *__restrict__ o_lastct,
                                         uint32_t *__restrict__ o_count,
                                         uint32_t *__restrict__ o_flags,
                                         uint32_t *__restrict__ o_err,
                                         uint64_t *__restrict__ o_mask) {
    const int lane = lane_id();
    const uint64_t i = k.i;
    if (k.corrupt) {
        if (lane == 0) {  // erlang:error(corrupted_ops_cache) (:190-191)
            o_flags[i] = AGN_F_ERR_CORRUPTED;
            o_err[i] = 0xffffffffu;
        }
        return;
    }
    if (lane < 4) {
        u64x2 v;
        v.x = r.ct_ign ? 0ull : s.ctA;
        v.y = r.ct_ign ? 0ull : s.ctB;
        reinterpret_cast<u64x2 *>(o_lastct + i * 8u)[lane] = v;
    }
    if (lane == 0) {
        o_value[i] = r.value;
        o_hole[i] = r.hole;
        o_count[i] = r.cnt;
        o_err[i] = r.err;
        o_flags[i] = r.fl;
        if (r.wm) o_mask[i] = r.mo;
    }
}

typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// Requests i0 (even) and i0 + 1, both served: their slots are adjacent in
// every result array, so each array takes one store -- the two LastOpCt rows
// are one 128-byte line, written by lanes 0-3 (key 0) and 4-7 (key 1).  Six
// store instructions per wave where two q2_store issue twelve; the arrays'
// alignment is the launcher's condition (launch_quad2).
__device__ __forceinline__ void q2_store2(uint64_t i0, const Q2Acc &s0, const Q2Acc &s1,
                                          const Q2Out &r0, const Q2Out &r1,
                                          int64_t *__restrict__ o_value,
                                          int64_t *__restrict__ o_hole,
                                          uint64_t *__restrict__ o_lastct,
                                          uint32_t *__restrict__ o_count,
                                          uint32_t *__restrict__ o_flags,
                                          uint32_t *__restrict__ o_err,
                                          uint64_t *__restrict__ o_mask) {
    const int lane = lane_id();
    if (lane < 8) {
        const bool hi = lane >= 4;
        const bool ign = hi ? r1.ct_ign : r0.ct_ign;
        u64x2 v;
        v.x = ign ? 0ull : (hi ? s1.ctA : s0.ctA);
        v.y = ign ? 0ull : (hi ? s1.ctB : s0.ctB);
        reinterpret_cast<u64x2 *>(o_lastct + i0 * 8u)[lane] = v;
    }
    if (lane == 0) {
        *reinterpret_cast<i64x2 *>(o_value + i0) = i64x2{r0.value, r1.value};
        *reinterpret_cast<i64x2 *>(o_hole + i0) = i64x2{r0.hole, r1.hole};
        *reinterpret_cast<u32x2 *>(o_count + i0) = u32x2{r0.cnt, r1.cnt};
        *reinterpret_cast<u32x2 *>(o_err + i0) = u32x2{r0.err, r1.err};
        *reinterpret_cast<u32x2 *>(o_flags + i0) = u32x2{r0.fl, r1.fl};
        if (r0.wm && r1.wm) {
            *reinterpret_cast<u64x2 *>(o_mask + i0) = u64x2{r0.mo, r1.mo};
        } else {
            if (r0.wm) o_mask[i0] = r0.mo;
            if (r1.wm) o_mask[i0 + 1u] = r1.mo;
        }
    }
}

// k_counter_q8e2's parameters as one block (kparams: each stage reads the
// fields it uses; as 26 separate arguments it spilled 62 SGPRs, 43-47 so).
// k_counter_quad2 keeps its by-value arguments: read this way its dense warm
// form ran 9.47 against 8.32 ms (the parameter loads joined the prologue's
// dependent chain; profiles/r05/ab_masked_warm_quad2_kparams.log).
struct Q2Params {
    DenseArgs a;
    MaskArgs mk;
    const uint64_t *keys, *key_off, *key_len;
    const uint8_t *key_type;
    const uint32_t *key_id0;
    const uint64_t *oc;
    const uint32_t *op_id;
    const int64_t *eff;
    const uint64_t *log_txid, *R, *sct;
    const uint8_t *sct_ignore;
    const uint64_t *req_txid;
    const int64_t *base_value;
    int64_t *o_value, *o_hole;
    uint64_t *o_lastct;
    uint32_t *o_count, *o_flags, *o_err, *list, *list_n;
};

template <class T>
__device__ __forceinline__ DenseArgs dense_of(const T &x) {
    return DenseArgs{x.n_req, x.n_entries, x.req_type, x.xcd, x.pair, x.qnt, x.hints, x.ql_cap};
}
template <class T>
__device__ __forceinline__ MaskArgs mask_of(const T &x) {
    return MaskArgs{x.key_mask, x.oc_mask, x.R_mask, x.sct_mask, x.o_mask};
}

// Lane g of `old` becomes the wave-uniform v.
__device__ __forceinline__ uint32_t put_lane(uint32_t v, int g, uint32_t old) {
    return lane_id() == g ? v : old;
}

// k_counter_quad2's parameters past Q2Params' (its PACK form): the packed index
// of the log (agn_log_index_pack), read from the kernarg segment where used.
struct Q2PackParams {
    DenseArgs a;
    MaskArgs mk;
    const void *args[20];  // keys .. o_err
    const uint32_t *rows;
    const uint64_t *base;
    const uint8_t *ok;
};
static_assert(offsetof(Q2PackParams, rows) == offsetof(Q2Params, list),
              "Q2PackParams follows k_counter_quad2's parameter list");

// p8_verdict's thresholds: R - base per column, saturated, moved from the
// lanes that hold DCs 2p', 2p'+1 (p' = lane & 3) to the packed layout -- lane
// l compares DCs 4p .. 4p+3 (p = l & 1), held by lanes 2p and 2p+1 of its
// quad.  noR: R < base in some column.
__device__ __forceinline__ u32x4 q2_pack_thr(const Q2Key &k, const Q2Pack &p, bool &noR) {
    noR = ballot(k.rA < p.bq.x || k.rB < p.bq.y) != 0ull;
    const uint64_t dA = k.rA - p.bq.x, dB = k.rB - p.bq.y;
    const uint32_t tA = (dA >> 32) ? 0xFFFFFFFFu : (uint32_t)dA;
    const uint32_t tB = (dB >> 32) ? 0xFFFFFFFFu : (uint32_t)dB;
    u32x4 t;
    t.x = __builtin_amdgcn_update_dpp(0u, tA, 0x88, 0xF, 0xF, false);  // quad_perm 0,2,0,2
    t.y = __builtin_amdgcn_update_dpp(0u, tB, 0x88, 0xF, 0xF, false);
    t.z = __builtin_amdgcn_update_dpp(0u, tA, 0xDD, 0xF, 0xF, false);  // quad_perm 1,3,1,3
    t.w = __builtin_amdgcn_update_dpp(0u, tB, 0xDD, 0xF, 0xF, false);
    return t;
}

// LastOpCt of a cold read over packed rows (q2_ctfold's place): the lanes'
// delta maxima fold by xor-shuffles over strides 2 .. 32 (even lanes then hold
// DCs 0-3, odd lanes DCs 4-7), go back to the lanes of DCs 2p', 2p'+1, and
// ct = base + max delta when an op was included, else SCT's value: 0, cold.
__device__ __forceinline__ void q2_pack_ct(const Q2Pack &p, u32x4 mx, Q2Acc &s) {
#pragma unroll
    for (int x = 2; x < AGN_WAVE; x <<= 1) {
        const uint32_t a = (uint32_t)__shfl_xor((int)mx.x, x, AGN_WAVE);
        const uint32_t b = (uint32_t)__shfl_xor((int)mx.y, x, AGN_WAVE);
        const uint32_t c = (uint32_t)__shfl_xor((int)mx.z, x, AGN_WAVE);
        const uint32_t d = (uint32_t)__shfl_xor((int)mx.w, x, AGN_WAVE);
        mx.x = a > mx.x ? a : mx.x;
        mx.y = b > mx.y ? b : mx.y;
        mx.z = c > mx.z ? c : mx.z;
        mx.w = d > mx.w ? d : mx.w;
    }
    // quad_perm 0,0,1,1: lanes p' = 0, 1 read the even lane's maxima, 2, 3 the odd lane's
    const uint32_t g0 = __builtin_amdgcn_update_dpp(0u, mx.x, 0x50, 0xF, 0xF, false);
    const uint32_t g1 = __builtin_amdgcn_update_dpp(0u, mx.y, 0x50, 0xF, 0xF, false);
    const uint32_t g2 = __builtin_amdgcn_update_dpp(0u, mx.z, 0x50, 0xF, 0xF, false);
    const uint32_t g3 = __builtin_amdgcn_update_dpp(0u, mx.w, 0x50, 0xF, 0xF, false);
    const bool hi = (lane_id() & 1) != 0;
    s.ctA = s.cnt ? p.bq.x + (uint64_t)(hi ? g2 : g0) : 0ull;
    s.ctB = s.cnt ? p.bq.y + (uint64_t)(hi ? g3 : g1) : 0ull;
}

// One request of a cold dense batch that the packed rows do not serve, read
// from oc: its own prologue (scalar-cache hits where the caller has loaded
// the metadata before), the quad-row scan and q2_epilogue, with every pointer
// from the kernarg segment (Q2Params: k_counter_quad2's parameter list), so
// the caller's straight path holds none of this in registers.  No TxIds are
// passed: a cold read includes an op whatever its TxId (nip is all ones).
// Same functions, same results as k_counter_quad2 without an index.
__device__ __forceinline__ void q2_serve_oc(const DenseArgs &a, uint64_t i) {
    const MaskArgs mk{};
    const auto &p = kparams<Q2Params>();
    const Q2Key k = q2_prologue<false, false>(a, mk, i, p.keys, p.key_off, p.key_len, p.key_type,
                                              p.key_id0, p.R, p.sct, p.sct_ignore, p.req_txid);
    Q2Acc s;
    s.ctA = k.eA;
    s.ctB = k.eB;
    if (a.n_entries != 0 && !k.corrupt)
        scan_key_q8<false, true, false, false>(p.oc, p.eff, nullptr, 0ull, k.off, k.n, a.n_entries,
                                               k.rA, k.rB, k.sA, k.sB, s.ctA, s.ctB, s.sum, s.cnt,
                                               s.first_excl, s.first_err, k.noR);
    const auto &pe = kparams<Q2Params>();
    q2_epilogue<false>(k, s, a.hints, pe.op_id, pe.base_value, pe.o_value, pe.o_hole, pe.o_lastct,
                       pe.o_count, pe.o_flags, pe.o_err, nullptr);
}

// The dense warm form runs at 6 waves per SIMD: 80 VGPRs and 2 scratch
// spills instead of 84 VGPRs (5 waves) and 24 spilled SGPRs, 8.13 against
// 8.33 ms on warm cfg2 (profiles/r05/ab_quad2_w6.log).  The masked forms spill
// far more under that budget and keep the default.
//
// Q2_EFF (AGN_Q2_EFF): chunk 0's effects are fetched after the verdict, by the
// included ops' lanes only.  The wave issues both keys' rows, then per key
// computes the verdict (q2_verdict) and issues the effect load (q8_load_eff;
// the other lanes read the request's R row, which q2_load has fetched), runs
// both keys' LastOpCt folds under those loads, folds the effects, and only
// then stores: loads and stores share one VM counter, and a store between an
// effect load and its use would make that wait vmcnt(0).
// Q2_STORE (AGN_Q2_STORE): one set of stores for a pair of served requests
// (q2_store2); a pair with a corrupt request and an unpaired last request
// store per key.
// Both forms serve the pairs whose two keys fit one chunk; a pair with a
// longer key (or, masked, a mixed one) runs the kernel as it was before
// either, and so does every pair when both are 0.
//
// PACK (cold dense, with both forms above): the log carries a packed index
// (agn_log_index_pack) and the straight path scans its 32-byte rows -- a pair
// whose two keys fit one chunk and are both packed (pack_ok).  Every other
// pair reads oc in the code below, as the kernel without an index does.
template <bool ANY_WARM, bool MSK, bool Q2_EFF, bool Q2_STORE, bool PACK = false>
__global__ __launch_bounds__(64, (ANY_WARM && !MSK) ? 6 : 1) void k_counter_quad2(
    DenseArgs a, MaskArgs mk, const uint64_t *__restrict__ keys,
    const uint64_t *__restrict__ key_off, const uint64_t *__restrict__ key_len,
    const uint8_t *__restrict__ key_type, const uint32_t *__restrict__ key_id0,
    const uint64_t *__restrict__ oc, const uint32_t *__restrict__ op_id,
    const int64_t *__restrict__ eff, const uint64_t *__restrict__ log_txid,
    const uint64_t *__restrict__ R, const uint64_t *__restrict__ sct,
    const uint8_t *__restrict__ sct_ignore, const uint64_t *__restrict__ req_txid,
    const int64_t *__restrict__ base_value, int64_t *__restrict__ o_value,
    int64_t *__restrict__ o_hole, uint64_t *__restrict__ o_lastct,
    uint32_t *__restrict__ o_count, uint32_t *__restrict__ o_flags,
    uint32_t *__restrict__ o_err, const uint32_t *__restrict__ pack_rows,
    const uint64_t *__restrict__ pack_base, const uint8_t *__restrict__ pack_ok) {
    static_assert(!PACK || (!ANY_WARM && !MSK && Q2_EFF && Q2_STORE),
                  "packed rows: the cold dense form only");
    const uint32_t blk = block_order(a.xcd, blockIdx.x, gridDim.x);
    const uint64_t i0 = uniform_u64((uint64_t)blk * 2u);
    if (i0 >= a.n_req) return;
    const bool two = i0 + 1u < a.n_req;
    const uint64_t i1 = two ? i0 + 1u : i0;
    Q2Pack pk0{}, pk1{};
    const Q2Key k0 = q2_prologue<ANY_WARM, MSK, PACK>(a, mk, i0, keys, key_off, key_len, key_type,
                                                      key_id0, R, sct, sct_ignore, req_txid,
                                                      pack_base, pack_ok, &pk0);
    const Q2Key k1 = q2_prologue<ANY_WARM, MSK, PACK>(a, mk, i1, keys, key_off, key_len, key_type,
                                                      key_id0, R, sct, sct_ignore, req_txid,
                                                      pack_base, pack_ok, &pk1);
    Q2Acc s0, s1;
    s0.ctA = k0.eA;
    s0.ctB = k0.eB;
    s1.ctA = k1.eA;
    s1.ctB = k1.eB;
    if constexpr (Q2_EFF || Q2_STORE) {
        // The straight path: both keys within one chunk and on the dense
        // scan, so no loop lies between the loads and the stores (behind a
        // loop's exit the effects were waited for before the folds).  Any
        // other pair runs the code below, as before.
        const bool one = k0.n <= (uint64_t)AGN_WAVE && k1.n <= (uint64_t)AGN_WAVE;
        if (a.n_entries != 0 && one && (!MSK || (k0.uni && k1.uni)) &&
            (!PACK || (pk0.ok & pk1.ok) != 0u)) {
            const bool d0 = !k0.corrupt, d1 = !k1.corrupt;
            uint64_t in0 = 0, in1 = 0;  // chunk 0's included ops
            int64_t ev0 = 0, ev1 = 0;   // and their effects (lane = op)
            u32x4 m0 = {0u, 0u, 0u, 0u}, m1 = {0u, 0u, 0u, 0u};  // PACK: maxima of included deltas
            if constexpr (PACK) {
                const uint32_t *const rows = kparams<Q2PackParams>().rows;
                const P8Rows c0 = p8_load_rows<true>(rows, k0.off, 0, a.n_entries);
                const P8Rows c1 = p8_load_rows<true>(rows, k1.off, 0, a.n_entries);
                // eff and R (the effect loads' dummy rows) are read here, under the
                // rows, as the result pointers below and for their reason
                const int64_t *const l_eff = (const int64_t *)kparams<Q2Params>().eff;
                const uint64_t *const l_R = (const uint64_t *)kparams<Q2Params>().R;
                __builtin_amdgcn_sched_barrier(0);
                bool nr0, nr1;
                const u32x4 th0 = q2_pack_thr(k0, pk0, nr0), th1 = q2_pack_thr(k1, pk1, nr1);
                // unconditional verdicts, dropped for a corrupt key (see below)
                Q2Acc t0 = s0, t1 = s1;
                in0 = p8_verdict(c0, 0, k0.n, th0, nr0, m0, t0.cnt, t0.first_excl);
                in0 = d0 ? in0 : 0ull;
                if (d0) s0 = t0;
                ev0 = q8_load_eff(l_eff, k0.off, 0, in0, reinterpret_cast<const int64_t *>(l_R + k0.i * 8u));
                in1 = p8_verdict(c1, 0, k1.n, th1, nr1, m1, t1.cnt, t1.first_excl);
                in1 = d1 ? in1 : 0ull;
                if (d1) s1 = t1;
                ev1 = q8_load_eff(l_eff, k1.off, 0, in1, reinterpret_cast<const int64_t *>(l_R + k1.i * 8u));
                __builtin_amdgcn_sched_barrier(0);  // both effect loads are in flight from here
            } else if constexpr (Q2_EFF) {
                const Q8Rows c0 = q8_load_rows<true>(oc, k0.off, 0, a.n_entries);
                const Q8Rows c1 = q8_load_rows<true>(oc, k1.off, 0, a.n_entries);
                __builtin_amdgcn_sched_barrier(0);
                // the verdicts run unconditionally and are dropped for a corrupt
                // key: under a branch on d0 the compiler sinks k0's row loads
                // into it, behind k1's
                Q2Acc t0 = s0, t1 = s1;
                in0 = q2_verdict<ANY_WARM>(k0, c0, log_txid, a.n_entries, t0);
                in0 = d0 ? in0 : 0ull;
                if (d0) s0 = t0;
                ev0 = q8_load_eff(eff, k0.off, 0, in0, reinterpret_cast<const int64_t *>(R + k0.i * 8u));
                in1 = q2_verdict<ANY_WARM>(k1, c1, log_txid, a.n_entries, t1);
                in1 = d1 ? in1 : 0ull;
                if (d1) s1 = t1;
                ev1 = q8_load_eff(eff, k1.off, 0, in1, reinterpret_cast<const int64_t *>(R + k1.i * 8u));
                __builtin_amdgcn_sched_barrier(0);  // both effect loads are in flight from here
            } else {
                const Q8Chunk c0 = q8_load<true, false>(oc, eff, k0.off, 0, a.n_entries);
                const Q8Chunk c1 = q8_load<true, false>(oc, eff, k1.off, 0, a.n_entries);
                __builtin_amdgcn_sched_barrier(0);
                if (d0) q2_fold<ANY_WARM>(k0, c0, 0, log_txid, a.n_entries, s0);
                if (d1) q2_fold<ANY_WARM>(k1, c1, 0, log_txid, a.n_entries, s1);
            }
            // The pointers the results need are read from the kernarg segment
            // here, under the effect loads, instead of as arguments: held in
            // SGPRs from the kernel's entry they crowd the scan's scalar state
            // out to VGPR lanes.  Q2Params lists this kernel's parameters in
            // order.
            const auto &pr = kparams<Q2Params>();
            const uint32_t *const l_op_id = pr.op_id;
            const int64_t *const l_base = pr.base_value;
            int64_t *const l_value = pr.o_value, *const l_hole = pr.o_hole;
            uint64_t *const l_lastct = pr.o_lastct;
            uint32_t *const l_count = pr.o_count, *const l_flags = pr.o_flags, *const l_err = pr.o_err;
            if constexpr (PACK) {
                q2_pack_ct(pk0, m0, s0);
                q2_pack_ct(pk1, m1, s1);
            } else {
                q2_ctfold<MSK>(k0, s0);
                q2_ctfold<MSK>(k1, s1);
            }
            if constexpr (Q2_EFF) {
                __builtin_amdgcn_sched_barrier(0);  // the wait for the effects: after the folds
                q8_fold_eff(in0, ev0, 0, s0.sum, s0.first_err);
                q8_fold_eff(in1, ev1, 0, s1.sum, s1.first_err);
                __builtin_amdgcn_sched_barrier(0);  // and no store before it
            }
            Q2Out r0{}, r1{};
            if (d0) r0 = q2_result<MSK>(k0, s0, a.hints, l_op_id, l_base, mk.o_mask != nullptr);
            if (two && d1) r1 = q2_result<MSK>(k1, s1, a.hints, l_op_id, l_base, mk.o_mask != nullptr);
            if (Q2_STORE && two && d0 && d1) {
                q2_store2(i0, s0, s1, r0, r1, l_value, l_hole, l_lastct, l_count, l_flags, l_err, mk.o_mask);
            } else {
                q2_store(k0, s0, r0, l_value, l_hole, l_lastct, l_count, l_flags, l_err, mk.o_mask);
                if (two) q2_store(k1, s1, r1, l_value, l_hole, l_lastct, l_count, l_flags, l_err, mk.o_mask);
            }
            return;
        }
    }
    if constexpr (PACK) {
        // A pair the packed rows do not serve (a key longer than a chunk or not
        // packed, an empty log) reads oc one request after the other
        // (q2_serve_oc): kept side by side as below, the two requests' scan
        // state costs the straight path a wave per SIMD.
#pragma nounroll
        for (uint32_t h = 0; h < (two ? 2u : 1u); ++h) q2_serve_oc(a, i0 + h);
        return;
    }
    if (a.n_entries != 0) {
        const Q8Chunk c0 = q8_load<true, false>(oc, eff, k0.off, 0, a.n_entries);
        const Q8Chunk c1 = q8_load<true, false>(oc, eff, k1.off, 0, a.n_entries);
        __builtin_amdgcn_sched_barrier(0);
        const bool d0 = !k0.corrupt && (!MSK || k0.uni), d1 = !k1.corrupt && (!MSK || k1.uni);
        if (d0) q2_fold<ANY_WARM>(k0, c0, 0, log_txid, a.n_entries, s0);
        if (d1) q2_fold<ANY_WARM>(k1, c1, 0, log_txid, a.n_entries, s1);
        if (d0) q2_rest<ANY_WARM>(k0, oc, eff, log_txid, a.n_entries, s0);
        if (d1) q2_rest<ANY_WARM>(k1, oc, eff, log_txid, a.n_entries, s1);
        if constexpr (MSK) {
            if (!k0.corrupt && !k0.uni)
                q2_msk<ANY_WARM>(k0, oc, mk.oc_mask, eff, log_txid, a.n_entries, s0);
            if (!k1.corrupt && !k1.uni)
                q2_msk<ANY_WARM>(k1, oc, mk.oc_mask, eff, log_txid, a.n_entries, s1);
        }
    }
    if constexpr (Q2_EFF || Q2_STORE) {  // no result pointer held as an argument (see above)
        const auto &pe = kparams<Q2Params>();
        q2_epilogue<MSK>(k0, s0, a.hints, pe.op_id, pe.base_value, pe.o_value, pe.o_hole, pe.o_lastct,
                         pe.o_count, pe.o_flags, pe.o_err, mk.o_mask);
        if (two)
            q2_epilogue<MSK>(k1, s1, a.hints, pe.op_id, pe.base_value, pe.o_value, pe.o_hole,
                             pe.o_lastct, pe.o_count, pe.o_flags, pe.o_err, mk.o_mask);
        return;
    }
    q2_epilogue<MSK>(k0, s0, a.hints, op_id, base_value, o_value, o_hole, o_lastct, o_count, o_flags, o_err,
                     mk.o_mask);
    if (two)
        q2_epilogue<MSK>(k1, s1, a.hints, op_id, base_value, o_value, o_hole, o_lastct, o_count, o_flags,
                         o_err, mk.o_mask);
}

// Four requests per wave over the packed index: the whole-partition cold read
// (identity key map, req.keys == NULL), where requests 4b .. 4b+3 are keys
// 4b .. 4b+3 and everything per key or per request is contiguous -- one scalar
// load per metadata array, one 8-byte-per-lane load each for the four R rows
// and the four pack_base rows, one store per result array.  The wave holds
// eight 16-byte row loads in flight (8 KiB) where k_counter_quad2's PACK form
// holds four, and nothing else: no warm, masked or long-key form, every
// pointer read from the kernarg segment where it is used (Q2PackParams is
// k_counter_quad2's parameter list).
//
// The straight path serves a group whose four requests exist, are packed
// (pack_ok), fit one chunk and are not corrupt, over a non-empty log.  Per
// (key, DC) values sit in the slot layout (counter_scan.hpp, p4_slot), so
// the thresholds reach p8_verdict's layout by four shuffles per key, the four
// LastOpCt rows fold as one transposed reduction (p4_maxfold: 16 shuffles;
// four q2_pack_ct take 80 and sixteen DPP moves) and leave as one 256-byte
// store.  Order: metadata -> the eight row loads -> per key verdict and
// deferred effect load -> the fold, under the effects -> the effects' fold ->
// stores (loads and stores share the VM counter: no store before the last
// use of a load).  Every other group -- and the last one of a batch that is
// no multiple of four, which reads nothing past request n_req - 1 -- runs its
// requests one after the other through oc (q2_serve_oc).  Same results as
// k_counter_quad2.
__global__ __launch_bounds__(64) void k_counter_pack4(Q2PackParams) {
    const DenseArgs a = dense_of(kparams<Q2Params>().a);
    const uint32_t blk = block_order(a.xcd, blockIdx.x, gridDim.x);
    const uint64_t i0 = uniform_u64((uint64_t)blk * 4u);
    if (i0 >= a.n_req) return;
    const int lane = lane_id();
    if (i0 + 3u < a.n_req) {
        // One scalar round trip, every address a function of the block alone;
        // absent arrays read an in-bounds dummy (key_meta's convention).  With
        // key_len the segment ends need no key_off[4b + 4] (the array may end
        // at n_keys entries), without it the fifth offset exists: 4b + 4 <= n_keys.
        const auto &pm = kparams<Q2Params>();
        const uint64_t *const key_off = pm.key_off, *const key_len = pm.key_len;
        const uint32_t *const key_id0 = pm.key_id0;
        const uint8_t *const key_type = pm.key_type;
        const uint64_t *const R = pm.R;
        // (one kernarg read for both views: Q2PackParams extends Q2Params' list)
        const auto &pq = *(const __attribute__((address_space(4))) Q2PackParams *)&pm;
        const uint64_t *const pbase = pq.base;
        const uint8_t *const pok = pq.ok;
        const int64_t *const bvp = pm.base_value;
        const u64x4 offv = ldc_u64x4(key_off + i0);
        const u64x4 lenv = ldc_u64x4(key_len ? key_len + i0 : key_off + i0);
        const u32x4 idv = ldc_u32x4(key_id0 ? key_id0 + i0
                                            : reinterpret_cast<const uint32_t *>(key_off + i0));
        const uint8_t *const ktp = key_type ? key_type : reinterpret_cast<const uint8_t *>(key_off);
        uint64_t off[5], ln[4];
        uint32_t id0[4];
        off[4] = uniform_u64(ldc(key_len ? key_off + i0 : key_off + i0 + 4u));
        uint32_t ktw = __builtin_amdgcn_readfirstlane(ldc(reinterpret_cast<const uint32_t *>(ktp) + (i0 >> 2)));
        uint32_t okw = __builtin_amdgcn_readfirstlane(ldc(reinterpret_cast<const uint32_t *>(pok) + (i0 >> 2)));
        // R and pack_base of the four requests, in the slot layout: 256
        // contiguous bytes each, needing only the block index
        const uint64_t slot = i0 * 8u + (uint64_t)p4_slot(lane);
        const uint64_t rv = R[slot], bv = pbase[slot];
        // base_value of request 4b + (lane & 3): lanes 0-3 compute the results
        const uint64_t bvl = *(bvp ? reinterpret_cast<const uint64_t *>(bvp) + (i0 + (uint64_t)(lane & 3))
                                   : R + slot);
        const uint64_t reqbase = bvp ? bvl : 0ull;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            off[g] = uniform_u64(offv[g]);
            ln[g] = uniform_u64(lenv[g]);
            id0[g] = (uint32_t)__builtin_amdgcn_readfirstlane(idv[g]);
        }
        // every load above is issued before the first use of any (q2_pin): left
        // alone, a load used under one condition only sinks behind the wait
        // for the others
        asm volatile("" : "+s"(off[0]), "+s"(off[1]), "+s"(off[2]), "+s"(off[3]), "+s"(off[4]),
                          "+s"(ln[0]), "+s"(ln[1]), "+s"(ln[2]), "+s"(ln[3]), "+s"(id0[0]),
                          "+s"(id0[1]), "+s"(id0[2]), "+s"(id0[3]), "+s"(ktw), "+s"(okw));
        const bool has_len = key_len != nullptr, has_id0 = key_id0 != nullptr;
        const uint32_t want = key_type != nullptr ? (a.req_type & 0xffu) * 0x01010101u : ktw;
        uint32_t n[4];
        // served: all packed, a log to read; each key within a chunk and of the
        // request's type (an empty key's type is not looked at)
        uint32_t bad = (okw ^ 0x01010101u) | (a.n_entries == 0 ? 1u : 0u);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint64_t n64 = has_len ? ln[g] : off[g + 1] - off[g];
            n[g] = (uint32_t)n64;
            id0[g] = has_id0 ? id0[g] : AGN_ID0_NONE;
            const uint32_t kdiff = ((ktw ^ want) >> (8 * g)) & 0xffu;
            bad |= (n64 > (uint64_t)AGN_WAVE ? 1u : 0u) | (n64 != 0 ? kdiff : 0u);
        }
        if (bad == 0u) {
            // (read here: held over the check, the pointer costs the SGPR file a spill)
            const uint32_t *const rows = kparams<Q2PackParams>().rows;
            P8Rows c[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) c[g] = p8_load_rows<true>(rows, off[g], 0, a.n_entries);
            const int64_t *const l_eff = kparams<Q2Params>().eff;
            // all eight row loads are in flight before the first verdict
            __builtin_amdgcn_sched_barrier(0);
            // thresholds min(R - base, 2^32 - 1); noR of key g: its 16 lanes' bits
            const uint64_t below = ballot(rv < bv);
            const uint64_t dl = rv - bv;
            const uint32_t t = (dl >> 32) ? 0xFFFFFFFFu : (uint32_t)dl;
            // Request g's scalars move to lane g as they are made, where
            // the results are computed once for the four: held as
            // scalars to the stores, four requests' state does not fit the
            // SGPR file.  first_excl and first_err are positions < 64 or -1.
            uint32_t v_off_lo = 0, v_off_hi = 0, v_n = 0, v_id0 = 0, v_cnt = 0, v_fx = 0, v_fe = 0,
                     v_sum_lo = 0, v_sum_hi = 0;
            uint32_t cg = 0;  // the count of key lane >> 4, the slot layout's key
            const int kg = lane >> 4;
            u32x4 mx[4];
            uint64_t in[4];
            int64_t ev[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const u32x4 th = p4_thr(t, g);
                const bool noR = ((below >> (16 * g)) & 0xFFFFull) != 0ull;
                uint32_t cnt = 0;
                int64_t fx = -1;
                mx[g] = u32x4{0u, 0u, 0u, 0u};
                in[g] = p8_verdict(c[g], 0, (uint64_t)n[g], th, noR, mx[g], cnt, fx);
                ev[g] = q8_load_eff(l_eff, off[g], 0, in[g],
                                    reinterpret_cast<const int64_t *>(R + (i0 + (uint64_t)g) * 8u));
                __builtin_amdgcn_sched_barrier(0);  // key g's effects go out before key g + 1's verdict
                cg = kg == g ? cnt : cg;
                v_cnt = put_lane(cnt, g, v_cnt);
                v_fx = put_lane((uint32_t)fx, g, v_fx);
                v_off_lo = put_lane((uint32_t)off[g], g, v_off_lo);
                v_off_hi = put_lane((uint32_t)(off[g] >> 32), g, v_off_hi);
                v_n = put_lane(n[g], g, v_n);
                v_id0 = put_lane(id0[g], g, v_id0);
            }
            __builtin_amdgcn_sched_barrier(0);  // the four effect loads are in flight from here
            // The pointers the results need are read here, under the effects
            // (k_counter_quad2).  Where the log has no id index, lanes 0-3 load
            // the op id that defines their request's NewLastOp -- one load; the
            // other lanes read an address the wave has fetched.
            const auto &pr = kparams<Q2Params>();
            const uint32_t *const l_op_id = pr.op_id;
            int64_t *const l_value = pr.o_value, *const l_hole = pr.o_hole;
            uint64_t *const l_lastct = pr.o_lastct;
            uint32_t *const l_count = pr.o_count, *const l_flags = pr.o_flags, *const l_err = pr.o_err;
            const uint64_t v_off = ((uint64_t)v_off_hi << 32) | v_off_lo;
            const int32_t fx = (int32_t)v_fx;
            const uint32_t pos = fx >= 0 ? (uint32_t)fx : v_n - 1u;
            const bool need = lane < 4 && v_id0 == AGN_ID0_NONE && v_n != 0u;
            const uint32_t *const ip = need ? l_op_id + (v_off + (uint64_t)pos)
                                            : reinterpret_cast<const uint32_t *>(R + slot);
            const uint32_t opid = *ip;
            // LastOpCt = base + max delta where the key included an op, else 0 (cold)
            const uint32_t md = p4_maxfold(mx);
            const uint64_t ct = cg ? bv + (uint64_t)md : 0ull;
            __builtin_amdgcn_sched_barrier(0);  // the wait for the effects: after the fold
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                int64_t sum = 0, fe = -1;
                q8_fold_eff(in[g], ev[g], 0, sum, fe);
                const uint64_t total = (uint64_t)wave_sum_dpp(sum);
                v_fe = put_lane((uint32_t)fe, g, v_fe);
                v_sum_lo = put_lane((uint32_t)total, g, v_sum_lo);
                v_sum_hi = put_lane((uint32_t)(total >> 32), g, v_sum_hi);
            }
            __builtin_amdgcn_sched_barrier(0);  // and no store before it
            // lane g < 4: request g's result, as q2_result's of a cold read
            const uint64_t idh = v_id0 != AGN_ID0_NONE ? (uint64_t)v_id0 + (uint64_t)pos : (uint64_t)opid;
            const int64_t hid = v_n ? (int64_t)idh : 0;  // get_first_id of no ops: 0
            const int32_t fe = (int32_t)v_fe;
            uint32_t fl = v_cnt ? AGN_F_NEWSS : AGN_F_CT_IGNORE;
            fl |= fe >= 0 ? AGN_F_ERR_UNEXPECTED : 0u;
            if ((lane & 2) == 0) l_lastct[slot] = ct;  // the four rows: 256 contiguous bytes
            if (lane < 4) {  // one store per array
                const uint64_t i = i0 + (uint64_t)lane;
                l_value[i] = (int64_t)(reqbase + (((uint64_t)v_sum_hi << 32) | v_sum_lo));
                l_hole[i] = fx >= 0 ? hid - 1 : hid;
                l_count[i] = v_cnt;
                l_err[i] = fe >= 0 ? (uint32_t)(v_off + (uint64_t)fe) : 0xffffffffu;
                l_flags[i] = fl;
            }
            return;
        }
    }
    const uint64_t left = a.n_req - i0;
    const uint32_t m = left < 4u ? (uint32_t)left : 4u;
#pragma nounroll
    for (uint32_t h = 0; h < m; ++h) q2_serve_oc(a, i0 + h);
}

// k_counter_pack4's parameters and the narrow tier of the packed index
// (agn_log_index_pack16).
struct Q2Pack8Params {
    DenseArgs a;
    MaskArgs mk;
    const void *args[20];  // keys .. o_err
    const uint32_t *rows;
    const uint64_t *base;
    const uint8_t *ok;
    const uint16_t *rows16;
    const uint8_t *narrow;
    const int16_t *eff16;  // the effect tier (agn_log_index_eff16); E16 only
};
static_assert(offsetof(Q2Pack8Params, rows) == offsetof(Q2PackParams, rows) &&
                  offsetof(Q2Pack8Params, base) == offsetof(Q2PackParams, base),
              "Q2Pack8Params extends Q2PackParams");

// Eight requests per wave over the narrow tier: k_counter_pack4's launch
// (cold, dense, the identity key map) where the log's keys are narrow -- u16
// deltas, 16 bytes per op, a 64-op key 1 KiB: lane l loads the whole row of
// op l, so eight keys are the same eight 16-byte loads per lane (8 KiB in
// flight per wave) that four keys are over the u32 rows.
//
// The straight path serves a group whose eight requests exist, are narrow
// (both dwords of `narrow`), fit one chunk and are not corrupt, over a
// non-empty log.  The per-key metadata is loaded and the results are computed
// as vectors in lanes 0-7 (eight requests' scalars do not fit the SGPR file);
// a key's offset and length are lane reads where a wave-uniform value is
// needed.  R, pack_base, the thresholds and LastOpCt are one value per lane
// (key l >> 3, DC l & 7): 512 contiguous bytes per array.  Order: metadata ->
// the eight row loads -> per key verdict (one ballot: a lane holds every DC of
// its op) and deferred effect load, the row registers keeping the included
// op's deltas -> one transposed max fold and the op-id load, under the
// effects -> the effects' transposed sum -> stores.  Every other group -- and
// the last one of a batch that is no multiple of eight, which reads nothing
// past request n_req - 1 -- runs its requests one after the other through oc
// (q2_serve_oc).  Same results as k_counter_quad2.
//
// E16: over the effect tier (agn_log_index_eff16).  Each key's i16 effects --
// one 128-byte line of a 64-op key -- are loaded with its rows, before any
// verdict: sixteen loads in flight, two dependent round trips (metadata ->
// rows and effects -> stores) where the 8-byte gathers of `eff` make a third.
// The included lanes' terms are i32 (64 terms of magnitude at most 32 767), so
// the sums fold as u32 (n8_sumfold32) and are sign-extended once per key.  An
// included lane that holds the escape 0x8000 sets bit g of v_esc; one
// wave-uniform branch after the fold (rare: the launcher bounds the log's
// escapes) reads those lanes' `eff`, where alone an AGN_EFFECT_INVALID can be
// met, and adds their i64 sum.  The op id is loaded only when a lane needs
// one: a non-empty key without an id base (no id index, or AGN_ID0_NONE in it).
template <bool E16>
__global__ __launch_bounds__(64) void k_counter_pack8(Q2Pack8Params) {
    const DenseArgs a = dense_of(kparams<Q2Params>().a);
    const uint32_t blk = block_order(a.xcd, blockIdx.x, gridDim.x);
    const uint64_t i0 = uniform_u64((uint64_t)blk * 8u);
    if (i0 >= a.n_req) return;
    const int lane = lane_id();
    if (i0 + 7u < a.n_req) {
        // One round trip, every address a function of the block and the lane
        // alone; absent arrays read an in-bounds dummy (key_meta's
        // convention).  Lanes 0-7 hold requests 8b .. 8b+7, lane 8 the ninth
        // offset, which exists without key_len: 8b + 8 <= n_keys.
        const auto &pm = kparams<Q2Params>();
        const uint64_t *const key_off = pm.key_off, *const key_len = pm.key_len;
        const uint32_t *const key_id0 = pm.key_id0;
        const uint8_t *const key_type = pm.key_type;
        const uint64_t *const R = pm.R;
        const int64_t *const bvp = pm.base_value;
        const auto &pq = *(const __attribute__((address_space(4))) Q2Pack8Params *)&pm;
        const uint64_t *const pbase = pq.base;
        const uint8_t *const pnar = pq.narrow;
        const bool has_len = key_len != nullptr, has_id0 = key_id0 != nullptr;
        const uint32_t m8 = (uint32_t)lane & 7u;
        const uint64_t *const op = key_off + i0 + (uint64_t)((!has_len && lane >= 8) ? 8u : m8);
        const uint64_t v_off = *op;
        const uint64_t v_lr = *(has_len ? key_len + i0 + m8 : op);
        const uint32_t v_ir = *(has_id0 ? key_id0 + i0 + m8 : reinterpret_cast<const uint32_t *>(op));
        const uint8_t *const ktp = key_type ? key_type : reinterpret_cast<const uint8_t *>(key_off);
        uint32_t ktw0 = __builtin_amdgcn_readfirstlane(ldc(reinterpret_cast<const uint32_t *>(ktp) + (i0 >> 2)));
        uint32_t ktw1 = __builtin_amdgcn_readfirstlane(ldc(reinterpret_cast<const uint32_t *>(ktp) + (i0 >> 2) + 1u));
        uint32_t nw0 = __builtin_amdgcn_readfirstlane(ldc(reinterpret_cast<const uint32_t *>(pnar) + (i0 >> 2)));
        uint32_t nw1 = __builtin_amdgcn_readfirstlane(ldc(reinterpret_cast<const uint32_t *>(pnar) + (i0 >> 2) + 1u));
        // R and pack_base of the eight requests: 512 contiguous bytes each
        const uint64_t slot = i0 * 8u + (uint64_t)lane;
        const uint64_t rv = R[slot], bv = pbase[slot];
        const uint64_t bvl = *(bvp ? reinterpret_cast<const uint64_t *>(bvp) + (i0 + m8) : R + slot);
        const uint64_t reqbase = bvp ? bvl : 0ull;
        // the next lane's offset (row_shl:1; lanes 0-7 sit in one row)
        const uint64_t v_nx =
            ((uint64_t)__builtin_amdgcn_update_dpp(0u, (uint32_t)(v_off >> 32), 0x101, 0xF, 0xF, false) << 32) |
            __builtin_amdgcn_update_dpp(0u, (uint32_t)v_off, 0x101, 0xF, 0xF, false);
        const uint64_t v_n64 = has_len ? v_lr : v_nx - v_off;
        const uint32_t v_n = (uint32_t)v_n64;
        const uint32_t v_id0 = has_id0 ? v_ir : AGN_ID0_NONE;
        // served: all narrow, a log to read; each key within a chunk and of the
        // request's type (an empty key's type is not looked at)
        const uint32_t kt = (((lane & 4) ? ktw1 : ktw0) >> (8u * ((uint32_t)lane & 3u))) & 0xffu;
        const uint32_t want = key_type != nullptr ? (a.req_type & 0xffu) : kt;
        const bool lbad = lane < 8 && (v_n64 > (uint64_t)AGN_WAVE || (v_n64 != 0 && kt != want));
        const bool bad = ballot(lbad) != 0ull || nw0 != 0x01010101u || nw1 != 0x01010101u ||
                         a.n_entries == 0;
        if (!bad) {
            const uint16_t *const rows16 = kparams<Q2Pack8Params>().rows16;
            u32x4 c[8];
#pragma unroll
            for (int g = 0; g < 8; ++g)
                c[g] = n8_load_rows<true>(rows16, n8_readlane_u64(v_off, g), a.n_entries);
            const int64_t *const l_eff = kparams<Q2Params>().eff;
            uint32_t e16[E16 ? 8 : 1];  // E16 only: written and read under if constexpr (E16)
            if constexpr (E16) {
                const int16_t *const eff16 = kparams<Q2Pack8Params>().eff16;
#pragma unroll
                for (int g = 0; g < 8; ++g)
                    e16[g] = n8_load_eff16(eff16, n8_readlane_u64(v_off, g), a.n_entries);
            }
            // all eight row loads (E16: all sixteen loads) are in flight before
            // the first verdict
            __builtin_amdgcn_sched_barrier(0);
            // thresholds min(R - base, 2^16 - 1); noR of key g: its 8 lanes' bits
            const uint64_t below = ballot(rv < bv);
            const uint64_t dl = rv - bv;
            const uint32_t tp = n8_thr_pack(dl > 0xFFFFull ? 0xFFFFu : (uint32_t)dl);
            // first_excl and first_err are positions < 64 or -1; request g's go
            // to lane g, the lanes' own verdicts to bit g of v_inc
            uint32_t v_cnt = 0, v_fx = 0, v_fe = E16 ? 0xFFFFFFFFu : 0u, v_inc = 0;
            uint32_t cg = 0;  // the count of key lane >> 3, this lane's key
            const int kg = lane >> 3;
            int64_t ev[E16 ? 1 : 8];  // !E16 only: written and read under if constexpr (!E16)
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const uint32_t th0 = __builtin_amdgcn_readlane(tp, 8 * g);
                const uint32_t th1 = __builtin_amdgcn_readlane(tp, 8 * g + 2);
                const uint32_t th2 = __builtin_amdgcn_readlane(tp, 8 * g + 4);
                const uint32_t th3 = __builtin_amdgcn_readlane(tp, 8 * g + 6);
                const uint32_t noR = (uint32_t)(below >> (8 * g)) & 0xFFu;
                const uint32_t n_g = __builtin_amdgcn_readlane(v_n, g);
                const uint64_t off_g = n8_readlane_u64(v_off, g);
                const bool valid = (uint32_t)lane < n_g;
                const bool ex = (noR | n8_excl(c[g], th0, th1, th2, th3)) != 0u;
                const bool mine = valid & !ex;
                const uint64_t exm = ballot(valid & ex);
                const uint32_t cnt = (uint32_t)__builtin_popcountll(ballot(mine));
                const uint32_t fx = exm ? (uint32_t)__builtin_ctzll(exm) : 0xFFFFFFFFu;
                if constexpr (!E16)
                    ev[g] = n8_load_eff(l_eff, off_g, mine,
                                        reinterpret_cast<const int64_t *>(R + (i0 + (uint64_t)g) * 8u));
                // LastOpCt's terms in place of the row: the included op's deltas
                c[g].x = mine ? c[g].x : 0u;
                c[g].y = mine ? c[g].y : 0u;
                c[g].z = mine ? c[g].z : 0u;
                c[g].w = mine ? c[g].w : 0u;
                v_inc |= mine ? (1u << g) : 0u;
                __builtin_amdgcn_sched_barrier(0);  // key g's effects go out before key g + 1's verdict
                cg = kg == g ? cnt : cg;
                v_cnt = put_lane(cnt, g, v_cnt);
                v_fx = put_lane(fx, g, v_fx);
            }
            __builtin_amdgcn_sched_barrier(0);  // the eight effect loads are in flight from here
            // The pointers the results need are read here, under the effects
            // (k_counter_quad2).  Where the log has no id index, lanes 0-7 load
            // the op id that defines their request's NewLastOp -- one load; the
            // other lanes read an address the wave has fetched.
            const auto &pr = kparams<Q2Params>();
            const uint32_t *const l_op_id = pr.op_id;
            int64_t *const l_value = pr.o_value, *const l_hole = pr.o_hole;
            uint64_t *const l_lastct = pr.o_lastct;
            uint32_t *const l_count = pr.o_count, *const l_flags = pr.o_flags, *const l_err = pr.o_err;
            const int32_t fx = (int32_t)v_fx;
            const uint32_t pos = fx >= 0 ? (uint32_t)fx : v_n - 1u;
            const bool need = lane < 8 && v_id0 == AGN_ID0_NONE && v_n != 0u;
            const uint32_t *const ip = need ? l_op_id + (v_off + (uint64_t)pos)
                                            : reinterpret_cast<const uint32_t *>(R + slot);
            // E16: nothing hides a dummy's round trip, so the load is issued
            // only when some lane needs its op id (wave-uniform)
            uint32_t opid = 0;
            if (!E16 || ballot(need) != 0ull) opid = *ip;
            // E16: the i32 terms and their fold first -- the effects came in
            // with the rows, and eight registers are one before the max fold
            uint32_t v_esc = 0, ks32 = 0;
            if constexpr (E16) {
                uint32_t sm[8];
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const bool mine = ((v_inc >> g) & 1u) != 0u;
                    const bool esc = mine && e16[g] == 0x8000u;
                    v_esc |= esc ? (1u << g) : 0u;
                    sm[g] = (mine && !esc) ? (uint32_t)(int32_t)(int16_t)e16[g] : 0u;
                }
                // key (lane >> 3)'s i32 sum in every lane
                ks32 = n8_sumfold32(sm);
                __builtin_amdgcn_sched_barrier(0);
            }
            // LastOpCt = base + max delta where the key included an op, else 0 (cold)
            const uint32_t md = n8_maxfold(c);
            const uint64_t ct = cg ? bv + (uint64_t)md : 0ull;
            __builtin_amdgcn_sched_barrier(0);  // the wait for the effects: after the fold
            uint64_t total;
            if constexpr (E16) {
                // lane g < 8 takes key g's sum, sign-extended once
                total = (uint64_t)(int64_t)(int32_t)__shfl((int)ks32, 8 * (int)m8, AGN_WAVE);
                if (ballot(v_esc != 0u) != 0ull) {
                    // the escaped lanes (and only they) read eff; lane g takes
                    // key g's first invalid position and the others' i64 sum
#pragma nounroll
                    for (int g = 0; g < 8; ++g) {
                        const bool esc = ((v_esc >> g) & 1u) != 0u;
                        if (ballot(esc) == 0ull) continue;
                        const uint64_t off_g = n8_readlane_u64(v_off, g);
                        int64_t x = 0;
                        if (esc) x = l_eff[off_g + (uint64_t)lane];
                        const bool badv = esc && x == AGN_EFFECT_INVALID;
                        const uint64_t be = ballot(badv);
                        const uint64_t xs = (uint64_t)wave_sum_dpp(badv ? 0 : x);
                        v_fe = put_lane(be ? (uint32_t)__builtin_ctzll(be) : 0xFFFFFFFFu, g, v_fe);
                        total += lane == g ? xs : 0ull;
                    }
                }
            } else {
                uint64_t sm[8];
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const bool mine = ((v_inc >> g) & 1u) != 0u;
                    const bool badv = mine && ev[g] == AGN_EFFECT_INVALID;
                    const uint64_t be = ballot(badv);
                    v_fe = put_lane(be ? (uint32_t)__builtin_ctzll(be) : 0xFFFFFFFFu, g, v_fe);
                    sm[g] = (mine && !badv) ? (uint64_t)ev[g] : 0ull;
                }
                // key (lane >> 3)'s sum in every lane; lane g < 8 takes key g's
                const uint64_t ks = n8_sumfold(sm);
                total =
                    ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(ks >> 32), 8 * (int)m8, AGN_WAVE) << 32) |
                    (uint32_t)__shfl((int)(uint32_t)ks, 8 * (int)m8, AGN_WAVE);
            }
            __builtin_amdgcn_sched_barrier(0);  // and no store before it
            // lane g < 8: request g's result, as q2_result's of a cold read
            const uint64_t idh = v_id0 != AGN_ID0_NONE ? (uint64_t)v_id0 + (uint64_t)pos : (uint64_t)opid;
            const int64_t hid = v_n ? (int64_t)idh : 0;  // get_first_id of no ops: 0
            const int32_t fe = (int32_t)v_fe;
            uint32_t fl = v_cnt ? AGN_F_NEWSS : AGN_F_CT_IGNORE;
            fl |= fe >= 0 ? AGN_F_ERR_UNEXPECTED : 0u;
            l_lastct[slot] = ct;  // the eight rows: 512 contiguous bytes
            if (lane < 8) {  // one store per array
                const uint64_t i = i0 + (uint64_t)lane;
                l_value[i] = (int64_t)(reqbase + total);
                l_hole[i] = fx >= 0 ? hid - 1 : hid;
                l_count[i] = v_cnt;
                l_err[i] = fe >= 0 ? (uint32_t)(v_off + (uint64_t)fe) : 0xffffffffu;
                l_flags[i] = fl;
            }
            return;
        }
    }
    const uint64_t left = a.n_req - i0;
    const uint32_t m = left < 8u ? (uint32_t)left : 8u;
#pragma nounroll
    for (uint32_t h = 0; h < m; ++h) q2_serve_oc(a, i0 + h);
}

// ROWS_QUAD with the first chunk EARLY (D = 8, one request per wave; the
// sparse batches, MSK): the key's segment metadata (key_off, key_len,
// key_id0) is the only scalar round trip before the rows -- chunk 0's quad
// rows and effects are issued as soon as it lands, and R, SCT, the side
// bytes, the TxId and the mask words load under them.  In k_counter_key all
// of those share the metadata's round trip, and scalar loads return out of
// order, so the first row load waits for the slowest of them (lgkmcnt(0)).
// A key whose DC set U is known (agn_log.key_mask) is served by the dense
// scan, also when R lacks one of U's DCs (every op excluded, :245-247); a key
// whose entries carry different DC sets is appended to `list` for
// k_counter_q8m, so this kernel holds no per-entry-mask scan (inlined, it
// cost 73-98 VGPRs: 4-6 waves per SIMD, or spills at a 7-wave cap;
// profiles/r04/ab_masked_*.log).  KM: the key's DC set loads with the
// segment metadata (1) or under the chunk (0).  Same results as
// k_counter_key.
template <bool ANY_WARM, bool KEYS, int KM>
__global__ __launch_bounds__(64) void k_counter_q8e(
    DenseArgs a, MaskArgs mk, const uint64_t *__restrict__ keys,
    const uint64_t *__restrict__ key_off, const uint64_t *__restrict__ key_len,
    const uint8_t *__restrict__ key_type, const uint32_t *__restrict__ key_id0,
    const uint64_t *__restrict__ oc, const uint32_t *__restrict__ op_id,
    const int64_t *__restrict__ eff, const uint64_t *__restrict__ log_txid,
    const uint64_t *__restrict__ R, const uint64_t *__restrict__ sct,
    const uint8_t *__restrict__ sct_ignore, const uint64_t *__restrict__ req_txid,
    const int64_t *__restrict__ base_value, int64_t *__restrict__ o_value,
    int64_t *__restrict__ o_hole, uint64_t *__restrict__ o_lastct,
    uint32_t *__restrict__ o_count, uint32_t *__restrict__ o_flags,
    uint32_t *__restrict__ o_err, uint32_t *__restrict__ list, uint32_t *__restrict__ list_n) {
    const uint32_t blk = block_order(a.xcd, blockIdx.x, gridDim.x);
    const uint64_t i = uniform_u64((uint64_t)blk);
    if (i >= a.n_req) return;
    Q2Key k;
    q2_meta(k, i, KEYS ? keys : nullptr, key_off, key_len, key_id0);
    // a key whose entries carry different DC sets: k_counter_q8m's
    auto mixed = [&](uint64_t kmw) {
        return !(mk.oc_mask == nullptr || (mk.key_mask && (kmw & 0xFFull)) || k.n == 0);
    };
    // QL_S sub-lists (request i -> i mod QL_S), each with its own counter in
    // its own 128-byte line: one shared counter serialised every hand-on of
    // a batch of mixed keys at one L2 channel (10M atomics, 16x the scan)
    auto hand_on = [&]() {
        if (lane_id() == 0) {
            const uint32_t sl = (uint32_t)(i % QL_S);
            list[(uint64_t)sl * a.ql_cap + atomicAdd(list_n + sl * QL_STRIDE, 1u)] = (uint32_t)i;
        }
    };
    uint64_t kmw = 0;
    if constexpr (KM == 1) {
        kmw = key_word(mk, k.key, key_off);
        if (mixed(kmw)) {
            hand_on();
            return;
        }
    }
    const bool any = a.n_entries != 0;
    Q8Chunk c0{};
    if (any) c0 = q8_load<true, false>(oc, eff, k.off, 0, a.n_entries);
    // the request's side values: one group of scalar loads under the rows,
    // used only past the barrier (one lgkmcnt wait, see q2_load)
    Q2Raw x = q2_load<ANY_WARM, true>(k, a, mk, KM == 0, key_off, key_type, R, sct, sct_ignore,
                                      req_txid);
    __builtin_amdgcn_sched_barrier(0);
    q2_pin(x);
    if constexpr (KM == 0) kmw = x.kmw;
    q2_apply<ANY_WARM, true>(k, a, mk, x, kmw, key_type, sct, sct_ignore, req_txid);
    if (KM == 0 && mixed(kmw)) {
        hand_on();
        return;
    }
    Q2Acc s;
    s.ctA = k.eA;
    s.ctB = k.eB;
    if (any && !k.corrupt) {
        q2_fold<ANY_WARM>(k, c0, 0, log_txid, a.n_entries, s);
        q2_rest<ANY_WARM>(k, oc, eff, log_txid, a.n_entries, s);
    }
    q2_epilogue<true>(k, s, a.hints, op_id, base_value, o_value, o_hole, o_lastct, o_count, o_flags,
                      o_err, mk.o_mask);
}

// Sparse batches, cold and warm: k_counter_q8e with two requests per wave,
// as k_counter_quad2 serves dense warm batches -- both keys' segment
// metadata in one scalar round trip, both first chunks issued under it, the
// side loads (R, SCT, the DC sets) under the chunks.  Mixed keys are handed
// on to k_counter_q8m as in q8e.  (Round 3's two-request masked form carried
// the per-entry-mask scan inline: 118 VGPRs, slower than one request.)
template <bool ANY_WARM, bool KEYS>
__global__ __launch_bounds__(64) void k_counter_q8e2(Q2Params) {
    const DenseArgs a = dense_of(kparams<Q2Params>().a);
    const uint32_t blk = block_order(a.xcd, blockIdx.x, gridDim.x);
    const uint64_t i0 = uniform_u64((uint64_t)blk * 2u);
    if (i0 >= a.n_req) return;
    const bool two = i0 + 1u < a.n_req;
    const uint64_t i1 = two ? i0 + 1u : i0;
    Q2Key k0, k1;
    {
        const auto &p = kparams<Q2Params>();
        q2_meta(k0, i0, KEYS ? p.keys : nullptr, p.key_off, p.key_len, p.key_id0);
        q2_meta(k1, i1, KEYS ? p.keys : nullptr, p.key_off, p.key_len, p.key_id0);
    }
    const bool any = a.n_entries != 0;
    Q8Chunk c0{}, c1{};
    if (any) {
        const auto &p = kparams<Q2Params>();
        c0 = q8_load<true, false>(p.oc, p.eff, k0.off, 0, a.n_entries);
        c1 = q8_load<true, false>(p.oc, p.eff, k1.off, 0, a.n_entries);
    }
    __builtin_amdgcn_sched_barrier(0);
    const auto &ps = kparams<Q2Params>();
    const MaskArgs mk = mask_of(ps.mk);
    const uint64_t kmw0 = key_word(mk, k0.key, ps.key_off), kmw1 = key_word(mk, k1.key, ps.key_off);
    q2_side<ANY_WARM, true>(k0, a, mk, kmw0, ps.key_off, ps.key_type, ps.R, ps.sct,
                            ps.sct_ignore, ps.req_txid);
    q2_side<ANY_WARM, true>(k1, a, mk, kmw1, ps.key_off, ps.key_type, ps.R, ps.sct,
                            ps.sct_ignore, ps.req_txid);
    auto mixed = [&](const Q2Key &k, uint64_t kmw) {
        return !(mk.oc_mask == nullptr || (mk.key_mask && (kmw & 0xFFull)) || k.n == 0);
    };
    auto hand_on = [&](uint64_t i) {  // q8e's sub-lists
        if (lane_id() == 0) {
            const auto &p = kparams<Q2Params>();
            const uint32_t sl = (uint32_t)(i % QL_S);
            p.list[(uint64_t)sl * a.ql_cap + atomicAdd(p.list_n + sl * QL_STRIDE, 1u)] = (uint32_t)i;
        }
    };
    const bool m0 = mixed(k0, kmw0), m1 = two && mixed(k1, kmw1);
    if (m0) hand_on(i0);
    if (m1) hand_on(i1);
    Q2Acc s0, s1;
    s0.ctA = k0.eA;
    s0.ctB = k0.eB;
    s1.ctA = k1.eA;
    s1.ctB = k1.eB;
    const bool d0 = any && !k0.corrupt && !m0, d1 = two && any && !k1.corrupt && !m1;
    {
        const auto &p = kparams<Q2Params>();
        if (d0) q2_fold<ANY_WARM>(k0, c0, 0, p.log_txid, a.n_entries, s0);
        if (d1) q2_fold<ANY_WARM>(k1, c1, 0, p.log_txid, a.n_entries, s1);
        if (d0) q2_rest<ANY_WARM>(k0, p.oc, p.eff, p.log_txid, a.n_entries, s0);
        if (d1) q2_rest<ANY_WARM>(k1, p.oc, p.eff, p.log_txid, a.n_entries, s1);
    }
    const auto &pe = kparams<Q2Params>();
    if (!m0)
        q2_epilogue<true>(k0, s0, a.hints, pe.op_id, pe.base_value, pe.o_value, pe.o_hole,
                          pe.o_lastct, pe.o_count, pe.o_flags, pe.o_err, pe.mk.o_mask);
    if (two && !m1)
        q2_epilogue<true>(k1, s1, a.hints, pe.op_id, pe.base_value, pe.o_value, pe.o_hole,
                          pe.o_lastct, pe.o_count, pe.o_flags, pe.o_err, pe.mk.o_mask);
}

// The keys k_counter_q8e handed on (entries with different DC sets): the
// per-entry-mask quad scan (scan_key_q8_msk), one request per wave, the
// waves striding over the sub-lists -- the grid does not know their
// lengths, and empty lists cost one short launch.
template <bool ANY_WARM, bool KEYS>
__global__ __launch_bounds__(64) void k_counter_q8m(
    DenseArgs a, MaskArgs mk, const uint64_t *__restrict__ keys,
    const uint64_t *__restrict__ key_off, const uint64_t *__restrict__ key_len,
    const uint8_t *__restrict__ key_type, const uint32_t *__restrict__ key_id0,
    const uint64_t *__restrict__ oc, const uint32_t *__restrict__ op_id,
    const int64_t *__restrict__ eff, const uint64_t *__restrict__ log_txid,
    const uint64_t *__restrict__ R, const uint64_t *__restrict__ sct,
    const uint8_t *__restrict__ sct_ignore, const uint64_t *__restrict__ req_txid,
    const int64_t *__restrict__ base_value, int64_t *__restrict__ o_value,
    int64_t *__restrict__ o_hole, uint64_t *__restrict__ o_lastct,
    uint32_t *__restrict__ o_count, uint32_t *__restrict__ o_flags,
    uint32_t *__restrict__ o_err, const uint32_t *__restrict__ list,
    const uint32_t *__restrict__ list_n) {
    // block b walks sub-list b mod QL_S, entries b / QL_S, + gridDim.x / QL_S
    const uint32_t sl = blockIdx.x % QL_S, per = gridDim.x / QL_S;
    const uint32_t cnt = __builtin_amdgcn_readfirstlane(list_n[sl * QL_STRIDE]);
    for (uint32_t j = blockIdx.x / QL_S; j < cnt; j += per) {
        const uint64_t i = __builtin_amdgcn_readfirstlane(list[(uint64_t)sl * a.ql_cap + j]);
        const Q2Key k = q2_prologue<ANY_WARM, true>(a, mk, i, KEYS ? keys : nullptr, key_off,
                                                    key_len, key_type, key_id0, R, sct, sct_ignore,
                                                    req_txid);
        Q2Acc s;
        s.ctA = k.eA;
        s.ctB = k.eB;
        if (a.n_entries != 0 && !k.corrupt)
            q2_msk<ANY_WARM>(k, oc, mk.oc_mask, eff, log_txid, a.n_entries, s);
        q2_epilogue<true>(k, s, a.hints, op_id, base_value, o_value, o_hole, o_lastct, o_count,
                          o_flags, o_err, mk.o_mask);
    }
}

MaskArgs mask_args(const agn_log &log, const agn_read &req, const agn_result &out) {
    MaskArgs m;
    m.key_mask = log.oc_mask ? log.key_mask : nullptr;
    m.oc_mask = log.oc_mask;
    m.R_mask = req.R_mask;
    m.sct_mask = req.sct ? req.sct_mask : nullptr;
    m.o_mask = out.lastct_mask;
    return m;
}

inline bool sparse_batch(const agn_log &log, const agn_read &req, const agn_result &out) {
    return log.oc_mask || req.R_mask || (req.sct && req.sct_mask) || out.lastct_mask;
}

int launch_quad2(const agn_log &log, const agn_read &req, const agn_result &out, hipStream_t st) {
    DenseArgs a{req.n_req, log.n_entries, req.req_type, counter_order(req.n_req, BULK_CHUNK), 0u, 1u,
                req.hints};
    const MaskArgs mk = mask_args(log, req, out);
    const uint64_t nb = (req.n_req + 1) / 2;
    if (nb > 0x7fffffffull) return fail(AGN_EINVAL, "batch too large: %llu requests",
                                        (unsigned long long)req.n_req);
    PackIdx pk{};
#define AGN_Q2L_(W, M, E, S, ...)                                                               \
    hipLaunchKernelGGL((k_counter_quad2<W, M, E, S, ##__VA_ARGS__>), dim3((unsigned)nb),        \
                       dim3(64), 0, st, a,                                                      \
                       mk, req.keys, log.key_off, log.key_len, log.key_type, id0_index(log),    \
                       log.oc, log.op_id, log.eff, log.txid, req.R, req.sct, req.sct_ignore,    \
                       req.txid, req.base_value, out.value, out.hole, out.lastct, out.count,    \
                       out.flags, out.err_pos, pk.rows, pk.base, pk.ok)
#define AGN_Q2L(W, M)                                                                           \
    do {                                                                                        \
        if (q2e && q2s) AGN_Q2L_(W, M, true, true);                                             \
        else if (q2e) AGN_Q2L_(W, M, true, false);                                              \
        else if (q2s) AGN_Q2L_(W, M, false, true);                                              \
        else AGN_Q2L_(W, M, false, false);                                                      \
    } while (0)
    const bool msk = sparse_batch(log, req, out);
    // AGN_Q2_EFF / AGN_Q2_STORE = 0|1 (A/B knobs; k_counter_quad2).  Both are
    // the default of the cold dense path: cold cfg2 in one process 7.72 ms
    // before, 7.54 with the effects after the verdict, 7.66 with the paired
    // stores, 7.39 with both (62 VGPRs, 98 SGPRs, 8 waves per SIMD, no spill).
    // The warm dense path keeps the kernel as it was (8.13 ms against 8.52 /
    // 8.93 / 8.31: under its 6-wave budget the forms spill 44-48 bytes per
    // lane), and so do the masked forms, which lose a wave per SIMD or gain
    // SGPR spills (profiles/r07/ab_q2_eff_store_*.log, resource_usage_quad2.txt).
    // The pair stores write 16 bytes to the 8-byte arrays and 8 to the 4-byte
    // ones: result arrays that are not aligned so keep the per-key stores.
    const bool dflt = !req.sct && !msk;
    const char *ev = AGN_KNOB("AGN_Q2_EFF"), *sv = AGN_KNOB("AGN_Q2_STORE");
    const bool q2e = (ev && (ev[0] == '0' || ev[0] == '1')) ? ev[0] == '1' : dflt;
    const uintptr_t a16 = (uintptr_t)out.value | (uintptr_t)out.hole | (uintptr_t)out.lastct |
                          (uintptr_t)mk.o_mask;
    const uintptr_t a8 = (uintptr_t)out.count | (uintptr_t)out.flags | (uintptr_t)out.err_pos;
    const bool q2s = ((sv && (sv[0] == '0' || sv[0] == '1')) ? sv[0] == '1' : dflt) &&
                     (a16 & 15u) == 0 && (a8 & 7u) == 0;
    // AGN_Q2_PACK = 0|1 (A/B knob, default on): a cold dense batch over a log
    // with a registered packed index (agn_log_index_pack) scans its 32-byte
    // rows.  The PACK form has both forms above, so it needs both in effect.
    const char *pv = AGN_KNOB("AGN_Q2_PACK");
    const bool pack = dflt && q2e && q2s && log.n_entries != 0 && !(pv && pv[0] == '0') &&
                      pack_lookup(log, &pk);
    // AGN_Q2_FOUR = 0|1 (A/B knob): the packed read of a whole partition
    // (identity key map) runs four requests per wave, k_counter_pack4.
    // A log of more than 64 entries per key on average keeps two per wave: its
    // groups mostly hold a key longer than a chunk and would run four
    // requests one after the other (3M keys x 200 ops: 8.37 against 8.31 ms).
    const char *fv = AGN_KNOB("AGN_Q2_FOUR");
    const bool four = pack && !req.keys && log.n_entries / 64u <= log.n_keys &&
                      ((fv && (fv[0] == '0' || fv[0] == '1')) ? fv[0] == '1' : Q2_FOUR_DEFAULT);
    // AGN_Q2_NARROW = 0|1 (A/B knob, default on): that read over a log whose
    // index has a narrow tier (agn_log_index_pack16) with nearly every key
    // narrow runs eight requests per wave over the u16 rows, k_counter_pack8.
    // Set to 1 it takes the kernel whatever the count of wide keys (the bound
    // is a matter of speed, not of results; the tests reach the kernel's
    // fallback on small logs this way).
    const char *nv = AGN_KNOB("AGN_Q2_NARROW");
    const bool eight = four && pk.rows16 && pk.narrow &&
                       ((nv && (nv[0] == '0' || nv[0] == '1'))
                            ? nv[0] == '1'
                            : pk.n_wide * NARROW_WIDE_DIV <= log.n_keys);
    // AGN_Q2_EFF16 = 0|1 (A/B knob, AGN_Q2_NARROW's convention): the narrow
    // read of a log with an effect tier (agn_log_index_eff16) built from this
    // log.eff, of whose entries at most one in EFF16_ESC_DIV escaped, loads
    // the i16 effects with the rows, k_counter_pack8<true>.  Set to 1 it takes
    // the tier whatever the count of escapes (a matter of speed, not of
    // results).
    const char *xv = AGN_KNOB("AGN_Q2_EFF16");
    const bool e16 = eight && pk.eff16 && log.eff == pk.eff_src &&
                     ((xv && (xv[0] == '0' || xv[0] == '1'))
                          ? xv[0] == '1'
                          : EFF16_DEFAULT && pk.n_esc * EFF16_ESC_DIV <= log.n_entries);
    if (eight) {
        a.xcd = counter_order(req.n_req, BULK_CHUNK8);
        const Q2Pack8Params p{a, mk,
                              {req.keys, log.key_off, log.key_len, log.key_type, id0_index(log),
                               log.oc, log.op_id, log.eff, log.txid, req.R, req.sct, req.sct_ignore,
                               req.txid, req.base_value, out.value, out.hole, out.lastct, out.count,
                               out.flags, out.err_pos},
                              pk.rows, pk.base, pk.ok, pk.rows16, pk.narrow, pk.eff16};
        const dim3 grid((unsigned)((req.n_req + 7) / 8));
        if (e16) hipLaunchKernelGGL(k_counter_pack8<true>, grid, dim3(64), 0, st, p);
        else hipLaunchKernelGGL(k_counter_pack8<false>, grid, dim3(64), 0, st, p);
    } else if (four) {
        a.xcd = counter_order(req.n_req, BULK_CHUNK4);
        const Q2PackParams p{a, mk,
                             {req.keys, log.key_off, log.key_len, log.key_type, id0_index(log),
                              log.oc, log.op_id, log.eff, log.txid, req.R, req.sct, req.sct_ignore,
                              req.txid, req.base_value, out.value, out.hole, out.lastct, out.count,
                              out.flags, out.err_pos},
                             pk.rows, pk.base, pk.ok};
        hipLaunchKernelGGL(k_counter_pack4, dim3((unsigned)((req.n_req + 3) / 4)), dim3(64), 0, st, p);
    } else if (pack) {
        AGN_Q2L_(false, false, true, true, true);
    } else if (req.sct) {
        if (msk) AGN_Q2L(true, true);
        else AGN_Q2L(true, false);
    } else {
        if (msk) AGN_Q2L(false, true);
        else AGN_Q2L(false, false);
    }
#undef AGN_Q2L
#undef AGN_Q2L_
    AGN_HIP(hipGetLastError());
    return AGN_OK;
}

// Sparse batches (D = 8, quad rows) run k_counter_q8e + k_counter_q8m,
// unless AGN_COUNTER_EARLY=0 (A/B knob) or the batch carries AGN_HINT_MIXED:
// k_counter_key, which scans a mixed key in the same pass (cfg2 with one
// entry in 8 lacking a DC: 1.24x dense there, 2.56x through the hand-on,
// whose first pass reads the key's only chunk for nothing;
// profiles/r04/ab_masked_*).  The hint comes from the caller, from the read
// batcher (the op log's host copy of the key DC sets) or from agn_materialize
// itself for a key_mask that agn_log_index_masks built (many_mixed).  By
// default q8e loads the key's DC set under the first chunk; AGN_Q8E_KM=1
// loads it with the segment metadata instead.
inline bool early_chunk() {
    const char *v = AGN_KNOB("AGN_COUNTER_EARLY");
    return !(v && v[0] == '0');
}

int launch_q8e(const agn_log &log, const agn_read &req, const agn_result &out, hipStream_t st) {
    DenseArgs a{req.n_req, log.n_entries, req.req_type, counter_order(req.n_req, BULK_CHUNK), 0u, 1u,
                req.hints};
    const MaskArgs mk = mask_args(log, req, out);
    if (req.n_req > 0x7fffffffull) return fail(AGN_EINVAL, "batch too large: %llu requests",
                                               (unsigned long long)req.n_req);
    // the key's DC set loaded under the first chunk (default; cold masked
    // cfg2 1.047x dense vs 1.107x with the metadata, profiles/r04/), or with
    // the segment metadata (AGN_Q8E_KM=1)
    const char *kv = AGN_KNOB("AGN_Q8E_KM");
    const bool km0 = !(kv && kv[0] == '1');
    // QL_S counters (QL_STRIDE apart), then QL_S sub-lists of ql_cap indices
    a.ql_cap = (uint32_t)((req.n_req + QL_S - 1) / QL_S);
    const size_t hdr = (size_t)QL_S * QL_STRIDE;
    uint32_t *lst = nullptr;
    AGN_HIP(pool_malloc(&lst, (hdr + (size_t)QL_S * a.ql_cap) * sizeof(uint32_t), st));
    int rc = AGN_OK;
    if (hipMemsetAsync(lst, 0, hdr * sizeof(uint32_t), st) != hipSuccess)
        rc = fail(AGN_EHIP, "counter q8e: list reset");
#define AGN_ARGS                                                                                \
    a, mk, req.keys, log.key_off, log.key_len, log.key_type, id0_index(log), log.oc, log.op_id,  \
        log.eff, log.txid, req.R, req.sct, req.sct_ignore, req.txid, req.base_value, out.value,  \
        out.hole, out.lastct, out.count, out.flags, out.err_pos, lst + hdr, lst
#define AGN_Q8E_(W, K, KM)                                                                      \
    hipLaunchKernelGGL((k_counter_q8e<W, K, KM>), dim3((unsigned)req.n_req), dim3(64), 0, st,   \
                       AGN_ARGS)
#define AGN_Q8E(W, K)                                                                           \
    do {                                                                                        \
        if (km0) AGN_Q8E_(W, K, 0);                                                             \
        else AGN_Q8E_(W, K, 1);                                                                 \
    } while (0)
    const unsigned mb = QL_S * 16u;  // a multiple of QL_S
#define AGN_Q8M(W, K)                                                                           \
    hipLaunchKernelGGL((k_counter_q8m<W, K>), dim3(mb), dim3(64), 0, st, AGN_ARGS)
    // two requests per wave (k_counter_q8e2; AGN_Q8E_TWO=0: one).
    // Warm masked cfg2 8.55 ms against q8e's 9.27 and the dense warm
    // kernel's 8.27 (profiles/r05/ab_masked_warm_q8e2_ldc.log)
    // cold batches too since the dense path went two per wave: masked cfg2
    // with the bench's hints 7.36 against 8.00 ms in one process
    // (profiles/r06/ab_masked_cold_two.log); AGN_Q8E_TWO=1: warm batches only
    const char *tv = AGN_KNOB("AGN_Q8E_TWO");
    const bool two = !(tv && tv[0] == '0');
    const bool two_cold = two && !(tv && tv[0] == '1');
    const unsigned nb2 = (unsigned)((req.n_req + 1) / 2);
#define AGN_Q8E2(W, K)                                                                          \
    hipLaunchKernelGGL((k_counter_q8e2<W, K>), dim3(nb2), dim3(64), 0, st, Q2Params{AGN_ARGS})
    if (rc == AGN_OK) {
        if (req.sct && two) {
            if (req.keys) { AGN_Q8E2(true, true); AGN_Q8M(true, true); }
            else { AGN_Q8E2(true, false); AGN_Q8M(true, false); }
        } else if (two_cold) {
            if (req.keys) { AGN_Q8E2(false, true); AGN_Q8M(false, true); }
            else { AGN_Q8E2(false, false); AGN_Q8M(false, false); }
        } else if (req.sct) {
            if (req.keys) { AGN_Q8E(true, true); AGN_Q8M(true, true); }
            else { AGN_Q8E(true, false); AGN_Q8M(true, false); }
        } else {
            if (req.keys) { AGN_Q8E(false, true); AGN_Q8M(false, true); }
            else { AGN_Q8E(false, false); AGN_Q8M(false, false); }
        }
        if (hipGetLastError() != hipSuccess) rc = fail(AGN_EHIP, "counter q8e: launch");
    }
#undef AGN_Q8E2
#undef AGN_Q8M
#undef AGN_Q8E
#undef AGN_Q8E_
#undef AGN_ARGS
    const hipError_t ef = hipFreeAsync(lst, st);
    if (rc == AGN_OK && ef != hipSuccess) rc = fail(AGN_EHIP, "hipFreeAsync: %s", hipGetErrorString(ef));
    return rc;
}

// Two chunks per step for D <= 4 (scan_key PAIR), unless AGN_COUNTER_PAIR=0
// (A/B knob).
inline uint32_t pair_chunks() {
    const char *v = AGN_KNOB("AGN_COUNTER_PAIR");
    return (v && v[0] == '0') ? 0u : 1u;
}

// Row-load variant per device.  LDS-DMA rows (even D) are box-dependent: on
// two MI355X boxes they beat the VGPR-load path by 7-10 % (cfg2 7.29-7.55 vs
// 8.16-8.44 ms), on three others they lost by 6-14 % (8.86-9.28 vs 7.95-8.39
// ms), consistently across processes on one box (profiles/r01/ab_counter_
// glds*.log).  Quad rows (D = 8) beat VGPR rows by 4-6 % on the boxes
// measured (cfg2 7.81 vs 8.24-8.30 ms, warm 8.35 vs 8.68 ms;
// profiles/r02/ab_counter_quad*.log), so they are the untuned default for
// D = 8 and VGPR rows for other D.  agn_tune times the bit-identical variants
// on the caller's batch and keeps another one for the device only when it is
// at least 3 % faster than that default.  AGN_COUNTER_VARIANT=0/1/2 (or the
// older AGN_COUNTER_GLDS=0/1) forces the choice.
constexpr int kMaxDev = 64;
// per device: 0 untuned (the default of the shape), else 1 + ROWS_VGPR /
// ROWS_GLDS / ROWS_QUAD
std::atomic<int> g_rows_choice[kMaxDev];

template <int D>
constexpr int default_variant() { return D == 8 ? ROWS_QUAD : ROWS_VGPR; }

inline int cur_dev() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d >= 0 && d < kMaxDev ? d : 0;
}

inline int forced_variant() {
    const char *v = AGN_KNOB("AGN_COUNTER_VARIANT");
    if (v && v[0] >= '0' && v[0] <= '3') return v[0] - '0';
    v = AGN_KNOB("AGN_COUNTER_GLDS");
    if (v && (v[0] == '0' || v[0] == '1')) return v[0] - '0';
    return -1;
}

inline int tuned_variant() {  // -1 = untuned
    return g_rows_choice[cur_dev()].load(std::memory_order_relaxed) - 1;
}

template <int D>
int counter_variant() {
    const int f = forced_variant();
    if (f >= 0) return f;
    const int t = tuned_variant();
    return t >= 0 ? t : default_variant<D>();
}

template <int D, int WPB, int VAR, bool KEYS, bool MSK>
int launch_key_k(const agn_log &log, const agn_read &req, const agn_result &out, hipStream_t st) {
    const char *qv = AGN_KNOB("AGN_COUNTER_QUAD_NT");
    DenseArgs a{req.n_req, log.n_entries, req.req_type, counter_order(req.n_req, BULK_CHUNK), pair_chunks(),
                (qv && qv[0] >= '0' && qv[0] <= '3') ? (uint32_t)(qv[0] - '0') : 1u};
    const MaskArgs mk = mask_args(log, req, out);
    const uint64_t nb = (req.n_req + WPB - 1) / WPB;
    if (nb > 0x7fffffffull) return fail(AGN_EINVAL, "batch too large: %llu requests",
                                        (unsigned long long)req.n_req);
    if (req.sct)
        hipLaunchKernelGGL((k_counter_key<D, true, WPB, VAR, KEYS, MSK>), dim3((unsigned)nb),
                           dim3(64 * WPB), 0, st, a, mk, req.keys, log.key_off, log.key_len,
                           log.key_type, id0_index(log), log.oc, log.op_id, log.eff, log.txid,
                           req.R, req.sct, req.sct_ignore, req.txid, req.base_value, out.value,
                           out.hole, out.lastct, out.count, out.flags, out.err_pos);
    else
        hipLaunchKernelGGL((k_counter_key<D, false, WPB, VAR, KEYS, MSK>), dim3((unsigned)nb),
                           dim3(64 * WPB), 0, st, a, mk, req.keys, log.key_off, log.key_len,
                           log.key_type, id0_index(log), log.oc, log.op_id, log.eff, log.txid,
                           req.R, req.sct, req.sct_ignore, req.txid, req.base_value, out.value,
                           out.hole, out.lastct, out.count, out.flags, out.err_pos);
    AGN_HIP(hipGetLastError());
    return AGN_OK;
}

template <int D, int WPB, int VAR, bool MSK>
int launch_key_g(const agn_log &log, const agn_read &req, const agn_result &out, hipStream_t st) {
    return req.keys ? launch_key_k<D, WPB, VAR, true, MSK>(log, req, out, st)
                    : launch_key_k<D, WPB, VAR, false, MSK>(log, req, out, st);
}

// The variants this D has: VGPR rows always, LDS-DMA rows for even D, quad
// rows for D = 8.
template <int D>
constexpr bool has_variant(int v) {
    return v == ROWS_VGPR || (v == ROWS_GLDS && D % 2 == 0) || (v == ROWS_QUAD && D == 8);
}

// A sparse batch (presence masks, MSK) runs VGPR or quad rows: the LDS-DMA
// variant has no per-entry-mask scan for its mixed keys.
template <int D, int WPB, bool MSK>
int launch_var(int v, const agn_log &log, const agn_read &req, const agn_result &out,
               hipStream_t st) {
    if constexpr (D % 2 == 0 && !MSK)
        if (v == ROWS_GLDS) return launch_key_g<D, WPB, ROWS_GLDS, false>(log, req, out, st);
    if constexpr (D == 8)
        if (v == ROWS_QUAD || (MSK && v == ROWS_GLDS)) {
            if (MSK && WPB == 1 && early_chunk() && !(req.hints & AGN_HINT_MIXED))
                return launch_q8e(log, req, out, st);
            return launch_key_g<D, WPB, ROWS_QUAD, MSK>(log, req, out, st);
        }
    return launch_key_g<D, WPB, ROWS_VGPR, MSK>(log, req, out, st);
}

template <int D, int WPB>
int launch_key(const agn_log &log, const agn_read &req, const agn_result &out, hipStream_t st) {
    const int v = counter_variant<D>();
    // quad rows, dense batch, not forced: two requests per wave -- warm cfg2
    // 8.37-8.45 vs 8.83-9.02 ms (profiles/r02/ab_counter_quad2.log); cold
    // batches too since the blocks go to the XCDs in runs (block_order):
    // cold cfg2 7.28 vs 7.46 ms in one process (round 2, identity order: no
    // change; profiles/r06/ab_counter_quad2_cold.log).  A masked batch keeps
    // one request per wave (its two-request form takes 118 VGPRs, 4 waves per
    // SIMD: warm masked cfg2 13.06 vs 11.06 ms, mixed keys 17.32 vs 13.00;
    // profiles/r03/ab_masked_warm_quad{2,1}.log)
    const bool masked = sparse_batch(log, req, out);
    if constexpr (D == 8)
        if (v == ROWS_QUAD2 || (v == ROWS_QUAD && !masked && forced_variant() < 0))
            return launch_quad2(log, req, out, st);
    const int v2 = v == ROWS_QUAD2 ? default_variant<D>() : v;
    return masked ? launch_var<D, WPB, true>(v2, log, req, out, st)
                  : launch_var<D, WPB, false>(v2, log, req, out, st);
}

// Waves (= requests) per block: 1 measured 1.4-3.4 % faster than 2 and
// 0-1.6 % faster than 4 on cfg2 (profiles/r01/ab_counter_wpb.log), so only
// WPB = 1 is instantiated.
template <int D>
int launch_dense(const agn_log &log, const agn_read &req, const agn_result &out,
                 hipStream_t st) {
    return launch_key<D, 1>(log, req, out, st);
}

// agn_log_index_masks: one wave per key; out[k] = the mask word every entry
// of the segment carries (low D bits), 0 when they differ or the key is empty.
// The block's mixed keys (non-empty, entries differ) are added to one of
// IM_CNT counters (IM_STRIDE words apart: one counter per 128-byte line).
constexpr uint32_t IM_CNT = 256, IM_STRIDE = 16;
__global__ __launch_bounds__(256) void k_index_masks(const uint64_t *__restrict__ key_off,
                                                    const uint64_t *__restrict__ key_len,
                                                    const uint64_t *__restrict__ oc_mask,
                                                    uint64_t full, uint64_t n_keys,
                                                    uint64_t *__restrict__ out,
                                                    unsigned long long *__restrict__ mixed) {
    __shared__ uint32_t blk_mixed;
    if (threadIdx.x == 0) blk_mixed = 0;
    __syncthreads();
    const uint64_t k = uniform_u64((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6));
    const int lane = lane_id();
    if (k < n_keys) {
        const uint64_t off = key_off[k];
        const uint64_t n = key_len ? key_len[k] : key_off[k + 1] - off;
        if (n == 0 || oc_mask == nullptr) {
            if (lane == 0) out[k] = n ? full : 0ull;
        } else {
            const uint64_t m0 = uniform_u64(oc_mask[off]) & full;
            bool ok = true;
            for (uint64_t b = 0; ok && b < n; b += AGN_WAVE) {
                const uint64_t p = b + (uint64_t)lane;
                const bool bad = p < n && (oc_mask[off + p] & full) != m0;
                ok = ballot(bad) == 0;
            }
            if (lane == 0) {
                out[k] = ok ? m0 : 0ull;
                if (!ok) atomicAdd(&blk_mixed, 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && blk_mixed && mixed)
        atomicAdd(&mixed[(blockIdx.x % IM_CNT) * IM_STRIDE], (unsigned long long)blk_mixed);
}

// agn_log_index_ids: one wave per key, lanes over the segment's positions.
__global__ __launch_bounds__(256) void k_index_ids(const uint64_t *__restrict__ key_off,
                                                  const uint64_t *__restrict__ key_len,
                                                  const uint32_t *__restrict__ op_id,
                                                  uint64_t n_keys, uint32_t *__restrict__ out) {
    const uint64_t k = uniform_u64((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6));
    if (k >= n_keys) return;
    const int lane = lane_id();
    const uint64_t off = key_off[k];
    const uint64_t n = key_len ? key_len[k] : key_off[k + 1] - off;
    if (n == 0) {
        if (lane == 0) out[k] = AGN_ID0_NONE;
        return;
    }
    const uint64_t id0 = op_id[off];
    bool ok = id0 + (n - 1) < (uint64_t)AGN_ID0_NONE;  // id0 + p fits and is never NONE
    for (uint64_t b = 0; ok && b < n; b += AGN_WAVE) {
        const uint64_t p = b + (uint64_t)lane;
        const bool bad = p < n && (uint64_t)op_id[off + p] != id0 + p;
        ok = ballot(bad) == 0;
    }
    if (lane == 0) out[k] = ok ? (uint32_t)id0 : AGN_ID0_NONE;
}

// agn_log_index_pack (D = 8): one wave per key.  Pass 1 takes the segment's
// column minima and maxima (lane = entry), pass 2 writes the u32 deltas of a
// key whose every column spans at most 2^32 - 1 -- lane-contiguous 16-byte
// stores in the layout p8_load_rows reads: lane l of store j holds DCs
// 4p .. 4p+3 (p = l & 1) of entry 32 j + (l >> 1).  An empty key is packed
// with an all-zero base.  The block's unpacked keys are counted as
// k_index_masks counts its mixed ones.
__global__ __launch_bounds__(256) void k_index_pack(const uint64_t *__restrict__ key_off,
                                                   const uint64_t *__restrict__ key_len,
                                                   const uint64_t *__restrict__ oc,
                                                   uint64_t n_keys, uint32_t *__restrict__ rows,
                                                   uint64_t *__restrict__ base,
                                                   uint8_t *__restrict__ ok,
                                                   unsigned long long *__restrict__ unpacked) {
    constexpr int D = 8;
    __shared__ uint32_t blk_un;
    if (threadIdx.x == 0) blk_un = 0;
    __syncthreads();
    const uint64_t k = uniform_u64((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6));
    const int lane = lane_id();
    if (k < n_keys) {
        const uint64_t off = key_off[k];
        const uint64_t n = key_len ? key_len[k] : key_off[k + 1] - off;
        uint64_t mn[D], mx[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            mn[d] = ~0ull;
            mx[d] = 0ull;
        }
        for (uint64_t b = 0; b < n; b += AGN_WAVE) {
            const uint64_t p = b + (uint64_t)lane;
            if (p < n) {
                uint64_t o[D];
                load_row<D, false>(oc + (off + p) * D, o);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    mn[d] = o[d] < mn[d] ? o[d] : mn[d];
                    mx[d] = umax64(mx[d], o[d]);
                }
            }
        }
        bool fits = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int x = 1; x < AGN_WAVE; x <<= 1) {
                const uint64_t a = shfl_xor_u64(mn[d], x);
                mn[d] = a < mn[d] ? a : mn[d];
                mx[d] = umax64(mx[d], shfl_xor_u64(mx[d], x));
            }
            if (n == 0) mn[d] = 0ull;
            fits = fits && (n == 0 || mx[d] - mn[d] <= 0xFFFFFFFFull);
        }
        if (lane == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) base[k * D + d] = mn[d];
            ok[k] = fits ? 1 : 0;
            if (!fits) atomicAdd(&blk_un, 1u);
        }
        if (fits) {
            const bool hi = (lane & 1) != 0;
            const uint64_t b0 = hi ? mn[4] : mn[0], b1 = hi ? mn[5] : mn[1];
            const uint64_t b2 = hi ? mn[6] : mn[2], b3 = hi ? mn[7] : mn[3];
            for (uint64_t b = 0; b < n; b += AGN_WAVE / 2) {
                const uint64_t p = b + (uint64_t)(lane >> 1);
                if (p < n) {
                    const uint64_t u = (off + p) * 2u + (hi ? 1u : 0u);  // 16-byte unit of rows
                    const u64x2 *src = reinterpret_cast<const u64x2 *>(oc) + u * 2u;
                    const u64x2 lo = src[0], hh = src[1];
                    u32x4 v;
                    v.x = (uint32_t)(lo.x - b0);
                    v.y = (uint32_t)(lo.y - b1);
                    v.z = (uint32_t)(hh.x - b2);
                    v.w = (uint32_t)(hh.y - b3);
                    reinterpret_cast<u32x4 *>(rows)[u] = v;
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && blk_un && unpacked)
        atomicAdd(&unpacked[(blockIdx.x % IM_CNT) * IM_STRIDE], (unsigned long long)blk_un);
}

// agn_log_index_pack16: one wave per key, from the u32 index.  Pass 1 decides
// whether the key is narrow -- packed, and no u32 delta above 2^16 - 1 (lane =
// entry) -- pass 2 writes a narrow key's u16 deltas: lane l stores the 16-byte
// unit of entry b + l, the layout n8_load_rows reads.  The block's wide keys
// are counted as k_index_pack counts its unpacked ones.
__global__ __launch_bounds__(256) void k_index_pack16(const uint64_t *__restrict__ key_off,
                                                     const uint64_t *__restrict__ key_len,
                                                     const uint32_t *__restrict__ rows,
                                                     const uint8_t *__restrict__ ok, uint64_t n_keys,
                                                     uint16_t *__restrict__ rows16,
                                                     uint8_t *__restrict__ narrow,
                                                     unsigned long long *__restrict__ wide) {
    __shared__ uint32_t blk_w;
    if (threadIdx.x == 0) blk_w = 0;
    __syncthreads();
    const uint64_t k = uniform_u64((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6));
    const int lane = lane_id();
    if (k < n_keys) {
        const uint64_t off = key_off[k];
        const uint64_t n = key_len ? key_len[k] : key_off[k + 1] - off;
        const u32x4 *src = reinterpret_cast<const u32x4 *>(rows);
        bool fits = ok[k] != 0;
        for (uint64_t b = 0; fits && b < n; b += AGN_WAVE) {
            const uint64_t p = b + (uint64_t)lane;
            bool big = false;
            if (p < n) {
                const u32x4 lo = src[(off + p) * 2u], hh = src[(off + p) * 2u + 1u];
                big = ((lo.x | lo.y | lo.z | lo.w | hh.x | hh.y | hh.z | hh.w) >> 16) != 0u;
            }
            fits = ballot(big) == 0ull;
        }
        if (lane == 0) {
            narrow[k] = fits ? 1 : 0;
            if (!fits) atomicAdd(&blk_w, 1u);
        }
        if (fits) {
            for (uint64_t b = 0; b < n; b += AGN_WAVE) {
                const uint64_t p = b + (uint64_t)lane;
                if (p < n) {
                    const u32x4 lo = src[(off + p) * 2u], hh = src[(off + p) * 2u + 1u];
                    u32x4 v;
                    v.x = lo.x | (lo.y << 16);
                    v.y = lo.z | (lo.w << 16);
                    v.z = hh.x | (hh.y << 16);
                    v.w = hh.z | (hh.w << 16);
                    reinterpret_cast<u32x4 *>(rows16)[off + p] = v;
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && blk_w)
        atomicAdd(&wide[(blockIdx.x % IM_CNT) * IM_STRIDE], (unsigned long long)blk_w);
}

// agn_log_index_eff16: a grid-stride pass, eight entries per lane -- eight
// 8-byte loads (eff is aligned to its elements only) and one 16-byte store;
// the log's last entries, short of eight, one lane each.  An effect outside
// [-32767, 32767] becomes the escape 0x8000; the block's escaped entries are
// counted as k_index_pack16 counts its wide keys.
__global__ __launch_bounds__(256) void k_index_eff16(const int64_t *__restrict__ eff,
                                                    uint64_t n_entries,
                                                    int16_t *__restrict__ eff16,
                                                    unsigned long long *__restrict__ escaped) {
    __shared__ uint32_t blk_e;
    if (threadIdx.x == 0) blk_e = 0;
    __syncthreads();
    auto narrow16 = [](int64_t x, uint32_t &esc) {
        const bool fits = x >= -32767 && x <= 32767;
        esc += fits ? 0u : 1u;
        return fits ? (uint32_t)x & 0xFFFFu : 0x8000u;
    };
    uint32_t esc = 0;
    const uint64_t units = n_entries / 8u, stride = (uint64_t)gridDim.x * 256u;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    for (uint64_t u = t; u < units; u += stride) {
        int64_t x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = eff[u * 8u + (uint64_t)j];
        uint32_t h[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = narrow16(x[j], esc);
        u32x4 v;
        v.x = h[0] | (h[1] << 16);
        v.y = h[2] | (h[3] << 16);
        v.z = h[4] | (h[5] << 16);
        v.w = h[6] | (h[7] << 16);
        reinterpret_cast<u32x4 *>(eff16)[u] = v;
    }
    const uint64_t e = units * 8u + t;  // the tail: fewer than eight entries
    if (e < n_entries) eff16[e] = (int16_t)(uint16_t)narrow16(eff[e], esc);
    if (esc) atomicAdd(&blk_e, esc);
    __syncthreads();
    if (threadIdx.x == 0 && blk_e)
        atomicAdd(&escaped[(blockIdx.x % IM_CNT) * IM_STRIDE], (unsigned long long)blk_e);
}

}  // namespace

int launch_index_eff16(const agn_log &log, int16_t *eff16, uint64_t *n_esc, hipStream_t st) {
    *n_esc = 0;
    if (log.n_entries == 0) return AGN_OK;
    // eight entries per lane; 8192 blocks hold every CU's waves many times over
    const uint64_t want = (log.n_entries / 8u + 255u) / 256u;
    const unsigned nb = (unsigned)(want < 1u ? 1u : want > 8192u ? 8192u : want);
    unsigned long long *cnt = nullptr;
    const size_t cb = (size_t)IM_CNT * IM_STRIDE * sizeof(unsigned long long);
    AGN_HIP(pool_malloc(&cnt, cb, st));
    if (hipMemsetAsync(cnt, 0, cb, st) != hipSuccess) {
        (void)hipFreeAsync(cnt, st);
        return fail(AGN_EHIP, "index_eff16: counter reset");
    }
    hipLaunchKernelGGL(k_index_eff16, dim3(nb), dim3(256), 0, st, log.eff, log.n_entries, eff16, cnt);
    int rc = hipGetLastError() == hipSuccess ? AGN_OK : fail(AGN_EHIP, "index_eff16: launch");
    // the count is read back here: the call blocks until the tier is built
    std::vector<unsigned long long> h((size_t)IM_CNT * IM_STRIDE);
    if (rc == AGN_OK &&
        (hipMemcpyAsync(h.data(), cnt, cb, hipMemcpyDeviceToHost, st) != hipSuccess ||
         hipStreamSynchronize(st) != hipSuccess))
        rc = fail(AGN_EHIP, "index_eff16: escape count");
    if (rc == AGN_OK)
        for (uint32_t i = 0; i < IM_CNT; ++i) *n_esc += h[(size_t)i * IM_STRIDE];
    (void)hipFreeAsync(cnt, st);
    return rc;
}

int launch_index_pack16(const agn_log &log, const uint32_t *rows, const uint8_t *ok,
                        uint16_t *rows16, uint8_t *narrow, uint64_t *n_wide, hipStream_t st) {
    const uint64_t nb = (log.n_keys + 3) / 4;
    *n_wide = 0;
    if (nb == 0) return AGN_OK;
    if (nb > 0x7fffffffull) return fail(AGN_EINVAL, "index_pack16: too many keys");
    unsigned long long *cnt = nullptr;
    const size_t cb = (size_t)IM_CNT * IM_STRIDE * sizeof(unsigned long long);
    AGN_HIP(pool_malloc(&cnt, cb, st));
    if (hipMemsetAsync(cnt, 0, cb, st) != hipSuccess) {
        (void)hipFreeAsync(cnt, st);
        return fail(AGN_EHIP, "index_pack16: counter reset");
    }
    hipLaunchKernelGGL(k_index_pack16, dim3((unsigned)nb), dim3(256), 0, st, log.key_off,
                       log.key_len, rows, ok, log.n_keys, rows16, narrow, cnt);
    int rc = hipGetLastError() == hipSuccess ? AGN_OK : fail(AGN_EHIP, "index_pack16: launch");
    // the count is read back here: the call blocks until the tier is built
    std::vector<unsigned long long> h((size_t)IM_CNT * IM_STRIDE);
    if (rc == AGN_OK &&
        (hipMemcpyAsync(h.data(), cnt, cb, hipMemcpyDeviceToHost, st) != hipSuccess ||
         hipStreamSynchronize(st) != hipSuccess))
        rc = fail(AGN_EHIP, "index_pack16: wide-key count");
    if (rc == AGN_OK)
        for (uint32_t i = 0; i < IM_CNT; ++i) *n_wide += h[(size_t)i * IM_STRIDE];
    (void)hipFreeAsync(cnt, st);
    return rc;
}

int launch_index_pack(const agn_log &log, uint32_t *rows, uint64_t *base, uint8_t *ok,
                      uint64_t *n_unpacked, hipStream_t st) {
    const uint64_t nb = (log.n_keys + 3) / 4;
    if (n_unpacked) *n_unpacked = 0;
    if (nb == 0) return AGN_OK;
    if (nb > 0x7fffffffull) return fail(AGN_EINVAL, "index_pack: too many keys");
    unsigned long long *cnt = nullptr;
    const size_t cb = (size_t)IM_CNT * IM_STRIDE * sizeof(unsigned long long);
    if (n_unpacked) {
        AGN_HIP(pool_malloc(&cnt, cb, st));
        if (hipMemsetAsync(cnt, 0, cb, st) != hipSuccess) {
            (void)hipFreeAsync(cnt, st);
            return fail(AGN_EHIP, "index_pack: counter reset");
        }
    }
    hipLaunchKernelGGL(k_index_pack, dim3((unsigned)nb), dim3(256), 0, st, log.key_off,
                       log.key_len, log.oc, log.n_keys, rows, base, ok, cnt);
    int rc = hipGetLastError() == hipSuccess ? AGN_OK : fail(AGN_EHIP, "index_pack: launch");
    if (cnt) {
        // the count is read back here: the call blocks until the index is built
        std::vector<unsigned long long> h((size_t)IM_CNT * IM_STRIDE);
        if (rc == AGN_OK &&
            (hipMemcpyAsync(h.data(), cnt, cb, hipMemcpyDeviceToHost, st) != hipSuccess ||
             hipStreamSynchronize(st) != hipSuccess))
            rc = fail(AGN_EHIP, "index_pack: unpacked-key count");
        if (rc == AGN_OK)
            for (uint32_t i = 0; i < IM_CNT; ++i) *n_unpacked += h[(size_t)i * IM_STRIDE];
        (void)hipFreeAsync(cnt, st);
    }
    return rc;
}

int launch_index_masks(const agn_log &log, uint64_t *out, uint64_t *mixed, hipStream_t st) {
    const uint64_t nb = (log.n_keys + 3) / 4;
    if (mixed) *mixed = 0;
    if (nb == 0) return AGN_OK;
    if (nb > 0x7fffffffull) return fail(AGN_EINVAL, "index_masks: too many keys");
    if (log.n_dcs > 64) return fail(AGN_ENOTSUP, "index_masks: n_dcs %u > 64", log.n_dcs);
    unsigned long long *cnt = nullptr;
    const size_t cb = (size_t)IM_CNT * IM_STRIDE * sizeof(unsigned long long);
    if (mixed) {
        AGN_HIP(pool_malloc(&cnt, cb, st));
        if (hipMemsetAsync(cnt, 0, cb, st) != hipSuccess) {
            (void)hipFreeAsync(cnt, st);
            return fail(AGN_EHIP, "index_masks: counter reset");
        }
    }
    hipLaunchKernelGGL(k_index_masks, dim3((unsigned)nb), dim3(256), 0, st, log.key_off,
                       log.key_len, log.oc_mask, low_bits(log.n_dcs), log.n_keys, out, cnt);
    int rc = hipGetLastError() == hipSuccess ? AGN_OK : fail(AGN_EHIP, "index_masks: launch");
    if (cnt) {
        // the count is read back here: the call blocks until the index is built
        std::vector<unsigned long long> h((size_t)IM_CNT * IM_STRIDE);
        if (rc == AGN_OK &&
            (hipMemcpyAsync(h.data(), cnt, cb, hipMemcpyDeviceToHost, st) != hipSuccess ||
             hipStreamSynchronize(st) != hipSuccess))
            rc = fail(AGN_EHIP, "index_masks: mixed-key count");
        if (rc == AGN_OK)
            for (uint32_t i = 0; i < IM_CNT; ++i) *mixed += h[(size_t)i * IM_STRIDE];
        (void)hipFreeAsync(cnt, st);
    }
    return rc;
}

int launch_index_ids(const agn_log &log, uint32_t *out, hipStream_t st) {
    const uint64_t nb = (log.n_keys + 3) / 4;
    if (nb == 0) return AGN_OK;
    if (nb > 0x7fffffffull) return fail(AGN_EINVAL, "index_ids: too many keys");
    hipLaunchKernelGGL(k_index_ids, dim3((unsigned)nb), dim3(256), 0, st, log.key_off,
                       log.key_len, log.op_id, log.n_keys, out);
    AGN_HIP(hipGetLastError());
    return AGN_OK;
}

// agn_tune for the dense counter path: alternate the row-load variants this
// D has over the caller's batch (`rounds` launches each, on `st`), keep each
// variant's fastest launch, and select another variant than the shape's
// default for this device only when it is at least 3 % faster.  All write
// the same results, so `out` holds the batch's results afterwards.  ms[v] =
// fastest launch of variant v (0 when absent).
template <int D>
int tune_dense(const agn_log &log, const agn_read &req, const agn_result &out, hipStream_t st,
               int rounds, int *choice, float *ms) {
    hipEvent_t e0, e1;
    AGN_HIP(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return fail(AGN_EHIP, "tune: hipEventCreate");
    }
    constexpr int NV = 3;
    float best[NV] = {3.4e38f, 3.4e38f, 3.4e38f};
    int rc = AGN_OK;
    for (int r = 0; r < rounds && rc == AGN_OK; ++r) {
        for (int k = 0; k < NV && rc == AGN_OK; ++k) {
            const int var = (r & 1) ? NV - 1 - k : k;  // alternate which variant goes first
            if (!has_variant<D>(var)) continue;
            if (hipEventRecord(e0, st) != hipSuccess) { rc = fail(AGN_EHIP, "tune: record"); break; }
            // quad rows run two requests per wave on a dense batch (launch_key)
            if constexpr (D == 8)
                rc = var == ROWS_QUAD ? launch_quad2(log, req, out, st)
                                      : launch_var<D, 1, false>(var, log, req, out, st);
            else
                rc = launch_var<D, 1, false>(var, log, req, out, st);
            if (rc) break;
            float t = 0.f;
            if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                hipEventElapsedTime(&t, e0, e1) != hipSuccess) {
                rc = fail(AGN_EHIP, "tune: event timing");
                break;
            }
            best[var] = t < best[var] ? t : best[var];
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    const int d0 = default_variant<D>();
    int c = d0;
    for (int v = 0; v < NV; ++v)
        if (v != d0 && has_variant<D>(v) && best[v] < 0.97f * best[d0] && best[v] < best[c]) c = v;
    g_rows_choice[cur_dev()].store(c + 1, std::memory_order_relaxed);
    *choice = c;
    if (ms)
        for (int v = 0; v < NV; ++v) ms[v] = has_variant<D>(v) ? best[v] : 0.f;
    return AGN_OK;
}

// Dense fast path applies when every clock is dense and D <= 8; returns
// AGN_ENOTSUP otherwise so the caller uses the general kernel.
int launch_counter_dense(const agn_log &log, const agn_read &req, const agn_result &out,
                         hipStream_t st) {
    // presence masks (D <= 8: one word per clock) run the MSK instantiations
    switch (log.n_dcs) {
        case 1: return launch_dense<1>(log, req, out, st);
        case 2: return launch_dense<2>(log, req, out, st);
        case 3: return launch_dense<3>(log, req, out, st);
        case 4: return launch_dense<4>(log, req, out, st);
        case 5: return launch_dense<5>(log, req, out, st);
        case 6: return launch_dense<6>(log, req, out, st);
        case 7: return launch_dense<7>(log, req, out, st);
        case 8: return launch_dense<8>(log, req, out, st);
        default: return AGN_ENOTSUP;
    }
}

// Tunable only for the dense counter path with even D (the LDS-DMA variant
// exists there); AGN_ENOTSUP otherwise, before anything is launched.
int tune_counter_dense(const agn_log &log, const agn_read &req, const agn_result &out,
                       hipStream_t st, int rounds, int *choice, float *ms) {
    if (log.crdt_type != AGN_COUNTER_PN || log.oc_mask || req.R_mask || req.sct_mask ||
        out.lastct_mask || req.n_req == 0)
        return AGN_ENOTSUP;
    const char *impl = AGN_KNOB("AGN_COUNTER_IMPL");
    if (impl && impl[0] == 'g') return AGN_ENOTSUP;  // general kernel forced
    switch (log.n_dcs) {
        case 2: return tune_dense<2>(log, req, out, st, rounds, choice, ms);
        case 4: return tune_dense<4>(log, req, out, st, rounds, choice, ms);
        case 6: return tune_dense<6>(log, req, out, st, rounds, choice, ms);
        case 8: return tune_dense<8>(log, req, out, st, rounds, choice, ms);
        default: return AGN_ENOTSUP;
    }
}

}  // namespace agn
