// mat_bcounter.hip — batched clocksi_materializer:materialize/4 for
// antidote_crdt_counter_b on gfx950 (one wave per key, grid-stride).
//
// Reference: materialize/4 src/clocksi_materializer.erl:89-101,
// apply_operations :113-121 with counter_b update/2 = orddict:update_counter
// on the P key {From, To} (increment, transfer) or the D key Id (decrement)
// (antidote_crdt 0.1.2, restated in SURVEY.md §8(a) a5.5).  The state is what
// src/clocksi_downstream.erl:61-64 reads for every bounded-counter write and
// src/bcounter_mgr.erl:165-185 before each remote permission request.  The
// snapshot filter is filter.hpp, the bookkeeping (NewLastOp, Count, LastOpCt,
// the error position) that of mat_lww.hip.
//   slot  = an orddict key (a P key or a D key, interned apart): tag
//   state = the set of (slot, sum): a slot is present iff a base pair or an
//           included entry with a valid tag names it; its sum is the base
//           sums (duplicate base tags add up) plus the included amounts, mod
//           2^64.  An amount of 0 is a value: the slot exists.
//   result pairs in ascending tag order, unsigned, each slot once
// The fold is a group-by-sum.  Each wave keeps a slot table in LDS (tag[256],
// sum[256]) and a wave-uniform count.  Base pairs go in first, 64 per step;
// then, per chunk, the lead lanes of the included entries: the lowest pending
// lane leads, its tag is read across, one ballot finds the lanes of that tag,
// their amounts are summed over the wave, the table is searched by all 64
// lanes at once and one lane adds to the hit or appends.  One round per
// distinct slot of the chunk -- a handful for a real bounded counter (one
// DC's increments and decrements plus a transfer or two), 64 at worst.  An
// append past 256 slots sets the overflow bit and the scan goes on, so hole,
// count, LastOpCt and a later invalid entry come out as without the limit.
//
// tag / amount loads: issued with the chunk's rows for every valid op (k_lww's
// early form: 8*D + 12 bytes per op); they do not depend on the verdict.
// Per key: 16 (key_off pair) + 8*D (R) + 8*D (LastOpCt) + 20 (hole, count,
// flags, err_pos) + 16 (out_off pair) + 4 (out_n) + 12 per pair.
// LDS per block: 12 KiB of tables + 4 * DPL * 512 B of LastOpCt stage (28 KiB
// at DPL = 8: five blocks per CU).
#include "cache_dev.hpp"
#include "filter.hpp"
#include "tags_serve.hpp"

namespace agn {
namespace {

// One (slot, amount), both wave-uniform, into the wave's table.  Lane j looks
// at entries j, j + 64, ...; tags are unique in the table, so at most one hits.
__device__ __forceinline__ void bc_put(uint32_t *tt, uint64_t *ts, uint32_t &ns, bool &ovf,
                                       uint32_t t, uint64_t amt) {
    const uint32_t lane = (uint32_t)lane_id();
    uint32_t hit = 0xffffffffu;
    for (uint32_t b = 0; b < ns; b += AGN_WAVE) {
        const uint32_t j = b + lane;
        const uint64_t hb = ballot(j < ns && tt[j] == t);
        if (hb) {
            hit = b + (uint32_t)__builtin_ctzll(hb);
            break;
        }
    }
    if (hit != 0xffffffffu) {
        if (lane == 0) ts[hit] += amt;
    } else if (ns < AGN_BCOUNTER_SLOTS_MAX) {
        if (lane == 0) {
            tt[ns] = t;
            ts[ns] = amt;
        }
        ++ns;
    } else {
        ovf = true;
    }
    wave_sync();  // the next search reads what lane 0 wrote
}

// The pending lanes' (tag, amount) into the table, one round per distinct tag.
__device__ __forceinline__ void bc_fold(uint32_t *tt, uint64_t *ts, uint32_t &ns, bool &ovf,
                                        bool p, uint32_t tag, uint64_t amt) {
    uint64_t pend = ballot(p);
    while (pend) {
        const int leader = __builtin_ctzll(pend);
        const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)tag, leader);
        const bool same = p && tag == t;
        pend &= ~ballot(same);
        const uint64_t s = (uint64_t)wave_sum_i64(same ? (int64_t)amt : 0);
        bc_put(tt, ts, ns, ovf, t, s);
    }
}

// The one-lane-per-op shapes are held to k_lww's five waves per SIMD.
template <int DPL, int LPO, bool SPARSE>
__global__ __launch_bounds__(256, (LPO == 1 ? 5 : 1)) void k_bcounter(agn_log log, agn_read req,
                                                                      agn_result out) {
    using F = KeyFilter<DPL, LPO, SPARSE>;
    __shared__ uint64_t stage[4][DPL][AGN_WAVE];
    __shared__ uint64_t Tsum[4][AGN_BCOUNTER_SLOTS_MAX];
    __shared__ uint32_t Ttag[4][AGN_BCOUNTER_SLOTS_MAX];
    // wave-uniform: the table's LDS addresses then take no VGPR
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t nw = (uint64_t)gridDim.x * 4u;
    uint32_t *tt = Ttag[w];
    uint64_t *ts = Tsum[w];

    for (uint64_t i = (uint64_t)blockIdx.x * 4u + (uint64_t)w; i < req.n_req; i += nw) {
        const uint64_t key = req.keys ? uniform_u64(req.keys[i]) : i;
        const uint64_t off = uniform_u64(log.key_off[key]);
        const uint64_t n = uniform_u64(key_n(log.key_off, log.key_len, key));
        const int lane = lane_id();

        if (n != 0 && log.key_type != nullptr && log.key_type[key] != (uint8_t)req.req_type) {
            if (lane == 0) {  // erlang:error(corrupted_ops_cache) (:190-191)
                out.flags[i] = AGN_F_ERR_CORRUPTED;
                out.err_pos[i] = 0xffffffffu;
                out.out_n[i] = 0;
            }
            continue;
        }

        uint32_t ns = 0;
        bool ovf = false;

        // the base state, 64 pairs per step: through the CSR or an
        // AGN_SS_STATE(start, pairs) reference in base_value
        if (req.base_tag != nullptr && req.base_tok != nullptr) {
            uint64_t b0 = 0, B = 0;
            if (req.base_off) {
                b0 = uniform_u64(req.base_off[i]);
                B = uniform_u64(req.base_off[i + 1]) - b0;
            } else if (req.base_value) {
                const uint64_t ref = uniform_u64((uint64_t)req.base_value[i]);
                b0 = AGN_SS_STATE_START(ref);
                B = AGN_SS_STATE_PAIRS(ref);
            }
            for (uint64_t x = 0; x < B; x += AGN_WAVE) {
                const bool p = x + (uint64_t)lane < B;
                const uint32_t tg = p ? req.base_tag[b0 + x + (uint64_t)lane] : 0u;
                const uint64_t am = p ? req.base_tok[b0 + x + (uint64_t)lane] : 0ull;
                bc_fold(tt, ts, ns, ovf, p, tg, am);
            }
        }

        F f;
        f.init(log, req, i);
        uint32_t cnt = 0;
        int64_t first_err = -1;
        for (uint64_t b = 0; b < n; b += F::S::OPI) {
            const uint64_t e = off + b + (uint64_t)f.slot;
            uint64_t am = 0;
            uint32_t tg = AGN_TAG_INVALID;
            if (f.sub == 0 && b + (uint64_t)f.slot < n) {
                am = log.add_tok[e];
                tg = log.tag[e];
            }
            bool valid;
            const bool incl = f.step(log, off, n, b, valid);
            const bool lead = incl && f.sub == 0;
            const bool bad = lead && tg == AGN_TAG_INVALID;
            cnt += (uint32_t)__builtin_popcountll(ballot(lead));
            if (first_err < 0) {
                const uint64_t be = ballot(bad);
                if (be) first_err = (int64_t)b + (int64_t)(__builtin_ctzll(be) / LPO);
            }
            bc_fold(tt, ts, ns, ovf, lead && !bad, tg, am);
        }

        const bool ct_ign = f.sct_ign && cnt == 0u;
        f.write_ct(stage[w], out, i, ct_ign);

        // room and the verdict, wave-uniform
        const uint64_t o = uniform_u64(out.out_off[i]);
        const uint64_t room = uniform_u64(out.out_off[i + 1]) - o;
        const bool err = first_err >= 0;
        const bool fits = !err && !ovf && (uint64_t)ns <= room;
        if (fits) {
            // rank = the count of smaller tags (unique in the table)
            for (uint32_t j = (uint32_t)lane; j < ns; j += AGN_WAVE) {
                const uint32_t t = tt[j];
                uint32_t r = 0;
                for (uint32_t x = 0; x < ns; ++x) r += tt[x] < t ? 1u : 0u;
                out.out_tag[o + r] = t;
                out.out_tok[o + r] = ts[j];
            }
        }

        if (lane == 0) {
            int64_t hole;
            if (f.first_excl >= 0) hole = (int64_t)log.op_id[off + (uint64_t)f.first_excl] - 1;
            else hole = n ? (int64_t)log.op_id[off + n - 1] : 0;
            uint32_t fl = 0;
            if (cnt) fl |= AGN_F_NEWSS;
            if (ct_ign) fl |= AGN_F_CT_IGNORE;
            uint32_t n_live = 0;
            if (err) {
                fl |= AGN_F_ERR_UNEXPECTED;
            } else if (ovf) {
                fl |= AGN_F_ERR_CAPACITY;  // more than AGN_BCOUNTER_SLOTS_MAX slots: out_n = 0
            } else {
                n_live = ns;
                if (!fits) fl |= AGN_F_ERR_CAPACITY;  // out_n = the room to come back with
            }
            out.hole[i] = hole;
            out.count[i] = cnt;
            out.flags[i] = fl;
            out.err_pos[i] =
                first_err >= 0 ? (uint32_t)(off + (uint64_t)first_err) : 0xffffffffu;
            out.out_n[i] = n_live;
        }
        wave_sync();  // the table is read to the end before the next request's writes
    }
}

template <int DPL, int LPO, bool SPARSE>
int launch_shape(const agn_log &log, const agn_read &req, const agn_result &out, hipStream_t st) {
    const unsigned blocks = grid_for(req.n_req, 4, 0x7fffffffu);  // one wave per request
    hipLaunchKernelGGL((k_bcounter<DPL, LPO, SPARSE>), dim3(blocks), dim3(256), 0, st, log, req,
                       out);
    AGN_HIP(hipGetLastError());
    return AGN_OK;
}

template <bool SPARSE>
int dispatch(const agn_log &log, const agn_read &req, const agn_result &out, hipStream_t st) {
#define AGN_L(DPL, LPO) launch_shape<DPL, LPO, SPARSE>(log, req, out, st)
    AGN_DISPATCH_SHAPES(log.n_dcs, AGN_L)
#undef AGN_L
}

// The fused cached read (tags_serve.hpp): per request, one wave runs
// get_from_snapshot_cache (materializer_vnode.erl:384-413), k_bcounter's fold
// from the hit slot's state in the arena, and materialize_snapshot's store
// (:466-509) of the result's state.  The lookup's verdict and base reference
// stay in registers; LastOpCt (+ its mask word) and the state go to the store
// through LDS, so no result array -- pinned host memory in the batcher -- is
// read back.  Every value the store branches on (hole, count, flags, n_live)
// is computed wave-uniformly.  The table is sorted once, in place, before the
// result store and the arena store read it: the kernel sequence stores the
// result's pairs, which are ascending, so the arena's are too.
// LDS per block: 12 KiB of tables + 4 * DPL * 512 B of stage + Sct[4][DC+1].
template <int DPL, int LPO, bool SPARSE>
__global__ __launch_bounds__(256) void k_bcounter_serve(agn_log log, agn_read req, agn_result out,
                                                        TagServe sv) {
    using F = KeyFilter<DPL, LPO, SPARSE>;
    constexpr int DC = F::S::DC;
    static_assert(DC <= AGN_WAVE, "one lane per LastOpCt column");
    static_assert(AGN_BCOUNTER_SLOTS_MAX == 4 * AGN_WAVE, "four table entries per lane");
    __shared__ uint64_t stage[4][DPL][AGN_WAVE];
    __shared__ uint64_t Sct[4][DC + 1];  // LastOpCt row + mask word for the store
    __shared__ uint64_t Tsum[4][AGN_BCOUNTER_SLOTS_MAX];
    __shared__ uint32_t Ttag[4][AGN_BCOUNTER_SLOTS_MAX];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t nw = (uint64_t)gridDim.x * 4u;
    const uint32_t D = log.n_dcs, W = n_words(D);
    const int lane = lane_id();
    const Grp<AGN_WAVE> g;
    uint32_t *tt = Ttag[w];
    uint64_t *ts = Tsum[w];

    for (uint64_t i = (uint64_t)blockIdx.x * 4u + (uint64_t)w; i < req.n_req; i += nw) {
        const uint64_t key = req.keys ? uniform_u64(req.keys[i]) : i;
        const LookupOut lk = ss_lookup_one<AGN_WAVE>(
            g, sv.c, key, req.R + i * D, req.R_mask ? req.R_mask + i * W : nullptr, sv.sct + i * D,
            sv.sctm ? sv.sctm + i * W : nullptr);
        if (lane == 0) {
            sv.ign[i] = lk.ign;
            sv.base[i] = lk.base;
            sv.first[i] = lk.first;
            sv.status[i] = lk.status;
            if (sv.dkeys) sv.dkeys[i] = key;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // other lanes read the rows
        // no-store outcomes (lane 0): prune[i] and the deltas
        auto sv_mark = [&](bool pr, const uint64_t *dl) {
            if (lane == 0) {
                sv.prune[i] = (uint8_t)((pr ? 1u : 0u) | ((sv.delta && dl[2]) ? 2u : 0u));
                if (sv.dprune) sv.dprune[i] = pr ? 1 : 0;
                if (sv.delta) {
                    sv.delta[2 * i] = dl[0];
                    sv.delta[2 * i + 1] = dl[1];
                }
            }
        };
        uint64_t dl[3] = {0ull, 0ull, 0ull};
        const uint64_t off = uniform_u64(log.key_off[key]);
        const uint64_t n = uniform_u64(key_n(log.key_off, log.key_len, key));

        if (n != 0 && log.key_type != nullptr && log.key_type[key] != (uint8_t)req.req_type) {
            if (lane == 0) {  // erlang:error(corrupted_ops_cache) (:190-191)
                out.flags[i] = AGN_F_ERR_CORRUPTED;
                out.err_pos[i] = 0xffffffffu;
                out.out_n[i] = 0;
            }
            sv_mark(false, dl);  // not stored (materialize_snapshot sees the error)
            continue;
        }

        uint32_t ns = 0;
        bool ovf = false;

        // the base state: the hit slot's pairs in the arena, 64 per step
        // (duplicate tags of a planted state add up)
        {
            const uint64_t ref = uniform_u64((uint64_t)lk.base);
            const uint64_t b0 = AGN_SS_STATE_START(ref);
            const uint64_t B = AGN_SS_STATE_PAIRS(ref);
            for (uint64_t x = 0; x < B; x += AGN_WAVE) {
                const bool p = x + (uint64_t)lane < B;
                const uint32_t tg = p ? sv.c.state_tag[b0 + x + (uint64_t)lane] : 0u;
                const uint64_t am = p ? sv.c.state_tok[b0 + x + (uint64_t)lane] : 0ull;
                bc_fold(tt, ts, ns, ovf, p, tg, am);
            }
        }

        F f;
        f.init_ign(log, req, i, lk.ign != 0);
        uint32_t cnt = 0;
        int64_t first_err = -1;
        for (uint64_t b = 0; b < n; b += F::S::OPI) {
            const uint64_t e = off + b + (uint64_t)f.slot;
            uint64_t am = 0;
            uint32_t tg = AGN_TAG_INVALID;
            if (f.sub == 0 && b + (uint64_t)f.slot < n) {
                am = log.add_tok[e];
                tg = log.tag[e];
            }
            bool valid;
            const bool incl = f.step(log, off, n, b, valid);
            const bool lead = incl && f.sub == 0;
            const bool bad = lead && tg == AGN_TAG_INVALID;
            cnt += (uint32_t)__builtin_popcountll(ballot(lead));
            if (first_err < 0) {
                const uint64_t be = ballot(bad);
                if (be) first_err = (int64_t)b + (int64_t)(__builtin_ctzll(be) / LPO);
            }
            bc_fold(tt, ts, ns, ovf, lead && !bad, tg, am);
        }

        const bool ct_ign = f.sct_ign && cnt == 0u;
        f.template write_ct<true>(stage[w], out, i, ct_ign, Sct[w]);

        // room and the verdict, wave-uniform
        const uint64_t o = uniform_u64(out.out_off[i]);
        const uint64_t room = uniform_u64(out.out_off[i + 1]) - o;
        const bool err = first_err >= 0;
        const bool fits = !err && !ovf && (uint64_t)ns <= room;

        int64_t hole;
        if (f.first_excl >= 0) hole = (int64_t)log.op_id[off + (uint64_t)f.first_excl] - 1;
        else hole = n ? (int64_t)log.op_id[off + n - 1] : 0;
        uint32_t fl = 0;
        if (cnt) fl |= AGN_F_NEWSS;
        if (ct_ign) fl |= AGN_F_CT_IGNORE;
        uint32_t n_live = 0;
        if (err) {
            fl |= AGN_F_ERR_UNEXPECTED;
        } else if (ovf) {
            fl |= AGN_F_ERR_CAPACITY;  // more than AGN_BCOUNTER_SLOTS_MAX slots: out_n = 0
        } else {
            n_live = ns;
            if (!fits) fl |= AGN_F_ERR_CAPACITY;  // out_n = the room to come back with
        }

        if (fits) {
            // ascending tag order, in place: each lane takes its entries and
            // their ranks (the count of smaller tags, unique in the table)
            // into registers, then writes them back at the ranks
            uint32_t et[4], er[4];
            uint64_t es[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t j = (uint32_t)lane + (uint32_t)q * AGN_WAVE;
                et[q] = 0u;
                es[q] = 0ull;
                er[q] = 0u;
                if (j < ns) {
                    et[q] = tt[j];
                    es[q] = ts[j];
                    for (uint32_t x = 0; x < ns; ++x) er[q] += tt[x] < et[q] ? 1u : 0u;
                }
            }
            wave_sync();  // every lane has read the table
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t j = (uint32_t)lane + (uint32_t)q * AGN_WAVE;
                if (j < ns) {
                    tt[er[q]] = et[q];
                    ts[er[q]] = es[q];
                }
            }
            wave_sync();
            for (uint32_t j = (uint32_t)lane; j < ns; j += AGN_WAVE) {
                out.out_tag[o + j] = tt[j];
                out.out_tok[o + j] = ts[j];
            }
        }

        if (lane == 0) {
            out.hole[i] = hole;
            out.count[i] = cnt;
            out.flags[i] = fl;
            out.err_pos[i] =
                first_err >= 0 ? (uint32_t)(off + (uint64_t)first_err) : 0xffffffffu;
            out.out_n[i] = n_live;
        }
        const bool pr = ss_store_one<AGN_WAVE>(
            g, sv.c, key, n, lk.status, lk.first, sv.gc != nullptr && sv.gc[i] != 0, Sct[w],
            (SPARSE && out.lastct_mask != nullptr) ? &Sct[w][DC] : nullptr, hole, 0, cnt, fl,
            sv.thr, sv.thrm, tt, ts, n_live, dl);
        sv_mark(pr, dl);
        wave_sync();  // the table is read to the end before the next request's writes
    }
}

template <int DPL, int LPO, bool SPARSE>
int serve_shape(const agn_log &log, const agn_read &req, const agn_result &out, const TagServe &sv,
                hipStream_t st) {
    const unsigned blocks = grid_for(req.n_req, 4, 0x7fffffffu);  // one wave per request
    hipLaunchKernelGGL((k_bcounter_serve<DPL, LPO, SPARSE>), dim3(blocks), dim3(256), 0, st, log,
                       req, out, sv);
    AGN_HIP(hipGetLastError());
    return AGN_OK;
}

// the AGN_DISPATCH_SHAPES rows with LPO <= 8
template <bool SPARSE>
int serve_dispatch(const agn_log &log, const agn_read &req, const agn_result &out,
                   const TagServe &sv, hipStream_t st) {
#define AGN_L(DPL, LPO) serve_shape<DPL, LPO, SPARSE>(log, req, out, sv, st)
    switch (log.n_dcs) {
        case 1: return AGN_L(1, 1);
        case 2: return AGN_L(2, 1);
        case 3: return AGN_L(3, 1);
        case 4: return AGN_L(4, 1);
        case 5: return AGN_L(5, 1);
        case 6: return AGN_L(6, 1);
        case 7: return AGN_L(7, 1);
        case 8: return AGN_L(8, 1);
        default: break;
    }
    if (log.n_dcs <= 16) return AGN_L(8, 2);
    if (log.n_dcs <= 32) return AGN_L(8, 4);
    return AGN_L(8, 8);
#undef AGN_L
}

}  // namespace

bool bcounter_serve_supported(const agn_log &shape, bool) {
    return shape.crdt_type == AGN_COUNTER_B && shape.n_dcs >= 1 && shape.n_dcs <= 64;
}

int launch_bcounter_serve(const agn_log &log, const agn_read &req, const agn_result &out,
                          const TagServe &sv, hipStream_t st) {
    if (req.n_req == 0) return AGN_OK;
    const bool sparse = log.oc_mask || req.R_mask || req.sct_mask || out.lastct_mask;
    if (!bcounter_serve_supported(log, sparse)) return AGN_ENOTSUP;
    if (!sv.c.state_tag || !sv.c.state_tok || !sv.c.state_ctl || !sv.sct || !sv.ign || !sv.base ||
        !sv.first || !sv.status || !sv.prune || req.sct != sv.sct || req.sct_mask != sv.sctm ||
        (sv.c.clock_mask && !sv.sctm))
        return fail(AGN_EINVAL, "counter_b fused read: incomplete TagServe");
    // A masked log over a dense cache (agn_read_cached: log.oc_mask alone, no
    // sctm / R_mask / lastct_mask) runs the SPARSE kernel with those rows
    // null, as the sequence runs k_bcounter: the lookup, the filter and the
    // store read a null mask as "every DC".
    return sparse ? serve_dispatch<true>(log, req, out, sv, st)
                  : serve_dispatch<false>(log, req, out, sv, st);
}

int launch_bcounter(const agn_log &log, const agn_read &req, const agn_result &out,
                    hipStream_t st) {
    if (req.n_req == 0) return AGN_OK;
    // base_value without base_off names AGN_SS_STATE references into
    // base_tag / base_tok: both arrays are required for them
    if (!req.base_off && req.base_value && (!req.base_tag || !req.base_tok))
        return fail(AGN_EINVAL, "counter_b read: base_value (state references) without base_tag/base_tok");
    const bool sparse = log.oc_mask || req.R_mask || req.sct_mask || out.lastct_mask;
    return sparse ? dispatch<true>(log, req, out, st) : dispatch<false>(log, req, out, st);
}

}  // namespace agn
