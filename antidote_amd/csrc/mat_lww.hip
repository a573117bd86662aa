// mat_lww.hip — batched clocksi_materializer:materialize/4 for
// antidote_crdt_register_lww on gfx950 (one wave per key, grid-stride).
//
// Reference: materialize/4 src/clocksi_materializer.erl:89-101,
// apply_operations :113-121 with register_lww update(Effect, State) =
// max(Effect, State) over {Ts, Value} (antidote_crdt 0.1.2, restated in
// SURVEY.md §8(a) a5.4; parity-unpinned beyond the sequential assign).  The
// snapshot filter is filter.hpp, the bookkeeping (NewLastOp, Count, LastOpCt,
// the error position) that of mat_counter.hip.
//   candidates = the base pair (if any) and every included entry whose tag is
//           valid; wts = their largest ts, T = the distinct tags at wts
//   state = (wts, the tag of T with the largest (label(tag), tag)), unsigned
//           and lexicographic; label(tag) = order[tag] below the table's
//           length, else 0 (LwwOrder: the engine-owned log's value-order
//           table, agn_oplog_tag_order; no table: every label 0, so the
//           largest tag id wins as it always did)
//   AGN_F_TS_TIE: |T| > 1 and some tag of T has label 0 (tag ids are interner
//           ids, not Erlang term order: only labels settle a tie exactly)
// Every lane keeps the best (ts, tag) of the included ops it saw plus an
// "unlabelled tag tied at my best ts" bit; the wave then reduces in two steps,
// the u64 maximum of ts and the u32 maximum of tag among the lanes at that ts.
// Only when those lanes disagree on the tag do they load their labels
// (lww_settle, behind both reductions): a u64 maximum of the label, then the
// u32 maximum of tag among the lanes at that label.
//
// ts / tag loads: a chunk's ts and tag do not depend on its verdict.  EARLY
// issues them with the chunk's rows for every valid op (8*D + 12 bytes per op);
// the late form loads them for the included ops only, after the verdict (8*D
// bytes per op + 12 per included op, one more dependent round trip per chunk).
// The default is the early form: cfg2's shape (10M keys x 64 ops, D = 8, cold,
// 32 % included) 15.90 ms against 16.04 ms late and 14.32 ms for k_counter at
// 8*D + 8 (scripts/ab_lww.py); AGN_LWW_LOAD=late selects the
// other (A/B knob).
// Per key: 16 (key_off pair) + 8*D (R) + 8*D (LastOpCt) + 20 (hole, count,
// flags, err_pos) + 16 (out_off pair) + 4 (out_n) + 12 (the pair).
#include <cstdlib>

#include "cache_dev.hpp"
#include "filter.hpp"
#include "tags_serve.hpp"

namespace agn {
namespace {

__device__ __forceinline__ uint64_t lww_label(const LwwOrder &ord, uint32_t tag) {
    return tag < ord.n ? ord.label[tag] : 0ull;
}

// Two tags at one ts (rare: two DCs assigning in the same microsecond).  Bit
// 0: `tag` beats `btag`; bit 1: one of them has no label.
__device__ __forceinline__ uint32_t lww_tie(const LwwOrder &ord, uint32_t tag, uint32_t btag) {
    const uint64_t la = lww_label(ord, tag), lb = lww_label(ord, btag);
    return ((la > lb || (la == lb && tag > btag)) ? 1u : 0u) |
           ((la == 0ull || lb == 0ull) ? 2u : 0u);
}
// Out of line: the label loads and their addresses then take no register of
// the fold loop.  k_lww's late form needs that to keep its waves per SIMD
// (inline, <6, 1, dense, late> goes from 79 to 81 VGPRs and from six waves to
// five).  The early form and k_lww_serve are the other way round (out of
// line, <8, 1, dense, early> takes 4 more bytes of scratch and three serve
// shapes lose a wave to the call's register convention), so they inline.
__device__ __attribute__((noinline)) uint32_t lww_tie_ool(const uint64_t *label, uint32_t n,
                                                          uint32_t tag, uint32_t btag) {
    LwwOrder ord;
    ord.label = label;
    ord.n = n;
    return lww_tie(ord, tag, btag);
}

// One more candidate into a lane's running maximum.  Labels are loaded only
// where two tags meet at the lane's best ts; `unl`: one of them had none.
template <bool OOL>
__device__ __forceinline__ void lww_take(bool c, uint64_t ts, uint32_t tag, const LwwOrder &ord,
                                         bool &have, uint64_t &bts, uint32_t &btag, bool &unl) {
    if (!c) return;
    if (!have || ts > bts) {
        bts = ts;
        btag = tag;
        unl = false;
    } else if (ts == bts && tag != btag) {
        const uint32_t r = OOL ? lww_tie_ool(ord.label, ord.n, tag, btag) : lww_tie(ord, tag, btag);
        unl = unl || (r & 2u) != 0u;
        if (r & 1u) btag = tag;
    }
    have = true;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, AGN_WAVE);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = umax64(v, shfl_xor_u64(v, m));
    return v;
}

// Behind the two reductions (wts, and wtag = the largest tag among the lanes
// at wts): when those lanes disagree on the tag -- wave-uniform, rare -- each
// loads its tag's label and the wave takes the largest (label, tag).  The
// no-tie path loads nothing here.
__device__ __forceinline__ void lww_settle(const LwwOrder &ord, bool at, uint32_t btag, bool unl,
                                           uint32_t &wtag, bool &tied) {
    tied = ballot(at && unl) != 0ull;
    if (ballot(at && btag != wtag) != 0ull) {
        const uint64_t lb = at ? lww_label(ord, btag) : 0ull;
        const uint64_t wl = wave_max_u64(lb);
        wtag = wave_max_u32((at && lb == wl) ? btag : 0u);
        tied = tied || ballot(at && lb == 0ull) != 0ull;
    }
}

// The one-lane-per-op shapes are held to k_counter's five waves per SIMD (96
// VGPRs; left alone the kernel takes 100 and runs four).
template <int DPL, int LPO, bool SPARSE, bool EARLY>
__global__ __launch_bounds__(256, (LPO == 1 ? 5 : 1)) void k_lww(agn_log log, agn_read req,
                                                                 agn_result out, LwwOrder ord) {
    using F = KeyFilter<DPL, LPO, SPARSE>;
    __shared__ uint64_t stage[4][DPL][AGN_WAVE];
    const int w = threadIdx.x >> 6;
    const uint64_t nw = (uint64_t)gridDim.x * 4u;

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

        F f;
        f.init(log, req, i);
        bool have = false, unl = false;
        uint64_t bts = 0;
        uint32_t btag = 0;
        uint32_t cnt = 0;
        int64_t first_err = -1;
        for (uint64_t b = 0; b < n; b += F::S::OPI) {
            const uint64_t e = off + b + (uint64_t)f.slot;
            uint64_t ts = 0;
            uint32_t tg = AGN_TAG_INVALID;
            if (EARLY && f.sub == 0 && b + (uint64_t)f.slot < n) {
                ts = log.add_tok[e];
                tg = log.tag[e];
            }
            bool valid;
            const bool incl = f.step(log, off, n, b, valid);
            const bool lead = incl && f.sub == 0;
            if (!EARLY && lead) {
                ts = log.add_tok[e];
                tg = log.tag[e];
            }
            const bool bad = lead && tg == AGN_TAG_INVALID;
            cnt += (uint32_t)__builtin_popcountll(ballot(lead));
            if (first_err < 0) {
                const uint64_t be = ballot(bad);
                if (be) first_err = (int64_t)b + (int64_t)(__builtin_ctzll(be) / LPO);
            }
            lww_take<!EARLY>(lead && !bad, ts, tg, ord, have, bts, btag, unl);
        }

        // the base state: at most one pair (the first of more), through the
        // CSR or an AGN_SS_STATE(start, pairs) reference in base_value
        if (lane == 0 && req.base_tag != nullptr && req.base_tok != nullptr) {
            uint64_t b0 = 0;
            uint32_t B = 0;
            if (req.base_off) {
                b0 = req.base_off[i];
                B = (uint32_t)(req.base_off[i + 1] - b0);
            } else if (req.base_value) {
                const uint64_t ref = (uint64_t)req.base_value[i];
                b0 = AGN_SS_STATE_START(ref);
                B = AGN_SS_STATE_PAIRS(ref);
            }
            if (B != 0u) lww_take<!EARLY>(true, req.base_tok[b0], req.base_tag[b0], ord, have, bts, btag, unl);
        }

        const bool any = ballot(have) != 0ull;
        const uint64_t wts = wave_max_u64(have ? bts : 0ull);
        const bool at = have && bts == wts;
        uint32_t wtag = wave_max_u32(at ? btag : 0u);
        bool tied;
        lww_settle(ord, at, btag, unl, wtag, tied);

        const bool ct_ign = f.sct_ign && cnt == 0u;
        f.write_ct(stage[w], out, i, ct_ign);

        if (lane == 0) {
            int64_t hole;
            if (f.first_excl >= 0) hole = (int64_t)log.op_id[off + (uint64_t)f.first_excl] - 1;
            else hole = n ? (int64_t)log.op_id[off + n - 1] : 0;
            uint32_t fl = 0;
            if (cnt) fl |= AGN_F_NEWSS;
            if (ct_ign) fl |= AGN_F_CT_IGNORE;
            uint32_t n_live = 0;
            if (first_err >= 0) {
                fl |= AGN_F_ERR_UNEXPECTED;
            } else if (any) {
                n_live = 1;
                if (tied) fl |= AGN_F_TS_TIE;
                const uint64_t o = out.out_off[i];
                if (out.out_off[i + 1] - o == 0ull) {
                    fl |= AGN_F_ERR_CAPACITY;
                } else {
                    out.out_tag[o] = wtag;
                    out.out_tok[o] = wts;
                }
            }
            out.hole[i] = hole;
            out.count[i] = cnt;
            out.flags[i] = fl;
            out.err_pos[i] =
                first_err >= 0 ? (uint32_t)(off + (uint64_t)first_err) : 0xffffffffu;
            out.out_n[i] = n_live;
        }
    }
}

template <int DPL, int LPO, bool SPARSE, bool EARLY>
int launch_shape(const agn_log &log, const agn_read &req, const agn_result &out,
                 hipStream_t st, LwwOrder ord) {
    const unsigned blocks = grid_for(req.n_req, 4, 0x7fffffffu);  // one wave per request
    hipLaunchKernelGGL((k_lww<DPL, LPO, SPARSE, EARLY>), dim3(blocks), dim3(256), 0, st, log,
                       req, out, ord);
    AGN_HIP(hipGetLastError());
    return AGN_OK;
}

template <bool SPARSE, bool EARLY>
int dispatch(const agn_log &log, const agn_read &req, const agn_result &out, hipStream_t st,
             LwwOrder ord) {
#define AGN_L(DPL, LPO) launch_shape<DPL, LPO, SPARSE, EARLY>(log, req, out, st, ord)
    AGN_DISPATCH_SHAPES(log.n_dcs, AGN_L)
#undef AGN_L
}

// The fused cached read (tags_serve.hpp): per request, one wave runs
// get_from_snapshot_cache (materializer_vnode.erl:384-413), k_lww's fold from
// the hit slot's pair, and materialize_snapshot's store (:466-509) of the
// winning pair.  The lookup's verdict and base reference stay in registers;
// LastOpCt (+ its mask word) and the pair go to the store through LDS, so no
// result array -- pinned host memory in the batcher -- is read back.  Every
// value the store branches on (hole, count, flags) is computed wave-uniformly.
template <int DPL, int LPO, bool SPARSE>
__global__ __launch_bounds__(256) void k_lww_serve(agn_log log, agn_read req, agn_result out,
                                                   TagServe sv, LwwOrder ord) {
    using F = KeyFilter<DPL, LPO, SPARSE>;
    constexpr int DC = F::S::DC;
    static_assert(DC <= AGN_WAVE, "one lane per LastOpCt column");
    __shared__ uint64_t stage[4][DPL][AGN_WAVE];
    __shared__ uint64_t Sct[4][DC + 1];  // LastOpCt row + mask word for the store
    __shared__ uint64_t Ptok[4];         // the winning pair
    __shared__ uint32_t Ptag[4];
    const int w = threadIdx.x >> 6;
    const uint64_t nw = (uint64_t)gridDim.x * 4u;
    const uint32_t D = log.n_dcs, W = n_words(D);
    const int lane = lane_id();
    const Grp<AGN_WAVE> g;

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

        F f;
        f.init_ign(log, req, i, lk.ign != 0);
        bool have = false, unl = false;
        uint64_t bts = 0;
        uint32_t btag = 0;
        uint32_t cnt = 0;
        int64_t first_err = -1;
        for (uint64_t b = 0; b < n; b += F::S::OPI) {
            const uint64_t e = off + b + (uint64_t)f.slot;
            uint64_t ts = 0;
            uint32_t tg = AGN_TAG_INVALID;
            if (f.sub == 0 && b + (uint64_t)f.slot < n) {
                ts = log.add_tok[e];
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
            lww_take<false>(lead && !bad, ts, tg, ord, have, bts, btag, unl);
        }

        // the base state: the hit slot's pair in the arena (at most one)
        if (lane == 0 && AGN_SS_STATE_PAIRS((uint64_t)lk.base) != 0u) {
            const uint64_t b0 = AGN_SS_STATE_START((uint64_t)lk.base);
            lww_take<false>(true, sv.c.state_tok[b0], sv.c.state_tag[b0], ord, have, bts, btag, unl);
        }

        const bool any = ballot(have) != 0ull;
        const uint64_t wts = wave_max_u64(have ? bts : 0ull);
        const bool at = have && bts == wts;
        uint32_t wtag = wave_max_u32(at ? btag : 0u);
        bool tied;
        lww_settle(ord, at, btag, unl, wtag, tied);

        const bool ct_ign = f.sct_ign && cnt == 0u;
        f.template write_ct<true>(stage[w], out, i, ct_ign, Sct[w]);

        int64_t hole;
        if (f.first_excl >= 0) hole = (int64_t)log.op_id[off + (uint64_t)f.first_excl] - 1;
        else hole = n ? (int64_t)log.op_id[off + n - 1] : 0;
        uint32_t fl = 0;
        if (cnt) fl |= AGN_F_NEWSS;
        if (ct_ign) fl |= AGN_F_CT_IGNORE;
        uint32_t n_live = 0;
        if (first_err >= 0) {
            fl |= AGN_F_ERR_UNEXPECTED;
        } else if (any) {
            n_live = 1;
            if (tied) fl |= AGN_F_TS_TIE;
            const uint64_t o = out.out_off[i];
            if (out.out_off[i + 1] - o == 0ull) {
                fl |= AGN_F_ERR_CAPACITY;
            } else if (lane == 0) {
                out.out_tag[o] = wtag;
                out.out_tok[o] = wts;
            }
        }
        if (lane == 0) {
            Ptag[w] = wtag;
            Ptok[w] = wts;
            out.hole[i] = hole;
            out.count[i] = cnt;
            out.flags[i] = fl;
            out.err_pos[i] =
                first_err >= 0 ? (uint32_t)(off + (uint64_t)first_err) : 0xffffffffu;
            out.out_n[i] = n_live;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const bool pr = ss_store_one<AGN_WAVE>(
            g, sv.c, key, n, lk.status, lk.first, sv.gc != nullptr && sv.gc[i] != 0, Sct[w],
            (SPARSE && out.lastct_mask != nullptr) ? &Sct[w][DC] : nullptr, hole, 0, cnt, fl,
            sv.thr, sv.thrm, &Ptag[w], &Ptok[w], n_live, dl);
        sv_mark(pr, dl);
    }
}

template <int DPL, int LPO, bool SPARSE>
int serve_shape(const agn_log &log, const agn_read &req, const agn_result &out, const TagServe &sv,
                hipStream_t st, LwwOrder ord) {
    const unsigned blocks = grid_for(req.n_req, 4, 0x7fffffffu);  // one wave per request
    hipLaunchKernelGGL((k_lww_serve<DPL, LPO, SPARSE>), dim3(blocks), dim3(256), 0, st, log, req,
                       out, sv, ord);
    AGN_HIP(hipGetLastError());
    return AGN_OK;
}

// the AGN_DISPATCH_SHAPES rows with LPO <= 8
template <bool SPARSE>
int serve_dispatch(const agn_log &log, const agn_read &req, const agn_result &out,
                   const TagServe &sv, hipStream_t st, LwwOrder ord) {
#define AGN_L(DPL, LPO) serve_shape<DPL, LPO, SPARSE>(log, req, out, sv, st, ord)
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

bool lww_serve_supported(const agn_log &shape, bool) {
    return shape.crdt_type == AGN_REGISTER_LWW && shape.n_dcs >= 1 && shape.n_dcs <= 64;
}

int launch_lww_serve(const agn_log &log, const agn_read &req, const agn_result &out,
                     const TagServe &sv, hipStream_t st, LwwOrder ord) {
    if (req.n_req == 0) return AGN_OK;
    const bool sparse = log.oc_mask || req.R_mask || req.sct_mask || out.lastct_mask;
    if (!lww_serve_supported(log, sparse)) return AGN_ENOTSUP;
    if (!sv.c.state_tag || !sv.c.state_tok || !sv.c.state_ctl || !sv.sct || !sv.ign || !sv.base ||
        !sv.first || !sv.status || !sv.prune || req.sct != sv.sct || req.sct_mask != sv.sctm ||
        (sv.c.clock_mask && !sv.sctm))
        return fail(AGN_EINVAL, "register_lww fused read: incomplete TagServe");
    // A masked log over a dense cache (agn_read_cached: log.oc_mask alone, no
    // sctm / R_mask / lastct_mask) runs the SPARSE kernel with those rows
    // null, as the sequence runs k_lww: the lookup, the filter and the store
    // read a null mask as "every DC".
    return sparse ? serve_dispatch<true>(log, req, out, sv, st, ord)
                  : serve_dispatch<false>(log, req, out, sv, st, ord);
}

int launch_lww(const agn_log &log, const agn_read &req, const agn_result &out, hipStream_t st,
               LwwOrder ord) {
    if (req.n_req == 0) return AGN_OK;
    // base_value without base_off names AGN_SS_STATE references into
    // base_tag / base_tok: both arrays are required for them
    if (!req.base_off && req.base_value && (!req.base_tag || !req.base_tok))
        return fail(AGN_EINVAL, "register_lww read: base_value (state references) without base_tag/base_tok");
    // AGN_LWW_LOAD=late loads ts / tag after the verdict (A/B)
    const bool late = [] {
        const char *v = AGN_KNOB("AGN_LWW_LOAD");
        return v && v[0] == 'l';
    }();
    const bool sparse = log.oc_mask || req.R_mask || req.sct_mask || out.lastct_mask;
    if (late) return sparse ? dispatch<true, false>(log, req, out, st, ord)
                            : dispatch<false, false>(log, req, out, st, ord);
    return sparse ? dispatch<true, true>(log, req, out, st, ord)
                  : dispatch<false, true>(log, req, out, st, ord);
}

}  // namespace agn
