// oplog_load.hip -- the device side of agn_oplog_load (recovery): a device log
// (agn_log_ingest's CSR output, or another op log's segmented view) moved into
// the segments of a pristine engine-owned op log without a per-entry byte
// crossing PCIe.  The host side (oplog.hip, agn_oplog_load) does O(keys) work
// between the two passes here:
//
//   k_load_index  per key: length, token length, ListLen, first id and
//                 whether the ids are consecutive (key_id0), last id (the op
//                 counter), id validity, the DC set its entries share
//                 (key_mask), the slots its segment and token segment take.
//   scans         (hipcub) slots -> segment starts; their totals are all the
//                 host needs to refuse, or to allocate arenas of that size.
//   k_load_keys   key_off / key_len / key_id0 / key_lcap / key_mask, and the
//                 live starts of the host's per-key records.
//   k_load_copy   per key: every entry array of the key is one contiguous run
//                 in both layouts (len * D * 8 bytes of rows, len * 8 of txid,
//                 len * 4 of op_id, ...); each run moves with 16-byte
//                 lane-contiguous non-temporal loads and stores, four loads in
//                 flight before the first store.  rem_off is rebased onto the
//                 destination token segment.  The host fills its per-key
//                 metadata from the records while this pass runs.
//
// Both passes give a key G = 4, 16 or 64 lanes (the host picks G from the
// log's mean key length), so a wave carries 16 short keys, 4 medium ones or
// one long key: short keys do not each cost a wave's latency, and a 64-entry
// D = 8 key is the 4 KiB-per-wave shape of the copy probe (tools/bwprobe.hip).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "serve.hpp"

namespace agn {
namespace {

// 16 bytes that need only 4-byte alignment: a segment starts 8-byte (rows,
// txid, eff, tokens) or 4-byte (op_id, tag) aligned on either side, and source
// and destination differ in their offset within a 16-byte unit (odd D: 24-byte
// rows at D = 3).  Stores are aligned by a head of up to three dwords; the
// loads then take whatever alignment the source has (global_load_dwordx4
// needs dword alignment only).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(4)));

// n dwords from s to d (no overlap), by the G lanes of a group (gl = lane in
// the group).  Head: dwords up to d's 16-byte boundary; body: 16-byte
// accesses, G lanes contiguous (G = 64: eight whole 128-byte lines per store
// instruction), four loads before the first store; tail: the last dwords.
template <int G>
__device__ __forceinline__ void copy_run(const uint32_t *__restrict__ s, uint32_t *__restrict__ d,
                                         uint64_t n, int gl) {
    static_assert(G >= 4, "head and tail use up to three lanes");
    uint64_t h = ((16u - (uint32_t)((uintptr_t)d & 15u)) & 15u) >> 2;
    if (h > n) h = n;
    if ((uint64_t)gl < h) __builtin_nontemporal_store(__builtin_nontemporal_load(s + gl), d + gl);
    s += h;
    d += h;
    n -= h;
    const uint64_t nv = n >> 2;
    const u32x4_u *sv = reinterpret_cast<const u32x4_u *>(s);
    u32x4 *dv = reinterpret_cast<u32x4 *>(d);
    for (uint64_t i = (uint64_t)gl; i < nv; i += 4 * G) {
        u32x4 x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j * G < nv) x[j] = __builtin_nontemporal_load(sv + i + j * G);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j * G < nv) __builtin_nontemporal_store(x[j], dv + i + j * G);
    }
    const uint64_t t = n & 3u, o = nv << 2;
    if ((uint64_t)gl < t)
        __builtin_nontemporal_store(__builtin_nontemporal_load(s + o + gl), d + o + gl);
}

template <int G, class T>
__device__ __forceinline__ void copy_arr(const T *s, T *d, uint64_t n_elems, int gl) {
    static_assert(sizeof(T) % 4 == 0, "dword arrays");
    copy_run<G>(reinterpret_cast<const uint32_t *>(s), reinterpret_cast<uint32_t *>(d),
                n_elems * (sizeof(T) / 4), gl);
}

template <int G>
__device__ __forceinline__ uint32_t group_and(uint32_t v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v &= (uint32_t)__shfl_xor((int)v, m, AGN_WAVE);
    return v;
}

// Per key k (G lanes): the records of LoadIndex.  bad: bit 0 an invalid id
// (0, AGN_ID0_NONE, or smaller than its predecessor), bit 1 a length or
// ListLen beyond 32 bits, bit 2 removal tokens without a rem_tok array.
template <int G>
__global__ void __launch_bounds__(256) k_load_index(
    const uint64_t *__restrict__ key_off, const uint64_t *__restrict__ key_len,
    const uint32_t *__restrict__ op_id, const uint64_t *__restrict__ oc_mask, uint32_t W,
    uint32_t D, const uint32_t *__restrict__ rem_off, bool has_tok, uint64_t K,
    uint32_t init_slots, LoadIndex o) {
    const int gl = threadIdx.x & (G - 1);
    const uint64_t k = (uint64_t)blockIdx.x * (256 / G) + (threadIdx.x / G);
    const bool live = k < K;  // every lane stays for the group reductions
    uint64_t a = 0, n = 0;
    if (live) {
        a = key_off[k];
        n = key_n(key_off, key_len, k);
    }
    uint32_t bad = 0;
    if (n > 0xfffffffeull) {
        bad = 2;
        n = 0;
    }
    uint32_t first = 0;
    uint64_t m0 = 0;
    if (n) {
        first = op_id[a];
        if (o.umask) m0 = oc_mask[a * W] & low_bits(D);
    }
    uint32_t ok = 1, cons = 1, same = 1;
    for (uint64_t p = (uint64_t)gl; p < n; p += G) {
        const uint32_t id = op_id[a + p];
        const uint32_t prev = p ? op_id[a + p - 1] : id;
        ok &= (uint32_t)(id != 0u && id != AGN_ID0_NONE && id >= prev);
        cons &= (uint32_t)((uint64_t)id == (uint64_t)first + p);
        if (o.umask) same &= (uint32_t)((oc_mask[(a + p) * W] & low_bits(D)) == m0);
    }
    const uint32_t all = group_and<G>(ok | (cons << 1) | (same << 2));
    if (!live || gl != 0) return;
    uint64_t lc = 0;
    if (n) {
        lc = init_slots;
        while (lc < n) lc *= 2;
        if (lc > 0xfffffffeull) {
            bad |= 2u;
            lc = 0;
        }
    }
    if (!(all & 1u)) bad |= 1u;
    const uint32_t tl = (n && rem_off) ? rem_off[a + n] - rem_off[a] : 0u;
    if (tl && !has_tok) bad |= 4u;
    o.len[k] = (uint32_t)n;
    o.tlen[k] = tl;
    o.lcap[k] = (uint32_t)lc;
    // slots: ListLen + 1 per non-empty key; tokens: 16 doubled up to the key's
    o.slots[k] = n ? lc + 1 : 0ull;
    if (o.tslots) {
        uint64_t c = 0;
        if (tl) {
            c = 16;
            while (c < tl) c *= 2;
        }
        o.tslots[k] = c;
    }
    o.id0[k] = (n && (all & 2u)) ? first : AGN_ID0_NONE;
    o.last[k] = n ? op_id[a + n - 1] : 0u;
    if (o.umask) o.umask[k] = (n && (all & 4u)) ? m0 : 0ull;
    if (bad) atomicOr(o.bad, bad);  // refusals only
}

struct CopyDst {  // the fresh arenas (null where the type lacks the array)
    uint64_t *oc, *mask, *txid, *add, *tok;
    int64_t *eff;
    uint32_t *op_id, *tag, *rem_off;
};

// Key k's entries [a, a + len) of src into [ds, ds + len) of dst, its tokens
// into [dt, dt + tlen); rem_off[ds .. ds + len] rebased onto dt.
template <int G>
__global__ void __launch_bounds__(256) k_load_copy(
    const uint64_t *__restrict__ key_off, const uint64_t *__restrict__ s_oc,
    const uint64_t *__restrict__ s_mask, const uint32_t *__restrict__ s_op_id,
    const uint64_t *__restrict__ s_txid, const int64_t *__restrict__ s_eff,
    const uint32_t *__restrict__ s_tag, const uint64_t *__restrict__ s_add,
    const uint32_t *__restrict__ s_rem_off, const uint64_t *__restrict__ s_tok, CopyDst b,
    uint32_t D, uint32_t W, uint64_t K, const uint32_t *__restrict__ len,
    const uint32_t *__restrict__ tlen, const uint64_t *__restrict__ lstart,
    const uint64_t *__restrict__ ltstart) {
    const int gl = threadIdx.x & (G - 1);
    const uint64_t k = (uint64_t)blockIdx.x * (256 / G) + (threadIdx.x / G);
    if (k >= K) return;
    const uint64_t n = len[k];
    if (n == 0) return;
    const uint64_t a = key_off[k], ds = lstart[k];
    copy_arr<G>(s_oc + a * D, b.oc + ds * D, n * D, gl);
    if (b.mask) copy_arr<G>(s_mask + a * W, b.mask + ds * W, n * W, gl);
    copy_arr<G>(s_op_id + a, b.op_id + ds, n, gl);
    if (s_txid) {
        copy_arr<G>(s_txid + a, b.txid + ds, n, gl);
    } else {  // txid NULL = none
        for (uint64_t j = (uint64_t)gl; j < n; j += G) b.txid[ds + j] = 0ull;
    }
    if (b.eff) copy_arr<G>(s_eff + a, b.eff + ds, n, gl);
    if (b.tag) {
        copy_arr<G>(s_tag + a, b.tag + ds, n, gl);
        copy_arr<G>(s_add + a, b.add + ds, n, gl);
        const uint32_t ts = s_rem_off[a], dt = (uint32_t)ltstart[k];
        for (uint64_t j = (uint64_t)gl; j <= n; j += G)
            b.rem_off[ds + j] = s_rem_off[a + j] - ts + dt;
        const uint64_t nt = tlen[k];
        if (nt) copy_arr<G>(s_tok + ts, b.tok + dt, nt, gl);
    }
}

__global__ void __launch_bounds__(256) k_load_keys(
    uint64_t K, const uint32_t *__restrict__ len, const uint32_t *__restrict__ id0,
    const uint32_t *__restrict__ lcap, const uint64_t *__restrict__ lstart,
    const uint64_t *__restrict__ ltstart, const uint64_t *__restrict__ umask,
    uint32_t *__restrict__ rec_lstart, uint32_t *__restrict__ rec_ltstart,
    uint64_t *__restrict__ key_off, uint64_t *__restrict__ key_len,
    uint32_t *__restrict__ key_id0, uint32_t *__restrict__ key_lcap,
    uint64_t *__restrict__ key_mask) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    key_off[k] = lstart[k];
    rec_lstart[k] = (uint32_t)lstart[k];
    rec_ltstart[k] = ltstart ? (uint32_t)ltstart[k] : 0u;
    key_len[k] = len[k];
    key_id0[k] = id0[k];
    key_lcap[k] = lcap[k];
    if (key_mask) key_mask[k] = umask[k];
}

// Lanes per key from the mean run length in 16-byte units (u): one lane
// should find about four units.
inline int group_for(uint64_t units, uint64_t K) {
    const uint64_t u = units / (K ? K : 1);
    return u >= 128 ? 64 : u >= 16 ? 16 : 4;
}

}  // namespace

size_t load_scan_bytes(uint64_t K) {
    size_t b = 0;
    if (hipcub::DeviceScan::InclusiveSum(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr,
                                         (int)K) != hipSuccess)
        return 0;
    return b ? b : 1;
}

int launch_load_index(const agn_log &s, uint32_t init_slots, const LoadIndex &o, void *scan_tmp,
                      size_t scan_bytes, hipStream_t st) {
    const uint64_t K = s.n_keys;
    if (K == 0) return AGN_OK;
    if (K > 0x7fffffffull) return fail(AGN_ENOTSUP, "oplog_load: %llu keys", (unsigned long long)K);
    const uint32_t W = n_words(s.n_dcs);
    // 4 bytes of op_id per entry: four 16-byte units per lane = 16 entries
    const int G = group_for(s.n_entries / 4, K);
    const uint64_t nb = (K + 256 / G - 1) / (256 / G);
    if (nb > 0x7fffffffull) return fail(AGN_ENOTSUP, "oplog_load: %llu keys", (unsigned long long)K);
#define AGN_LOAD_INDEX(GG)                                                                       \
    k_load_index<GG><<<(unsigned)nb, 256, 0, st>>>(s.key_off, s.key_len, s.op_id, s.oc_mask, W, \
                                                   s.n_dcs, s.rem_off, s.rem_tok != nullptr, K,  \
                                                   init_slots, o)
    if (G == 64) AGN_LOAD_INDEX(64);
    else if (G == 16) AGN_LOAD_INDEX(16);
    else AGN_LOAD_INDEX(4);
#undef AGN_LOAD_INDEX
    AGN_HIP(hipGetLastError());
    // slots -> inclusive sums, in place: behind the caller's zero word
    // (o.slots = starts + 1) they are the segment starts, the total last
    AGN_HIP(hipcub::DeviceScan::InclusiveSum(scan_tmp, scan_bytes, o.slots, o.slots, (int)K, st));
    if (o.tslots)
        AGN_HIP(hipcub::DeviceScan::InclusiveSum(scan_tmp, scan_bytes, o.tslots, o.tslots, (int)K,
                                                 st));
    return AGN_OK;
}

int launch_load_copy(const agn_log &s, const agn_log &d, uint64_t n_entries, const uint32_t *len,
                     const uint32_t *tlen, const uint64_t *lstart, const uint64_t *ltstart,
                     hipStream_t st) {
    const uint64_t K = s.n_keys;
    if (K == 0 || n_entries == 0) return AGN_OK;
    const uint32_t D = s.n_dcs, W = n_words(D);
    CopyDst b;
    b.oc = const_cast<uint64_t *>(d.oc);
    b.mask = const_cast<uint64_t *>(d.oc_mask);
    b.txid = const_cast<uint64_t *>(d.txid);
    b.add = const_cast<uint64_t *>(d.add_tok);
    b.tok = const_cast<uint64_t *>(d.rem_tok);
    b.eff = const_cast<int64_t *>(d.eff);
    b.op_id = const_cast<uint32_t *>(d.op_id);
    b.tag = const_cast<uint32_t *>(d.tag);
    b.rem_off = const_cast<uint32_t *>(d.rem_off);
    const int G = group_for(n_entries * D / 2, K);  // rows: D * 8 bytes per entry
    const uint64_t nb = (K + 256 / G - 1) / (256 / G);
    if (nb > 0x7fffffffull) return fail(AGN_ENOTSUP, "oplog_load: %llu keys", (unsigned long long)K);
#define AGN_LOAD_COPY(GG)                                                                        \
    k_load_copy<GG><<<(unsigned)nb, 256, 0, st>>>(s.key_off, s.oc, s.oc_mask, s.op_id, s.txid,   \
                                                  s.eff, s.tag, s.add_tok, s.rem_off, s.rem_tok, \
                                                  b, D, W, K, len, tlen, lstart, ltstart)
    if (G == 64) AGN_LOAD_COPY(64);
    else if (G == 16) AGN_LOAD_COPY(16);
    else AGN_LOAD_COPY(4);
#undef AGN_LOAD_COPY
    AGN_HIP(hipGetLastError());
    return AGN_OK;
}

int launch_load_keys(uint64_t K, const uint32_t *len, const uint32_t *id0, const uint32_t *lcap,
                     const uint64_t *lstart, const uint64_t *ltstart, const uint64_t *umask,
                     uint32_t *rec_lstart, uint32_t *rec_ltstart, uint64_t *key_off,
                     uint64_t *key_len, uint32_t *key_id0, uint32_t *key_lcap,
                     uint64_t *key_mask, hipStream_t st) {
    if (K == 0) return AGN_OK;
    const uint64_t nb = (K + 255) / 256;
    if (nb > 0x7fffffffull) return fail(AGN_ENOTSUP, "oplog_load: %llu keys", (unsigned long long)K);
    k_load_keys<<<(unsigned)nb, 256, 0, st>>>(K, len, id0, lcap, lstart, ltstart, umask,
                                              rec_lstart, rec_ltstart, key_off, key_len, key_id0,
                                              key_lcap, key_mask);
    AGN_HIP(hipGetLastError());
    return AGN_OK;
}

}  // namespace agn
