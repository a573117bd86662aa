// tagorder.hip — value-order labels for register_lww (host code).
//
// update/2 of antidote_crdt_register_lww is max(Effect, State) over {Ts,
// Value} in Erlang term order, and the device compares tag ids, which are
// interner ids in arrival order.  The term order travels beside the ids as
// u64 labels (agn_oplog_tag_order, the tie rule of mat_lww.hip).  This object
// allocates them: it holds the tags in sorted order -- the caller finds a new
// value's position with its own comparator -- and gives each a label strictly
// between its neighbours', reassigning all of them evenly when a gap closes.
// Depends on the public header alone, so that it also builds as plain C++
// for a host sanitizer run (tests/tagorder_driver.cpp).
#include <new>
#include <unordered_map>
#include <vector>

#include "../../include/antidote_gpu.h"

namespace agn {
int fail(int code, const char *fmt, ...);
}

struct agn_tagorder {
    std::vector<uint32_t> tags;     // sorted position -> tag id
    std::vector<uint64_t> labels;   // sorted position -> label
    std::unordered_map<uint32_t, uint64_t> by_id;  // tag id -> label
};

using agn::fail;

extern "C" {

int agn_tagorder_create(agn_tagorder **out) {
    if (!out) return fail(AGN_EINVAL, "tagorder_create: null out");
    *out = new (std::nothrow) agn_tagorder;
    if (!*out) return fail(AGN_ENOMEM, "tagorder_create");
    return AGN_OK;
}

int agn_tagorder_destroy(agn_tagorder *o) {
    delete o;
    return AGN_OK;
}

int agn_tagorder_size(const agn_tagorder *o, uint32_t *n) {
    if (!o || !n) return fail(AGN_EINVAL, "tagorder_size: null argument");
    *n = (uint32_t)o->tags.size();
    return AGN_OK;
}

int agn_tagorder_at(const agn_tagorder *o, uint32_t pos, uint32_t *tag) {
    if (!o || !tag) return fail(AGN_EINVAL, "tagorder_at: null argument");
    if (pos >= o->tags.size())
        return fail(AGN_EINVAL, "tagorder_at: position %u of %zu", pos, o->tags.size());
    *tag = o->tags[pos];
    return AGN_OK;
}

int agn_tagorder_insert(agn_tagorder *o, uint32_t pos, uint32_t tag, int *relabelled) {
    if (!o) return fail(AGN_EINVAL, "tagorder_insert: null order");
    if (relabelled) *relabelled = 0;
    const size_t n0 = o->tags.size();
    if (pos > n0) return fail(AGN_EINVAL, "tagorder_insert: position %u of %zu", pos, n0);
    if (tag == AGN_TAG_INVALID) return fail(AGN_EINVAL, "tagorder_insert: AGN_TAG_INVALID");
    if (n0 >= 0xfffffffeull) return fail(AGN_ECAPACITY, "tagorder_insert: %zu tags", n0);
    if (o->by_id.count(tag)) return fail(AGN_EINVAL, "tagorder_insert: tag %u twice", tag);
    const uint64_t lo = pos ? o->labels[pos - 1] : 0ull;
    const uint64_t hi = pos < n0 ? o->labels[pos] : UINT64_MAX;
    const uint64_t mid = lo + (hi - lo) / 2;
    // even spacing over [1, 2^64 - 2] when the gap has closed
    const bool even = mid == lo;
    const uint64_t n = n0 + 1, step = UINT64_MAX / (n + 1);
    try {
        o->tags.reserve(n);  // room first: a failure leaves the order as it was
        o->labels.reserve(n);
        o->by_id[tag] = mid;
    } catch (const std::bad_alloc &) {
        return fail(AGN_ENOMEM, "tagorder_insert");
    }
    o->tags.insert(o->tags.begin() + pos, tag);
    o->labels.insert(o->labels.begin() + pos, mid);
    if (!even) return AGN_OK;
    for (uint64_t i = 0; i < n; ++i) {
        o->labels[i] = (i + 1) * step;
        o->by_id.find(o->tags[i])->second = o->labels[i];
    }
    if (relabelled) *relabelled = 1;
    return AGN_OK;
}

int agn_tagorder_labels(const agn_tagorder *o, uint32_t first, uint32_t n, uint64_t *labels) {
    if (!o || (n && !labels)) return fail(AGN_EINVAL, "tagorder_labels: null argument");
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t id = (uint64_t)first + i;
        uint64_t l = 0;
        if (id <= 0xffffffffull) {
            const auto it = o->by_id.find((uint32_t)id);
            if (it != o->by_id.end()) l = it->second;
        }
        labels[i] = l;
    }
    return AGN_OK;
}

}  // extern "C"
