// Stand-alone driver for antidote_amd/csrc/tagorder.hip (host code): built with
// the helper's source under -fsanitize=address,undefined and run as a program
// by tests/test_tagorder_cpu.py.  The same sequences as the Python tests: 2000
// random inserts against a sorted vector (the whole order and every label
// checked after each), the front-insert sequence that
// relabels at the 64th insert, back inserts and one middle gap to a relabel,
// labels over a range with holes, the error cases.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/antidote_gpu.h"

namespace agn {
int fail(int code, const char *, ...) { return code; }
}  // namespace agn

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// order and labels against the model: same tags, labels strictly increasing,
// in [1, 2^64 - 2]
static void check_order(agn_tagorder *o, const std::vector<uint32_t> &want) {
    uint32_t n = 0;
    CHECK(agn_tagorder_size(o, &n) == AGN_OK && n == want.size());
    uint64_t prev = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t t = 0;
        uint64_t l = 0;
        CHECK(agn_tagorder_at(o, i, &t) == AGN_OK && t == want[i]);
        CHECK(agn_tagorder_labels(o, t, 1, &l) == AGN_OK);
        CHECK(l > prev && l <= UINT64_MAX - 1);
        prev = l;
    }
}

static void check_even(agn_tagorder *o, uint32_t n) {
    const uint64_t step = UINT64_MAX / ((uint64_t)n + 1);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t t = 0;
        uint64_t l = 0;
        CHECK(agn_tagorder_at(o, i, &t) == AGN_OK);
        CHECK(agn_tagorder_labels(o, t, 1, &l) == AGN_OK && l == (uint64_t)(i + 1) * step);
    }
}

int main() {
    agn_tagorder *o = nullptr;
    int rel = 0;
    // random inserts (tag ids scattered over the u32 range)
    CHECK(agn_tagorder_create(&o) == AGN_OK);
    std::vector<uint32_t> want;
    int relabels = 0;
    for (uint32_t i = 0; i < 2000; ++i) {
        uint32_t pos = (uint32_t)(rnd() % (want.size() + 1));
        if (i % 7 == 0) {  // front, back and one fixed gap: gaps close, relabels happen
            const uint32_t n = (uint32_t)want.size(), at[3] = {0, n, n < 5 ? n : 5};
            pos = at[(i / 7) % 3];
        }
        const uint32_t tag = (i % 3 == 0) ? (uint32_t)(0xfffffffeu - i) : i;
        CHECK(agn_tagorder_insert(o, pos, tag, &rel) == AGN_OK);
        relabels += rel;
        want.insert(want.begin() + pos, tag);
        check_order(o, want);  // the whole order and every label, after every insert
    }
    std::printf("random: 2000 inserts, %d relabels\n", relabels);
    CHECK(relabels >= 1);  // 96 scripted front inserts: the 64th halving of the first label reaches 0
    // errors: nothing changes
    CHECK(agn_tagorder_insert(o, 2001, 5000, &rel) == AGN_EINVAL);
    CHECK(agn_tagorder_insert(o, 0, want[7], &rel) == AGN_EINVAL);
    CHECK(agn_tagorder_insert(o, 0, AGN_TAG_INVALID, &rel) == AGN_EINVAL);
    uint32_t t = 0;
    CHECK(agn_tagorder_at(o, 2000, &t) == AGN_EINVAL);
    check_order(o, want);
    CHECK(agn_tagorder_destroy(o) == AGN_OK);

    // front inserts: 2^63 - 1, 2^62 - 1, ..., 1, then the relabel
    CHECK(agn_tagorder_create(&o) == AGN_OK);
    for (uint32_t i = 0; i < 63; ++i) {
        uint64_t l = 0;
        CHECK(agn_tagorder_insert(o, 0, i, &rel) == AGN_OK && rel == 0);
        CHECK(agn_tagorder_labels(o, i, 1, &l) == AGN_OK && l == (1ull << (63 - i)) - 1);
    }
    CHECK(agn_tagorder_insert(o, 0, 63, &rel) == AGN_OK && rel == 1);
    check_even(o, 64);
    // holes
    uint64_t ls[8];
    CHECK(agn_tagorder_labels(o, 60, 8, ls) == AGN_OK);
    for (int i = 0; i < 8; ++i) CHECK((ls[i] != 0) == (i < 4));
    CHECK(agn_tagorder_labels(o, 0xfffffffcu, 8, ls) == AGN_OK);  // past the id range
    for (int i = 0; i < 8; ++i) CHECK(ls[i] == 0);
    CHECK(agn_tagorder_destroy(o) == AGN_OK);

    // back inserts, then one middle gap
    CHECK(agn_tagorder_create(&o) == AGN_OK);
    uint32_t n = 0;
    for (rel = 0; !rel; ++n) CHECK(agn_tagorder_insert(o, n, n, &rel) == AGN_OK);
    CHECK(n == 65);  // the gap to 2^64 - 1 halves 64 times
    check_even(o, n);
    for (rel = 0; !rel; ++n) CHECK(agn_tagorder_insert(o, 11, n, &rel) == AGN_OK && n < 200);
    check_even(o, n);
    std::printf("back / middle: relabelled at %u tags\n", n);
    CHECK(agn_tagorder_destroy(o) == AGN_OK);
    CHECK(agn_tagorder_destroy(nullptr) == AGN_OK);
    std::printf("tagorder_driver: ok\n");
    return 0;
}
