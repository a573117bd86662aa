"""Conditions on the inputs of tests/test_counter_eff16.py (no GPU): the cases
of tests/eff16_cases.py contain what they claim -- fitting and escaping effects
on the stated boundary values, the i32 sums' extremes, escapes at lanes 0 and
63 under a wrapping base, invalid effects on included and on excluded ops,
escapes behind a short key and at the log's last entry, all inside served
groups -- and the poisons of the path test change the oracle's results of the
served groups and of no other."""
import numpy as np
import pytest

import eff16_cases as e16
import pack8_cases as p8
import pack_cases as pc
from antidote_amd import _abi

M64 = (1 << 64) - 1
_WANT = {}


def want_of(oracle_lib, name):
    if name not in _WANT:
        c = e16.case(name)
        _WANT[name] = (c, e16.run_oracle(oracle_lib, c))
    return _WANT[name]


def same(a, b, idx):
    return all(np.array_equal(getattr(a, f)[idx], getattr(b, f)[idx]) for f in pc.FIELDS)


def seg(c, k):
    a = int(c.log.key_off[k])
    return slice(a, a + int(e16.lens_of(c)[k]))


def wrapped_sum(c, k, inc):
    s = int(c.req.base_value[k]) + sum(int(v) for v in c.log.eff[seg(c, k)][inc[seg(c, k)]])
    s &= M64
    return s - (1 << 64) if s >> 63 else s


def test_reference_boundaries():
    eff = np.array([0, 32767, -32767, 32768, -32768, e16.INVALID, e16.I64MAX, e16.I64MIN + 1, -1], np.int64)
    ref, n = e16.eff16_reference(eff)
    assert ref.tolist() == [0, 32767, -32767, -32768, -32768, -32768, -32768, -32768, -1] and n == 5
    assert np.uint16(ref[3]) == 0x8000


@pytest.mark.parametrize("name", e16.EDGE_CASES)
def test_edge_logs_are_served_and_sum_as_numpy(oracle_lib, name):
    c, want = want_of(oracle_lib, name)
    K = c.log.n_keys
    assert K == {"edges8": 8, "edges16": 16, "edges17": 17, "two_keys": 16}[name]
    served, inc = e16.served8(c), e16.included_of(c)
    assert served[:K // 8 * 8].all() and not served[K // 8 * 8:].any() and p8.narrow_of(c).all()
    assert e16.lens_of(c).max() == (24 if name == "two_keys" else 64)
    assert int(c.log.key_off[-1]) == c.log.n_entries       # the last key ends at the log's end
    err = (want.flags & _abi.F_ERR_UNEXPECTED) != 0
    for k in range(K):
        bad = np.flatnonzero(inc[seg(c, k)] & (c.log.eff[seg(c, k)] == e16.INVALID))
        assert err[k] == (len(bad) > 0), c.names[k]
        if err[k]:                         # the first included invalid op wins
            assert int(want.err_pos[k]) == int(c.log.key_off[k]) + int(bad[0])
        else:                              # the included ops' effects, mod 2^64
            assert int(want.count[k]) == int(inc[seg(c, k)].sum())
            assert int(want.value[k]) == wrapped_sum(c, k, inc), c.names[k]


@pytest.mark.parametrize("name", p8.CASES + e16.EDGE_CASES + e16.ID_CASES)
def test_expected_value_is_the_oracles_where_it_defines_one(oracle_lib, name):
    """e16.expected_value (numpy) against the oracle wherever the oracle's value
    counts: no error flag.  Under AGN_F_ERR_UNEXPECTED the oracle stops at the
    invalid op; there numpy's sum is the reference of the GPU test."""
    c, want = want_of(oracle_lib, name)
    ok = (want.flags & (_abi.F_ERR_CORRUPTED | _abi.F_ERR_UNEXPECTED)) == 0
    assert ok.any() and np.array_equal(e16.expected_value(c)[ok], want.value[ok])


def test_id_index_without_a_base(oracle_lib):
    c, want = want_of(oracle_lib, "id0_gap")
    base, wb = want_of(oracle_lib, "id0")
    assert c.index_ids and e16.served8(c).all() and c.log.n_keys == 16
    lens = e16.lens_of(c)
    for k in range(16):
        ids = c.log.op_id[seg(c, k)].astype(np.int64)
        gap = lens[k] > 1 and not (np.diff(ids) == 1).all()
        assert gap == (k in e16.GAP_KEYS)
    for k in e16.GAP_KEYS:                 # non-empty, some ops included, the hole past the gap
        assert lens[k] >= 40 and want.count[k] > 2
        assert int(want.hole[k]) == int(wb.hole[k]) + 500 and int(want.hole[k]) not in (0, -1)
    assert {k // 8 for k in e16.GAP_KEYS} == {0, 1}
    others = np.setdiff1d(np.arange(16), e16.GAP_KEYS)
    assert np.array_equal(want.hole[others], wb.hole[others])


def test_group_a_edges(oracle_lib):
    c, want = want_of(oracle_lib, "edges8")
    inc, esc, eff = e16.included_of(c), e16.escaped_of(c), c.log.eff
    lens = e16.lens_of(c)
    # the i32 sum's extremes: 64 included ops of 32767 / -32767, none escaped
    for k, v in ((0, 32767), (1, -32767)):
        assert lens[k] == 64 and inc[seg(c, k)].all() and (eff[seg(c, k)] == v).all() and not esc[seg(c, k)].any()
        assert int(want.value[k]) == int(c.req.base_value[k]) + 64 * v
    # 32767 and -32767 fit, 32768 and -32768 escape, all included
    a = int(c.log.key_off[2])
    assert eff[a:a + 4].tolist() == [32767, -32767, 32768, -32768] and inc[a:a + 4].all()
    assert esc[a:a + 4].tolist() == [False, False, True, True]
    # escapes at lanes 0 and 63, INT64_MAX and INT64_MIN + 1, the sum wrapping past the base
    a = int(c.log.key_off[3])
    assert lens[3] == 64 and inc[seg(c, 3)].all()
    assert int(eff[a]) == e16.I64MAX and int(eff[a + 63]) == e16.I64MIN + 1 and esc[a] and esc[a + 63]
    assert int(c.req.base_value[3]) + e16.I64MAX > e16.I64MAX          # base + the first term leaves i64
    assert np.flatnonzero(esc[seg(c, 3)]).tolist() == [0, 31, 63]
    # two included invalid ops: the first wins; an escape before it and one after it
    bad = np.flatnonzero(eff[seg(c, 4)] == e16.INVALID)
    assert bad.tolist() == [5, 17] and inc[seg(c, 4)].all()
    assert int(want.err_pos[4]) == e16.entry(c, 4, 5) and want.flags[4] & _abi.F_ERR_UNEXPECTED
    # an invalid op and an escape on excluded ops only, an escape on an included one: no error
    assert not inc[e16.entry(c, 5, 39)] and not inc[e16.entry(c, 5, 38)] and inc[e16.entry(c, 5, 2)]
    assert int(eff[e16.entry(c, 5, 39)]) == e16.INVALID and not want.flags[5] & _abi.F_ERR_UNEXPECTED
    # a 9-op key whose successor opens on an invalid op and escapes: lanes 9.. must not count them
    assert lens[6] == 9 and not esc[seg(c, 6)].any() and not want.flags[6] & _abi.F_ERR_UNEXPECTED
    a = int(c.log.key_off[7])
    assert int(eff[a]) == e16.INVALID and esc[a:a + 3].all() and int(want.err_pos[7]) == a
    # the log's last op: an included escape at entry n_entries - 1
    last = c.log.n_entries - 1
    assert e16.entry(c, 7, int(lens[7]) - 1) == last and esc[last] and inc[last] and lens[7] < 64


def test_group_b_edges(oracle_lib):
    c, want = want_of(oracle_lib, "edges16")
    inc, esc, eff, lens = e16.included_of(c), e16.escaped_of(c), c.log.eff, e16.lens_of(c)
    assert lens[8] == 0 and e16.served8(c)[8] and want.count[8] == 0          # an empty key, served
    assert int(want.err_pos[9]) == e16.entry(c, 9, 63) and lens[9] == 64      # invalid at lane 63 alone
    assert int(eff[e16.entry(c, 9, 0)]) == -32767 and not esc[e16.entry(c, 9, 0)]
    assert sorted(lens[8:].tolist()) == [0, 1, 2, 5, 33, 63, 64, 64]
    assert not inc[e16.entry(c, 11, 62)] and inc[e16.entry(c, 11, 10)]        # b3: invalid excluded, escape included
    last = c.log.n_entries - 1
    assert e16.entry(c, 15, 4) == last and esc[last] and inc[last] and lens[15] == 5
    assert int(c.req.base_value[15]) + 2 * e16.I64MAX > e16.I64MAX            # wraps
    t, wt = want_of(oracle_lib, "edges17")
    assert not e16.served8(t)[16] and wt.flags[16] & _abi.F_ERR_UNEXPECTED    # the tail goes through oc and eff


def test_two_keys_of_one_group(oracle_lib):
    c, want = want_of(oracle_lib, "two_keys")
    hit = e16.escaped_of(c) & e16.included_of(c)
    keys = sorted(set(pc.key_of_entry(c.log)[hit].tolist()))
    assert keys == [1, 6] and e16.served8(c).all()
    assert not e16.escaped_of(c)[int(c.log.key_off[8]):].any()                # none in the neighbouring group
    assert not (want.flags & _abi.F_ERR_UNEXPECTED).any()


def test_bound_cases():
    for short, entries in ((False, 1024), (True, 1023)):
        c = e16.bound_case(short)
        n_esc = e16.eff16_reference(c.log.eff)[1]
        assert c.log.n_entries == entries and c.log.n_keys == 16 and n_esc == 1
        assert (n_esc * 1024 <= entries) == (not short)
        assert e16.served8(c).all() and p8.narrow_of(c).all() and e16.included_of(c).all()
        assert entries // 64 <= c.log.n_keys                                  # the whole-partition launch's rule


@pytest.mark.parametrize("name", e16.POISON_CASES)
def test_eff_poison_proves_the_path(oracle_lib, name):
    c, clean = want_of(oracle_lib, name)
    served, inc, esc = e16.served8(c), e16.included_of(c), e16.escaped_of(c)
    dirty = e16.run_oracle(oracle_lib, c, e16.poison_eff(c))
    assert same(clean, dirty, ~served)                        # the fallback's groups see no poison
    koe_hit = np.zeros(c.log.n_keys, bool)
    for k in np.flatnonzero(served):                          # the oracle stops at a key's first included invalid op
        bad = np.flatnonzero(inc[seg(c, k)] & (c.log.eff[seg(c, k)] == e16.INVALID))
        stop = int(bad[0]) if len(bad) else int(e16.lens_of(c)[k])
        koe_hit[k] = (inc[seg(c, k)] & ~esc[seg(c, k)])[:stop].any()
    for i in np.flatnonzero(koe_hit):                         # an included op that the tier holds, before it: noticed
        assert not same(clean, dirty, [i]), c.names[i]
    assert koe_hit.any()
    # and the eff16 poison (every effect 0x7F7F, no escape) changes every served request with an op
    live = served & (clean.count > 0)
    for k in np.flatnonzero(live):
        s = seg(c, k)
        had_err = bool(clean.flags[k] & _abi.F_ERR_UNEXPECTED)
        true_sum = sum(int(v) for v in c.log.eff[s][inc[s]] if int(v) != e16.INVALID)
        assert had_err or true_sum != 0x7F7F * int(inc[s].sum()), c.names[k]
