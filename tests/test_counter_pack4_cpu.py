"""Conditions on the inputs of tests/test_counter_pack4.py (no GPU): the cases
of tests/pack4_cases.py contain what they claim -- fully served groups, each
unservable reason at each position of a group, tail groups of 1, 2 and 3
requests, and isolated keys whose oracle results differ from their
neighbours' -- and the oc poison of the GPU test shows exactly where the
straight path must have served a request."""
import numpy as np
import pytest

import pack4_cases as p4
import pack_cases as pc
from antidote_amd import _abi

_WANT = {}


def want_of(oracle_lib, name):
    if name not in _WANT:
        c = p4.case(name)
        _WANT[name] = (c, p4.run_oracle(oracle_lib, c))
    return _WANT[name]


def same(a, b, idx):
    return all(np.array_equal(getattr(a, f)[idx], getattr(b, f)[idx]) for f in pc.FIELDS)


def test_tail_groups_and_served_groups():
    tails, after_full = set(), set()
    for K in p4.N_KEYS:
        c = p4.case(f"n{K}")
        assert c.log.n_keys == c.req.n_req == K and np.array_equal(c.req.keys, np.arange(K))
        served = p4.served4(c)
        assert served[:K // 4 * 4].all() and not served[K // 4 * 4:].any()
        if K % 4:
            tails.add(K % 4)
            if K > 4:
                after_full.add(K % 4)
    assert tails == {1, 2, 3} and after_full == {1, 3}
    assert {len(p4.case(f"n{K}").names) for K in (4, 8)} == {4, 8}     # no tail: full groups only


@pytest.mark.parametrize("name", p4.REASONS + ("empty",))
def test_each_reason_at_each_position(oracle_lib, name):
    c, want = want_of(oracle_lib, name)
    why, served = p4.unservable(c), p4.served4(c)
    assert c.log.n_keys == 20 and served[:4].all()          # group 0 is fully served
    assert [k % 4 for k in c.special[name]] == [0, 1, 2, 3]
    for k in c.special[name]:
        g = k // 4 * 4
        if name == "empty":       # served, with count 0
            assert served[g:g + 4].all() and p4.lens_of(c)[k] == 0
            assert want.count[k] == 0 and not want.lastct[k].any()
        else:
            assert why[k] == name and [w for w in why[g:g + 4] if w] == [name]
            assert not served[g:g + 4].any()
    if name == "corrupt":
        assert (want.flags[c.special[name]] == _abi.F_ERR_CORRUPTED).all()
    assert p4.lens_of(c).max() == (65 if name == "long" else 24)


@pytest.mark.parametrize("name", tuple(p4.ISO))
def test_isolated_key_differs_from_its_neighbours(oracle_lib, name):
    c, want = want_of(oracle_lib, name)
    assert p4.served4(c).all()
    oc = np.asarray(c.log.oc, np.uint64).reshape(-1, p4.D)
    for k in c.special[name]:
        g = k // 4 * 4
        a, n = int(c.log.key_off[k]), 24
        base = oc[a:a + n].min(axis=0)
        for j in range(g, g + 4):
            if j == k:
                continue
            b = int(c.log.key_off[j])
            assert np.array_equal(oc[b:b + n], oc[a:a + n])      # the same rows: only R differs
            assert want.count[j] != want.count[k] and not np.array_equal(want.lastct[j], want.lastct[k])
        R = c.req.R[k]
        if name == "noR":
            assert (R < base).sum() == 1 and want.count[k] == 0 and not want.lastct[k].any()
        if name == "count0":
            assert (R == base).all() and want.count[k] == 0 and not want.lastct[k].any()
            assert want.flags[k] == _abi.F_CT_IGNORE
        if name == "saturate":
            assert ((R - base) >> np.uint64(32) > 0).sum() == 1 and want.count[k] == n
        if name == "thr_eq":
            assert R[3] == oc[a + n // 2 + 3, 3] and want.count[k] == n // 2 + 4


def test_ctmax_bases_and_columns(oracle_lib):
    c, want = want_of(oracle_lib, "ctmax")
    oc = np.asarray(c.log.oc, np.uint64).reshape(4, 30, p4.D)
    base = oc.min(axis=1)
    for d in range(p4.D):
        assert len(set(base[:, d].tolist())) == 4
    delta = want.lastct - base
    assert [int(np.argmax(delta[g])) for g in range(4)] == [1, 3, 5, 7]
    assert p4.served4(c).all() and (want.count == 30).all()


def test_lengths_and_log_end():
    a, b = p4.case("len_64_last"), p4.case("len_short_last")
    assert list(p4.lens_of(a)) == [1, 63, 64, 64] and list(p4.lens_of(b)) == [64, 63, 1, 5]
    assert p4.served4(a).all() and p4.served4(b).all()
    assert int(a.log.key_off[-1]) == a.log.n_entries and int(b.log.key_off[-1]) == b.log.n_entries


def test_invalid_effects(oracle_lib):
    c, want = want_of(oracle_lib, "invalid")
    err = (want.flags & _abi.F_ERR_UNEXPECTED) != 0
    assert err[:4].all() and not err[4:].any() and p4.served4(c).all()
    pos = want.err_pos[:4].astype(np.int64) - c.log.key_off[:4].astype(np.int64)
    assert list(pos) == [0, 5, 17, 30]
    assert (want.err_pos[4:] == 0xFFFFFFFF).all()
    eff = np.asarray(c.log.eff)
    assert [(eff[int(c.log.key_off[k]):int(c.log.key_off[k + 1])] == _abi.EFFECT_INVALID).sum()
            for k in range(8)] == [1] * 8


def test_side_arrays(oracle_lib):
    assert p4.case("n8").req.base_value.any() and p4.case("nobase").req.base_value is None
    c = p4.case("id0")
    for k in range(c.log.n_keys):
        a, b = int(c.log.key_off[k]), int(c.log.key_off[k + 1])
        assert np.array_equal(c.log.op_id[a:b], 1000 * k + np.arange(b - a))
    plain_ids = p4.case("n8").log.op_id
    assert (np.diff(plain_ids[:17]) == 2).all()               # not consecutive: no id base, the op_id load
    s, csr = p4.case("segmented"), p4.case("n8")
    assert s.key_len is not None and np.array_equal(s.key_len, np.diff(csr.log.key_off))
    gaps = np.diff(s.log.key_off).astype(np.int64) - s.key_len.astype(np.int64)
    assert (gaps >= 1).all() and len(set(gaps.tolist())) == 3
    ws, wc = p4.run_oracle(oracle_lib, s), p4.run_oracle(oracle_lib, csr)
    assert all(np.array_equal(getattr(ws, f), getattr(wc, f)) for f in pc.FIELDS if f != "err_pos")


@pytest.mark.parametrize("name", p4.CASES)
def test_oc_poison_proves_the_path(oracle_lib, name):
    c, clean = want_of(oracle_lib, name)
    served = p4.served4(c)
    dirty = p4.run_oracle(oracle_lib, c, p4.poison_oc(c))
    assert same(clean, dirty, ~served)                        # the fallback's groups see no poison
    live = served & (clean.count > 0)
    for i in np.flatnonzero(live):
        assert not same(clean, dirty, [i]), c.names[i]
    if c.log.n_keys >= 4 and name not in ("noR", "count0"):
        assert live.any()
