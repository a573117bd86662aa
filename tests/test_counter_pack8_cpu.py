"""Conditions on the inputs of tests/test_counter_pack8.py (no GPU): the cases
of tests/pack8_cases.py contain what they claim -- fully served groups of
eight, tails of 1 and 7, each unservable reason at each of the eight positions,
isolated keys whose oracle results differ from their neighbours', spans and
thresholds on the stated boundary values, half-word patterns that exclude on
exactly one half, and the fold case's maxima where stated."""
import numpy as np
import pytest

import pack8_cases as p8
import pack_cases as pc
from antidote_amd import _abi

U64, D, M16 = p8.U64, p8.D, p8.M16
_WANT = {}


def want_of(oracle_lib, name):
    if name not in _WANT:
        c = p8.case(name)
        _WANT[name] = (c, p8.run_oracle(oracle_lib, c))
    return _WANT[name]


def same(a, b, idx):
    return all(np.array_equal(getattr(a, f)[idx], getattr(b, f)[idx]) for f in pc.FIELDS)


def rows_of(c, k):
    a = int(c.log.key_off[k])
    return np.asarray(c.log.oc, U64).reshape(-1, D)[a:a + int(p8.lens_of(c)[k])]


def test_tail_groups_and_served_groups():
    tails, after_full, no_tail = set(), set(), set()
    for K in p8.N_KEYS:
        c = p8.case(f"n{K}")
        assert c.log.n_keys == c.req.n_req == K and np.array_equal(c.req.keys, np.arange(K))
        assert (p8.lens_of(c) == 24).all() and p8.narrow_of(c).all()
        served = p8.served8(c)
        assert served[:K // 8 * 8].all() and not served[K // 8 * 8:].any()
        if K % 8:
            tails.add(K % 8)
            if K > 8:
                after_full.add(K % 8)
        else:
            no_tail.add(K)
    assert tails == {1, 7} and after_full == {1, 7} and no_tail == {8, 16, 24}


@pytest.mark.parametrize("name", p8.REASONS + ("empty",))
def test_each_reason_at_each_position(oracle_lib, name):
    c, want = want_of(oracle_lib, name)
    why, served, nar = p8.unservable(c), p8.served8(c), p8.narrow_of(c)
    ok = (p8.spans_of(c) <= U64(p8.M32)).all(axis=1)
    assert c.log.n_keys == 72 and served[:8].all()           # group 0 is fully served
    assert [k % 8 for k in c.special[name]] == list(range(8))
    for k in c.special[name]:
        g = k // 8 * 8
        if name == "empty":        # served, with count 0
            assert served[g:g + 8].all() and p8.lens_of(c)[k] == 0 and nar[k]
            assert want.count[k] == 0 and not want.lastct[k].any()
        else:
            assert why[k] == name and [w for w in why[g:g + 8] if w] == [name]
            assert not served[g:g + 8].any()
        if name == "wide":         # one column spans exactly 65 536: packed, not narrow
            assert int(p8.spans_of(c)[k].max()) == M16 + 1 and ok[k] and not nar[k]
        if name == "unpacked":
            assert int(p8.spans_of(c)[k].max()) >= 1 << 32 and not ok[k] and not nar[k]
    if name == "corrupt":
        assert (want.flags[c.special[name]] == _abi.F_ERR_CORRUPTED).all()
    assert p8.lens_of(c).max() == (65 if name == "long" else 24)
    others = np.setdiff1d(np.arange(72), c.special[name])
    assert nar[others].all()


@pytest.mark.parametrize("name", tuple(p8.ISO))
def test_isolated_key_differs_from_its_neighbours(oracle_lib, name):
    c, want = want_of(oracle_lib, name)
    assert p8.served8(c).all() and p8.narrow_of(c).all()
    n = p8.N_SPECIAL
    for k in c.special[name]:
        g = k // 8 * 8
        rows = rows_of(c, k)
        base = rows.min(axis=0)
        for j in range(g, g + 8):
            if j == k:
                continue
            assert np.array_equal(rows_of(c, j), rows)           # the same rows: only R differs
            assert not np.array_equal(c.req.R[j], c.req.R[k])
            assert want.count[j] != want.count[k] and not np.array_equal(want.lastct[j], want.lastct[k])
        R = c.req.R[k]
        if name == "noR":
            assert (R < base).sum() == 1 and want.count[k] == 0 and not want.lastct[k].any()
        if name == "count0":
            assert (R == base).all() and want.count[k] == 0 and not want.lastct[k].any()
            assert want.flags[k] == _abi.F_CT_IGNORE
        if name == "thr_eq":
            assert R[3] == rows[n // 2 + 3, 3] and want.count[k] == n // 2 + 4
        if name in ("span_full", "span_minus1"):
            span = rows.max(axis=0) - base
            assert int(span[3]) == M16 and int(span.max()) == M16
            assert int((rows[:, 3] - base[3] == U64(M16)).sum()) == 1      # the last op alone
            assert (R >= rows.max(axis=0)).sum() == (D if name == "span_full" else D - 1)
            assert int(R[3] - base[3]) == (M16 if name == "span_full" else M16 - 1)
            assert want.count[k] == (n if name == "span_full" else n - 1)
        if name == "saturate":
            d = (R - base).astype(U64)
            assert int(d[3]) == M16 + 1 and int(d[5]) >= 1 << 32 and want.count[k] == n
            assert np.array_equal(want.lastct[k], rows.max(axis=0))


@pytest.mark.parametrize("thr", (M16 - 1, 0))
def test_half_words_exclude_on_one_half(oracle_lib, thr):
    c, want = want_of(oracle_lib, f"half_{thr}")
    assert c.log.n_keys == 8 and p8.served8(c).all()
    for k in range(8):
        j, h = k // 2, k % 2
        rows = rows_of(c, k)
        delta = rows - rows.min(axis=0)
        pair = delta[:, 2 * j:2 * j + 2].astype(np.int64)
        assert {tuple(p) for p in pair.tolist()} == {(0, 0), (M16, 0), (0, M16)}
        t = (c.req.R[k] - rows.min(axis=0)).astype(np.int64)
        over = delta.astype(np.int64) > t[None, :]
        # the threshold excludes in column 2j + h alone, there exactly the ops at 65 535
        assert not np.delete(over, 2 * j + h, axis=1).any()
        assert np.array_equal(over[:, 2 * j + h], pair[:, h] == M16) and over[:, 2 * j + h].sum() == 4
        assert t[2 * j + h] == thr and t[2 * j + (1 - h)] == M16
        assert want.count[k] == p8.HALF_N - 4
        assert int(want.lastct[k][2 * j + h] - rows.min(axis=0)[2 * j + h]) == 0
        assert int(want.lastct[k][2 * j + 1 - h] - rows.min(axis=0)[2 * j + 1 - h]) == M16


def test_fold_maxima(oracle_lib):
    c, want = want_of(oracle_lib, "fold")
    oc = np.asarray(c.log.oc, U64).reshape(8, p8.FOLD_N, D)
    base = oc.min(axis=1)
    for d in range(D):
        assert len(set(base[:, d].tolist())) == 8                # eight distinct bases per column
    assert p8.served8(c).all() and (want.count == p8.FOLD_N).all()
    assert np.array_equal(want.lastct, oc.max(axis=1))           # LastOpCt per key and DC, from numpy
    for g in range(8):
        for d in range(D):
            col = oc[g, :, d]
            assert int(np.argmax(col)) == p8.fold_op(g, d) and (col == col.max()).sum() == 1
            assert int(col.max() - base[g, d]) <= M16
    assert len({p8.fold_op(g, d) for g in range(8) for d in range(D)}) > 32   # spread over the lanes


def test_high_clocks(oracle_lib):
    c, want = want_of(oracle_lib, "high")
    oc = np.asarray(c.log.oc, U64).reshape(8, 24, D)
    assert p8.served8(c).all()
    assert (U64(p8.TOP) - oc.min(axis=1) <= U64(M16)).all()      # bases within 65 535 of 2^64 - 2
    assert int(oc.max()) == p8.TOP and (oc[[2, 5]].max(axis=(1, 2)) == U64(p8.TOP)).all()
    assert int(want.lastct[5].max()) == p8.TOP and int(want.lastct[2].max()) < p8.TOP
    assert (want.count > 0).all()


def test_lengths_and_log_end():
    a, b = p8.case("len_64_last"), p8.case("len_short_last")
    assert list(p8.lens_of(a)) == [1, 63, 64, 24, 64, 1, 63, 64]
    assert list(p8.lens_of(b)) == [64, 63, 1, 64, 24, 63, 1, 5]
    assert p8.served8(a).all() and p8.served8(b).all()
    assert int(a.log.key_off[-1]) == a.log.n_entries and int(b.log.key_off[-1]) == b.log.n_entries


def test_invalid_effects(oracle_lib):
    c, want = want_of(oracle_lib, "invalid")
    err = (want.flags & _abi.F_ERR_UNEXPECTED) != 0
    assert c.log.n_keys == 8 and err[:4].all() and not err[4:].any() and p8.served8(c).all()
    pos = want.err_pos[:4].astype(np.int64) - c.log.key_off[:4].astype(np.int64)
    assert list(pos) == [0, 5, 17, 30]
    assert (want.err_pos[4:] == 0xFFFFFFFF).all()


def test_side_arrays(oracle_lib):
    assert p8.case("n8").req.base_value.any() and p8.case("nobase").req.base_value is None
    c = p8.case("id0")
    assert c.log.n_keys == 16 and p8.served8(c).all()
    for k in range(c.log.n_keys):
        a, b = int(c.log.key_off[k]), int(c.log.key_off[k + 1])
        assert np.array_equal(c.log.op_id[a:b], 1000 * k + np.arange(b - a))
    assert (np.diff(p8.case("nobase").log.op_id[:17]) == 2).all()   # not consecutive: the op_id load
    s, csr = p8.case("segmented"), p8.case("nobase")
    assert s.key_len is not None and np.array_equal(s.key_len, np.diff(csr.log.key_off))
    gaps = np.diff(s.log.key_off).astype(np.int64) - s.key_len.astype(np.int64)
    assert (gaps >= 1).all() and len(set(gaps.tolist())) == 3 and p8.served8(s).all()


def test_index_and_bound_cases():
    c = p8.mixed_index_case()
    why = p8.unservable(c)
    assert {"wide", "unpacked", "long", ""} == set(why) and 0 in p8.lens_of(c)
    nar, rows = p8.rows16_reference(c)
    assert nar[[c.names.index("long narrow 65"), c.names.index("span 65535")]].all()
    assert not nar[[c.names.index("wide 65536"), c.names.index("long wide 65")]].any()
    assert int(rows.max()) == M16
    for n_keys in (1024, 1016):
        b = p8.bound_case(n_keys)
        nb = p8.narrow_of(b)
        assert not nb[0] and nb[1:].all() and ((~nb).sum() * 1024 <= n_keys) == (n_keys == 1024)


@pytest.mark.parametrize("name", p8.CASES)
def test_oc_poison_proves_the_path(oracle_lib, name):
    c, clean = want_of(oracle_lib, name)
    served = p8.served8(c)
    dirty = p8.run_oracle(oracle_lib, c, p8.poison_oc(c))
    assert same(clean, dirty, ~served)                        # the fallback's groups see no poison
    live = served & (clean.count > 0)
    for i in np.flatnonzero(live):
        assert not same(clean, dirty, [i]), c.names[i]
    if c.log.n_keys >= 8:
        assert live.any()
