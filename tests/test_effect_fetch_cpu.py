"""Conditions on the inputs of tests/test_effect_fetch.py (no GPU): every
named edge of tests/effect_cases.py is reached, both slots of a pair hold
every pattern, and the poison is invisible -- the C oracle gives the same
result on the poisoned log as on the clean one in every field, because it
reads an effect only for an included entry (oracle.c, apply_operations).

In the cold form (no SCT) the P entries are included, so there their poison
is data: the X poison alone must be invisible."""
import ctypes as C

import numpy as np
import pytest

import effect_cases as ec
from antidote_amd import _abi
from antidote_amd.encode import alloc_result, log_struct, read_struct, result_struct

FIELDS = ("value", "hole", "lastct", "count", "flags", "err_pos")


def run_oracle(oracle_lib, log, req, sparse):
    res = alloc_result(req.n_req, log.n_dcs, sparse=bool(sparse))
    ls, rs, os_ = log_struct(log), read_struct(req, sparse=bool(sparse)), result_struct(res)
    if not sparse:
        ls.oc_mask = None
    assert oracle_lib.oracle_materialize(C.byref(ls), C.byref(rs), C.byref(os_), 4) == 0
    return res


def same(a, b, sparse):
    for f in FIELDS + (("lastct_mask",) if sparse else ()):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_named_edges_reached():
    pats = ec.base_patterns()
    assert {len(p) for p in pats} == set(ec.LENGTHS)
    assert all(len(p) <= 257 for p in pats) and 100 < len(pats) < 500
    for n in ec.LENGTHS:
        mine = [p for p in pats if len(p) == n]
        for whole in "IXP":
            assert whole * n in mine
        for p in ec.spots(n):
            for one, rest in (("I", "X"), ("I", "P"), ("X", "I"), ("T", "P")):
                hit = [q for q in mine if q[p] == one and q.count(one) == 1 and
                       q.count(rest) == n - 1]
                assert hit, (n, p, one, rest)
        assert {0, 15, 16, 63, 64, n - 1} & set(range(n)) == set(ec.spots(n))
        if n >= 2:
            assert any(q[:2] == "IX" and set(q[::2]) == {"I"} and set(q[1::2]) == {"X"} for q in mine)
            assert any(q[:2] == "XI" and set(q[::2]) == {"X"} and set(q[1::2]) == {"I"} for q in mine)
        if n >= 32:   # line edges: 16 I then 16 X, and the inverse
            assert any(q[:32] == "I" * 16 + "X" * 16 for q in mine)
            assert any(q[:32] == "X" * 16 + "I" * 16 for q in mine)
        if n >= 3:
            assert any(q.startswith("XEI") for q in mine) and any(q.startswith("IXE") for q in mine)
        for p in (63, 64):   # an E on either side of the chunk edge, an X beside it
            if p < n:
                assert any(q[p] == "E" and "X" in q[max(p - 1, 0):p + 2] for q in mine), (n, p)
        if n >= 129:         # an E in each chunk
            assert any("E" in q[:64] and "E" in q[64:128] and "E" in q[128:] for q in mine)
            assert any(q[63] == "E" and q[64] == "E" for q in mine)
    # every letter that gets poisoned sits beside every letter that is read
    assert all(c in "".join(pats) for c in "IXPTE")


def test_both_slots_and_unpaired_tail():
    a, b = ec.patterns_of("a"), ec.patterns_of("b")
    assert b[1:] == a and len(b[0]) == 1
    # request j of list a is request j + 1 of list b: the other slot of its wave
    assert len(a) % 2 != len(b) % 2          # one list ends on a single-key block
    for case in ("a", "b", "b_keys"):
        log, req, names, pats = ec.build(case)
        assert req.n_req == len(pats)
        ident = np.array_equal(req.keys, np.arange(req.n_req, dtype=np.uint64))
        assert ident == (case != "b_keys")


def test_pair_fallback_cases():
    log, req, names, pats = ec.build("corrupt")
    bad = set(ec.CORRUPT)
    pairs = {(2 * j in bad, 2 * j + 1 in bad) for j in range(len(pats) // 2)}
    assert pairs == {(True, False), (False, True), (True, True), (False, False)}
    assert len(pats) % 2 == 1 and len(pats) - 1 in bad   # and a corrupt unpaired tail
    assert all(len(pats[k]) > 0 for k in bad)             # an empty key is never corrupt


def test_log_end_cases():
    for case, n in (("end1", 1), ("end65", 65)):
        log, req, names, pats = ec.build(case)
        assert len(pats[-1]) == n and pats[-1].count("I") == 1 and pats[-1][-1] == "I"
        assert int(log.key_off[-1]) == log.n_entries == sum(len(p) for p in pats)


@pytest.mark.parametrize("style", [None, "uniform"])
@pytest.mark.parametrize("kind", ec.POISONS)
@pytest.mark.parametrize("case", ec.CASES)
def test_poison_is_invisible(oracle_lib, case, kind, style):
    log, req, names, pats = ec.build(case, style)
    clean = run_oracle(oracle_lib, log, req, style)
    same(run_oracle(oracle_lib, ec.poison(log, pats, kind), req, style), clean, style)
    # the cases are not trivial: some request includes ops, one excludes, one fails
    assert (clean.count > 0).any() and (clean.flags & _abi.F_NEWSS).any()
    if case in ("a", "b", "b_keys"):
        assert (clean.flags & _abi.F_ERR_UNEXPECTED).any()
    if case == "corrupt":
        got = (clean.flags & _abi.F_ERR_CORRUPTED) != 0
        assert set(np.flatnonzero(got)) == set(ec.CORRUPT)
    # cold: P is included, X stays unread
    creq = ec.cold(req)
    same(run_oracle(oracle_lib, ec.poison(log, pats, kind), creq, style),
         run_oracle(oracle_lib, ec.poison(log, pats, kind, "P"), creq, style), style)
