"""The fused counter_b cached read under the NIF's own C (nif/antidote_gpu_nif.c
on tests/nif_rt): a counter_b partition opened with AGN_BCOUNTER_FUSED=1 (its
batcher reads the knob when it is created) beside a twin opened with the knob
unset, driven as antidote_gpu_nif.erl drives them.  Every read's term is equal
between the two and equal to the literal sequential update/2, {error,
ecapacity} and {error, {unexpected_operation, ...}} included."""
import pytest

from antidote_amd import _abi
from oracle import py_oracle as po
from test_nif_bcounter import (BC_ATOM, DEC, ERROR, IDS, IGNORE, INC, OK, TRANSFER, TYPE, D, K,  # noqa: F401
                               Part, Script, drive_read, drive_update, literal, nif, pairs)
from terms import Atom

pytestmark = pytest.mark.gpu

KNOB = "AGN_BCOUNTER_FUSED"


def twin_parts(rt, ctx, monkeypatch, n_keys):
    monkeypatch.setenv(KNOB, "1")
    a = Part(rt, ctx, D, n_keys)
    monkeypatch.delenv(KNOB)
    b = Part(rt, ctx, D, n_keys)
    return a, b


def test_twin_partitions_read_for_read(nif, monkeypatch):
    """update/3 and read/4 over a few hundred steps on both partitions: GC
    reads run (keys pass 50 ops), old clocks are read, and every answer is the
    literal fold of the effects inside the read's snapshot."""
    rt, ctx = nif
    s = Script(11)
    pa, pb = twin_parts(rt, ctx, monkeypatch, K)
    da, db, marks = [], [], []
    served = old = 0
    try:
        for step in range(500):
            typ = BC_ATOM if step % 2 == 0 else _abi.COUNTER_B
            key = int(s.rng.integers(0, K))
            if s.rng.random() < 0.8:
                c, ss, ct, oc, eff = s.op(key)
                pay = po.Payload(key, TYPE, eff, {d: int(t) for d, t in enumerate(ss)}, (c, ct),
                                 step + 1)
                ia = drive_update(pa, da, typ, key, pay, oc, step + 1)
                ib = drive_update(pb, db, typ, key, pay, oc, step + 1)
                assert ia == ib == len(s.done[key])
                assert pa.call("part_key_meta", key, typ) == pb.call("part_key_meta", key, typ)
                if step % 50 == 0:
                    marks.append(s.clk.copy())
                continue
            R = s.clk.copy()
            if marks and s.rng.random() < 0.25:
                R = marks[int(s.rng.integers(0, len(marks)))]
                old += 1
            ga = pa.call("part_read", key, typ, pairs(R), IGNORE, False)
            gb = pb.call("part_read", key, typ, pairs(R), IGNORE, False)
            assert ga == gb, (step, key, ga, gb)
            got, _was_log = drive_read(pa, da, typ, key, R)
            drive_read(pb, db, typ, key, R)
            assert got == s.state_at(key, R), (step, key, got)
            served += 1
        assert pa.call("part_stats") == pb.call("part_stats")
    finally:
        pa.close()
        pb.close()
    assert served > 60 and old > 5, (served, old)


def test_twin_partitions_error_terms(nif, monkeypatch):
    """An included invalid effect and a key past 256 orddict keys: the same
    error terms from both partitions; 256 keys are still served, in order."""
    rt, ctx = nif
    pa, pb = twin_parts(rt, ctx, monkeypatch, 4)
    a = IDS[0]
    R = pairs([10 ** 6, 10 ** 6])
    bad = ((Atom("reset"), 1), a)
    try:
        for p in (pa, pb):
            assert p.call("part_update", 0, BC_ATOM, pairs([10, 5]), 1, ((INC, 3), a))[0] == OK
            assert p.call("part_update", 0, 6, pairs([11, 5]), 2, bad)[0] == OK
            assert p.call("part_read", 0, BC_ATOM, R, IGNORE, False) == \
                (ERROR, (Atom("unexpected_operation"), bad, BC_ATOM))
            # transfers to descending ids: the slots first appear out of term order
            for i in range(257):
                assert p.call("part_update", 1, 6, pairs([40 + i, 5]), 40 + i,
                              ((TRANSFER, i + 1, 1000 - i), a))[0] == OK
                if i == 255:
                    g = p.call("part_read", 1, BC_ATOM, R, IGNORE, False)
                    assert g[0] == OK and g[1][1] == [], g[:1]
                    assert g[1][0] == [((a, 1000 - j), j + 1) for j in range(255, -1, -1)]
            assert p.call("part_read", 1, BC_ATOM, R, IGNORE, False) == (ERROR, Atom("ecapacity"))
        # a second read of the 2-op key hits what the first cached, on both
        assert pa.call("part_read", 0, 6, pairs([10, 5]), IGNORE, False) == \
            pb.call("part_read", 0, 6, pairs([10, 5]), IGNORE, False)
    finally:
        pa.close()
        pb.close()
