"""antidote_crdt_counter_b through the NIF's own C (nif/antidote_gpu_nif.c on the
minimal erl_nif runtime, tests/nif_rt): partitions driven as
antidote_gpu_nif.erl's update/3, read/4, read_from/6 and gc/3 drive them, with
the type's atom and with its id 6, against a literal sequential update/2 --
every state term {P, D} both ways, the error term with the stored effect, the
corrupted_ops_cache raise of a mis-typed read, and a partition holding
counter_b beside the other four types."""
import os
import sys

import numpy as np
import pytest

import bcounter_model as bm
from antidote_amd import _abi
from antidote_amd import clocksi_materializer as cm
from oracle import py_oracle as po
from test_ss_states import log_response

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "nif_rt"))
import terms  # noqa: E402
from terms import Atom, NifBadarg, NifRaise  # noqa: E402

pytestmark = pytest.mark.gpu

TYPE = bm.BC_TYPE
BC_ATOM = Atom(TYPE)
OK, ERROR, IGNORE = Atom("ok"), Atom("error"), Atom("ignore")
TRUE, FALSE = Atom("true"), Atom("false")
NEW = ([], [])
D, K = 2, 6
IDS = [Atom("dc1"), Atom("dc2"), Atom("dc3")]
INC, DEC, TRANSFER = Atom("increment"), Atom("decrement"), Atom("transfer")


def dc(d):
    return (Atom(f"antidote_{d}@127.0.0.1"), (1700, 0, d))


def pairs(row):
    return [(dc(d), int(t)) for d, t in enumerate(row)]


def dict_pairs(clock):
    return [(dc(d), int(t)) for d, t in sorted(clock.items())]


@pytest.fixture(scope="module")
def nif():
    terms.build()
    rt = terms.NifRuntime()
    r = rt.call("open", 0, keep=True)
    assert r[0] == OK, r
    yield rt, r[1]
    rt.release_all()


class Part:
    def __init__(self, rt, ctx, d, n_keys, first=BC_ATOM, cached=True):
        self.rt = rt
        r = rt.call("part_open", ctx, first, d, n_keys, cached, keep=True)
        assert r[0] == OK, r
        self.part, self.ref = r[1], rt.kept[-1]

    def close(self):
        self.rt.kept.remove(self.ref)
        self.rt.lib.rt_release(self.ref)

    def call(self, name, *args):
        return self.rt.call(name, self.part, *args)


def literal(effects, state=NEW):
    """A sequential update/2 over the effects, as the two orddicts."""
    st = (dict(state[0]), dict(state[1]))
    for e in effects:
        st = bm.update(e, st)
    return bm.as_orddicts(st)


class Script:
    """Causal clocks that only grow: op i is inside a read snapshot iff it was
    written before the clock the read uses was taken."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.clk = np.array([100, 100], np.int64)
        self.done = {k: [] for k in range(K)}     # key -> [(effect, clock after it)]

    def effect(self):
        r, v = self.rng.random(), int(self.rng.integers(-3, 12))
        a, b = (IDS[int(x)] for x in self.rng.choice(3, 2, replace=False))
        if r < 0.5:
            return ((INC, v), a)
        return ((DEC, v), a) if r < 0.75 else ((TRANSFER, v, b), a)

    def op(self, key, eff=None):
        c = int(self.rng.integers(0, D))
        ss = self.clk.copy()
        self.clk[c] += int(self.rng.integers(1, 9))
        oc = ss.copy()
        oc[c] = self.clk[c]
        eff = self.effect() if eff is None else eff
        self.done[key].append((eff, self.clk.copy()))
        return c, ss, int(self.clk[c]), oc, eff

    def state_at(self, key, R):
        return literal([e for e, at in self.done[key] if (at <= R).all()])


def drive_update(p, disk, typ, key, pay, oc, txid):
    """antidote_gpu_nif:update/3: op_insert_gc's GC read when due, then the op."""
    disk.append(pay)
    if p.call("part_gc_due", key, typ) == TRUE:
        g = p.call("part_read", key, typ, dict_pairs(pay.snapshot_time), IGNORE, True)
        if g == (ERROR, Atom("no_snapshot")):
            from_log(p, disk, typ, key, pay.snapshot_time, True)
    r = p.call("part_update", key, typ, pairs(oc), txid, pay.op_param)
    assert r[0] == OK, r
    return r[1]


def from_log(p, disk, typ, key, R_dict, gc):
    """read_from_log/6: the log's ops through the per-call mirror; a GC read's
    result is stored with its GC (part_store/8)."""
    resp = log_response(disk, key, R_dict, NEW)
    if resp.number_of_ops == 0:
        return NEW
    r = cm.materialize(TYPE, po.IGNORE, R_dict, resp)
    assert r[0] == "ok", r
    _, value, hole, ct, _newss, count = r
    if gc and ct != po.IGNORE:
        assert p.call("part_store", key, typ, dict_pairs(ct), int(hole), int(count), value,
                      True) == OK
    return value


def drive_read(p, disk, typ, key, R):
    """antidote_gpu_nif:read/4: the cached read, the log when it has none."""
    g = p.call("part_read", key, typ, pairs(R), IGNORE, False)
    if g == (ERROR, Atom("no_snapshot")):
        return from_log(p, disk, typ, key, {d: int(t) for d, t in enumerate(R)}, False), True
    assert g[0] == OK and len(g) == 6, g
    return g[1], False


def test_partition_of_the_type_opens(nif):
    """part_open with the type first (badarg on the parent), by atom and by id;
    a never-written key reads as new() = {[], []}; id 5 is no type."""
    rt, ctx = nif
    for first in (BC_ATOM, _abi.COUNTER_B):
        p = Part(rt, ctx, 3, 4, first)
        try:
            g = p.call("part_read", 2, first, pairs([5, 5, 5]), IGNORE, False)
            assert g == (OK, NEW, 0, IGNORE, FALSE, 0), g
            assert p.call("part_key_meta", 2, BC_ATOM) == (0, 0, 0)
            for bad in (5, 0, 7, Atom("antidote_crdt_counter_fat")):
                with pytest.raises(NifBadarg):
                    p.call("part_read", 2, bad, pairs([5, 5, 5]), IGNORE, False)
        finally:
            p.close()
    with pytest.raises(NifBadarg):
        rt.call("part_open", ctx, 5, 3, 4, True)


def test_cached_partition_vs_literal_update(nif):
    """update/3 and read/4 over a few hundred steps, the type given as the
    atom on even steps and as 6 on odd ones: every state equals the literal
    fold of the effects inside the read's snapshot; GC reads run (keys pass
    50 ops); the key meta follows."""
    rt, ctx = nif
    s = Script(5)
    p = Part(rt, ctx, D, K)
    disk, marks = [], []
    served = old = logs = gcs = 0
    try:
        for step in range(700):
            typ = BC_ATOM if step % 2 == 0 else _abi.COUNTER_B
            key = int(s.rng.integers(0, K))
            if s.rng.random() < 0.8:
                n0 = p.call("part_key_meta", key, typ)[0]
                c, ss, ct, oc, eff = s.op(key)
                pay = po.Payload(key, TYPE, eff, {d: int(t) for d, t in enumerate(ss)}, (c, ct),
                                 step + 1)
                op_id = drive_update(p, disk, typ, key, pay, oc, step + 1)
                assert op_id == len(s.done[key])
                gcs += p.call("part_key_meta", key, typ)[0] <= n0
                if step % 50 == 0:
                    marks.append(s.clk.copy())
                continue
            R = s.clk.copy()
            if marks and s.rng.random() < 0.25:
                R = marks[int(s.rng.integers(0, len(marks)))]
                old += 1
            got, was_log = drive_read(p, disk, typ, key, R)
            assert got == s.state_at(key, R), (step, key, got)
            served += 1
            logs += was_log
        e, _sl, _tk = p.call("part_stats")
        assert e == sum(p.call("part_key_meta", k, BC_ATOM)[0] for k in range(K))
        for k in range(K):
            assert p.call("part_key_meta", k, 6)[2] == len(s.done[k])
    finally:
        p.close()
    assert served > 100 and old > 10 and gcs > 0, (served, old, logs, gcs)


def test_error_terms_and_mistyped_reads(nif):
    """An effect the encoder refuses comes back verbatim in {error,
    {unexpected_operation, Effect, Type}}; amounts at the ends of int64 are
    carried; a read of the key under another type raises corrupted_ops_cache,
    and so does a counter_b read of another type's key."""
    rt, ctx = nif
    p = Part(rt, ctx, D, 16)
    a = IDS[0]
    try:
        R = pairs([10 ** 6, 10 ** 6])
        good = ((INC, 3), a)
        bad = [((INC, 1 << 63), a), ((DEC, -(1 << 63) - 1), a), ((Atom("reset"), 1), a),
               ((TRANSFER, 1), a), ((INC, 1, 2, 3), a), INC, 17, (INC, 1, a), [(INC, 1), a],
               ((TRANSFER, b"x", a), a)]
        for k, e in enumerate(bad):
            assert p.call("part_update", k, BC_ATOM, pairs([10, 5]), 1, good)[0] == OK
            assert p.call("part_update", k, 6, pairs([11, 5]), 2, e)[0] == OK
            for typ in (BC_ATOM, 6):
                assert p.call("part_read", k, typ, R, IGNORE, False) == \
                    (ERROR, (Atom("unexpected_operation"), e, BC_ATOM)), e
            g = p.call("part_read", k, BC_ATOM, pairs([10, 5]), IGNORE, False)
            assert g == (ERROR, Atom("no_snapshot")) or g[:2] == (OK, literal([good])), g
        top, low = (1 << 63) - 1, -(1 << 63)
        k = 12
        effs = [((INC, top), a), ((INC, 1), a), ((DEC, low), a), ((TRANSFER, 0, IDS[1]), a),
                ((DEC, -1), IDS[1])]
        for i, e in enumerate(effs):
            assert p.call("part_update", k, BC_ATOM, pairs([20 + i, 5]), 10 + i, e)[0] == OK
        g = p.call("part_read", k, 6, R, IGNORE, False)
        assert g[:2] == (OK, ([((a, a), low), ((a, IDS[1]), 0)], [(a, low), (IDS[1], -1)])), g
        assert g[5] == len(effs)
        for other in ("antidote_crdt_counter_pn", "antidote_crdt_set_aw",
                      "antidote_crdt_register_mv", "antidote_crdt_register_lww"):
            with pytest.raises(NifRaise) as ei:
                p.call("part_read", k, Atom(other), R, IGNORE, False)
            assert ei.value.reason == Atom("corrupted_ops_cache")
        assert p.call("part_update", 13, Atom("antidote_crdt_counter_pn"), pairs([30, 5]), 20,
                      4)[0] == OK
        with pytest.raises(NifRaise) as ei:
            p.call("part_read", 13, BC_ATOM, R, IGNORE, False)
        assert ei.value.reason == Atom("corrupted_ops_cache")
        # 257 distinct orddict keys: past the engine's table, an error and no state
        for i in range(257):
            assert p.call("part_update", 14, 6, pairs([40 + i, 5]), 40 + i,
                          ((TRANSFER, 1, i), a))[0] == OK
            if i == 255:
                g = p.call("part_read", 14, BC_ATOM, R, IGNORE, False)
                assert g[0] == OK and len(g[1][0]) == 256 and g[1][1] == [], g[:1]
        assert p.call("part_read", 14, BC_ATOM, R, IGNORE, False) == (ERROR, Atom("ecapacity"))
        for st in ([(1, 2)], (1, 2), ([((a, a), b"x")], []), ([(a, 1)], [])):
            with pytest.raises(NifBadarg):
                p.call("part_store", 12, BC_ATOM, pairs([30, 5]), 6, 6, st, True)
    finally:
        p.close()


def test_uncached_read_from_and_gc(nif):
    """read_from/6 (part_materialize) from caller bases given as {P, D} terms,
    with and without a base snapshot time; gc/3 (part_gc) prunes the key's ops
    at a threshold and later reads from that snapshot's state agree."""
    rt, ctx = nif
    s = Script(9)
    p = Part(rt, ctx, D, K, cached=False)
    try:
        clocks = []
        for step in range(60):
            c, ss, ct, oc, eff = s.op(1)
            typ = BC_ATOM if step % 2 else 6
            assert p.call("part_update", 1, typ, pairs(oc), step + 1, eff)[:2] == (OK, step + 1)
            clocks.append(s.clk.copy())
        now = pairs(s.clk)
        full = s.state_at(1, s.clk)
        g = p.call("part_materialize", 1, BC_ATOM, now, IGNORE, IGNORE, NEW)
        assert g[:2] == (OK, full) and g[5] == 60 and g[4] == TRUE, g
        # a base state on top of which every op applies again: sums double
        g = p.call("part_materialize", 1, 6, now, IGNORE, IGNORE, full)
        dbl = ([(k, 2 * v) for k, v in full[0]], [(k, 2 * v) for k, v in full[1]])
        assert g[:2] == (OK, dbl), g
        # from the snapshot at op 30: the base is its state, SCT its clock
        mid = clocks[29]
        base = s.state_at(1, mid)
        g = p.call("part_materialize", 1, BC_ATOM, now, pairs(mid), IGNORE, base)
        assert g[:2] == (OK, full) and g[5] == 30, g
        # a base slot the log never names stays; a never-written key returns its base
        extra = (base[0] + [((Atom("zz"), Atom("zz")), 0)], base[1] + [(Atom("zz"), -4)])
        g = p.call("part_materialize", 1, BC_ATOM, now, pairs(mid), IGNORE, extra)
        want = literal([e for e, at in s.done[1] if not (at <= mid).all()],
                       (dict(extra[0]), dict(extra[1])))
        assert g[:2] == (OK, want), g
        assert p.call("part_materialize", 3, 6, now, IGNORE, IGNORE, base)[:2] == (OK, base)
        # gc/3 at the snapshot's clock: its ops go, the same read still holds
        n0 = p.call("part_key_meta", 1, BC_ATOM)[0]
        assert n0 == 60 and p.call("part_gc", 1, pairs(mid)) == OK
        n1 = p.call("part_key_meta", 1, 6)[0]
        assert 0 < n1 <= 30, n1
        g = p.call("part_materialize", 1, BC_ATOM, now, pairs(mid), IGNORE, base)
        assert g[:2] == (OK, full) and g[5] == 30, g
        with pytest.raises(NifBadarg):
            p.call("part_materialize", 1, BC_ATOM, now, IGNORE, IGNORE, [(1, 2)])
    finally:
        p.close()


def test_partition_with_all_five_types(nif):
    """counter_b beside counter_pn, set_aw, register_mv and register_lww in one
    partition: each key reads back under its own type, part_stats counts every
    log, and gc/3 runs over them all."""
    rt, ctx = nif
    p = Part(rt, ctx, D, 8, first=Atom("antidote_crdt_counter_pn"))
    a, b = IDS[0], IDS[1]
    R = pairs([10 ** 6, 10 ** 6])
    writes = [
        (0, Atom("antidote_crdt_counter_pn"), [5, -2]),
        (1, Atom("antidote_crdt_set_aw"), [[(b"e", [b"t1"], [])], [(b"f", [b"t2"], [])]]),
        (2, Atom("antidote_crdt_register_mv"), [(b"v", b"t3", [])]),
        (3, Atom("antidote_crdt_register_lww"), [(7, b"w"), (9, b"x")]),
        (4, BC_ATOM, [((INC, 10), a), ((TRANSFER, 5, b), a), ((DEC, 5), b)]),
        (5, _abi.COUNTER_B, [((INC, 10), a), ((DEC, 4), a)]),
    ]
    try:
        t = 10
        n = 0
        for key, typ, effs in writes:
            for e in effs:
                t += 1
                n += 1
                assert p.call("part_update", key, typ, pairs([t, 5]), t, e)[0] == OK
        assert p.call("part_stats")[0] == n
        want = {0: 3, 1: [(b"e", [b"t1"]), (b"f", [b"t2"])], 2: [(b"v", b"t3")], 3: (9, b"x"),
                4: ([((a, a), 10), ((a, b), 5)], [(b, 5)]), 5: ([((a, a), 10)], [(a, 4)])}
        for key, typ, _effs in writes:
            g = p.call("part_read", key, typ, R, IGNORE, False)
            assert g[:2] == (OK, want[key]), (key, g)
        assert cm.permissions(want[4]) == 5 and cm.permissions(want[5]) == 6
        assert cm.local_permissions(a, want[4]) == 5 and cm.local_permissions(b, want[4]) == 0
        with pytest.raises(NifRaise):
            p.call("part_read", 0, BC_ATOM, R, IGNORE, False)
        for key in (4, 5, 0):
            assert p.call("part_gc", key, R) == OK
        assert p.call("part_key_meta", 4, BC_ATOM)[0] <= 1
        assert p.call("part_stats")[0] < n
    finally:
        p.close()
