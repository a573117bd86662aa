"""set_aw / register_mv snapshot states on the device (ABI v4 state arena).

materializer_vnode's snapshot cache stores, for every CRDT type, the full
#materialized_snapshot{value} -- for set_aw / register_mv the state orddict
(src/materializer_vnode.erl:384-413, 466-509, include/antidote.hrl:169-176) --
and a read materializes from that cached state.  Here the cached states live
in a device arena next to the cache (agn_ss_cache.state_*): agn_ss_lookup
hands the hit slot's state to the tags kernel as its base, agn_ss_store
appends the result's state.  Checked against the reference's transcription
(oracle/py_oracle.MaterializerVnode: ETS ops tuple, snapshot cache, GC,
resize) read for read:

  * the cached read batcher (the NIF's read/4 on a Cached partition), with
    update/2's GC reads, dense and presence-masked logs; for D <= 64
    the batch is the fused read (lookup -> fast tags pass -> store in one
    kernel, tags_serve.hpp), with its hand-on path for states past the fast
    table; AGN_READ6=0 runs the kernel sequence on the same workload;
  * keys whose entries carry different DC sets (the fused read hands them
    on to the per-entry-mask passes): against the transcription (the GC read
    at the op's own snapshot dict, as op_insert_gc reads), and the fused
    batch against the kernel sequence, result for result;
  * agn_read_cached over device arrays, rounds of whole-partition batches,
    with the GC applied and the arena re-packed (agn_ss_state_compact).
"""
import ctypes as C

import numpy as np
import pytest

from antidote_amd import _abi
from antidote_amd import clocksi_materializer as cm
from antidote_amd.engine import Batcher, OpLog
from antidote_amd.records import IGNORE, MaterializedSnapshot, SnapshotGetResponse
from oracle import py_oracle as po

pytestmark = pytest.mark.gpu

D = 3
LWW = _abi.REGISTER_LWW
PTYPE = {_abi.SET_AW: po.SET_AW, _abi.REGISTER_MV: po.REGISTER_MV, _abi.COUNTER_PN: po.COUNTER_PN,
         LWW: po.REGISTER_LWW}
PAIR_TYPES = [_abi.SET_AW, _abi.REGISTER_MV, LWW]
# register_lww timestamps an encoder accepts (Ts >= 1), at the edges of the domain
LWW_TS_EDGE = [1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1]
LWW_NEW = (0, b"")


def vc(row, mask=None):
    return {d: int(row[d]) for d in range(len(row)) if mask is None or (mask >> d) & 1}


class TagWorkload:
    """Causal clocks as in test_vnode_replay; effects built the way the CRDTs'
    downstream does: set_aw add = {Elem, [new token], observed tokens of Elem},
    remove = {Elem, [], observed}; register_mv assign = {V, new token, all
    observed}, reset = {reset, all observed} (observed = the writer's view);
    register_lww assign = {Ts, V}: V an integer 0..4 (its own tag id, so the
    device's tie break by tag is update/2's by term), Ts from the edges of the
    u64 domain on even keys and from 1..8 on odd keys, where ties are common.
    A state is then no pair (new()) or one."""

    def __init__(self, seed, K, typ, d=D):
        self.rng = np.random.default_rng(seed)
        self.K, self.typ, self.D = K, typ, d
        self.clk = np.full(d, 1000, np.int64)
        self.live = [dict() for _ in range(K)]   # key -> elem -> [tok]
        self.tok = 1

    def op(self, key):
        D = self.D
        c = int(self.rng.integers(0, D))
        ss = np.maximum(self.clk - self.rng.integers(0, 40, D), 0)
        self.clk[c] += int(self.rng.integers(1, 30))
        oc = ss.copy()
        oc[c] = self.clk[c]
        live = self.live[key]
        if self.typ == LWW:
            v = int(self.rng.integers(0, 5))
            ts = int(self.rng.integers(1, 9)) if key % 2 else \
                LWW_TS_EDGE[int(self.rng.integers(0, len(LWW_TS_EDGE)))]
            return c, ss, int(self.clk[c]), oc, (ts, v), (v, ts, [])
        if self.typ == _abi.SET_AW:
            e = int(self.rng.integers(0, 6))
            obs = list(live.get(e, []))
            if self.rng.random() < 0.75:
                t = self.tok
                self.tok += 1
                live[e] = [t]
                eff, entry = [(e, [t], obs)], (e, t, obs)
            else:
                live[e] = []
                eff, entry = [(e, [], obs)], (e, 0, obs)
        else:
            obs = [t for ts in live.values() for t in ts]
            if self.rng.random() < 0.1:
                live.clear()
                eff, entry = ("reset", obs), (0, 0, obs)
            else:
                v, t = int(self.rng.integers(0, 5)), self.tok
                self.tok += 1
                live.clear()
                live[0] = [t]
                eff, entry = (v, t, obs), (v, t, obs)
        return c, ss, int(self.clk[c]), oc, eff, entry

    def read_clock(self, lag=400):
        return np.maximum(self.clk - self.rng.integers(0, lag, self.D), 0)


def state_of(typ, tags, toks):
    """Engine pairs -> the reference's state: set_aw orddict [{Elem, [Tok]}]
    (pairs grouped by elem, tokens in fold order), register_mv [{V, Tok}],
    register_lww {Ts, V} (no pair: new())."""
    if typ == LWW:
        assert len(tags) <= 1
        return (int(toks[0]), int(tags[0])) if len(tags) else LWW_NEW
    if typ == _abi.REGISTER_MV:
        return [(int(v), int(t)) for v, t in zip(tags, toks)]
    out = []
    for e, t in zip(tags, toks):
        if out and out[-1][0] == int(e):
            out[-1][1].append(int(t))
        else:
            out.append((int(e), [int(t)]))
    return out


def append_entry(ol, key, oc, entry, txid, mask=None):
    tag, add, rems = entry
    ol.append(np.array([key], np.uint64), oc.reshape(1, len(oc)).astype(np.uint64),
              oc_mask=None if mask is None else np.array([[mask]], np.uint64),
              tag=np.array([tag], np.uint32), add_tok=np.array([add], np.uint64),
              rem_off=np.array([0, len(rems)], np.uint32),
              rem_tok=np.array(rems if rems else [0], np.uint64),
              txid=np.array([txid], np.uint64))


def log_response(disk, key, R, new_value=None):
    """The Erlang side's read of the partition's disk log for a key
    (get_from_snapshot_log -> logging_vnode:get_up_to_time,
    src/logging_vnode.erl:185-190, 522-549, 586-591): its committed ops whose
    transaction snapshot <= R, newest first, ids from 0 at the oldest; base
    {0, Type:new()} (new_value; [] for set/register), snapshot time
    vectorclock:new(), not the newest."""
    ops = [p for p in disk if p.key == key and po.vc_le(p.snapshot_time, R)]
    return SnapshotGetResponse([(i, p) for i, p in enumerate(ops)][::-1], len(ops),
                               MaterializedSnapshot(0, [] if new_value is None else new_value),
                               {}, False)


class NifPartition:
    """A cached set/register partition driven the way nif/antidote_gpu_nif.erl
    drives it: update/2 runs op_insert_gc's GC read (when due) before the
    insert, and a read (GC or not) whose cache holds no snapshot <= its clock
    (AGN_SS_LOG) is served from the log: materialize/4 of the log's response
    through the engine's per-call path, then -- a GC read -- the result stored
    on the device cache with its GC (agn_batcher_store), as
    materialize_snapshot (:466-509) does with ShouldGc."""

    def __init__(self, ol, bt, typ, d, sparse):
        self.ol, self.bt, self.typ, self.d, self.sparse = ol, bt, typ, d, sparse
        self.disk = []          # the logging_vnode's committed payloads
        self.log_reads = self.log_gc = 0

    def from_log(self, key, R_dict, gc):
        counter = self.typ == _abi.COUNTER_PN
        new = 0 if counter else LWW_NEW if self.typ == LWW else None
        resp = log_response(self.disk, key, R_dict, new)
        if resp.number_of_ops == 0:
            return ("ok", [] if new is None else new)  # materialize_snapshot :468-471
        r = cm.materialize(PTYPE[self.typ], IGNORE, R_dict, resp)
        if r[0] != "ok":
            return r
        _, value, hole, ct, _newss, count = r
        if gc and ct != IGNORE:
            row = np.zeros(self.d, np.uint64)
            m = 0
            for dc, t in ct.items():
                row[dc] = t
                m |= 1 << dc
            if counter:
                self.bt.store(key, row, clock_mask=np.uint64(m) if self.sparse else None,
                              last_op=hole, count=count, value=value, gc=True)
            else:
                if self.typ == _abi.SET_AW:
                    pairs = [(e, t) for e, toks in value for t in toks]
                elif self.typ == LWW:
                    pairs = [] if value == LWW_NEW else [(value[1], value[0])]
                else:
                    pairs = list(value)
                self.bt.store(key, row, clock_mask=np.uint64(m), last_op=hole, count=count,
                              tags=[e for e, _ in pairs], toks=[t for _, t in pairs], gc=True)
            self.log_gc += 1
        return ("ok", value)

    def update(self, key, payload, oc, entry, txid, mask, R_gc):
        self.disk.append(payload)                 # logged before the materializer
        if self.ol.gc_due(key)[0]:                # op_insert_gc's GC read at the op's dict
            g = self.bt.read(key, R=R_gc.astype(np.uint64),
                             R_mask=np.array([mask]) if self.sparse else None, gc=True,
                             out_cap=4096)
            if g["status"] == _abi.SS_LOG:
                self.from_log(key, payload.snapshot_time, True)
        append_entry(self.ol, key, oc, entry, txid, mask if self.sparse else None)

    def read(self, key, R, rm=None):
        g = self.bt.read(key, R=R.astype(np.uint64), R_mask=rm, out_cap=4096)
        if g["status"] == _abi.SS_LOG:
            self.log_reads += 1
            m = int(rm[0]) if rm is not None else (1 << self.d) - 1
            return self.from_log(key, vc(R, m), False), g
        return ("ok", state_of(self.typ, g["out_tag"], g["out_tok"])), g


def placeholder(vn, key):
    tup = vn.ops_cache.get(key)
    return tup is not None and any(tup[po.FIRST_OP - 1 + i] == 0 for i in range(tup[1][0]))


# (D, log): "dense", "sparse" (every entry carries all D DCs), "mixed" (each
# entry a random DC subset holding its own DC: keys not uniform, the fused
# read hands them on); read6: the fused batch ("1") or the kernel sequence
BATCHER_CASES = [
    (d, lg, r6) for d in (3, 4, 8) for lg in ("dense", "sparse", "mixed") for r6 in ("1", "0")
] + [(1, "sparse", "1"), (2, "sparse", "1"), (5, "sparse", "1"), (6, "dense", "1"),
     (7, "dense", "1"), (7, "mixed", "1")] + [
    # D > 8: the fused read's wide shapes (mat_tags.hip serve_dispatch, 4 DCs
    # a lane) against the reference and the kernel sequence
    (16, lg, r6) for lg in ("dense", "sparse", "mixed") for r6 in ("1", "0")
] + [(64, "dense", "1"), (64, "sparse", "1"), (64, "mixed", "1"), (32, "mixed", "1")]


def reference_quirks(typ, d, logk, K=16, steps=2500):
    """The keys test_batcher_states_vs_reference leaves out of the comparison,
    from the reference side alone (the same workload, the transcription's
    vnode, no engine): its all-pruned placeholder and its
    badmatch crash paths."""
    sparse, mixed = logk != "dense", logk == "mixed"
    w = TagWorkload(31 + typ + 7 * d, K, typ, d)
    vn = po.MaterializerVnode(disk_log=True)
    quirk = set()
    full = (1 << d) - 1
    for s in range(steps):
        key = int(w.rng.integers(0, K))
        if w.rng.random() < 0.7:
            c, ss, ct, oc, eff, entry = w.op(key)
            mask = full
            if mixed and w.rng.random() < 0.3:
                mask = full & ~(1 << int(w.rng.choice([x for x in range(d) if x != c])))
            pay = po.Payload(key, PTYPE[typ], eff, vc(ss, int(mask)), (c, ct), s + 1)
            try:
                vn.update(key, pay)
            except po.BadMatch:
                quirk.add(key)
            if placeholder(vn, key):
                quirk.add(key)
        else:
            R = w.read_clock(lag=400 if w.rng.random() < 0.85 else 20000)
            if key in quirk:
                continue
            try:
                vn.read(key, PTYPE[typ], vc(R), po.IGNORE)
            except po.BadMatch:
                quirk.add(key)
                continue
            if placeholder(vn, key):
                quirk.add(key)
    _ = sparse
    return quirk


@pytest.mark.parametrize("d,logk,read6", BATCHER_CASES)
@pytest.mark.parametrize("typ", PAIR_TYPES)
def test_batcher_states_vs_reference(eng, typ, d, logk, read6, monkeypatch):
    """update/2 (+ its GC read) and read/6 through a cached set/register
    partition: every served state equals the reference's, and the ETS list
    sizes follow it slot for slot.  Reads (GC or not) that no cached snapshot
    serves go to the log on both sides (the transcription's disk log, the
    engine's per-call materialize + agn_batcher_store), so a key leaves the
    check only on a reference crash path (the all-pruned placeholder, a
    badmatch)."""
    monkeypatch.setenv("AGN_READ6", read6)
    sparse, mixed = logk != "dense", logk == "mixed"
    K, steps = 16, 2500
    w = TagWorkload(31 + typ + 7 * d, K, typ, d)
    vn = po.MaterializerVnode(disk_log=True)
    quirk, served = set(), 0
    full = np.uint64((1 << d) - 1)
    rm = np.array([full]) if sparse else None
    with OpLog(eng, typ, d, K, sparse=sparse) as ol, \
            Batcher(ol, max_batch=8, cached=True) as bt:
        part = NifPartition(ol, bt, typ, d, sparse)
        for s in range(steps):
            key = int(w.rng.integers(0, K))
            if w.rng.random() < 0.7:
                c, ss, ct, oc, eff, entry = w.op(key)
                mask = full
                if mixed and w.rng.random() < 0.3:  # one DC missing (never the op's own)
                    mask = np.uint64(int(full) & ~(1 << int(w.rng.choice(
                        [x for x in range(d) if x != c]))))
                pay = po.Payload(key, PTYPE[typ], eff, vc(ss, int(mask)), (c, ct), s + 1)
                try:
                    vn.update(key, pay)
                except po.BadMatch:
                    quirk.add(key)
                part.update(key, pay, oc, entry, s + 1, mask, ss)
                if placeholder(vn, key):
                    quirk.add(key)
            else:
                R = w.read_clock(lag=400 if w.rng.random() < 0.85 else 20000)
                got, g = part.read(key, R, rm)
                if key in quirk:
                    continue
                try:
                    want = vn.read(key, PTYPE[typ], vc(R), po.IGNORE)
                except po.BadMatch:
                    quirk.add(key)
                    continue
                assert want == got, (s, key, g["status"], want, got)
                served += 1
                if placeholder(vn, key):
                    quirk.add(key)
        ln, ll, ct = ol.key_meta()
    print(f"served={served} log_reads={part.log_reads} log_gc={part.log_gc} "
          f"quirk={len(quirk)}/{K}")
    # (at D = 64 the clocks a read picks are rarely below every kept snapshot
    # within the run: the log path is exercised at the narrower widths)
    assert served > (150 if mixed else 500) and (part.log_reads > 0 or d > 16), \
        (served, part.log_reads, len(quirk))
    # the reference-side exclusions are exactly the reference's own prediction
    # for this workload: none (reference_quirks, pinned on the CPU by
    # test_ss_states_cpu.py), so every key is compared
    assert quirk == set(), sorted(quirk)
    for k in range(K):
        if k in quirk or k not in vn.ops_cache:
            continue
        length, list_len = vn.ops_cache[k][1]
        assert (int(ln[k]), int(ll[k])) == (length, list_len), k


def rand_mask(rng, d):
    return int(sum(int(b) << i for i, b in enumerate(rng.integers(0, 2, d))))


@pytest.mark.parametrize("d", [3, 4, 8, 16, 64])
@pytest.mark.parametrize("typ", PAIR_TYPES)
def test_batcher_fused_vs_sequence_mixed_dcs(eng, typ, d, monkeypatch):
    """Entries with random DC sets (each holding its own DC; R with some DCs
    missing now and then): two partitions fed the same updates, one served by
    the fused read, one by the kernel sequence -- every result field, the
    status and the ETS list sizes agree, and every served state equals the
    reference transcription's (its disk log serving what no snapshot does)."""
    K, steps = 16, 2500
    w = TagWorkload(57 + typ + 7 * d, K, typ, d)
    full = (1 << d) - 1
    vn = po.MaterializerVnode(disk_log=True)
    quirk = set()
    with OpLog(eng, typ, d, K, sparse=True) as la, OpLog(eng, typ, d, K, sparse=True) as lb:
        monkeypatch.setenv("AGN_READ6", "1")
        ba = Batcher(la, max_batch=8, cached=True)
        monkeypatch.setenv("AGN_READ6", "0")
        bb = Batcher(lb, max_batch=8, cached=True)
        compared = checked = 0
        with ba, bb:
            pa, pb = NifPartition(la, ba, typ, d, True), NifPartition(lb, bb, typ, d, True)
            for s in range(steps):
                key = int(w.rng.integers(0, K))
                if w.rng.random() < 0.7:
                    c, ss, ct, oc, eff, entry = w.op(key)
                    mask = np.uint64(rand_mask(w.rng, d) | (1 << c))
                    pay = po.Payload(key, PTYPE[typ], eff, vc(ss, int(mask)), (c, ct), s + 1)
                    try:
                        vn.update(key, pay)
                    except po.BadMatch:
                        quirk.add(key)
                    for p in (pa, pb):
                        p.update(key, pay, oc, entry, s + 1, mask, ss)
                    if placeholder(vn, key):
                        quirk.add(key)
                else:
                    R = w.read_clock(lag=400 if w.rng.random() < 0.85 else 20000).astype(np.uint64)
                    rm = full if w.rng.random() < 0.8 else rand_mask(w.rng, d) | 1
                    (ra, ga), (rb, gb) = (p.read(key, R, np.array([rm], np.uint64)) for p in (pa, pb))
                    for f in ga:
                        assert np.array_equal(np.asarray(ga[f]), np.asarray(gb[f])), (s, key, f)
                    assert ra == rb, (s, key)
                    compared += 1
                    if key in quirk:
                        continue
                    try:
                        want = vn.read(key, PTYPE[typ], vc(R, rm), po.IGNORE)
                    except po.BadMatch:
                        quirk.add(key)
                        continue
                    assert want == ra, (s, key, ga["status"], want, ra)
                    checked += 1
                    if placeholder(vn, key):
                        quirk.add(key)
            print(f"compared={compared} checked={checked} log_reads={pa.log_reads} "
                  f"log_gc={pa.log_gc} quirk={len(quirk)}/{K}")
            assert compared > 500 and checked > 400
            assert len(quirk) <= K // 4
            for a, b in zip(la.key_meta(), lb.key_meta()):
                assert np.array_equal(a, b)


@pytest.mark.parametrize("d,read6", [(3, "1"), (3, "0"), (4, "1"), (8, "1"), (8, "0")])
def test_batcher_state_bound_grows(eng, d, read6, monkeypatch):
    """A key whose state outgrows the caller's buffer: the read reports
    AGN_ECAPACITY, a second read with room for the state is served (the NIF's
    retry) from the snapshot the first one stored.  300 live pairs: past the
    fast table, so the fused read hands the key on."""
    from antidote_amd._lib import EngineError
    monkeypatch.setenv("AGN_READ6", read6)
    K = 2
    with OpLog(eng, _abi.SET_AW, d, K) as ol, Batcher(ol, max_batch=4, cached=True) as bt:
        n = 300
        oc = np.tile(np.arange(1, n + 1, dtype=np.uint64)[:, None], (1, d))
        ol.append(np.zeros(n, np.uint64), oc, tag=np.arange(n, dtype=np.uint32),
                  add_tok=np.arange(1, n + 1, dtype=np.uint64),
                  rem_off=np.zeros(n + 1, np.uint32), rem_tok=np.zeros(1, np.uint64))
        R = np.full(d, n, np.uint64)
        with pytest.raises(EngineError):
            bt.read(0, R=R, out_cap=10)
        g = bt.read(0, R=R, out_cap=n)
        assert g["out_n"] == n
        assert state_of(_abi.SET_AW, g["out_tag"], g["out_tok"]) == \
            [(e, [e + 1]) for e in range(n)]


@pytest.mark.parametrize("typ", PAIR_TYPES)
def test_read_cached_states_vs_reference(eng, typ):
    """agn_read_cached over device arrays: rounds of reads of every key at a
    growing clock (with GC reads), the selected keys pruned in the log, and the
    arena re-packed into a fresh one every other round."""
    K, rounds = 64, 6
    w = TagWorkload(77 + typ, K, typ)
    vn = po.MaterializerVnode()
    S = _abi.SNAPSHOT_THRESHOLD
    with OpLog(eng, typ, D, K) as ol:
        bufs = {"n": eng.empty(4 * K), "clock": eng.empty(8 * K * S * D),
                "last_op": eng.empty(8 * K * S), "value": eng.empty(8 * K * S),
                "ctl": eng.empty(32), "status": eng.empty(K), "prune": eng.empty(K),
                "thr": eng.empty(8 * K * D)}
        eng.lib.agn_memset_d(eng.ctx, bufs["n"].ptr, 0, 4 * K, None)
        eng.lib.agn_memset_d(eng.ctx, bufs["ctl"].ptr, 0, 32, None)
        cap = 1 << 14
        arena = [eng.empty(4 * cap), eng.empty(8 * cap)]
        c = _abi.AgnSsCache()
        c.n_dcs, c.slots, c.n_keys = D, S, K
        c.n, c.clock, c.last_op, c.value = (bufs[x].ptr for x in ("n", "clock", "last_op", "value"))
        c.state_tag, c.state_tok, c.state_cap, c.state_ctl = arena[0].ptr, arena[1].ptr, cap, \
            bufs["ctl"].ptr
        keys = eng.upload(np.arange(K, dtype=np.uint64))
        quirk = set()
        s = 0
        for rnd in range(rounds):
            # ~3 ops per key per round: no key reaches op_insert_gc's GC
            # trigger (50 ops, :635), so the reference's GC runs only where the
            # batch's gc flags run it on the device too
            for _ in range(3 * K):
                key = int(w.rng.integers(0, K))
                c_, ss, ct, oc, eff, entry = w.op(key)
                s += 1
                try:
                    vn.update(key, po.Payload(key, PTYPE[typ], eff, vc(ss), (c_, ct), s))
                except po.BadMatch:
                    quirk.add(key)
                append_entry(ol, key, oc, entry, s)
                if placeholder(vn, key):
                    quirk.add(key)
            view = ol.flush()
            ln, _, _ = ol.key_meta()
            cap_off = np.zeros(K + 1, np.uint64)
            cap_off[1:] = np.cumsum(ln.astype(np.uint64) + np.uint64(512))
            dres = eng.alloc_result(K, D, sparse=False, cap_off=cap_off)
            R = w.read_clock(lag=300).astype(np.uint64)
            dR = eng.upload(np.tile(R, (K, 1)))
            gc = (w.rng.random(K) < 0.2).astype(np.uint8)
            dgc = eng.upload(gc)
            eng.read_cached(c, view, K, keys.ptr, dR.ptr, None, dgc.ptr, dres, bufs["status"].ptr,
                            bufs["prune"].ptr, bufs["thr"].ptr)
            res = eng.fetch_result(dres)
            status = eng.download(bufs["status"], np.uint8, (K,))
            for k in range(K):
                if k in quirk:
                    continue
                try:
                    want = vn.internal_read(k, PTYPE[typ], vc(R), po.IGNORE, bool(gc[k]))
                except NotImplementedError:
                    assert status[k] == _abi.SS_LOG, (rnd, k)
                    continue
                except po.BadMatch:
                    quirk.add(k)
                    continue
                assert status[k] in (_abi.SS_HIT, _abi.SS_NEW), (rnd, k, status[k])
                o, m = int(res.out_off[k]), int(res.out_n[k])
                got = state_of(typ, res.out_tag[o:o + m], res.out_tok[o:o + m])
                assert want == ("ok", got), (rnd, k, want, got)
                if placeholder(vn, k):
                    quirk.add(k)
            # the GC the store selected, in the log
            ol.prune(bufs["prune"].ptr, bufs["thr"].ptr)
            ctl = eng.download(bufs["ctl"], np.uint64, (4,))
            assert ctl[2] == 0, "state arena overflow"
            if rnd % 2 == 1:  # re-pack into a fresh arena
                live = int(ctl[0] - ctl[1])
                nt, nk = eng.empty(4 * cap), eng.empty(8 * cap)
                assert eng.lib.agn_ss_state_compact(eng.ctx, C.byref(c), nt.ptr, nk.ptr, cap,
                                                    None) == 0
                ctl = eng.download(bufs["ctl"], np.uint64, (4,))
                assert int(ctl[0]) == live and int(ctl[1]) == 0
                for b in arena:
                    b.free()
                arena = [nt, nk]
            for b in (dR, dgc):
                b.free()
            for b in dres.bufs.values():
                b.free()
        assert len(quirk) < K // 2


def _distinct_adds(ol, key, n, start, d):
    """n set_aw adds of distinct elements (one token each) to key, clocks
    start+1 .. start+n on every DC."""
    oc = np.tile(np.arange(start + 1, start + n + 1, dtype=np.uint64)[:, None], (1, d))
    ol.append(np.full(n, key, np.uint64), oc, tag=np.arange(start, start + n, dtype=np.uint32),
              add_tok=np.arange(start + 1, start + n + 1, dtype=np.uint64),
              rem_off=np.zeros(n + 1, np.uint32), rem_tok=np.zeros(1, np.uint64))


@pytest.mark.parametrize("read6", ["1", "0"])
def test_nif_gc_read_capacity_retry_runs_the_gc_once(eng, read6, monkeypatch):
    """nif/antidote_gpu_nif.c part_read_common: a GC read whose cached state
    does not fit the caller's buffer (ECAPACITY) is retried as a plain read
    -- AGN_READ_GC cleared, since the first pass already stored and pruned --
    so the resize of snapshot_insert_gc (:540-558) runs once: the key's
    Length / ListLen / counter equal a twin partition whose GC read had room.
    A buffer sized as the NIF now sizes it (key length + agn_batcher_state_bound
    + 16) fits on the first try."""
    monkeypatch.setenv("AGN_READ6", read6)
    d, K = 4, 2
    with OpLog(eng, _abi.SET_AW, d, K) as la, OpLog(eng, _abi.SET_AW, d, K) as lb, \
            Batcher(la, max_batch=4, cached=True) as ba, Batcher(lb, max_batch=4, cached=True) as bb:
        R = np.full(d, 1000, np.uint64)
        # six rounds of 10 adds, each read and cached (snapshots at 10 .. 60
        # pairs), then a GC read: it keeps the 3 newest snapshots and prunes
        # the ops below the oldest kept one (40), :523-527
        for b in range(6):
            for ol, bt in ((la, ba), (lb, bb)):
                _distinct_adds(ol, 0, 10, 10 * b, d)
                assert bt.read(0, R=R, out_cap=4096)["out_n"] == 10 * (b + 1)
        for bt in (ba, bb):
            bt.read(0, R=R, out_cap=4096, gc=True)
        for ol in (la, lb):
            _distinct_adds(ol, 0, 3, 100, d)
        length = int(la.key_meta([0])[0][0])
        assert length < 60 - 16
        R2 = np.full(d, 2000, np.uint64)
        ga = ba.read(0, R=R2, out_cap=4096, gc=True)
        first = bb.read(0, R=R2, out_cap=length + 16, gc=True, capacity_ok=True)
        assert first.get("ecapacity"), first
        gb = bb.read(0, R=R2, out_cap=first["out_n"] + 16, gc=False)   # the NIF's retry
        assert ga["out_n"] == gb["out_n"] == 63
        assert np.array_equal(ga["out_tag"], gb["out_tag"])
        for a, b in zip(la.key_meta(), lb.key_meta()):
            assert np.array_equal(a, b), (la.key_meta(), lb.key_meta())
        bound = ba.state_bound(0)
        assert bound >= 63
        g = ba.read(0, R=R2, out_cap=int(la.key_meta([0])[0][0]) + bound + 16, gc=True,
                    capacity_ok=True)
        assert not g.get("ecapacity") and g["out_n"] == 63


@pytest.mark.parametrize("typ", PAIR_TYPES)
def test_state_arena_repacks_vs_reference(eng, typ, monkeypatch):
    """A cached partition whose state arena starts tiny (AGN_SS_ARENA_INIT):
    the batcher re-packs / grows it again and again between batches
    (ensure_state_room: all-or-nothing commit of the moved references), and
    every served state still equals the reference's."""
    monkeypatch.setenv("AGN_SS_ARENA_INIT", "48")
    monkeypatch.setenv("AGN_READ6", "1")
    d, K, steps = 3, 16, 1500
    w = TagWorkload(91 + typ, K, typ, d)
    vn = po.MaterializerVnode(disk_log=True)
    quirk, served = set(), 0
    with OpLog(eng, typ, d, K) as ol, Batcher(ol, max_batch=8, cached=True) as bt:
        part = NifPartition(ol, bt, typ, d, False)
        for s in range(steps):
            key = int(w.rng.integers(0, K))
            if w.rng.random() < 0.6:
                c, ss, ct, oc, eff, entry = w.op(key)
                pay = po.Payload(key, PTYPE[typ], eff, vc(ss), (c, ct), s + 1)
                try:
                    vn.update(key, pay)
                except po.BadMatch:
                    quirk.add(key)
                part.update(key, pay, oc, entry, s + 1, np.uint64((1 << d) - 1), ss)
                if placeholder(vn, key):
                    quirk.add(key)
            else:
                R = w.read_clock(lag=300)
                got, _ = part.read(key, R)
                if key in quirk:
                    continue
                want = vn.read(key, PTYPE[typ], vc(R), po.IGNORE)
                assert want == got, (s, key, want, got)
                served += 1
    print(f"served={served} quirk={len(quirk)}/{K}")
    assert served > 400 and len(quirk) <= K // 4
