"""antidote_crdt_counter_b on the device, bit-exact against
tests/bcounter_model.py (whose filter and sums tests/test_bcounter_cpu.py pins
to the C oracle): agn_materialize over every kernel shape, chunk edge, slot
count and value-domain edge; the engine-owned op log (append, flush, read,
prune, load), agn_prune_ops and agn_log_ingest on the tag layout;
agn_read_cached and the read batcher against the lookup -> model ->
oracle_ss_store chain; the host mirror on the known answers."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import bcounter_model as bm
from antidote_amd import _abi
from antidote_amd import clocksi_materializer as cm
from antidote_amd import records
from antidote_amd.encode import (EncodedLog, EncodedRead, log_struct, result_struct,
                                 state_capacity)
from antidote_amd.engine import Batcher, OpLog
from test_ingest import Records, log_struct_of, oracle_ingest
from test_oplog import csr_key, segments
from test_prune import oracle_prune, thresholds
from test_ss_states import TagWorkload

pytestmark = pytest.mark.gpu

BC = _abi.COUNTER_B
TYP = records.COUNTER_B
GPU_CASES = bm.gpu_cases()
S = _abi.SNAPSHOT_THRESHOLD


def ptr(a):
    return None if a is None or (isinstance(a, np.ndarray) and a.size == 0) else a.ctypes.data


@functools.lru_cache(maxsize=None)
def case_and_model(idx):
    """A device batch and the model's answer, computed once per session."""
    log, req, cap, sparse, D = bm.make_case(GPU_CASES[idx])
    want, _incl, info = bm.model(log, req, sparse, cap)
    return log, req, cap, sparse, D, want, info


def free(*ds):
    for d in ds:
        for b in d.bufs.values():
            b.free()


def run_dev(eng, log, req, cap, sparse, drop_rem=False, call=None):
    dlog = eng.upload_log(log)
    if log.oc_mask is None:
        dlog.struct.oc_mask = None
    if drop_rem:
        dlog.struct.rem_off = dlog.struct.rem_tok = None
    dreq = eng.upload_read(req, sparse=sparse)
    dres = eng.alloc_result(req.n_req, log.n_dcs, sparse, cap_off=cap)
    (call or eng.materialize)(dlog, dreq, dres)
    eng.sync()
    got = eng.fetch_result(dres)
    free(dlog, dreq, dres)
    return got


@pytest.mark.parametrize("idx", range(len(GPU_CASES)), ids=[c[0] for c in GPU_CASES])
def test_materialize_vs_model(eng, idx):
    """agn_materialize: D over every LPO shape, key lengths at the chunk edges,
    dense and masked clocks, cold and warm reads, identity, permuted and
    repeated keys, reading txids, key_type mismatches, 1 to 257 distinct slots
    with and without base pairs, sums of 0 and wrapping sums, invalid entries
    included, excluded and past the overflow point, room 0 and one short; the
    bases through the CSR; rem_off present and NULL."""
    log, req, cap, sparse, D, want, _info = case_and_model(idx)
    got = run_dev(eng, log, req, cap, sparse, drop_rem=bool(idx % 2))
    bad = bm.compare_bc(D, got, want, sparse, req.n_req)
    assert not bad, bad[:8]


BASE_CASES = [i for i, c in enumerate(GPU_CASES) if bm.has_bases(c)]


@pytest.mark.parametrize("idx", BASE_CASES, ids=[GPU_CASES[i][0] for i in BASE_CASES])
def test_state_refs(eng, idx):
    """The same bases through AGN_SS_STATE references, for every case whose
    requests carry base pairs."""
    log, req, cap, sparse, D, want, _info = case_and_model(idx)
    assert len(req.base_tag) > 0
    got = run_dev(eng, log, bm.as_state_refs(req), cap, sparse)
    bad = bm.compare_bc(D, got, want, sparse, req.n_req)
    assert not bad, bad[:8]


def test_materialize_host_and_tune(eng):
    """agn_materialize_host stages the type's arrays (rem_off optional);
    agn_tune has one kernel for it (choice -1) and leaves its results."""
    idx = [c[0] for c in GPU_CASES].index("D8-dense-cold")
    log, req, cap, sparse, D, want, _info = case_and_model(idx)
    got = eng.materialize_host(log, req, sparse=sparse, cap_off=cap)
    assert not bm.compare_bc(D, got, want, sparse, req.n_req)
    got = eng.materialize_host(log, bm.as_state_refs(req), sparse=sparse, cap_off=cap)
    assert not bm.compare_bc(D, got, want, sparse, req.n_req)
    choice = []
    got = run_dev(eng, log, req, cap, sparse,
                  call=lambda a, b, c: choice.append(eng.tune(a, b, c, rounds=1)))
    assert not bm.compare_bc(D, got, want, sparse, req.n_req)
    ch = choice[0][0] if isinstance(choice[0], tuple) else choice[0]
    assert ch == -1


# ------------------------------------------------------------------ the op log
def renumber(log):
    """op ids as the engine-owned log assigns them: 1, 2, ... per key."""
    ids = np.concatenate([np.arange(1, int(b - a) + 1) for a, b in
                          zip(log.key_off[:-1], log.key_off[1:])] + [np.zeros(0, np.int64)])
    return EncodedLog(crdt_type=BC, n_dcs=log.n_dcs, key_off=log.key_off, key_type=log.key_type,
                      oc=log.oc, oc_mask=log.oc_mask, op_id=ids.astype(np.uint32), txid=log.txid,
                      tag=log.tag, add_tok=log.add_tok, rem_off=log.rem_off, rem_tok=log.rem_tok)


def append_all(ol, log, rng):
    """Every entry, keys interleaved, in random batches; rem_off NULL in every
    other batch (counter_b entries remove nothing)."""
    K = log.n_keys
    pos = log.key_off[:-1].astype(np.int64).copy()
    end = log.key_off[1:].astype(np.int64)
    order = []
    live = [k for k in range(K) if pos[k] < end[k]]
    while live:
        k = live[int(rng.integers(0, len(live)))]
        order.append((k, int(pos[k])))
        pos[k] += 1
        if pos[k] == end[k]:
            live.remove(k)
    i = b = 0
    while i < len(order):
        nb = int(rng.integers(1, 40))
        ks = np.array([k for k, _ in order[i:i + nb]], np.uint64)
        es = np.array([e for _, e in order[i:i + nb]], np.int64)
        i += nb
        kw = dict(oc=log.oc[es], txid=log.txid[es], tag=log.tag[es], add_tok=log.add_tok[es])
        if log.oc_mask is not None:
            kw["oc_mask"] = log.oc_mask[es]
        if b % 2:
            kw.update(rem_off=np.zeros(len(es) + 1, np.uint32), rem_tok=np.zeros(1, np.uint64))
        b += 1
        ids, _due = ol.append(ks, **kw)
        assert np.array_equal(ids, log.op_id[es]), "ids 1.. per key"
        if rng.random() < 0.3:
            ol.flush()


def oplog_read(eng, ol, req, cap, D, sparse):
    dreq = eng.upload_read(req, sparse=sparse)
    dres = eng.alloc_result(req.n_req, D, sparse, cap_off=cap)
    ol.read(dreq, dres)
    got = eng.fetch_result(dres)
    free(dreq, dres)
    return got


@pytest.mark.parametrize("D,sparse", [(8, False), (33, True)])
def test_oplog_path(eng, oracle_lib, D, sparse):
    """append (rem_off NULL and given) + flush + read equals agn_materialize on
    the same entries; agn_oplog_prune and agn_prune_ops (both output forms) equal
    oracle_prune_ops on the tag layout; agn_oplog_load from the flushed view
    into a twin serves the same reads."""
    rng = np.random.default_rng(D)
    log, req, cap = bm.bc_case(400 + D, D, lens=[0, 1, 5, 49, 50, 51, 70], reps=3, sparse=sparse,
                               warm=0.4, txid=0.3, base=0.4, n_slots=5)
    log = renumber(log)
    K, W = log.n_keys, (D + 63) // 64
    want, _incl, _info = bm.model(log, req, sparse, cap)
    with OpLog(eng, BC, D, K, sparse=sparse) as ol, OpLog(eng, BC, D, K, sparse=sparse) as ol2:
        append_all(ol, log, rng)
        view = ol.flush()
        assert view.crdt_type == BC and ol.stats()["entries"] == log.n_entries
        got = oplog_read(eng, ol, req, cap, D, sparse)
        assert not bm.compare_bc(D, got, want, sparse, req.n_req)
        # ---- GC: in the engine-owned log and out of place
        prune, thr, tm = thresholds(D + 17, log, sparse)
        pw, wflags, n_out = oracle_prune(oracle_lib, log, prune, thr, tm)
        assert 0 < n_out < log.n_entries
        bp, bt = eng.upload(prune), eng.upload(thr)
        btm = eng.upload(tm) if tm is not None else None
        fl = eng.empty(4 * K)
        ol.prune(bp.ptr, bt.ptr, btm.ptr if btm else None, fl.ptr)
        assert np.array_equal(eng.download(fl, np.uint32, (K,)), wflags)
        assert ol.stats()["entries"] == n_out
        view = ol.flush()
        segs = segments(eng, view, K, D, W, True, sparse)
        for k in range(K):
            for name, v in csr_key(pw, k, True).items():
                g = segs[k][name]
                assert (g == v) if name == "rems" else np.array_equal(np.asarray(g), np.asarray(v)), \
                    (k, name)
        dlog = eng.upload_log(log)
        if log.oc_mask is None:
            dlog.struct.oc_mask = None
        dout = eng.alloc_log_like(log)
        fl2, tot = eng.empty(4 * K), eng.empty(16)
        eng.prune_ops(dlog, bp.ptr, bt.ptr, btm.ptr if btm else None, dout, fl2.ptr, tot.ptr)
        eng.sync()
        assert int(eng.download(tot, np.uint64, (2,))[0]) == n_out
        assert np.array_equal(eng.download(fl2, np.uint32, (K,)), wflags)
        for name, (dt, shape) in dout.shapes.items():
            g = eng.download(dout.bufs[name], dt, shape)
            if name == "key_off":
                assert np.array_equal(g, pw[name])
            elif name == "rem_off":
                assert not g[:n_out + 1].any()
            elif name != "rem_tok":
                assert np.array_equal(g[:n_out], pw[name][:n_out]), name
        # ---- the segmented output form: each key at its input segment start
        dseg = eng.alloc_log_like(log)
        klen, kid = eng.empty(8 * K), eng.empty(4 * K)
        dseg.struct.key_len, dseg.struct.key_id0 = klen.ptr, kid.ptr
        fl3, tot3 = eng.empty(4 * K), eng.empty(16)
        eng.prune_ops(dlog, bp.ptr, bt.ptr, btm.ptr if btm else None, dseg, fl3.ptr, tot3.ptr)
        eng.sync()
        assert int(eng.download(tot3, np.uint64, (2,))[0]) == n_out
        assert np.array_equal(eng.download(fl3, np.uint32, (K,)), wflags)
        lens = eng.download(klen, np.uint64, (K,)).astype(np.int64)
        assert np.array_equal(lens, np.diff(pw["key_off"].astype(np.int64)))
        for name in ("op_id", "tag", "add_tok"):
            dt, shape = dseg.shapes[name]
            g = eng.download(dseg.bufs[name], dt, shape)
            for k in range(K):
                a, o = int(log.key_off[k]), int(pw["key_off"][k])
                assert np.array_equal(g[a:a + lens[k]], pw[name][o:o + lens[k]]), (name, k)
        # ---- the pruned log: read, recovery load, the same reads
        pruned = EncodedLog(crdt_type=BC, n_dcs=D, key_off=pw["key_off"], key_type=log.key_type,
                            oc=pw["oc"][:n_out],
                            oc_mask=None if log.oc_mask is None else pw["oc_mask"][:n_out],
                            op_id=pw["op_id"][:n_out], txid=pw["txid"][:n_out],
                            tag=pw["tag"][:n_out], add_tok=pw["add_tok"][:n_out],
                            rem_off=np.zeros(n_out + 1, np.uint32), rem_tok=np.zeros(1, np.uint64))
        cap_p = state_capacity(pruned, req)
        want_p, _, _ = bm.model(pruned, req, sparse, cap_p)
        got_p = oplog_read(eng, ol, req, cap_p, D, sparse)
        assert not bm.compare_bc(D, got_p, want_p, sparse, req.n_req)
        ol2.load(view)
        assert ol2.stats()["entries"] == n_out
        got_l = oplog_read(eng, ol2, req, cap_p, D, sparse)
        assert not bm.compare_bc(D, got_l, want_p, sparse, req.n_req)
        for b in (bp, bt, btm, fl, fl2, fl3, tot, tot3, klen, kid):
            if b is not None:
                b.free()
        free(dlog, dout, dseg)


@pytest.mark.parametrize("D,sparse", [(5, False), (16, True)])
def test_log_ingest_vs_oracle(eng, oracle_lib, D, sparse):
    """agn_log_ingest for the type: tag-type records whose removal ranges are
    empty and whose amounts include 0, every output array equal to
    oracle_log_ingest's (the C oracle's ingest is the type-free tag layout)."""
    rc = Records(D * 13 + BC, 1500, 200, D, _abi.REGISTER_LWW, sparse, 0.03)
    rc.with_max(D + 2)
    rng = np.random.default_rng(D)
    rc.add_tok = rng.choice(np.array(bm.AMT_EDGE + [5, 6], np.uint64), rc.n).astype(np.uint64)
    rc.rem_off, rc.rem_tok = np.zeros(rc.n + 1, np.uint32), np.zeros(1, np.uint64)
    want, n_out = oracle_ingest(oracle_lib, rc, 1)
    assert n_out > 100 and (rc.add_tok == 0).any()
    dev = {f: eng.upload(getattr(rc, f)) for f in ("kind", "txid", "key", "commit_dc",
                                                  "commit_time", "ss", "ss_mask", "tag",
                                                  "add_tok", "rem_off", "rem_tok")
           if getattr(rc, f) is not None}
    rs = rc.struct({f: b.ptr for f, b in dev.items()})
    outs = {f: (eng.empty(a.nbytes), a.dtype, a.shape) for f, a in want.items() if a is not None}
    os_ = log_struct_of({f: b.ptr for f, (b, _, _) in outs.items()})
    mt, mm = eng.upload(rc.max_t), (eng.upload(rc.max_m) if rc.max_m is not None else None)
    tot = eng.empty(16)
    rcode = eng.lib.agn_log_ingest(eng.ctx, C.byref(rs), BC, D, rc.K, mt.ptr,
                                   mm.ptr if mm else None, 1, C.byref(os_), tot.ptr, None)
    assert rcode == 0, eng.lib.agn_last_error()
    eng.sync()
    assert os_.crdt_type == BC
    assert int(eng.download(tot, np.uint64, (2,))[0]) == n_out
    for f, (b, dt, shape) in outs.items():
        g = eng.download(b, dt, shape)
        if f == "key_off":
            assert np.array_equal(g, want[f])
        elif f == "rem_off":
            assert not g[:n_out + 1].any()
        elif f != "rem_tok":
            assert np.array_equal(g[:n_out], want[f][:n_out]), f
    for b in list(dev.values()) + [x[0] for x in outs.values()] + [mt, mm, tot]:
        if b is not None:
            b.free()


# ------------------------------------------------------------------ cached reads
class Mirror:
    """read/6 on the host: the C oracle's snapshot cache (its value slot a
    handle into `states`, 0 = new()), the model as the materializer, the log
    as per-key entry lists pruned by oracle_prune_ops."""

    def __init__(self, lib, K, D):
        self.lib, self.K, self.D = lib, K, D
        self.arr = {"n": np.zeros(K, np.uint32), "clock": np.zeros((K, S, D), np.uint64),
                    "last_op": np.zeros((K, S), np.int64), "value": np.zeros((K, S), np.int64)}
        self.c = _abi.AgnSsCache()
        self.c.n_dcs, self.c.slots, self.c.n_keys = D, S, K
        self.c.n, self.c.clock, self.c.last_op, self.c.value = \
            (self.arr[x].ctypes.data for x in ("n", "clock", "last_op", "value"))
        self.states = [[]]
        self.ents = [[] for _ in range(K)]   # (oc row, op id, txid, tag, amount)
        self.ctr = np.zeros(K, np.int64)

    def append(self, k, oc, txid, tag, amt):
        self.ctr[k] += 1
        self.ents[k].append((np.asarray(oc, np.uint64).copy(), int(self.ctr[k]), txid, tag, amt))

    def log(self):
        K, D = self.K, self.D
        flat = [e for k in range(K) for e in self.ents[k]]
        n = len(flat)
        off = np.zeros(K + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in self.ents])
        return EncodedLog(crdt_type=BC, n_dcs=D, key_off=off, key_type=np.full(K, BC, np.uint8),
                          oc=np.array([e[0] for e in flat], np.uint64).reshape(n, D), oc_mask=None,
                          op_id=np.array([e[1] for e in flat], np.uint32),
                          txid=np.array([e[2] for e in flat], np.uint64),
                          tag=np.array([e[3] for e in flat], np.uint32),
                          add_tok=np.array([e[4] for e in flat], np.uint64),
                          rem_off=np.zeros(n + 1, np.uint32), rem_tok=np.zeros(1, np.uint64))

    def read(self, keys, R, gc):
        """A batch of distinct keys -> (model result, status, prune, thr, cap)."""
        lib, D, K = self.lib, self.D, self.K
        nr = len(keys)
        log = self.log()
        sct, ign = np.zeros((nr, D), np.uint64), np.zeros(nr + 8, np.uint8)
        base, first, status = np.zeros(nr, np.int64), np.zeros(nr + 8, np.uint8), \
            np.zeros(nr + 8, np.uint8)
        assert lib.oracle_ss_lookup(C.byref(self.c), nr, ptr(keys), ptr(R), None, ptr(sct), None,
                                    ptr(ign), ptr(base), ptr(first), ptr(status)) == 0
        bases = [self.states[int(h)] for h in base]   # stored states read back as bases
        req = EncodedRead(n_dcs=D, req_type=BC, keys=keys, R=R, R_mask=None, sct=sct,
                          sct_mask=None, sct_ignore=ign[:nr], txid=np.zeros(nr, np.uint64),
                          base_value=base, base_off=np.zeros(nr + 1, np.uint64),
                          base_tag=np.zeros(0, np.uint32), base_tok=np.zeros(0, np.uint64))
        lens = np.diff(log.key_off.astype(np.int64))[keys.astype(np.int64)]
        cap = np.concatenate([[0], np.cumsum(lens + 16)]).astype(np.uint64)
        res, _incl, _info = bm.model(log, req, False, cap, bases=bases)
        handle = np.zeros(nr, np.int64)
        for i in range(nr):
            if res.out_n[i]:
                o, m = int(cap[i]), int(res.out_n[i])
                self.states.append(list(zip(res.out_tag[o:o + m].tolist(),
                                            res.out_tok[o:o + m].tolist())))
                handle[i] = len(self.states) - 1
        rs = result_struct(res)
        rs.lastct_mask = None   # dense clocks, as the device store reads them
        ls = log_struct(log)
        ls.oc_mask = None
        prune, thr = np.zeros(K + 8, np.uint8), np.zeros((K, D), np.uint64)
        gc8 = np.concatenate([gc, np.zeros(8, np.uint8)])
        assert lib.oracle_ss_store(C.byref(self.c), C.byref(ls), nr, ptr(keys), ptr(first),
                                   ptr(status), ptr(gc8), C.byref(rs), ptr(handle), ptr(prune),
                                   ptr(thr), None) == 0
        prune = prune[:K]
        if prune.any():   # the GC the store selected, in the log
            pw, _fl, _n = oracle_prune(lib, log, np.concatenate([prune, np.zeros(8, np.uint8)]),
                                       thr, None)
            for k in np.nonzero(prune)[0]:
                a, b = int(pw["key_off"][k]), int(pw["key_off"][k + 1])
                self.ents[k] = [(pw["oc"][e].copy(), int(pw["op_id"][e]), int(pw["txid"][e]),
                                 int(pw["tag"][e]), int(pw["add_tok"][e])) for e in range(a, b)]
        return res, status[:nr], prune, thr, cap


N_SLOT_IDS = 6   # slots per key in the cached scripts: at most 6 pairs per state
ROUNDS = 17      # store rounds: enough for a snapshot list to pass 9 -> 10 and be collected


def bc_op(w, key):
    """A TagWorkload op's causal clock with a counter_b effect."""
    c, ss, ct, oc, _eff, _entry = w.op(key)
    return oc, int(w.rng.integers(0, N_SLOT_IDS)), int(w.rng.integers(-3, 4)) & bm.M64


def dev_append(ol, key, oc, txid, tag, amt):
    ids, _ = ol.append(np.array([key], np.uint64), oc.reshape(1, len(oc)).astype(np.uint64),
                       tag=np.array([tag], np.uint32), add_tok=np.array([amt], np.uint64),
                       txid=np.array([txid], np.uint64))
    return int(ids[0])


def test_read_cached_vs_chain(eng, oracle_lib):
    """agn_read_cached over rounds of whole-partition batches with GC reads,
    the snapshot lists growing through 9 -> 10 entries and collected, and a
    read below the collected range: results, status, prune flags, thresholds,
    the cache and the states in its arena against the lookup -> model ->
    oracle_ss_store chain."""
    K, D = 24, 3
    w = TagWorkload(123, K, _abi.REGISTER_MV)
    mir = Mirror(oracle_lib, K, D)
    with OpLog(eng, BC, D, K) as ol:
        bufs = {"n": eng.empty(4 * K), "clock": eng.empty(8 * K * S * D),
                "last_op": eng.empty(8 * K * S), "value": eng.empty(8 * K * S),
                "ctl": eng.empty(32), "status": eng.empty(K), "prune": eng.empty(K),
                "thr": eng.empty(8 * K * D)}
        for x in ("n", "ctl", "thr", "value", "clock", "last_op"):
            eng.lib.agn_memset_d(eng.ctx, bufs[x].ptr, 0, bufs[x].nbytes, None)
        acap = 1 << 13
        arena = [eng.empty(4 * acap), eng.empty(8 * acap)]
        c = _abi.AgnSsCache()
        c.n_dcs, c.slots, c.n_keys = D, S, K
        c.n, c.clock, c.last_op, c.value = (bufs[x].ptr for x in ("n", "clock", "last_op", "value"))
        c.state_tag, c.state_tok, c.state_cap, c.state_ctl = arena[0].ptr, arena[1].ptr, acap, \
            bufs["ctl"].ptr
        keys = np.arange(K, dtype=np.uint64)
        dkeys = eng.upload(keys)
        s = hits = pruned = logs = 0
        sizes, shrank = set(), False
        old_R = None
        for rnd in range(ROUNDS):
            for _ in range(4 * K):
                key = int(w.rng.integers(0, K))
                oc, tag, amt = bc_op(w, key)
                s += 1
                mir.append(key, oc, s, tag, amt)
                assert dev_append(ol, key, oc, s, tag, amt) == mir.ctr[key]
            view = ol.flush()
            R = np.tile(w.read_clock(lag=100).astype(np.uint64), (K, 1))
            if rnd == 0:
                old_R = R.copy()
            if rnd == ROUNDS - 1:   # below every key's collected range
                R = old_R
            gc = (w.rng.random(K) < 0.2).astype(np.uint8)
            n_before = mir.arr["n"].copy()
            want, wst, wpr, wthr, cap = mir.read(keys, R, gc)
            sizes |= set(mir.arr["n"].tolist()) | set(n_before.tolist())
            # a list of 9 took its 10th entry and was collected
            shrank = shrank or bool(((mir.arr["n"] < n_before) & (n_before == S - 1)).any())
            dres = eng.alloc_result(K, D, sparse=False, cap_off=cap)
            dR, dgc = eng.upload(R), eng.upload(gc)
            eng.read_cached(c, view, K, dkeys.ptr, dR.ptr, None, dgc.ptr, dres, bufs["status"].ptr,
                            bufs["prune"].ptr, bufs["thr"].ptr)
            eng.sync()
            got = eng.fetch_result(dres)
            bad = bm.compare_bc(D, got, want, False, K)
            assert not bad, (rnd, bad[:8])
            assert np.array_equal(eng.download(bufs["status"], np.uint8, (K,)), wst), rnd
            gp = eng.download(bufs["prune"], np.uint8, (K,))
            assert np.array_equal(gp & 1, wpr), rnd
            sel = np.nonzero(wpr)[0]
            assert np.array_equal(eng.download(bufs["thr"], np.uint64, (K, D))[sel], wthr[sel]), rnd
            n = eng.download(bufs["n"], np.uint32, (K,))
            assert np.array_equal(n, mir.arr["n"]), rnd
            live = np.arange(S)[None, :] < n[:, None]
            for name, dt, shape in (("clock", np.uint64, (K, S, D)), ("last_op", np.int64, (K, S))):
                x = eng.download(bufs[name], dt, shape)
                assert np.array_equal(x[live], mir.arr[name][live]), (rnd, name)
            refs = eng.download(bufs["value"], np.int64, (K, S))
            atag = eng.download(arena[0], np.uint32, (acap,))
            atok = eng.download(arena[1], np.uint64, (acap,))
            for k, j in zip(*np.nonzero(live)):
                start, pairs = _abi.ss_state_unpack(int(refs[k, j]))
                st = mir.states[int(mir.arr["value"][k, j])]
                have = list(zip(atag[start:start + pairs].tolist(),
                                atok[start:start + pairs].tolist()))
                assert have == st, (rnd, k, j)
            ctl = eng.download(bufs["ctl"], np.uint64, (4,))
            assert ctl[2] == 0, "state arena overflow"
            ol.prune(bufs["prune"].ptr, bufs["thr"].ptr)
            assert ol.stats()["entries"] == sum(len(x) for x in mir.ents)
            hits += int((wst == _abi.SS_HIT).sum())
            logs += int((wst == _abi.SS_LOG).sum())
            pruned += int(wpr.sum())
            for b in (dR, dgc):
                b.free()
            free(dres)
        assert hits > K // 2 and pruned > 0 and logs > 0
        assert sizes >= set(range(0, S)) and shrank, sizes
        for b in list(bufs.values()) + arena + [dkeys]:
            b.free()


@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "cached"])
def test_batcher_vs_chain(eng, oracle_lib, cached):
    """agn_batcher_create[_cached] accept the type (the kernel sequence: no
    fused pass serves it).  Rounds of appends, then 8 threads read the 8 keys
    at once into shared batches: caller bases (uncached) or the device
    snapshot cache with GC reads, its lists growing through 9 -> 10, and a
    last round below the collected range (cached)."""
    K, D = 8, 4
    w = TagWorkload(321 + cached, K, _abi.REGISTER_MV, D)
    mir = Mirror(oracle_lib, K, D)
    reads = hits = logs = 0
    sizes, s, shrank = set(), 0, False
    keys = np.arange(K, dtype=np.uint64)
    old_R = None
    with OpLog(eng, BC, D, K) as ol, \
            Batcher(ol, max_batch=8, max_wait_us=20000, cached=cached) as bt:
        for rnd in range(ROUNDS if cached else 5):
            for _ in range(5 * K):
                key = int(w.rng.integers(0, K))
                oc, tag, amt = bc_op(w, key)
                s += 1
                mir.append(key, oc, s, tag, amt)
                assert dev_append(ol, key, oc, s, tag, amt) == mir.ctr[key]
            R = w.read_clock(lag=100).astype(np.uint64)
            if rnd == 0:
                old_R = R.copy()
            if cached and rnd == ROUNDS - 1:
                R = old_R
            R2 = np.tile(R, (K, 1))
            gcs = (w.rng.random(K) < 0.25).astype(np.uint8)
            if cached:
                n_before = mir.arr["n"].copy()
                want, wst, _wpr, _thr, cap = mir.read(keys, R2, gcs)
                sizes |= set(mir.arr["n"].tolist())
                shrank = shrank or bool(((mir.arr["n"] < n_before) & (n_before == S - 1)).any())
                kws = [dict(gc=bool(gcs[k])) for k in range(K)]
            else:
                bases = [[(int(t), int(w.rng.integers(-5, 6)) & bm.M64)
                          for t in w.rng.choice(N_SLOT_IDS + 2, int(w.rng.integers(0, 4)),
                                                replace=False)] for _ in range(K)]
                log = mir.log()
                req = EncodedRead(n_dcs=D, req_type=BC, keys=keys, R=R2, R_mask=None, sct=None,
                                  sct_mask=None, sct_ignore=None, txid=np.zeros(K, np.uint64),
                                  base_value=None, base_off=None, base_tag=None, base_tok=None)
                cap = (np.arange(K + 1) * 16).astype(np.uint64)
                want, _incl, _info = bm.model(log, req, False, cap, bases=bases)
                kws = [dict(base_tag=[t for t, _ in b], base_tok=[v for _, v in b]) if b else {}
                       for b in bases]
            got = [None] * K

            def one(k):
                got[k] = bt.read(k, R=R, out_cap=16, **kws[k])
            th = [threading.Thread(target=one, args=(k,)) for k in range(K)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            for k in range(K):
                g = got[k]
                assert g is not None, (rnd, k)
                reads += 1
                fl = int(want.flags[k])
                assert g["flags"] == fl and g["count"] == int(want.count[k]), (rnd, k)
                assert g["hole"] == int(want.hole[k]), (rnd, k)
                if not fl & _abi.F_CT_IGNORE:
                    assert np.array_equal(g["lastct"], want.lastct[k]), (rnd, k)
                if cached:
                    assert g["status"] == int(wst[k]), (rnd, k)
                    hits += int(wst[k] == _abi.SS_HIT)
                    logs += int(wst[k] == _abi.SS_LOG)
                    if g["status"] == _abi.SS_LOG:
                        continue
                m, o = int(want.out_n[k]), int(cap[k])
                assert g["out_n"] == m, (rnd, k)
                assert g["out_tag"].tolist() == want.out_tag[o:o + m].tolist(), (rnd, k)
                assert g["out_tok"].tolist() == want.out_tok[o:o + m].tolist(), (rnd, k)
        st = bt.stats()
        assert st["reads"] == reads and st["batches"] < reads, st
        if cached:
            assert ol.stats()["entries"] == sum(len(x) for x in mir.ents)
            assert bt.path_stats()["fused"] == 0
    assert reads >= 40
    assert not cached or (hits > 0 and logs > 0 and shrank and sizes >= set(range(1, S)))


# ------------------------------------------------------------------ the host mirror
def _sequential(ops):
    st = ({}, {})
    for op in ops:
        st = bm.update(bm.kat_effect(op), st)
    return bm.as_orddicts(st)


@pytest.mark.parametrize("c", bm.kats()["cases"], ids=lambda c: c["name"])
def test_mirror_kats(eng, c):
    """materialize, materialize_batch, materialize_eager and permissions on
    the suites' sequences, for every transfer size they leave open."""
    variants = [c["ops"]]
    for v in c.get("transfer_range", []):
        ops = [list(o) for o in c["ops"]]
        ops[c["transfer_at"]][1] = v
        variants.append(ops)
    reads = [bm.kat_read(ops) for ops in variants]
    rb = cm.materialize_batch(TYP, reads)
    for ops, (txid, R, resp), b in zip(variants, reads, rb):
        want = _sequential(ops)
        r = cm.materialize(TYP, txid, R, resp)
        assert r == b and r[0] == "ok" and r[1] == want, r
        assert r[2] == len(ops) and r[5] == len(ops) and r[4] is (len(ops) > 0)
        assert cm.value(TYP, r[1]) == want
        assert cm.permissions(r[1]) == c["permissions"]
        effects = [bm.kat_effect(op) for op in ops]
        assert cm.materialize_eager(TYP, cm.new(TYP), effects) == want
        # from a stored state: the first op as the base, the rest on top
        if ops:
            assert cm.materialize_eager(TYP, _sequential(ops[:1]), effects[1:]) == want


def test_mirror_local_permissions_invalid_effect_and_new(eng):
    lp = bm.kats()["local_permissions"]
    st = cm.materialize_eager(TYP, cm.new(TYP), [bm.kat_effect(op) for op in lp["ops"]])
    for ident, want in lp["expect"].items():
        assert cm.local_permissions(ident, st) == want
    assert cm.materialize_eager(TYP, cm.new(TYP), []) == ([], [])
    kept = ([(("a", "a"), 0)], [("b", -2)])
    assert cm.materialize_eager(TYP, kept, []) == kept
    good = (("increment", 3), "a")
    for bad in ((("increment", 1 << 63), "a"), (("reset", 1), "a"), "increment"):
        assert cm.materialize_eager(TYP, cm.new(TYP), [good, bad, good]) == \
            ("error", ("unexpected_operation", bad, TYP))
    # a sum of 0 keeps its key; sums wrap as int64
    assert cm.materialize_eager(TYP, cm.new(TYP), [good, (("increment", -3), "a"),
                                                   (("decrement", 0), "b")]) == \
        ([(("a", "a"), 0)], [("b", 0)])
    big = (1 << 63) - 1
    assert cm.materialize_eager(TYP, ([(("a", "a"), big)], []), [(("increment", 1), "a")]) == \
        ([(("a", "a"), -(1 << 63))], [])


def test_gen_dev_matches_host(eng):
    """agn_gen_dev builds the host generator's log for the type, and the
    kernel reads it: no request fails, most include ops, every state's sums
    are those of the included entries."""
    from antidote_amd.engine import free_gen_host, gen_host, host_view
    K, N, D, E = 200, 64, 8, 4
    cfg = _abi.AgnGenCfg(crdt_type=BC, n_dcs=D, n_keys=K, ops_per_key=N, n_elems=E, seed=5,
                         key_base=0, key_stride=1)
    hl, hr = gen_host(cfg)
    dl_, dr = eng.gen_dev(cfg)
    try:
        for f, dt, n in (("oc", np.uint64, K * N * D), ("op_id", np.uint32, K * N),
                         ("tag", np.uint32, K * N), ("add_tok", np.uint64, K * N),
                         ("rem_off", np.uint32, K * N + 1), ("key_off", np.uint64, K + 1)):
            g = np.empty(n, dt)
            assert eng.lib.agn_memcpy_d2h(eng.ctx, g.ctypes.data, getattr(dl_, f), g.nbytes,
                                          None) == 0
            eng.sync()
            assert np.array_equal(g, host_view(getattr(hl, f), dt, n)), f
        assert dl_.crdt_type == BC and not dl_.eff
        cap = (np.arange(K + 1) * E).astype(np.uint64)
        dres = eng.alloc_result(K, D, sparse=False, cap_off=cap)
        eng.materialize(dl_, dr, dres)
        eng.sync()
        got = eng.fetch_result(dres)
        assert not (got.flags & (_abi.F_ERR_UNEXPECTED | _abi.F_ERR_CAPACITY |
                                 _abi.F_ERR_CORRUPTED)).any()
        assert 0.2 < got.count.mean() / N < 0.95
        assert (got.out_n <= E).all() and (got.out_n[got.count >= 16] == E).mean() > 0.5
        for i in range(K):
            o, m = int(cap[i]), int(got.out_n[i])
            assert (np.diff(got.out_tag[o:o + m].astype(np.int64)) > 0).all()
        free(dres)
    finally:
        eng.free_gen(dl_, dr)
        free_gen_host(hl, hr)
