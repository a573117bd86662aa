"""antidote_crdt_register_lww on the device, bit-exact against tests/lww_model.py
(whose filter tests/test_lww_cpu.py pins to the C oracle): agn_materialize over
every kernel shape, chunk edge and value-domain edge; the engine-owned op log
(append, flush, read, prune, load), agn_prune_ops and agn_log_ingest on the tag
layout; agn_read_cached and the read batcher against the lookup -> model ->
oracle_ss_store chain; the host mirror on the known answers."""
import ctypes as C
import functools

import numpy as np
import pytest

import lww_model as lm
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

LWW = _abi.REGISTER_LWW
GPU_CASES = lm.gpu_cases()
S = _abi.SNAPSHOT_THRESHOLD


def ptr(a):
    return None if a is None or (isinstance(a, np.ndarray) and a.size == 0) else a.ctypes.data


@functools.lru_cache(maxsize=None)
def case_and_model(idx, room0=False):
    """A device batch and the model's answer, computed once per session."""
    _id, seed, D, sparse, kw = GPU_CASES[idx]
    log, req, cap = lm.lww_case(seed, D, reps=lm.GPU_REPS, **kw)
    if room0:  # every third request comes with no room
        room = np.diff(cap.astype(np.int64))
        room[::3] = 0
        cap = np.concatenate([[0], np.cumsum(room)]).astype(np.uint64)
    want, _incl, info = lm.model(log, req, sparse, cap)
    return log, req, cap, want, info


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


@pytest.mark.parametrize("load", ["early", "late"])
@pytest.mark.parametrize("idx", range(len(GPU_CASES)), ids=[c[0] for c in GPU_CASES])
def test_materialize_vs_model(eng, monkeypatch, idx, load):
    """agn_materialize: D over every LPO shape, key lengths at the chunk edges,
    dense and masked clocks, cold and warm reads, identity and permuted keys,
    reading txids, key_type mismatches, invalid tags included and excluded,
    bases through the CSR; both orders of the ts / tag loads."""
    monkeypatch.setenv("AGN_LWW_LOAD", load)
    log, req, cap, want, _info = case_and_model(idx)
    _id, _seed, D, sparse, _kw = GPU_CASES[idx]
    got = run_dev(eng, log, req, cap, sparse, drop_rem=(load == "late"))
    bad = lm.compare_lww(D, got, want, sparse, req.n_req)
    assert not bad, bad[:8]


@pytest.mark.parametrize("idx", range(len(GPU_CASES)), ids=[c[0] for c in GPU_CASES])
def test_state_refs_and_capacity(eng, idx):
    """The same bases through AGN_SS_STATE references, and the capacity case:
    room 0 with one live pair is AGN_F_ERR_CAPACITY with out_n = 1."""
    log, req, cap, want, _info = case_and_model(idx)
    _id, _seed, D, sparse, _kw = GPU_CASES[idx]
    got = run_dev(eng, log, lm.as_state_refs(req), cap, sparse)
    bad = lm.compare_lww(D, got, want, sparse, req.n_req)
    assert not bad, bad[:8]
    log, req, cap0, want0, _ = case_and_model(idx, True)
    assert (want0.flags & _abi.F_ERR_CAPACITY).any()
    got = run_dev(eng, log, req, cap0, sparse)
    bad = lm.compare_lww(D, got, want0, sparse, req.n_req)
    assert not bad, bad[:8]


def test_value_domain_reached():
    """The domain batches: every edge timestamp and tag is a candidate, the
    winners spread over them, and ties at an edge timestamp occur."""
    n = 0
    for idx, c in enumerate(GPU_CASES):
        if not c[4].get("domain"):
            continue
        n += 1
        log, req, cap, want, _info = case_and_model(idx)
        assert set(log.add_tok.tolist()) | set(req.base_tok.tolist()) >= set(lm.TS_EDGE)
        assert set(log.tag.tolist()) >= set(lm.TAG_EDGE)
        live = (want.out_n == 1) & ((want.flags & _abi.F_ERR_CAPACITY) == 0)
        o = cap[:-1][live].astype(np.int64)
        assert len(set(want.out_tok[o].tolist())) >= 4 and (1 << 64) - 1 in want.out_tok[o]
        assert set(want.out_tag[o].tolist()) >= {0, 1, 0xFFFFFFFE}
        assert (want.flags & _abi.F_TS_TIE).any()
    assert n == 2


def test_materialize_host_and_tune(eng):
    """agn_materialize_host stages the type's arrays (rem_off optional);
    agn_tune has one kernel for it (choice -1) and leaves its results."""
    idx = 2
    log, req, cap, want, _info = case_and_model(idx)
    _id, _seed, D, sparse, _kw = GPU_CASES[idx]
    got = eng.materialize_host(log, req, sparse=sparse, cap_off=cap)
    assert not lm.compare_lww(D, got, want, sparse, req.n_req)
    got = eng.materialize_host(log, lm.as_state_refs(req), sparse=sparse, cap_off=cap)
    assert not lm.compare_lww(D, got, want, sparse, req.n_req)
    choice = []
    got = run_dev(eng, log, req, cap, sparse,
                  call=lambda a, b, c: choice.append(eng.tune(a, b, c, rounds=1)))
    assert not lm.compare_lww(D, got, want, sparse, req.n_req)
    ch = choice[0][0] if isinstance(choice[0], tuple) else choice[0]
    assert ch == -1


# ------------------------------------------------------------------ the op log
def renumber(log):
    """op ids as the engine-owned log assigns them: 1, 2, ... per key."""
    ids = np.concatenate([np.arange(1, int(b - a) + 1) for a, b in
                          zip(log.key_off[:-1], log.key_off[1:])] + [np.zeros(0, np.int64)])
    return EncodedLog(crdt_type=LWW, n_dcs=log.n_dcs, key_off=log.key_off, key_type=log.key_type,
                      oc=log.oc, oc_mask=log.oc_mask, op_id=ids.astype(np.uint32), txid=log.txid,
                      tag=log.tag, add_tok=log.add_tok, rem_off=log.rem_off, rem_tok=log.rem_tok)


def append_all(ol, log, rng):
    """Every entry, keys interleaved, in random batches; rem_off NULL in every
    other batch (register_lww entries remove nothing)."""
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
    """append + flush + read equals agn_materialize on the same entries;
    agn_oplog_prune and agn_prune_ops equal oracle_prune_ops on the tag layout;
    agn_oplog_load from the flushed view serves the same reads."""
    rng = np.random.default_rng(D)
    log, req, cap = lm.lww_case(400 + D, D, lens=[0, 1, 5, 49, 50, 51, 70], reps=3, sparse=sparse,
                                warm=0.4, txid=0.3, base=0.4)
    log = renumber(log)
    K, W = log.n_keys, (D + 63) // 64
    want, _incl, _info = lm.model(log, req, sparse, cap)
    with OpLog(eng, LWW, D, K, sparse=sparse) as ol, OpLog(eng, LWW, D, K, sparse=sparse) as ol2:
        append_all(ol, log, rng)
        view = ol.flush()
        assert view.crdt_type == LWW and ol.stats()["entries"] == log.n_entries
        got = oplog_read(eng, ol, req, cap, D, sparse)
        assert not lm.compare_lww(D, got, want, sparse, req.n_req)
        got_m = run_dev(eng, log, req, cap, sparse)
        assert not lm.compare_lww(D, got, got_m, sparse, req.n_req)
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
        # ---- the pruned log: read, recovery load, the same reads
        pruned = EncodedLog(crdt_type=LWW, n_dcs=D, key_off=pw["key_off"], key_type=log.key_type,
                            oc=pw["oc"][:n_out],
                            oc_mask=None if log.oc_mask is None else pw["oc_mask"][:n_out],
                            op_id=pw["op_id"][:n_out], txid=pw["txid"][:n_out],
                            tag=pw["tag"][:n_out], add_tok=pw["add_tok"][:n_out],
                            rem_off=np.zeros(n_out + 1, np.uint32), rem_tok=np.zeros(1, np.uint64))
        cap_p = state_capacity(pruned, req)
        want_p, _, _ = lm.model(pruned, req, sparse, cap_p)
        got_p = oplog_read(eng, ol, req, cap_p, D, sparse)
        assert not lm.compare_lww(D, got_p, want_p, sparse, req.n_req)
        ol2.load(view)
        assert ol2.stats()["entries"] == n_out
        got_l = oplog_read(eng, ol2, req, cap_p, D, sparse)
        assert not lm.compare_lww(D, got_l, want_p, sparse, req.n_req)
        for b in (bp, bt, btm, fl, fl2, tot):
            if b is not None:
                b.free()
        free(dlog, dout)


@pytest.mark.parametrize("D,sparse", [(5, False), (16, True)])
def test_log_ingest_vs_oracle(eng, oracle_lib, D, sparse):
    """agn_log_ingest for the type: tag-type records whose removal ranges are
    empty, every output array equal to oracle_log_ingest's."""
    rc = Records(D * 13 + LWW, 1500, 200, D, LWW, sparse, 0.03)
    rc.with_max(D + 2)
    rc.add_tok = np.random.default_rng(D).integers(0, 1 << 63, rc.n).astype(np.uint64)
    rc.rem_off, rc.rem_tok = np.zeros(rc.n + 1, np.uint32), np.zeros(1, np.uint64)
    want, n_out = oracle_ingest(oracle_lib, rc, 1)
    assert n_out > 100
    dev = {f: eng.upload(getattr(rc, f)) for f in ("kind", "txid", "key", "commit_dc",
                                                  "commit_time", "ss", "ss_mask", "tag",
                                                  "add_tok", "rem_off", "rem_tok")
           if getattr(rc, f) is not None}
    rs = rc.struct({f: b.ptr for f, b in dev.items()})
    outs = {f: (eng.empty(a.nbytes), a.dtype, a.shape) for f, a in want.items() if a is not None}
    os_ = log_struct_of({f: b.ptr for f, (b, _, _) in outs.items()})
    mt, mm = eng.upload(rc.max_t), (eng.upload(rc.max_m) if rc.max_m is not None else None)
    tot = eng.empty(16)
    rcode = eng.lib.agn_log_ingest(eng.ctx, C.byref(rs), LWW, D, rc.K, mt.ptr,
                                   mm.ptr if mm else None, 1, C.byref(os_), tot.ptr, None)
    assert rcode == 0, eng.lib.agn_last_error()
    eng.sync()
    assert os_.crdt_type == LWW
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
        self.states = [None]
        self.ents = [[] for _ in range(K)]   # (oc row, op id, txid, tag, ts)
        self.ctr = np.zeros(K, np.int64)

    def append(self, k, oc, txid, tag, ts):
        self.ctr[k] += 1
        self.ents[k].append((np.asarray(oc, np.uint64).copy(), int(self.ctr[k]), txid, tag, ts))

    def log(self):
        K, D = self.K, self.D
        flat = [e for k in range(K) for e in self.ents[k]]
        n = len(flat)
        off = np.zeros(K + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in self.ents])
        return EncodedLog(crdt_type=LWW, n_dcs=D, key_off=off, key_type=np.full(K, LWW, np.uint8),
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
        bases = [self.states[int(h)] for h in base]
        req = EncodedRead(n_dcs=D, req_type=LWW, keys=keys, R=R, R_mask=None, sct=sct,
                          sct_mask=None, sct_ignore=ign[:nr], txid=np.zeros(nr, np.uint64),
                          base_value=base, base_off=np.zeros(nr + 1, np.uint64),
                          base_tag=np.zeros(0, np.uint32), base_tok=np.zeros(0, np.uint64))
        lens = np.diff(log.key_off.astype(np.int64))[keys.astype(np.int64)]
        cap = np.concatenate([[0], np.cumsum(lens + 2)]).astype(np.uint64)
        res, _incl, _info = lm.model(log, req, False, cap, bases=bases)
        handle = np.zeros(nr, np.int64)
        for i in range(nr):
            if res.out_n[i]:
                o = int(cap[i])
                self.states.append((int(res.out_tag[o]), int(res.out_tok[o])))
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


def lww_op(w, key):
    """A TagWorkload op's causal clock with a register_lww effect."""
    c, ss, ct, oc, _eff, _entry = w.op(key)
    return oc, int(w.rng.integers(0, 3)), int(w.rng.integers(1, 9))


def dev_append(ol, key, oc, txid, tag, ts):
    ids, _ = ol.append(np.array([key], np.uint64), oc.reshape(1, len(oc)).astype(np.uint64),
                       tag=np.array([tag], np.uint32), add_tok=np.array([ts], np.uint64),
                       txid=np.array([txid], np.uint64))
    return int(ids[0])


def test_read_cached_vs_chain(eng, oracle_lib):
    """agn_read_cached over three rounds of whole-partition batches with GC
    reads: results, status, prune flags, thresholds, the cache and the states
    in its arena against the lookup -> model -> oracle_ss_store chain."""
    K, D = 48, 3
    w = TagWorkload(123, K, _abi.REGISTER_MV)
    mir = Mirror(oracle_lib, K, D)
    with OpLog(eng, LWW, D, K) as ol:
        bufs = {"n": eng.empty(4 * K), "clock": eng.empty(8 * K * S * D),
                "last_op": eng.empty(8 * K * S), "value": eng.empty(8 * K * S),
                "ctl": eng.empty(32), "status": eng.empty(K), "prune": eng.empty(K),
                "thr": eng.empty(8 * K * D)}
        for x in ("n", "ctl", "thr", "value", "clock", "last_op"):
            eng.lib.agn_memset_d(eng.ctx, bufs[x].ptr, 0, bufs[x].nbytes, None)
        acap = 1 << 12
        arena = [eng.empty(4 * acap), eng.empty(8 * acap)]
        c = _abi.AgnSsCache()
        c.n_dcs, c.slots, c.n_keys = D, S, K
        c.n, c.clock, c.last_op, c.value = (bufs[x].ptr for x in ("n", "clock", "last_op", "value"))
        c.state_tag, c.state_tok, c.state_cap, c.state_ctl = arena[0].ptr, arena[1].ptr, acap, \
            bufs["ctl"].ptr
        keys = np.arange(K, dtype=np.uint64)
        dkeys = eng.upload(keys)
        s = hits = pruned = 0
        for rnd in range(3):
            for _ in range(8 * K):
                key = int(w.rng.integers(0, K))
                oc, tag, ts = lww_op(w, key)
                s += 1
                mir.append(key, oc, s, tag, ts)
                assert dev_append(ol, key, oc, s, tag, ts) == mir.ctr[key]
            view = ol.flush()
            R = np.tile(w.read_clock(lag=300).astype(np.uint64), (K, 1))
            gc = (w.rng.random(K) < 0.3).astype(np.uint8)
            want, wst, wpr, wthr, cap = mir.read(keys, R, gc)
            dres = eng.alloc_result(K, D, sparse=False, cap_off=cap)
            dR, dgc = eng.upload(R), eng.upload(gc)
            eng.read_cached(c, view, K, dkeys.ptr, dR.ptr, None, dgc.ptr, dres, bufs["status"].ptr,
                            bufs["prune"].ptr, bufs["thr"].ptr)
            eng.sync()
            got = eng.fetch_result(dres)
            bad = lm.compare_lww(D, got, want, False, K)
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
                have = (int(atag[start]), int(atok[start])) if pairs else None
                assert pairs <= 1 and have == st, (rnd, k, j)
            ctl = eng.download(bufs["ctl"], np.uint64, (4,))
            assert ctl[2] == 0, "state arena overflow"
            ol.prune(bufs["prune"].ptr, bufs["thr"].ptr)
            assert ol.stats()["entries"] == sum(len(x) for x in mir.ents)
            hits += int((wst == _abi.SS_HIT).sum())
            pruned += int(wpr.sum())
            for b in (dR, dgc):
                b.free()
            free(dres)
        assert hits > K // 2 and pruned > 0
        for b in list(bufs.values()) + arena + [dkeys]:
            b.free()


@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "cached"])
def test_batcher_vs_chain(eng, oracle_lib, cached):
    """agn_batcher_create[_cached] accept the type (the kernel sequence: the
    fused tags pass does not serve it); a few dozen reads, with caller bases
    (uncached) or the device snapshot cache and GC reads (cached)."""
    K, D = 8, 4
    w = TagWorkload(321 + cached, K, _abi.REGISTER_MV, D)
    mir = Mirror(oracle_lib, K, D)
    reads = hits = 0
    with OpLog(eng, LWW, D, K) as ol, Batcher(ol, max_batch=8, cached=cached) as bt:
        for s in range(1, 500):
            key = int(w.rng.integers(0, K))
            if w.rng.random() < 0.88:
                oc, tag, ts = lww_op(w, key)
                mir.append(key, oc, s, tag, ts)
                assert dev_append(ol, key, oc, s, tag, ts) == mir.ctr[key]
                continue
            R = w.read_clock(lag=200).astype(np.uint64)
            keys, R2 = np.array([key], np.uint64), R.reshape(1, D)
            if cached:
                gc = bool(w.rng.random() < 0.3)
                want, wst, _wpr, _thr, cap = mir.read(keys, R2, np.array([gc], np.uint8))
                g = bt.read(key, R=R, out_cap=2, gc=gc)
                assert g["status"] == int(wst[0]), s
                hits += int(wst[0] == _abi.SS_HIT)
            else:
                base = (int(w.rng.integers(0, 3)), int(w.rng.integers(1, 11))) \
                    if w.rng.random() < 0.5 else None
                log = mir.log()
                req = EncodedRead(n_dcs=D, req_type=LWW, keys=keys, R=R2, R_mask=None, sct=None,
                                  sct_mask=None, sct_ignore=None, txid=np.zeros(1, np.uint64),
                                  base_value=None, base_off=None, base_tag=None, base_tok=None)
                cap = np.array([0, 1], np.uint64)
                want, _incl, _info = lm.model(log, req, False, cap, bases=[base])
                kw = {} if base is None else dict(base_tag=[base[0]], base_tok=[base[1]])
                g = bt.read(key, R=R, out_cap=2, **kw)
            reads += 1
            fl = int(want.flags[0])
            assert g["flags"] == fl and g["count"] == int(want.count[0]), s
            assert g["hole"] == int(want.hole[0]), s
            if not fl & _abi.F_CT_IGNORE:
                assert np.array_equal(g["lastct"], want.lastct[0]), s
            if cached and g["status"] == _abi.SS_LOG:
                continue
            assert g["out_n"] == int(want.out_n[0]), s
            if g["out_n"]:
                assert (int(g["out_tag"][0]), int(g["out_tok"][0])) == \
                    (int(want.out_tag[0]), int(want.out_tok[0])), s
        if cached:
            assert ol.stats()["entries"] == sum(len(x) for x in mir.ents)
    assert reads >= 36 and (hits > 0 or not cached)


# ------------------------------------------------------------------ the host mirror
@pytest.mark.parametrize("c", lm.kats(), ids=lambda c: c["name"])
def test_mirror_kats(eng, c):
    txid, R, resp, want = lm.kat_read(c)
    r = cm.materialize(records.REGISTER_LWW, txid, R, resp)
    assert r[0] == "ok" and r[1] == want, r
    assert r[2] == c["hole"] and r[5] == c["count"] and r[4] is (c["count"] > 0)
    assert cm.value(records.REGISTER_LWW, r[1]) == lm._val(c["value"])
    rb = cm.materialize_batch(records.REGISTER_LWW, [(txid, R, resp)] * 2)
    assert rb == [r, r]
    if c["sct"] is None:   # every op inside the snapshot: the eager fold
        effects = [p.op_param for _i, p in records.ops_oldest_first(resp.ops_list)
                   if p.commit_time[1] <= c["read"]]
        assert cm.materialize_eager(records.REGISTER_LWW, resp.materialized_snapshot.value,
                                    effects) == want


def test_mirror_invalid_effect_and_new(eng):
    typ = records.REGISTER_LWW
    assert cm.materialize_eager(typ, cm.new(typ), []) == (0, b"")
    assert cm.materialize_eager(typ, (4, b"kept"), []) == (4, b"kept")
    assert cm.materialize_eager(typ, cm.new(typ), [(3, b"x"), (0, b"zero"), (9, b"y")]) == \
        ("error", ("unexpected_operation", (0, b"zero"), typ))
    assert cm.materialize_eager(typ, cm.new(typ), [(3, b"x"), "assign"]) == \
        ("error", ("unexpected_operation", "assign", typ))
    # equal timestamps: the larger value term, whatever order the values arrive in
    for effs in ([(5, b"a"), (5, b"b")], [(5, b"b"), (5, b"a")]):
        assert cm.materialize_eager(typ, cm.new(typ), effs) == (5, b"b")
    assert cm.materialize_eager(typ, (5, b"c"), [(5, b"a"), (5, b"b")]) == (5, b"c")


def test_gen_dev_matches_host(eng):
    """agn_gen_dev builds the host generator's log for the type, and the
    kernel reads it: no request fails, most include ops."""
    from antidote_amd.engine import free_gen_host, gen_host, host_view
    K, N, D = 200, 64, 8
    cfg = _abi.AgnGenCfg(crdt_type=LWW, n_dcs=D, n_keys=K, ops_per_key=N, n_elems=16, seed=5,
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
        assert dl_.crdt_type == LWW and not dl_.eff
        cap = np.arange(K + 1, dtype=np.uint64)
        dres = eng.alloc_result(K, D, sparse=False, cap_off=cap)
        eng.materialize(dl_, dr, dres)
        eng.sync()
        got = eng.fetch_result(dres)
        assert not (got.flags & (_abi.F_ERR_UNEXPECTED | _abi.F_ERR_CAPACITY |
                                 _abi.F_ERR_CORRUPTED)).any()
        assert 0.2 < got.count.mean() / N < 0.95
        inc = got.count > 0
        assert np.array_equal(got.out_n, inc.astype(np.uint32))
        ts = host_view(hl.add_tok, np.uint64, K * N).reshape(K, N)
        assert (got.out_tok[cap[:-1].astype(np.int64)][inc] <= ts.max(axis=1)[inc]).all()
        free(dres)
    finally:
        eng.free_gen(dl_, dr)
        free_gen_host(hl, hr)
