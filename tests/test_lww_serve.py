"""The fused register_lww cached read (k_lww_serve) on the GPU:

  1  the path a cached batcher takes (agn_batcher_path_stats): fused at
     D <= 64, the sequence beyond and with AGN_LWW_FUSED=0;
  2  cache_edges' batcher scripts with (ts, tag) entries on two partitions, one
     fused and one on the kernel sequence: equal bit for bit after every read,
     and equal to the reference transcription where it serves the read;
  3  agn_read_cached over device arrays on the constructed keys of
     tests/lww_serve_cases.py (reach: test_lww_serve_cpu.py), fused against
     AGN_LWW_FUSED=0 on a twin cache and arena, and against the C oracle;
  4  an arena too small for a store, through the fused path."""
import threading

import numpy as np
import pytest

import cache_edges as ce
import lww_serve_cases as lc
from antidote_amd import _abi
from antidote_amd.engine import Batcher, OpLog
from lww_model import LWW, compare_lww
from oracle import py_oracle as po
from test_lww_serve_cpu import chain
from test_ss_states import state_of, vc

pytestmark = pytest.mark.gpu

ERRS = _abi.F_ERR_UNEXPECTED | _abi.F_ERR_CORRUPTED | _abi.F_ERR_CAPACITY


class Part:
    """A register_lww op log with its cached batcher."""

    def __init__(self, eng, D, sparse, K, **bk):
        self.D, self.sparse = D, sparse
        self.ol = OpLog(eng, LWW, D, K, sparse=sparse)
        self.bt = Batcher(self.ol, cached=True, **bk)
        self.tx = 1000

    def close(self):
        self.bt.close()
        self.ol.close()

    def append(self, k, oc, ts, tag, mk):
        self.tx += 1
        self.ol.append(np.array([k], np.uint64), oc.reshape(1, self.D),
                       oc_mask=None if mk is None else np.array([[mk]], np.uint64),
                       tag=np.array([tag], np.uint32), add_tok=np.array([ts], np.uint64),
                       rem_off=np.array([0, 0], np.uint32), rem_tok=np.array([0], np.uint64),
                       txid=np.array([self.tx], np.uint64))

    def read(self, k, R, rm=None, gc=False):
        m = None if rm is None else np.array([rm], np.uint64)
        if self.sparse and m is None:
            m = np.array([(1 << self.D) - 1], np.uint64)
        return self.bt.read(k, R=R, R_mask=m, gc=gc, out_cap=4)


def twins(eng, monkeypatch, D, sparse, K, **bk):
    """(fused, sequence): AGN_LWW_FUSED is read when a batcher is created."""
    monkeypatch.setenv("AGN_LWW_FUSED", "1")
    a = Part(eng, D, sparse, K, **bk)
    monkeypatch.setenv("AGN_LWW_FUSED", "0")
    b = Part(eng, D, sparse, K, **bk)
    monkeypatch.delenv("AGN_LWW_FUSED")
    return a, b


def same_result(ga, gb, ctx):
    assert set(ga) == set(gb), ctx
    for f in ga:
        assert np.array_equal(np.asarray(ga[f]), np.asarray(gb[f])), (ctx, f, ga[f], gb[f])


# ------------------------------------------------------------------ 1: the path taken
def _load(p, K, D, sparse, ops=6):
    clk = ce.Clock(D)
    t = 0
    for _ in range(ops):
        for k in range(K):
            _c, oc = clk.op()
            ts, tag = lc.script_entry(t)
            p.append(k, oc.astype(np.uint64), ts, tag, (1 << D) - 1 if sparse else None)
            t += 1
    return clk.R()


def _read_from_threads(p, K, R, rounds, T=4):
    errs = []

    def reader(j):
        try:
            for _ in range(rounds):
                for k in range(j, K, T):
                    p.read(k, R)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ths = [threading.Thread(target=reader, args=(j,)) for j in range(T)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs[0]


@pytest.mark.parametrize("D,sparse", [(8, False), (6, True), (16, False), (64, True)])
def test_path_fused(eng, monkeypatch, D, sparse):
    monkeypatch.delenv("AGN_LWW_FUSED", raising=False)
    K = 8
    p = Part(eng, D, sparse, K, max_batch=8, max_wait_us=200)
    try:
        R = _load(p, K, D, sparse)
        _read_from_threads(p, K, R, 5)
        st, ps = p.bt.stats(), p.bt.path_stats()
        assert st["reads"] == 40 and ps["fused"] == st["batches"] and ps["sequence"] == 0, (st, ps)
    finally:
        p.close()


@pytest.mark.parametrize("D,knob", [(8, "0"), (64, "0"), (65, None)])
def test_path_sequence(eng, monkeypatch, D, knob):
    if knob is None:
        monkeypatch.delenv("AGN_LWW_FUSED", raising=False)
    else:
        monkeypatch.setenv("AGN_LWW_FUSED", knob)
    K = 8
    p = Part(eng, D, False, K, max_batch=8, max_wait_us=200)
    try:
        R = _load(p, K, D, False)
        _read_from_threads(p, K, R, 5)
        st, ps = p.bt.stats(), p.bt.path_stats()
        assert st["reads"] == 40 and ps["fused"] == 0 and ps["sequence"] == st["batches"], (st, ps)
    finally:
        p.close()


@pytest.mark.parametrize("knob", [None, "0"])
def test_path_set_aw_keeps_its_own(eng, monkeypatch, knob):
    """A set_aw batcher at D = 8 reports fused batches (AGN_LWW_FUSED does not
    touch it), and none with AGN_TAGS_FUSED=0."""
    monkeypatch.setenv("AGN_LWW_FUSED", "0")
    if knob is not None:
        monkeypatch.setenv("AGN_TAGS_FUSED", knob)
    D, K = 8, 8
    with OpLog(eng, _abi.SET_AW, D, K) as ol, Batcher(ol, max_batch=8, cached=True) as bt:
        clk = ce.Clock(D)
        for t in range(24):
            _c, oc = clk.op()
            ol.append(np.array([t % K], np.uint64), oc.reshape(1, D).astype(np.uint64),
                      tag=np.array([t % 3], np.uint32), add_tok=np.array([t + 1], np.uint64),
                      rem_off=np.array([0, 0], np.uint32), rem_tok=np.array([0], np.uint64),
                      txid=np.array([t + 1], np.uint64))
        for k in range(K):
            bt.read(k, R=clk.R(), out_cap=64)
        st, ps = bt.stats(), bt.path_stats()
        assert ps["fused"] + ps["sequence"] == st["batches"] == K, (st, ps)
        assert (ps["fused"] == K) if knob is None else (ps["fused"] == 0), ps


# ------------------------------------------------------------------ 2: scripts
PT = po.REGISTER_LWW


class Ref:
    """The reference transcription's vnode fed the same steps."""

    def __init__(self):
        self.vn, self.quirk, self.s = po.MaterializerVnode(), set(), 0

    def update(self, k, c, oc, ts, tag, mk, D):
        ss = oc.astype(np.int64).copy()
        ss[c] = int(oc[c]) - 1
        self.s += 1
        eff = "invalid" if tag == _abi.TAG_INVALID else (int(ts), int(tag))
        full = (1 << D) - 1
        pay = po.Payload(k, PT, eff, vc(ss, full if mk is None else mk), (c, int(oc[c])), self.s)
        try:
            self.vn.update(k, pay)
        except po.BadMatch:
            self.quirk.add(k)

    def read(self, k, R, rm, gc, D):
        """("served", state) | ("log",) | ("error",) | None (a reference crash path)."""
        if k in self.quirk:
            return None
        full = (1 << D) - 1
        try:
            r = self.vn.internal_read(k, PT, vc(R, full if rm is None else rm), po.IGNORE,
                                      bool(gc))
        except NotImplementedError:
            return ("log",)
        except po.BadMatch:
            self.quirk.add(k)
            return None
        return ("served", r[1]) if r[0] == "ok" else ("error",)

    def sizes(self, k):
        return tuple(self.vn.ops_cache[k][1]) if k in self.vn.ops_cache else None


def run_step(pa, pb, ref, k, step, dcs, tcount, ctx, lock=None):
    """One script step of key k on both partitions and the reference."""
    D = pa.D
    if step[0] == "append":
        for oc, (ts, tag), mk in step[1]:
            c = dcs[tcount[k] % len(dcs)]
            tcount[k] += 1
            for p in (pa, pb):
                p.append(k, oc, ts, tag, mk)
            ref.update(k, c, oc, ts, tag, mk, D)
        return None
    _x, R, rm, gc, label = step
    ctx = ctx + (label,)
    ga, gb = pa.read(k, R, rm, gc), pb.read(k, R, rm, gc)
    same_result(ga, gb, ctx)
    ka = np.array([k], np.uint64)
    ma, mb = pa.ol.key_meta(ka), pb.ol.key_meta(ka)
    assert all(np.array_equal(x, y) for x, y in zip(ma, mb)), (ctx, "key_meta", ma, mb)
    if lock is not None:
        lock.acquire()
    try:
        want = ref.read(k, R, rm, gc, D)
        if want is None:
            return ga
        if want[0] == "log":
            assert ga["status"] == _abi.SS_LOG, (ctx, ga["status"])
            return ga
        assert ga["status"] in (_abi.SS_HIT, _abi.SS_NEW), (ctx, ga["status"])
        if want[0] == "error":
            assert ga["flags"] & _abi.F_ERR_UNEXPECTED, (ctx, ga["flags"])
        else:
            assert not ga["flags"] & ERRS, (ctx, ga["flags"])
            assert state_of(LWW, ga["out_tag"], ga["out_tok"]) == want[1], (ctx, want, ga)
        sz = ref.sizes(k)
        if sz is not None and k not in ref.quirk:
            assert (int(ma[0][0]), int(ma[1][0])) == sz, (ctx, "ETS sizes", ma, sz)
    finally:
        if lock is not None:
            lock.release()
    return ga


SCRIPT_SHAPES = [(1, False), (3, False), (5, True), (8, False), (8, True), (9, False), (16, True),
                 (33, False), (64, True)]


@pytest.mark.parametrize("D,sparse", SCRIPT_SHAPES)
def test_scripts_fused_vs_sequence_vs_reference(eng, monkeypatch, D, sparse):
    sc = ce.scripts(D, sparse)
    pa, pb = twins(eng, monkeypatch, D, sparse, len(sc), max_batch=8)
    ref = Ref()
    try:
        seen, ties, tcount = set(), 0, [0] * len(sc)
        for k, (name, s) in enumerate(sc.items()):
            for x, step in enumerate(lc.lww_steps(s)):
                g = run_step(pa, pb, ref, k, step, s.clk.dcs, tcount, (name, x))
                if g is not None:
                    seen.add(g["status"])
                    ties += bool(g["flags"] & _abi.F_TS_TIE)
        assert seen == {_abi.SS_NEW, _abi.SS_HIT, _abi.SS_LOG}, seen
        assert ties > 0 and len(ref.quirk) <= 1, (ties, ref.quirk)
        pa_, pb_ = pa.bt.path_stats(), pb.bt.path_stats()
        assert pa_["sequence"] == 0 and pa_["fused"] > 0 and pb_["fused"] == 0, (pa_, pb_)
    finally:
        pa.close()
        pb.close()


@pytest.mark.parametrize("D,sparse", [(8, False), (16, True)])
def test_scripts_from_threads(eng, monkeypatch, D, sparse):
    """The same scripts, each round's reads from 8 threads into shared batches."""
    sc = ce.scripts(D, sparse)
    order = ["grow", "deep", "below", "gc_twice", "grow4", "invalid", "grow", "below"]
    if sparse:
        order[6:] = ["mixed_sets", "r_lacks_dc"]
    T = len(order)
    pa, pb = twins(eng, monkeypatch, D, sparse, T, max_batch=8, max_wait_us=5000)
    ref, lock, errs = Ref(), threading.Lock(), []
    try:
        steps = [lc.lww_steps(sc[n]) for n in order]
        dcs = [sc[n].clk.dcs for n in order]
        tcount = [0] * T
        for x in range(max(len(s) for s in steps)):
            todo = []
            for k in range(T):
                if x >= len(steps[k]):
                    continue
                if steps[k][x][0] == "append":
                    run_step(pa, pb, ref, k, steps[k][x], dcs[k], tcount, (order[k], x))
                else:
                    todo.append(k)

            def reader(k, x=x):
                try:
                    run_step(pa, pb, ref, k, steps[k][x], dcs[k], tcount, (order[k], x), lock)
                except Exception as e:  # noqa: BLE001
                    errs.append(e)
            ths = [threading.Thread(target=reader, args=(k,)) for k in todo]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            assert not errs, errs[0]
        st, ps = pa.bt.stats(), pa.bt.path_stats()
        assert st["batches"] < st["reads"] and ps["fused"] == st["batches"], (st, ps)
    finally:
        pa.close()
        pb.close()


# ------------------------------------------------------------------ 3: agn_read_cached
def dev_cache(eng, fam, cap=None):
    """fam's cache with its arena on the device: (agn_ss_cache, buffers).
    cap: the arena's capacity, if not the family's (room for every store)."""
    bufs = {x: eng.upload(a) for x, a in fam.cache.items()}
    bufs["state_tag"], bufs["state_tok"] = eng.upload(fam.state_tag), eng.upload(fam.state_tok)
    bufs["ctl"] = eng.upload(fam.ctl)
    c = ce.cache_struct(fam.D, fam.S, fam.K, bufs, lambda b: b.ptr)
    c.state_tag, c.state_tok, c.state_ctl = (bufs[x].ptr for x in ("state_tag", "state_tok", "ctl"))
    c.state_cap = fam.arena_cap if cap is None else cap
    return c, bufs


def run_read_cached(eng, fam, dlog, order, cap=None):
    """agn_read_cached of fam's keys in `order` on a fresh device cache:
    results, status, prune, thresholds, the cache, its decoded states, ctl."""
    D, K, S = fam.D, fam.K, fam.S
    req, co, gc = lc.requests(fam, order)
    n = req.n_req
    c, bufs = dev_cache(eng, fam, cap)
    dk, dR, dtx, dgc = (eng.upload(x) for x in (req.keys, req.R, req.txid, gc))
    res = eng.alloc_result(n, D, sparse=False, cap_off=co)
    st, pr, thr = eng.empty(n), eng.empty(n), eng.empty(K * D * 8)
    for b, nb in [(thr, K * D * 8), (st, n), (pr, n)] + [
            (res.bufs[x], int(np.prod(res.shapes[x][1])) * np.dtype(res.shapes[x][0]).itemsize)
            for x in res.shapes if x != "out_off"]:
        eng.lib.agn_memset_d(eng.ctx, b.ptr, 0, nb, None)
    eng.read_cached(c, dlog, n, dk.ptr, dR.ptr, dtx.ptr, dgc.ptr, res, st.ptr, pr.ptr, thr.ptr)
    eng.sync()
    out = dict(res=eng.fetch_result(res), status=eng.download(st, np.uint8, (n,)),
               prune=eng.download(pr, np.uint8, (n,)), thr=eng.download(thr, np.uint64, (K, D)),
               n=eng.download(bufs["n"], np.uint32, (K,)),
               clock=eng.download(bufs["clock"], np.uint64, (K, S, D)),
               last_op=eng.download(bufs["last_op"], np.int64, (K, S)),
               ctl=eng.download(bufs["ctl"], np.uint64, (4,)))
    value = eng.download(bufs["value"], np.int64, (K, S))
    tg = eng.download(bufs["state_tag"], np.uint32, (fam.arena_cap,))
    tk = eng.download(bufs["state_tok"], np.uint64, (fam.arena_cap,))
    out["states"] = lc.decode_states(value, out["n"], tg, tk)
    for b in (dk, dR, dtx, dgc, st, pr, thr, *res.bufs.values(), *bufs.values()):
        b.free()
    return out


def same_run(a, b, fam, order, ctx):
    names = [fam.names[k] for k in order]
    ra, rb = a["res"], b["res"]
    for f in ("flags", "err_pos", "out_n", "hole", "count", "lastct"):
        x, y = getattr(ra, f), getattr(rb, f)
        bad = np.flatnonzero((x != y).reshape(len(order), -1).any(axis=1))
        assert not len(bad), (ctx, f, [(names[i], x[i], y[i]) for i in bad[:3]])
    assert np.array_equal(ra.out_tag, rb.out_tag) and np.array_equal(ra.out_tok, rb.out_tok), ctx
    for f in ("status", "prune"):
        bad = np.flatnonzero(a[f] != b[f])
        assert not len(bad), (ctx, f, [(names[i], int(a[f][i]), int(b[f][i])) for i in bad[:5]])
    ki = np.asarray(order)[a["prune"] == 1]
    assert np.array_equal(a["thr"][ki], b["thr"][ki]), (ctx, "thr")
    assert np.array_equal(a["n"], b["n"]), (ctx, "n", np.flatnonzero(a["n"] != b["n"])[:5])
    live = np.arange(fam.S)[None, :] < a["n"][:, None]
    assert np.array_equal(a["clock"][live], b["clock"][live]), (ctx, "clock")
    assert np.array_equal(a["last_op"][live], b["last_op"][live]), (ctx, "last_op")
    assert a["states"] == b["states"], (ctx, "states", [
        (fam.names[k[0]], k[1], a["states"][k], b["states"][k]) for k in a["states"]
        if a["states"][k] != b["states"][k]][:5])
    assert np.array_equal(a["ctl"][:3], b["ctl"][:3]), (ctx, "state_ctl", a["ctl"], b["ctl"])


@pytest.mark.parametrize("D", [1, 8, 16, 64])
def test_read_cached_edges(eng, oracle_lib, monkeypatch, D):
    fam = lc.family(D)
    dlog = eng.upload_log(fam.log)
    dlog.struct.oc_mask = None
    try:
        for oname, order in lc.orders(fam.K):
            ctx = (D, oname)
            monkeypatch.setenv("AGN_LWW_FUSED", "1")
            a = run_read_cached(eng, fam, dlog, order)
            monkeypatch.setenv("AGN_LWW_FUSED", "0")
            b = run_read_cached(eng, fam, dlog, order)
            same_run(a, b, fam, order, ctx)
            # ...and both are the C oracle's chain (the host model's, test_lww_serve_cpu)
            w = chain(oracle_lib, fam, order)
            bad = compare_lww(D, a["res"], w["res"], False, len(order))
            assert not bad, (ctx, [(fam.names[order[x[0]]],) + tuple(x[1:]) for x in bad[:5]])
            assert np.array_equal(a["status"], w["status"]), ctx
            assert np.array_equal(a["prune"], w["prune"][order]), ctx
            assert np.array_equal(a["n"], w["arrs"]["n"]), ctx
            assert a["ctl"][2] == 0, ctx
            for i, k in enumerate(order):   # a stored snapshot's state is the read's result
                if w["arrs"]["value"][k, 0] == w["handle"][i]:
                    o = int(a["res"].out_off[i])
                    want = (int(a["res"].out_tag[o]), int(a["res"].out_tok[o])) \
                        if a["res"].out_n[i] else None
                    assert a["states"][(int(k), 0)] == want, (ctx, fam.names[k])
    finally:
        for b_ in dlog.bufs.values():
            b_.free()


@pytest.mark.parametrize("D", [8, 16, 64])
def test_read_cached_masked_log_dense_cache(eng, oracle_lib, monkeypatch, D):
    """A register_lww log with presence masks (oc_mask) over a dense-clock
    cache with an arena -- no R / SCT / LastOpCt masks: the fused launch takes
    it (agn_read_cached_path says so) and equals the sequence and the oracle."""
    from antidote_amd.engine import read_cached_path
    fam = lc.masked(lc.family(D))
    dlog = eng.upload_log(fam.log)
    assert dlog.struct.oc_mask
    try:
        for oname, order in lc.orders(fam.K):
            ctx = (D, "masked log", oname)
            monkeypatch.setenv("AGN_LWW_FUSED", "1")
            c, bufs = dev_cache(eng, fam)
            assert read_cached_path(c, dlog, len(order)) is True
            for b_ in bufs.values():
                b_.free()
            a = run_read_cached(eng, fam, dlog, order)
            monkeypatch.setenv("AGN_LWW_FUSED", "0")
            b = run_read_cached(eng, fam, dlog, order)
            same_run(a, b, fam, order, ctx)
            w = chain(oracle_lib, fam, order)
            bad = compare_lww(D, a["res"], w["res"], False, len(order))
            assert not bad, (ctx, [(fam.names[order[x[0]]],) + tuple(x[1:]) for x in bad[:5]])
            assert np.array_equal(a["status"], w["status"]), ctx
            assert np.array_equal(a["prune"], w["prune"][order]), ctx
            assert np.array_equal(a["n"], w["arrs"]["n"]), ctx
    finally:
        for b_ in dlog.bufs.values():
            b_.free()


# ------------------------------------------------------------------ 4: arena pressure
def test_read_cached_store_does_not_fit(eng, monkeypatch):
    """An arena with no room left: every store that would prepend overflows
    (which stores lose a race for the last pairs would depend on the order of
    the atomics, so none fits).  The reads' results stand -- they are the
    roomy run's -- no such snapshot is cached, state_ctl[2] is raised, and
    everything equals the sequence's."""
    D = 8
    fam = lc.family(D)
    dlog = eng.upload_log(fam.log)
    dlog.struct.oc_mask = None
    order = np.arange(fam.K)
    used = int(fam.ctl[0])
    try:
        monkeypatch.setenv("AGN_LWW_FUSED", "1")
        roomy = run_read_cached(eng, fam, dlog, order)
        a = run_read_cached(eng, fam, dlog, order, cap=used)
        monkeypatch.setenv("AGN_LWW_FUSED", "0")
        b = run_read_cached(eng, fam, dlog, order, cap=used)
        same_run(a, b, fam, order, "no room")
        for f in ("flags", "err_pos", "out_n", "hole", "count", "lastct", "out_tag", "out_tok"):
            assert np.array_equal(getattr(a["res"], f), getattr(roomy["res"], f)), f
        assert np.array_equal(a["status"], roomy["status"])
        # the stores that prepended in the roomy run were not made here
        grew = roomy["ctl"][0] - used
        assert grew > 20 and a["ctl"][2] == 1 and roomy["ctl"][2] == 0, (a["ctl"], roomy["ctl"])
        assert a["ctl"][0] == used + grew and a["ctl"][1] >= grew, (a["ctl"], grew)
        lost = [k for k in range(fam.K) if roomy["states"].get((k, 0)) != a["states"].get((k, 0))
                or roomy["n"][k] != a["n"][k]]
        assert len(lost) > 20
        for k in lost:      # the cache keeps what the lookup left: nothing prepended, no prune
            assert a["n"][k] == max(int(fam.cache["n"][k]), 1) and a["prune"][k] == 0, fam.names[k]
    finally:
        for b_ in dlog.bufs.values():
            b_.free()


def test_arena_pressure_fused(eng, monkeypatch):
    """A cached batcher whose arena starts with one pair of room.  The batcher
    makes room before a batch (ensure_state_room), so here the pressure shows
    as a re-pack / growth in front of the batches (the store that does not fit
    is test_read_cached_store_does_not_fit's): every read's result stands,
    later reads are served from the snapshots cached meanwhile, and everything
    equals the sequence twin's."""
    monkeypatch.setenv("AGN_SS_ARENA_INIT", "1")
    D, K = 8, 2
    pa, pb = twins(eng, monkeypatch, D, False, K, max_batch=4)
    try:
        clk = ce.Clock(D)
        t = 0
        metas = []
        for rnd in range(6):
            for k in range(K):
                for _ in range(5):
                    _c, oc = clk.op()
                    ts, tag = lc.script_entry(t)
                    t += 1
                    for p in (pa, pb):
                        p.append(k, oc.astype(np.uint64), ts, tag, None)
                ga, gb = pa.read(k, clk.R()), pb.read(k, clk.R())
                same_result(ga, gb, (rnd, k))
                assert ga["status"] in (_abi.SS_HIT, _abi.SS_NEW) and ga["out_n"] == 1
                assert not ga["flags"] & ERRS and ga["count"] >= 5, ga
            metas.append(tuple(int(x) for x in pa.ol.key_meta()[1]))
        for a_, b_ in zip(pa.ol.key_meta(), pb.ol.key_meta()):
            assert np.array_equal(a_, b_)
        # the snapshots were cached after the re-packs: a read at an older
        # clock is still served, and the newest read needs no op beyond its five
        ps = pa.bt.path_stats()
        assert ps["sequence"] == 0 and ps["fused"] == pa.bt.stats()["batches"], ps
        g = pa.read(0, clk.R())
        assert g["status"] == _abi.SS_HIT and g["count"] == 0 and g["out_n"] == 1, g
    finally:
        pa.close()
        pb.close()
