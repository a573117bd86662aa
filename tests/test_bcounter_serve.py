"""The fused counter_b cached read (k_bcounter_serve, AGN_BCOUNTER_FUSED=1) on
the GPU.  Every run has a twin on the kernel sequence (the knob unset), and
both are held to tests/bcounter_model.py through the lookup -> model -> store
chain (tests/bcounter_serve_cases.chain; tests/test_bcounter.py's Mirror for
the batcher):

  1  the path a cached batcher takes (agn_batcher_path_stats);
  2  agn_read_cached over device arrays on the constructed keys of
     tests/bcounter_serve_cases.py (reach: test_bcounter_serve_cpu.py), the
     bases planted in the arena as cached snapshots; every result field, the
     cache, every live snapshot's pairs in arena order, state_ctl;
  3  a store that does not fit the arena;
  4  cache_edges' batcher scripts with counter_b effects on twin partitions,
     from one thread and from eight into shared batches; arena growth under
     the batcher with states of about 100 pairs."""
import threading

import numpy as np
import pytest

import bcounter_model as bm
import bcounter_serve_cases as bc
import cache_edges as ce
from antidote_amd import _abi
from antidote_amd.engine import Batcher, OpLog, read_cached_path
from test_bcounter import Mirror

pytestmark = pytest.mark.gpu

BC = _abi.COUNTER_B
KNOB = "AGN_BCOUNTER_FUSED"
ERRS = _abi.F_ERR_UNEXPECTED | _abi.F_ERR_CORRUPTED | _abi.F_ERR_CAPACITY


class Part:
    """A counter_b op log with its cached batcher."""

    def __init__(self, eng, D, sparse, K, **bk):
        self.D, self.sparse = D, sparse
        self.ol = OpLog(eng, BC, D, K, sparse=sparse)
        self.bt = Batcher(self.ol, cached=True, **bk)
        self.tx = 1000

    def close(self):
        self.bt.close()
        self.ol.close()

    def append(self, k, oc, tag, amt, mk):
        self.tx += 1
        self.ol.append(np.array([k], np.uint64), oc.reshape(1, self.D).astype(np.uint64),
                       oc_mask=None if mk is None else np.array([[mk]], np.uint64),
                       tag=np.array([tag], np.uint32), add_tok=np.array([amt], np.uint64),
                       txid=np.array([self.tx], np.uint64))

    def read(self, k, R, rm=None, gc=False, out_cap=16):
        m = None if rm is None else np.array([rm], np.uint64)
        if self.sparse and m is None:
            m = np.array([(1 << self.D) - 1], np.uint64)
        return self.bt.read(k, R=R, R_mask=m, gc=gc, out_cap=out_cap)


def twins(eng, monkeypatch, D, sparse, K, **bk):
    """(fused, sequence): the knob is read when a batcher is created."""
    monkeypatch.setenv(KNOB, "1")
    a = Part(eng, D, sparse, K, **bk)
    monkeypatch.delenv(KNOB)
    b = Part(eng, D, sparse, K, **bk)
    return a, b


def same_result(ga, gb, ctx):
    assert set(ga) == set(gb), ctx
    for f in ga:
        assert np.array_equal(np.asarray(ga[f]), np.asarray(gb[f])), (ctx, f, ga[f], gb[f])


# ------------------------------------------------------------------ 1: the path taken
def _load_and_read(p, K, D, sparse, rounds=3):
    clk = ce.Clock(D)
    t = 0
    for _ in range(6):
        for k in range(K):
            _c, oc = clk.op()
            tag, amt = bc.script_entry(t)
            p.append(k, oc, tag, amt, (1 << D) - 1 if sparse else None)
            t += 1
    for _ in range(rounds):
        for k in range(K):
            p.read(k, clk.R())
    return rounds * K


@pytest.mark.parametrize("D,sparse", [(8, False), (6, True), (16, False), (64, True)])
def test_path_fused_with_the_knob(eng, monkeypatch, D, sparse):
    monkeypatch.setenv(KNOB, "1")
    p = Part(eng, D, sparse, 4, max_batch=8)
    try:
        n = _load_and_read(p, 4, D, sparse)
        st, ps = p.bt.stats(), p.bt.path_stats()
        assert ps["fused"] > 0 and ps["sequence"] == 0, (st, ps)
        assert st["reads"] == n and ps["fused"] == st["batches"], (st, ps)
    finally:
        p.close()


@pytest.mark.parametrize("D,knob", [(8, None), (8, "0"), (64, None), (65, "1")])
def test_path_sequence(eng, monkeypatch, D, knob):
    if knob is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, knob)
    p = Part(eng, D, False, 4, max_batch=8)
    try:
        n = _load_and_read(p, 4, D, False)
        st, ps = p.bt.stats(), p.bt.path_stats()
        assert st["reads"] == n and ps["fused"] == 0 and ps["sequence"] == st["batches"], (st, ps)
    finally:
        p.close()


# ------------------------------------------------------------------ 2: agn_read_cached
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


def run_read_cached(eng, fam, dlog, want_fused, cap=None):
    """agn_read_cached of fam's keys on a fresh device cache: results, status,
    prune, thresholds, the cache, its decoded states, ctl."""
    D, K, S = fam.D, fam.K, fam.S
    req, co, gc = bc.requests(fam)
    n = req.n_req
    c, bufs = dev_cache(eng, fam, cap)
    assert read_cached_path(c, dlog, n) is want_fused
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
    out["states"] = bc.decode_states(value, out["n"], tg, tk)
    for b in (dk, dR, dtx, dgc, st, pr, thr, *res.bufs.values(), *bufs.values()):
        b.free()
    return out


def same_run(a, b, fam, ctx):
    ra, rb = a["res"], b["res"]
    for f in ("flags", "err_pos", "out_n", "hole", "count", "lastct"):
        x, y = getattr(ra, f), getattr(rb, f)
        bad = np.flatnonzero((x != y).reshape(fam.K, -1).any(axis=1))
        assert not len(bad), (ctx, f, [(fam.names[i], x[i], y[i]) for i in bad[:3]])
    assert np.array_equal(ra.out_tag, rb.out_tag) and np.array_equal(ra.out_tok, rb.out_tok), ctx
    for f in ("status", "prune"):
        bad = np.flatnonzero(a[f] != b[f])
        assert not len(bad), (ctx, f, [(fam.names[i], int(a[f][i]), int(b[f][i])) for i in bad[:5]])
    ki = np.flatnonzero(a["prune"] == 1)
    assert np.array_equal(a["thr"][ki], b["thr"][ki]), (ctx, "thr")
    assert np.array_equal(a["n"], b["n"]), (ctx, "n", np.flatnonzero(a["n"] != b["n"])[:5])
    live = np.arange(fam.S)[None, :] < a["n"][:, None]
    assert np.array_equal(a["clock"][live], b["clock"][live]), (ctx, "clock")
    assert np.array_equal(a["last_op"][live], b["last_op"][live]), (ctx, "last_op")
    assert a["states"] == b["states"], (ctx, "states", [
        (fam.names[k[0]], k[1], a["states"][k][:4], b["states"][k][:4]) for k in a["states"]
        if a["states"][k] != b["states"][k]][:5])
    assert np.array_equal(a["ctl"][:3], b["ctl"][:3]), (ctx, "state_ctl", a["ctl"], b["ctl"])


def against_chain(a, w, fam, ctx):
    """A device run against the reference chain: no read is left out."""
    bad = bm.compare_bc(fam.D, a["res"], w["res"], False, fam.K)
    assert not bad, (ctx, [(fam.names[x[0]],) + tuple(x[1:]) for x in bad[:5]])
    assert np.array_equal(a["status"], w["status"]), ctx
    assert np.array_equal(a["prune"] & 1, w["prune"]), ctx
    ki = np.flatnonzero(w["prune"] == 1)
    assert np.array_equal(a["thr"][ki], w["thr"][ki]), (ctx, "thr")
    assert np.array_equal(a["n"], w["arrs"]["n"]), ctx
    live = np.arange(fam.S)[None, :] < a["n"][:, None]
    assert np.array_equal(a["clock"][live], w["arrs"]["clock"][live]), (ctx, "clock")
    assert np.array_equal(a["last_op"][live], w["arrs"]["last_op"][live]), (ctx, "last_op")
    for (k, j), have in a["states"].items():   # each live snapshot's pairs, as a list in order
        want = w["states"][int(w["arrs"]["value"][k, j])]
        assert have == want, (ctx, fam.names[k], j, have[:6], want[:6])


@pytest.mark.parametrize("D,full,mask", bc.FAMILIES, ids=bc.FAMILY_IDS)
def test_read_cached_family(eng, oracle_lib, monkeypatch, D, full, mask):
    """The constructed keys, fused against the sequence on twin caches and
    against the chain.  A masked log runs over the dense-clock cache (no R /
    SCT / LastOpCt masks), as agn_read_cached takes it."""
    fam = bc.masked_family(D, full) if mask else bc.family(D, full)
    dlog = eng.upload_log(fam.log)
    if mask:
        assert dlog.struct.oc_mask
    else:
        dlog.struct.oc_mask = None
    ctx = (D, full, mask)
    try:
        monkeypatch.setenv(KNOB, "1")
        a = run_read_cached(eng, fam, dlog, True)
        monkeypatch.delenv(KNOB)
        b = run_read_cached(eng, fam, dlog, False)
        same_run(a, b, fam, ctx)
        w = bc.chain(oracle_lib, fam)
        against_chain(a, w, fam, ctx)
        against_chain(b, w, fam, ctx)
        assert a["ctl"][2] == 0, ctx
    finally:
        for b_ in dlog.bufs.values():
            b_.free()


# ------------------------------------------------------------------ 3: arena pressure
def test_read_cached_store_does_not_fit(eng, monkeypatch):
    """An arena with no room left: every store that would prepend overflows.
    The reads' results stand -- they are the roomy run's -- no such snapshot is
    cached, state_ctl[2] is raised, and everything equals the sequence's."""
    fam = bc.family(8, True)
    dlog = eng.upload_log(fam.log)
    dlog.struct.oc_mask = None
    used = int(fam.ctl[0])
    try:
        monkeypatch.setenv(KNOB, "1")
        roomy = run_read_cached(eng, fam, dlog, True)
        a = run_read_cached(eng, fam, dlog, True, cap=used)
        monkeypatch.delenv(KNOB)
        b = run_read_cached(eng, fam, dlog, False, cap=used)
        same_run(a, b, fam, "no room")
        for f in ("flags", "err_pos", "out_n", "hole", "count", "lastct", "out_tag", "out_tok"):
            assert np.array_equal(getattr(a["res"], f), getattr(roomy["res"], f)), f
        assert np.array_equal(a["status"], roomy["status"])
        grew = roomy["ctl"][0] - used
        assert grew > 20 and a["ctl"][2] == 1 and roomy["ctl"][2] == 0, (a["ctl"], roomy["ctl"])
        assert a["ctl"][0] == used + grew and a["ctl"][1] >= grew, (a["ctl"], grew)
        lost = [k for k in range(fam.K) if roomy["states"].get((k, 0)) != a["states"].get((k, 0))
                or roomy["n"][k] != a["n"][k]]
        assert len(lost) > 5
        for k in lost:      # the cache keeps what the lookup left: nothing prepended, no prune
            assert a["n"][k] == max(int(fam.cache["n"][k]), 1) and a["prune"][k] == 0, fam.names[k]
    finally:
        for b_ in dlog.bufs.values():
            b_.free()


# ------------------------------------------------------------------ 4: batcher scripts
def run_step(pa, pb, mir, k, step, ctx, lock=None):
    """One script step of key k on both partitions and the mirror."""
    if step[0] == "append":
        for oc, (tag, amt), mk in step[1]:
            for p in (pa, pb):
                p.append(k, oc, tag, amt, mk)
            mir.append(k, oc, pa.tx, tag, amt)
        return None
    _x, R, rm, gc, label = step
    assert rm is None
    ctx = ctx + (label,)
    ga, gb = pa.read(k, R, None, gc), pb.read(k, R, None, gc)
    same_result(ga, gb, ctx)
    ka = np.array([k], np.uint64)
    ma, mb = pa.ol.key_meta(ka), pb.ol.key_meta(ka)
    assert all(np.array_equal(x, y) for x, y in zip(ma, mb)), (ctx, "key_meta", ma, mb)
    if lock is not None:
        lock.acquire()
    try:
        want, wst, _wpr, _thr, cap = mir.read(ka, R.reshape(1, -1).astype(np.uint64),
                                              np.array([1 if gc else 0], np.uint8))
        fl = int(want.flags[0])
        assert ga["status"] == int(wst[0]), (ctx, ga["status"], wst)
        assert ga["flags"] == fl and ga["count"] == int(want.count[0]), (ctx, ga, fl)
        assert ga["hole"] == int(want.hole[0]), ctx
        if not fl & _abi.F_CT_IGNORE:
            assert np.array_equal(ga["lastct"], want.lastct[0]), ctx
        if ga["status"] != _abi.SS_LOG and not fl & ERRS:
            m, o = int(want.out_n[0]), int(cap[0])
            assert ga["out_n"] == m, ctx
            assert ga["out_tag"].tolist() == want.out_tag[o:o + m].tolist(), ctx
            assert ga["out_tok"].tolist() == want.out_tok[o:o + m].tolist(), ctx
        # the log's length after the GC this read selected
        assert int(ma[0][0]) == len(mir.ents[k]), (ctx, "log length", ma, len(mir.ents[k]))
    finally:
        if lock is not None:
            lock.release()
    return ga


SCRIPT_SHAPES = [(3, False), (8, False), (64, False), (5, True), (33, True)]


@pytest.mark.parametrize("D,sparse", SCRIPT_SHAPES)
def test_scripts_fused_vs_sequence_vs_mirror(eng, oracle_lib, monkeypatch, D, sparse):
    sc = ce.scripts(D, sparse)
    names = bc.SCRIPT_NAMES
    pa, pb = twins(eng, monkeypatch, D, sparse, len(names), max_batch=8)
    mir = Mirror(oracle_lib, len(names), D)
    try:
        seen, errs = set(), 0
        for k, name in enumerate(names):
            for x, step in enumerate(bc.bc_steps(sc[name])):
                g = run_step(pa, pb, mir, k, step, (name, x))
                if g is not None:
                    seen.add(g["status"])
                    errs += bool(g["flags"] & _abi.F_ERR_UNEXPECTED)
        assert seen == {_abi.SS_NEW, _abi.SS_HIT, _abi.SS_LOG}, seen
        assert errs > 0
        pa_, pb_ = pa.bt.path_stats(), pb.bt.path_stats()
        assert pa_["sequence"] == 0 and pa_["fused"] > 0 and pb_["fused"] == 0, (pa_, pb_)
    finally:
        pa.close()
        pb.close()


@pytest.mark.parametrize("D,sparse", SCRIPT_SHAPES)
def test_scripts_from_threads(eng, oracle_lib, monkeypatch, D, sparse):
    """The same scripts, each round's reads from 8 threads into shared batches."""
    sc = ce.scripts(D, sparse)
    order = ["grow", "deep", "below", "gc_twice", "invalid", "grow", "below", "deep"]
    T = len(order)
    pa, pb = twins(eng, monkeypatch, D, sparse, T, max_batch=8, max_wait_us=3500)
    mir, lock, errs = Mirror(oracle_lib, T, D), threading.Lock(), []
    try:
        steps = [bc.bc_steps(sc[n]) for n in order]
        for x in range(max(len(s) for s in steps)):
            todo = []
            for k in range(T):
                if x >= len(steps[k]):
                    continue
                if steps[k][x][0] == "append":
                    run_step(pa, pb, mir, k, steps[k][x], (order[k], x))
                else:
                    todo.append(k)

            def reader(k, x=x):
                try:
                    run_step(pa, pb, mir, k, steps[k][x], (order[k], x), lock)
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


def test_arena_growth_under_the_batcher(eng, oracle_lib, monkeypatch):
    """A cached batcher whose arena starts with one pair of room, and states of
    about 100 pairs: the batcher re-packs and grows the arena in front of the
    batches (ensure_state_room); every read's result stands, later reads are
    served from the snapshots cached meanwhile, and everything equals the
    sequence twin's and the mirror's."""
    monkeypatch.setenv("AGN_SS_ARENA_INIT", "1")
    D, K = 8, 2
    pa, pb = twins(eng, monkeypatch, D, False, K, max_batch=4)
    mir = Mirror(oracle_lib, K, D)
    try:
        clk = ce.Clock(D)
        t = 0
        hits = 0
        for rnd in range(6):
            for k in range(K):
                for _ in range(20):         # 20 new slots per round, first seen descending
                    _c, oc = clk.op()
                    tag, amt = 5000 - t, (t % 7 - 3) & bm.M64
                    for p in (pa, pb):
                        p.append(k, oc, tag, amt, None)
                    mir.append(k, oc, pa.tx, tag, amt)
                    t += 1
            R = clk.R()
            for k in range(K):
                ga, gb = pa.read(k, R, out_cap=256), pb.read(k, R, out_cap=256)
                same_result(ga, gb, (rnd, k))
                want, wst, _p, _t, cap = mir.read(np.array([k], np.uint64), R.reshape(1, D),
                                                  np.zeros(1, np.uint8))
                m = int(want.out_n[0])
                assert ga["status"] == int(wst[0]) and ga["out_n"] == m == 20 * (rnd + 1), (rnd, k)
                assert ga["out_tag"].tolist() == want.out_tag[:m].tolist(), (rnd, k)
                assert ga["out_tok"].tolist() == want.out_tok[:m].tolist(), (rnd, k)
                hits += ga["status"] == _abi.SS_HIT and ga["count"] == 20
        assert hits >= 2 * 4        # the stores were made: later reads fold 20 ops onto them
        assert pa.bt.state_bound(0) >= 100 and pa.bt.state_bound(0) == pb.bt.state_bound(0)
        ps = pa.bt.path_stats()
        assert ps["fused"] > 0 and ps["sequence"] == 0, ps
    finally:
        pa.close()
        pb.close()
