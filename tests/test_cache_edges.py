"""The device snapshot cache and the cached read on the constructed edges of
tests/cache_edges.py (their reach is checked in test_cache_edges_cpu.py),
every output bit-exact against the C oracle:

  Families L + S  agn_ss_lookup / agn_ss_store at every group width's first
                  and last D, dense and sparse, with 9 / 10 / 16 slots;
  Family R        agn_read_cached for D = 1..8 as the fused kernel (one
                  request per wave and pairs) and as the batched kernels, on
                  CSR and segmented logs, in both request orders;
  Family B        the cached read batcher's kernels (k_read6, its masked form,
                  k_read6w, the kernel sequence) on scripted reads, from one
                  thread and from eight;
  Family G        agn_select_base."""
import threading

import numpy as np
import pytest

import cache_edges as ce
from antidote_amd import _abi
from antidote_amd.engine import Batcher, OpLog
from synth import compare
from test_ss_cache import run_oracle

pytestmark = pytest.mark.gpu

LS_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130)
ERRS = _abi.F_ERR_UNEXPECTED | _abi.F_ERR_CORRUPTED | _abi.F_ERR_CAPACITY


def free(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


def dev_cache(eng, arrs, D, S, K):
    bufs = {x: eng.upload(a) for x, a in arrs.items() if a is not None}
    return ce.cache_struct(D, S, K, bufs, lambda b: b.ptr), bufs


def check_cache(eng, bufs, want, K, S, D, W, names, ctx):
    """n and every live slot of every key."""
    n = eng.download(bufs["n"], np.uint32, (K,))
    bad = np.flatnonzero(n != want["n"])
    assert not len(bad), (ctx, "n", [(names[k], int(n[k]), int(want["n"][k])) for k in bad[:5]])
    live = np.arange(S)[None, :] < n[:, None]
    for x, dt, shape in (("clock", np.uint64, (K, S, D)), ("mask", np.uint64, (K, S, W)),
                         ("last_op", np.int64, (K, S)), ("value", np.int64, (K, S))):
        if x not in bufs:
            continue
        g = eng.download(bufs[x], dt, shape)
        if g.ndim == 3:
            bad = np.flatnonzero(((g != want[x]).any(axis=2) & live).any(axis=1))
        else:
            bad = np.flatnonzero(((g != want[x]) & live).any(axis=1))
        assert not len(bad), (ctx, x, [names[k] for k in bad[:5]])


# ------------------------------------------------------------------ families L + S
@pytest.mark.parametrize("slots", ce.SLOTS)
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("D", LS_WIDTHS)
def test_lookup_store(eng, oracle_lib, D, sparse, slots):
    cs = ce.family_ls(D, slots, sparse)
    want_a, want = run_oracle(oracle_lib, cs)
    K, W, names = cs.K, cs.W, cs.names
    c, bufs = dev_cache(eng, cs.arrays(), D, slots, K)
    up = lambda x: eng.upload(x) if x is not None else None  # noqa: E731
    at = lambda b: b.ptr if b is not None else None          # noqa: E731
    keys, R, Rm = up(cs.keys), up(cs.R), up(cs.Rm)
    o = {"sct": eng.empty(K * D * 8), "sctm": eng.empty(K * W * 8), "ign": eng.empty(K),
         "base": eng.empty(K * 8), "first": eng.empty(K), "status": eng.empty(K)}
    eng.ss_lookup(c, K, keys.ptr, R.ptr, at(Rm), o["sct"].ptr, o["sctm"].ptr if sparse else None,
                  o["ign"].ptr, o["base"].ptr, o["first"].ptr, o["status"].ptr)
    for x, dt in (("status", np.uint8), ("first", np.uint8), ("base", np.int64), ("ign", np.uint8)):
        g = eng.download(o[x], dt, (K,))
        bad = np.flatnonzero(g != want[x])
        assert not len(bad), (x, [(names[i], int(g[i]), int(want[x][i])) for i in bad[:5]])
    hit = want["status"] == _abi.SS_HIT
    g = eng.download(o["sct"], np.uint64, (K, D))
    bad = np.flatnonzero((g != want["sct"]).any(axis=1) & hit)
    assert not len(bad), ("sct", [names[i] for i in bad[:5]])
    if sparse:
        g = eng.download(o["sctm"], np.uint64, (K, W))
        bad = np.flatnonzero((g != want["sctm"]).any(axis=1) & hit)
        assert not len(bad), ("sctm", [names[i] for i in bad[:5]])
    # the store, on the cache the lookup left (the empty snapshots of absent keys)
    log = _abi.AgnLog()
    log.n_keys, log.n_dcs = K, D
    ko = up(cs.key_off)
    log.key_off = ko.ptr
    res = _abi.AgnResult()
    rb = {x: up(getattr(cs, x)) for x in ("res_value", "hole", "lastct", "lastct_mask", "count",
                                          "flags")}
    res.value, res.hole, res.lastct = rb["res_value"].ptr, rb["hole"].ptr, rb["lastct"].ptr
    res.lastct_mask = at(rb["lastct_mask"])
    res.count, res.flags = rb["count"].ptr, rb["flags"].ptr
    gcb = up(cs.gc)
    pr, th, thm = eng.empty(K), eng.empty(K * D * 8), eng.empty(K * W * 8)
    eng.ss_store(c, log, K, keys.ptr, o["first"].ptr, o["status"].ptr, gcb.ptr, res, None,
                 pr.ptr, th.ptr, thm.ptr if sparse else None)
    gp = eng.download(pr, np.uint8, (K,))
    bad = np.flatnonzero(gp != want["prune"])
    assert not len(bad), ("prune", [names[i] for i in bad[:5]])
    sel = want["prune"] == 1
    g = eng.download(th, np.uint64, (K, D))
    bad = np.flatnonzero((g != want["thr"]).any(axis=1) & sel)
    assert not len(bad), ("thr", [(names[i], g[i].tolist(), want["thr"][i].tolist())
                                  for i in bad[:3]])
    if sparse:
        g = eng.download(thm, np.uint64, (K, W))
        bad = np.flatnonzero((g != want["thrm"]).any(axis=1) & sel)
        assert not len(bad), ("thrm", [names[i] for i in bad[:5]])
    check_cache(eng, bufs, want_a, K, slots, D, W, names, "store")
    free(keys, R, Rm, ko, gcb, pr, th, thm, *o.values(), *rb.values(), *bufs.values())


# ------------------------------------------------------------------ family R
FORMS = {"fused": ("0", "1"), "fused_pair": ("0", "2"), "batched": ("1", "")}


def r_orders(K, form):
    """Request orders: all K keys (an odd count: the pair form's last wave
    holds one request), the first K - 1 reversed (an even count, so every key
    changes between the first and the second request of its wave), and for the
    pair form the last two keys and one request alone."""
    assert K % 2 == 1
    orders = [("all", np.arange(K)), ("reversed", np.arange(K - 1)[::-1].copy())]
    if form == "fused_pair":
        orders += [("last two", np.array([K - 2, K - 1])), ("single", np.array([K // 2]))]
    return orders


@pytest.mark.parametrize("seg", [False, True], ids=["csr", "segments"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("D", range(1, 9))
def test_read_cached(eng, oracle_lib, monkeypatch, D, form, seg):
    split, np_ = FORMS[form]
    monkeypatch.setenv("AGN_READ_CACHED_SPLIT", split)
    monkeypatch.setenv("AGN_READ6_NP", np_)
    r = ce.family_r(D, seg=seg)
    K, S = r.K, r.S
    ls = ce.r_log_struct(r)
    dlog = eng.upload_log(r.log)
    dlog.struct.oc_mask = None
    kl = None
    if seg:
        kl = eng.upload(r.key_len)
        dlog.struct.key_len = kl.ptr
    eng.index_ids(dlog)
    # both key_id0 forms are there: consecutive ids, and AGN_ID0_NONE after a gap
    id0 = eng.download(dlog.bufs["key_id0"], np.uint32, (K,))
    lens = r.key_len if seg else np.diff(r.log.key_off.astype(np.int64))
    for k, e in enumerate(r.expect):
        if lens[k] >= 2:
            assert (int(id0[k]) != _abi.ID0_NONE) == e["id0"], r.names[k]
    assert (id0[lens >= 2] == _abi.ID0_NONE).any() and (id0[lens >= 2] == 5).any()
    for oname, order in r_orders(K, form):
        ctx = (form, oname)
        ks = r.keys[order]
        R, tx, gc = (np.ascontiguousarray(x[order]) for x in (r.R, r.txid, r.gc))
        names = [r.names[k] for k in order]
        nr = len(ks)
        m = ce.CacheMirror(oracle_lib, K, D, S, cache=r.cache)
        want = m.read_batch(ls, ks, R, tx, gc)
        if oname == "all" and form == "fused_pair":
            # a corrupted request as the first and (reversed) the second of its pair
            cor = [i for i, k in enumerate(order) if r.expect[k]["corrupt"]]
            assert cor and all((K - 2 - i) % 2 != i % 2 for i in cor)
        c, bufs = dev_cache(eng, r.cache, D, S, K)
        dk, dR, dtx, dgc = (eng.upload(x) for x in (ks, R, tx, gc))
        res = eng.alloc_result(nr, D, sparse=False)
        st, pr, thr = eng.empty(nr), eng.empty(nr), eng.empty(K * D * 8)
        eng.lib.agn_memset_d(eng.ctx, thr.ptr, 0, K * D * 8, None)
        eng.read_cached(c, dlog, nr, dk.ptr, dR.ptr, dtx.ptr, dgc.ptr, res, st.ptr, pr.ptr, thr.ptr)
        eng.sync()
        got = eng.fetch_result(res)
        bad = compare(_abi.COUNTER_PN, D, got, want["res"], False, nr)
        assert not bad, (ctx, [(names[b[0]],) + tuple(b[1:]) for b in bad[:5]])
        gs = eng.download(st, np.uint8, (nr,))
        bad = np.flatnonzero(gs != want["status"])
        assert not len(bad), (ctx, "status", [names[i] for i in bad[:5]])
        gp = eng.download(pr, np.uint8, (nr,))
        ki = ks.astype(np.int64)
        bad = np.flatnonzero(gp != want["prune"][ki])
        assert not len(bad), (ctx, "prune", [names[i] for i in bad[:5]])
        gt = eng.download(thr, np.uint64, (K, D))
        pk = ki[gp == 1]
        bad = [k for k in pk if not np.array_equal(gt[k], want["thr"][k])]
        assert not bad, (ctx, "thr", [(r.names[k], gt[k].tolist(), want["thr"][k].tolist())
                                      for k in bad[:3]])
        check_cache(eng, bufs, m.arr, K, S, D, 1, r.names, ctx)
        free(dk, dR, dtx, dgc, st, pr, thr, *res.bufs.values(), *bufs.values())
    free(kl, *dlog.bufs.values())


def test_read_cached_ten_slots(eng, oracle_lib, monkeypatch):
    """The production slot count (SNAPSHOT_THRESHOLD) under the fused kernel."""
    monkeypatch.setenv("AGN_READ_CACHED_SPLIT", "0")
    D = 5
    r = ce.family_r(D, slots=ce.THRESHOLD)
    K, S = r.K, r.S
    m = ce.CacheMirror(oracle_lib, K, D, S, cache=r.cache)
    want = m.read_batch(ce.r_log_struct(r), r.keys, r.R, r.txid, r.gc)
    dlog = eng.upload_log(r.log)
    dlog.struct.oc_mask = None
    eng.index_ids(dlog)
    c, bufs = dev_cache(eng, r.cache, D, S, K)
    dk, dR, dtx, dgc = (eng.upload(x) for x in (r.keys, r.R, r.txid, r.gc))
    res = eng.alloc_result(K, D, sparse=False)
    st, pr, thr = eng.empty(K), eng.empty(K), eng.empty(K * D * 8)
    eng.read_cached(c, dlog, K, dk.ptr, dR.ptr, dtx.ptr, dgc.ptr, res, st.ptr, pr.ptr, thr.ptr)
    eng.sync()
    bad = compare(_abi.COUNTER_PN, D, eng.fetch_result(res), want["res"], False, K)
    assert not bad, [(r.names[b[0]],) + tuple(b[1:]) for b in bad[:5]]
    assert np.array_equal(eng.download(st, np.uint8, (K,)), want["status"])
    gp = eng.download(pr, np.uint8, (K,))
    assert np.array_equal(gp, want["prune"])
    gt = eng.download(thr, np.uint64, (K, D))
    assert np.array_equal(gt[gp == 1], want["thr"][gp == 1])
    check_cache(eng, bufs, m.arr, K, S, D, 1, r.names, "slots=10")
    free(dk, dR, dtx, dgc, st, pr, thr, *res.bufs.values(), *bufs.values(), *dlog.bufs.values())


# ------------------------------------------------------------------ family B
def check_read(g, w, D, sparse, ctx):
    """A batcher result against the mirror's: the status alone where it is
    LOG (the result is void), the error alone where the read failed."""
    assert g["status"] == w["status"], (ctx, "status", g["status"], w["status"])
    if w["status"] == _abi.SS_LOG:
        return
    assert g["flags"] == w["flags"], (ctx, "flags", g["flags"], w["flags"])
    assert g["err_pos"] == w["err_pos"], (ctx, "err_pos", g["err_pos"], w["err_pos"])
    if w["flags"] & ERRS:
        return
    for f in ("value", "hole", "count"):
        assert g[f] == w[f], (ctx, f, g[f], w[f])
    if w["flags"] & _abi.F_CT_IGNORE:
        return
    if sparse:
        assert np.array_equal(g["lastct_mask"], w["lastct_mask"]), (ctx, "lastct_mask")
        keep = np.array([(int(w["lastct_mask"][d >> 6]) >> (d & 63)) & 1 for d in range(D)], bool)
        assert np.array_equal(g["lastct"][keep], w["lastct"][keep]), (ctx, "lastct")
    else:
        assert np.array_equal(g["lastct"], w["lastct"]), (ctx, "lastct")


class Partition:
    """An op log with its cached batcher, and the mirror of both."""

    def __init__(self, eng, lib, D, sparse, K, **bk):
        self.D, self.sparse = D, sparse
        self.ol = OpLog(eng, _abi.COUNTER_PN, D, K, sparse=sparse)
        self.bt = Batcher(self.ol, cached=True, **bk)
        self.m = ce.CacheMirror(lib, K, D, ce.THRESHOLD, sparse)
        self.tx = 1000

    def close(self):
        self.bt.close()
        self.ol.close()

    def append(self, k, ops):
        for oc, eff, mk in ops:
            self.tx += 1
            om = None if mk is None else np.array([[mk]], np.uint64)
            ids, _ = self.ol.append(np.array([k], np.uint64), oc.reshape(1, self.D), oc_mask=om,
                                    eff=np.array([eff], np.int64),
                                    txid=np.array([self.tx], np.uint64))
            self.m.append(k, oc, eff, int(ids[0]), self.tx, mk)

    def read(self, k, step, ctx):
        _x, R, rm, gc, label = step
        m = None if rm is None else np.array([rm], np.uint64)
        g = self.bt.read(k, R=R, R_mask=m, gc=gc)
        w = self.m.read(k, R, rm, 0, gc)
        check_read(g, w, self.D, self.sparse, ctx + (label,))
        return w

    def check_lengths(self, ctx):
        ln, _ll, _ct = self.ol.key_meta()
        want = [len(e) for e in self.m.entries]
        assert ln.tolist() == want, (ctx, ln.tolist(), want)


B_CASES = []
for _D in (3, 5, 8, 9, 16, 17, 32, 33, 64):
    for _sp in (False, True):
        for _r6 in ("1", "0"):
            B_CASES.append((_D, _sp, _r6, ""))
        if _D <= 8:
            B_CASES.append((_D, _sp, "1", "2"))
B_CASES += [(65, False, "1", ""), (65, False, "0", "")]


@pytest.mark.parametrize("D,sparse,read6,np_", B_CASES)
def test_batcher_scripts(eng, oracle_lib, monkeypatch, D, sparse, read6, np_):
    """Every script on a key of its own, reads from one thread in script
    order: every field after every read, the log's length after every step."""
    monkeypatch.setenv("AGN_READ6", read6)
    monkeypatch.setenv("AGN_READ6_NP", np_)
    sc = ce.scripts(D, sparse)
    p = Partition(eng, oracle_lib, D, sparse, len(sc), max_batch=8)
    try:
        seen = set()
        for k, (name, s) in enumerate(sc.items()):
            for x, step in enumerate(s.steps):
                ctx = (name, x)
                if step[0] == "append":
                    p.append(k, step[1])
                else:
                    w = p.read(k, step, ctx)
                    seen.add((w["status"], w["prune"]))
                p.check_lengths(ctx)
        assert {(_abi.SS_NEW, 0), (_abi.SS_HIT, 0), (_abi.SS_HIT, 1), (_abi.SS_LOG, 0)} <= seen
    finally:
        p.close()


@pytest.mark.parametrize("D,sparse", [(3, False), (5, True), (8, False), (9, False), (16, True),
                                      (17, False), (32, False), (33, True), (64, False),
                                      (65, False)])
def test_batcher_scripts_threads(eng, oracle_lib, monkeypatch, D, sparse):
    """Each round's reads from 8 threads on keys of their own, coalesced into
    batches (pairs of requests per wave for D <= 8); joined between rounds.
    The results are the single-thread run's: the mirror's."""
    monkeypatch.setenv("AGN_READ6_NP", "2" if D <= 8 else "")
    sc = ce.scripts(D, sparse)
    order = ["grow", "deep", "below", "gc_twice", "grow4", "invalid", "grow", "below"]
    if sparse and D >= 3:
        order[6:] = ["mixed_sets", "r_lacks_dc"]
    T = len(order)
    p = Partition(eng, oracle_lib, D, sparse, T, max_batch=8, max_wait_us=5000)
    errs = []
    try:
        steps = [sc[n].steps for n in order]
        for x in range(max(len(s) for s in steps)):
            todo = []
            for k in range(T):
                if x >= len(steps[k]):
                    continue
                if steps[k][x][0] == "append":
                    p.append(k, steps[k][x][1])
                else:
                    todo.append(k)

            def reader(k, x=x):
                try:
                    p.read(k, steps[k][x], (order[k], x))
                except Exception as e:  # noqa: BLE001
                    errs.append(e)
            ths = [threading.Thread(target=reader, args=(k,)) for k in todo]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            assert not errs, errs[0]
            p.check_lengths(x)
        st = p.bt.stats()
        assert st["batches"] < st["reads"], st
    finally:
        p.close()


# ------------------------------------------------------------------ family G
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("D", [1, 8, 64, 65, 130])
def test_select_base(eng, oracle_lib, D, sparse):
    g = ce.family_g(D, sparse)
    nq = len(g["names"])
    wi, wf = np.zeros(nq, np.int32), np.zeros(nq, np.uint8)
    p = ce.ptr
    assert oracle_lib.oracle_select_base(D, nq, p(g["off"]), p(g["clocks"]), p(g["cm"]), p(g["R"]),
                                         p(g["Rm"]), p(wi), p(wf)) == 0
    bufs = [eng.upload(g[x]) for x in ("off", "clocks", "cm", "R", "Rm")]
    oi, of = eng.empty(nq * 4), eng.empty(nq)
    eng.select_base(D, nq, *[b.ptr if b is not None else None for b in bufs], oi.ptr, of.ptr)
    gi, gf = eng.download(oi, np.int32, (nq,)), eng.download(of, np.uint8, (nq,))
    bad = np.flatnonzero((gi != wi) | (gf != wf))
    assert not len(bad), [(g["names"][i], int(gi[i]), int(wi[i]), int(gf[i]), int(wf[i]))
                          for i in bad[:5]]
    free(*bufs, oi, of)
