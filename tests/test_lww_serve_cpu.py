"""The fused register_lww cached read on the host: the path agn_read_cached
takes (agn_read_cached_path, no device), and the reach of the constructed
cases tests/test_lww_serve.py runs on the GPU -- every named edge is checked on
tests/lww_model.py and on the C oracle's chain (oracle_ss_lookup ->
oracle_materialize -> oracle_ss_store) over the same arrays, so a builder that
quietly stops producing an edge goes red here."""
import ctypes as C

import numpy as np
import pytest

import cache_edges as ce
import lww_serve_cases as lc
from antidote_amd import _abi
from antidote_amd._lib import EngineError, set_knob
from antidote_amd.encode import alloc_result, log_struct, read_struct, result_struct
from antidote_amd.engine import read_cached_path
from lww_model import LWW, compare_lww, model

FAKE = 0x1000      # a non-null pointer: the path function touches no array


def shapes(typ, D, K=16, arena=True, mask=False):
    c = _abi.AgnSsCache()
    c.n_dcs, c.slots, c.n_keys = D, _abi.SNAPSHOT_THRESHOLD, K
    c.n = c.clock = c.last_op = c.value = FAKE
    if mask:
        c.clock_mask = FAKE
    if arena:
        c.state_tag = c.state_tok = c.state_ctl = FAKE
        c.state_cap = 1 << 10
    log = _abi.AgnLog()
    log.crdt_type, log.n_dcs, log.n_keys = typ, D, K
    log.key_off = FAKE
    return c, log


def test_path_table():
    try:
        set_knob("AGN_LWW_FUSED", None)
        set_knob("AGN_READ_CACHED_SPLIT", None)
        for D in (1, 8, 9, 64):
            assert read_cached_path(*shapes(LWW, D), 100) is True, D
        assert read_cached_path(*shapes(LWW, 65), 100) is False
        assert read_cached_path(*shapes(LWW, 256), 100) is False
        # the bulk switch, as measured: the sequence from 2^14 requests
        for D in (1, 8, 16, 64):
            assert read_cached_path(*shapes(LWW, D), (1 << 14) - 1) is True
            assert read_cached_path(*shapes(LWW, D), 1 << 14) is False
        set_knob("AGN_READ_CACHED_SPLIT", "0")        # 0: never
        assert read_cached_path(*shapes(LWW, 8), 1 << 20) is True
        set_knob("AGN_READ_CACHED_SPLIT", "100")
        assert read_cached_path(*shapes(LWW, 8), 99) is True
        assert read_cached_path(*shapes(LWW, 8), 100) is False
        set_knob("AGN_READ_CACHED_SPLIT", None)
        # a masked log (oc_mask) over the dense-clock cache: the same path
        for D in (8, 16, 64):
            c, log = shapes(LWW, D)
            log.oc_mask = FAKE
            assert read_cached_path(c, log, 100) is True, D
            assert read_cached_path(c, log, 1 << 14) is False, D
        set_knob("AGN_LWW_FUSED", "0")
        for D in (1, 8, 9, 64, 65):
            assert read_cached_path(*shapes(LWW, D), 100) is False, D
        set_knob("AGN_LWW_FUSED", "1")
        assert read_cached_path(*shapes(LWW, 8), 100) is True
        set_knob("AGN_LWW_FUSED", None)
        # the existing refusals
        for kw in (dict(arena=False), dict(mask=True)):
            with pytest.raises(EngineError) as e:
                read_cached_path(*shapes(LWW, 8, **kw), 100)
            assert e.value.code == _abi.ENOTSUP
        c, log = shapes(LWW, 8)
        log.n_keys = 17
        with pytest.raises(EngineError) as e:
            read_cached_path(c, log, 100)
        assert e.value.code == _abi.EINVAL
        # the other types keep their answers
        for D in range(1, 9):
            split = 5_000_000 if D == 8 else 1 << 15
            assert read_cached_path(*shapes(_abi.COUNTER_PN, D, arena=False), split - 1) is True
            assert read_cached_path(*shapes(_abi.COUNTER_PN, D, arena=False), split) is False
        with pytest.raises(EngineError) as e:
            read_cached_path(*shapes(_abi.COUNTER_PN, 9, arena=False), 100)
        assert e.value.code == _abi.ENOTSUP
        for typ in (_abi.SET_AW, _abi.REGISTER_MV):
            for D in (3, 8, 64):
                assert read_cached_path(*shapes(typ, D), 100) is False
            with pytest.raises(EngineError) as e:
                read_cached_path(*shapes(typ, 8, arena=False), 100)
            assert e.value.code == _abi.ENOTSUP
    finally:
        set_knob("AGN_LWW_FUSED", None)
        set_knob("AGN_READ_CACHED_SPLIT", None)


def test_script_entries_tie_and_reach_the_edges():
    """The scripts' entries: ties (one ts, two tags) within a round of five,
    every edge timestamp, every tag, the invalid tag where the script says."""
    ents = [lc.script_entry(t) for t in range(60)]
    assert {e[0] for e in ents} == set(lc.TS_POOL)
    assert {e[1] for e in ents} == set(range(lc.N_TAGS))
    ties = 0
    for a in range(0, 55, 5):
        w = ents[a:a + 5]
        ties += any(x[0] == y[0] and x[1] != y[1] for x in w for y in w)
    assert ties >= 3
    for D, sparse in ((3, False), (5, True)):
        for name, s in ce.scripts(D, sparse).items():
            steps = lc.lww_steps(s)
            assert [st[0] for st in steps] == [st[0] for st in s.steps]
            bad = [e[1] for st in steps if st[0] == "append" for e in st[1]
                   if e[1][1] == _abi.TAG_INVALID]
            assert (len(bad) == 1) == (name == "invalid"), name


@pytest.mark.parametrize("D", [8, 16])
def test_masked_family_keeps_the_dense_outcomes(oracle_lib, D):
    """lc.masked: ops lack DCs (garbage above R in their place), and model and
    oracle agree that nothing else changes -- an absent DC neither excludes
    the op nor enters LastOpCt."""
    fam = lc.family(D)
    fm = lc.masked(fam)
    full = np.uint64((1 << D) - 1)
    lacking = fm.log.oc_mask[:, 0] != full
    assert lacking.sum() > fam.log.n_entries // 2
    assert (fm.log.oc[lacking] > np.uint64(1 << 60)).any(axis=1).all()
    order = np.arange(fam.K)
    a, b = chain(oracle_lib, fam, order), chain(oracle_lib, fm, order)
    for f in ("flags", "count", "hole", "out_n", "out_tag", "out_tok", "lastct", "err_pos"):
        assert np.array_equal(getattr(a["res"], f), getattr(b["res"], f)), f
    assert np.array_equal(a["arrs"]["n"], b["arrs"]["n"])
    assert np.array_equal(a["prune"], b["prune"])


def chain(lib, fam, order):
    """The C oracle's read/6 of fam's keys in `order` (the base state through
    a CSR built from the lookup's arena reference; the store's value a handle
    naming the request)."""
    D, K, S = fam.D, fam.K, fam.S
    arrs = {x: a.copy() for x, a in fam.cache.items()}
    c = ce.cache_struct(D, S, K, arrs, ce.ptr)
    req, co, gc = lc.requests(fam, order)
    n = req.n_req
    first, status = np.zeros(n + 8, np.uint8), np.zeros(n + 8, np.uint8)
    assert lib.oracle_ss_lookup(C.byref(c), n, ce.ptr(req.keys), ce.ptr(req.R), None,
                                ce.ptr(req.sct), None, ce.ptr(req.sct_ignore),
                                ce.ptr(req.base_value), ce.ptr(first), ce.ptr(status)) == 0
    bases, btag, btok = [], [], []
    boff = np.zeros(n + 1, np.uint64)
    for i in range(n):
        start, pairs = _abi.ss_state_unpack(int(req.base_value[i]))
        bases.append((int(fam.state_tag[start]), int(fam.state_tok[start])) if pairs else None)
        if pairs:
            btag.append(bases[-1][0])
            btok.append(bases[-1][1])
        boff[i + 1] = len(btag)
    req.base_off, req.base_tag, req.base_tok = boff, np.array(btag + [0], np.uint32), \
        np.array(btok + [0], np.uint64)
    res = alloc_result(n, D, sparse=False, cap_off=co)
    ls = log_struct(fam.log)     # dense, or lc.masked's oc_mask
    rs_, os_ = read_struct(req, sparse=False), result_struct(res)
    rs_.base_value = None
    assert lib.oracle_materialize(C.byref(ls), C.byref(rs_), C.byref(os_), 1) == 0
    want, incl, info = model(fam.log, req, False, co, bases=bases)
    bad = compare_lww(D, res, want, False, n)
    assert not bad, [(fam.names[order[b[0]]],) + tuple(b[1:]) for b in bad[:5]]
    handle = np.arange(n, dtype=np.int64) + 1000
    prune, thr = np.zeros(K + 8, np.uint8), np.zeros((K, D), np.uint64)
    n_before = arrs["n"].copy()
    head_before = arrs["clock"][:, 0].copy()
    assert lib.oracle_ss_store(C.byref(c), C.byref(ls), n, ce.ptr(req.keys), ce.ptr(first),
                               ce.ptr(status), ce.ptr(gc), C.byref(os_), ce.ptr(handle),
                               ce.ptr(prune), ce.ptr(thr), None) == 0
    return dict(res=res, info=info, status=status[:n], prune=prune, arrs=arrs, handle=handle,
                n_before=n_before, head_before=head_before, first=first[:n])


@pytest.mark.parametrize("D", [1, 8, 16, 64])
def test_family_reaches_its_edges(oracle_lib, D):
    fam = lc.family(D)
    o = fam.opi
    assert o == {1: 64, 8: 64, 16: 32, 64: 8}[D]
    assert fam.K % 2 == 1
    order = np.arange(fam.K)
    out = chain(oracle_lib, fam, order)
    res, arrs = out["res"], out["arrs"]
    seen = dict(length=set(), win=set(), tie=set(), look=set(), store=set(), nafter=set())
    for k, e in enumerate(fam.expect):
        s, nm = fam.specs[k], fam.names[k]
        fl = int(res.flags[k])
        st = int(out["status"][k])
        assert st == {"new": _abi.SS_NEW, "hit0": _abi.SS_HIT, "hit8": _abi.SS_HIT,
                      "log": _abi.SS_LOG}[e["look"]], nm
        assert int(out["first"][k]) == (0 if e["look"] == "hit8" else 1) or e["look"] == "log", nm
        seen["look"].add((e["look"], s["gc"]))
        if s["corrupt"]:
            assert fl == _abi.F_ERR_CORRUPTED and s["n"] > 0, nm
            assert int(arrs["n"][k]) == max(int(out["n_before"][k]), 1), nm
            continue
        assert int(res.hole[k]) == e["hole"], nm
        if "count" in e:
            assert int(res.count[k]) == e["count"], nm
        if e.get("err") is True:
            assert fl & _abi.F_ERR_UNEXPECTED and int(res.err_pos[k]) == int(
                fam.log.key_off[k]) + s["n"] - 1, nm
            continue
        if e.get("err") is False:
            assert not fl & _abi.F_ERR_UNEXPECTED and out["info"][k]["invalid_excluded"], nm
        if e.get("capacity"):
            assert fl & _abi.F_ERR_CAPACITY and int(res.out_n[k]) == 1, nm
            assert int(arrs["n"][k]) == int(out["n_before"][k]), nm
            continue
        got = None
        if int(res.out_n[k]):
            oo = int(res.out_off[k])
            got = (int(res.out_tag[oo]), int(res.out_tok[oo]))
        base_here = s["base"] is not None and st == _abi.SS_HIT
        if "length" in e:
            seen["length"].add(s["n"])
            if e["win"] is not None:
                # the placed op wins unless the read serves from the log (void)
                assert got == (s["tag"][e["win"]], lc.TOP), nm
                seen["win"].add((e["win"] == 0, e["win"] == o - 1, e["win"] == o,
                                 e["win"] == s["n"] - 1))
            else:
                assert got == (s["base"] if base_here else None), nm
        if "tie" in e:
            assert fl & _abi.F_TS_TIE and got == (e["win_tag"], lc.TOP), nm
            seen["tie"].add((e["tie"], e.get("base_wins"), s["name"]))
        elif "win_tag" in e:
            assert not fl & _abi.F_TS_TIE and got[0] == e["win_tag"], nm
        if "base_wins" in e:
            assert out["info"][k]["base_wins"] == e["base_wins"], nm
        if s["own_tx"]:
            assert int(res.count[k]) == 6 and fl & _abi.F_NEWSS, nm
        nb, na = int(out["n_before"][k]), int(arrs["n"][k])
        stored = arrs["value"][k, 0] == out["handle"][k]
        if "stored" in e:
            assert bool(stored) == e["stored"] or e.get("prepend") is False, nm
        if e.get("prepend") is False and s["gc"]:
            # a store that did not prepend: the head stays, the list is collected
            assert not stored and int(out["prune"][k]) == 1, nm
            assert np.array_equal(arrs["clock"][k, 0], out["head_before"][k]), nm
            seen["store"].add("not prepended")
        if "n_after" in e:
            assert na == e["n_after"] and int(out["prune"][k]) == int(e["prune"]), nm
            seen["nafter"].add((nb, na))
        if stored:
            seen["store"].add(("stored", s["gc"], int(out["prune"][k])))
    assert seen["length"] == set(lc.lengths(D)), seen["length"]
    want_win = {(True, False, False, False), (False, True, False, False),
                (False, False, True, False), (False, False, False, True)}
    assert all(any(all(a or not b for a, b in zip(w, t)) for w in seen["win"]) for t in want_win)
    assert {t[0] for t in seen["tie"]} == {"ops", "base"}
    assert {t[1] for t in seen["tie"] if t[0] == "base"} == {True, False}
    assert any("same chunk" in t[2] for t in seen["tie"]) or o == 1
    assert any("another chunk" in t[2] for t in seen["tie"])
    assert seen["look"] == {(lk, g) for lk in lc.LOOKS for g in (0, 1)}
    assert {(8, 9), (9, lc.KEEP)} <= seen["nafter"], seen["nafter"]
    assert "not prepended" in seen["store"]
    assert {("stored", 0, 0), ("stored", 1, 1), ("stored", 0, 1)} <= seen["store"], seen["store"]
    # count 4 / 5 and op-id gap 4 / 5 split on the policy's thresholds
    for label, want in (("count 4", False), ("count 5", True), ("op-id gap 4", False),
                        ("op-id gap 5", True)):
        ks = [k for k, s in enumerate(fam.specs) if s["name"] == label]
        assert ks and all((arrs["value"][k, 0] == out["handle"][k]) == want for k in ks), label
    # both request orders name the same keys' outcomes
    rev = lc.orders(fam.K)[1][1]
    out2 = chain(oracle_lib, fam, rev)
    assert np.array_equal(out2["res"].flags, res.flags[rev])
    assert np.array_equal(out2["arrs"]["n"][:fam.K - 1], arrs["n"][:fam.K - 1])
