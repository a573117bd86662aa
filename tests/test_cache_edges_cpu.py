"""The constructed cache edges of tests/cache_edges.py without a GPU:

* the C oracle (oracle_ss_lookup / oracle_ss_store / oracle_select_base)
  against the dict restatement (test_ss_cache.py_model on
  py_oracle.VectorOrddict) on every key of Families L, S and G, and
  oracle_materialize against py_oracle.materialize on Family R's keys;
* reach: every named edge produces the outcome it was built for -- the lookup
  status, the hit slot (the slot whose clock SCT is), is_first, the change of
  the list size, prune, and which kept slot supplied each threshold column --
  and every outcome class occurs at every width, so that a builder that loses
  its edge fails here instead of passing quietly on the GPU;
* Family B's scripts through CacheMirror: the exact list sizes of `grow`
  (1, 2, ..., 9, 3), the slots `deep` hits (8 down to 1), LOG for `below`;
* determinism: building a family twice gives identical arrays."""
import numpy as np
import pytest

import cache_edges as ce
import test_oracle_crosscheck as xc
from antidote_amd import _abi
from antidote_amd.encode import EncodedRead
from oracle import py_oracle as po
from test_ss_cache import check_oracle_vs_model, run_oracle, vc

HIT, NEW, LOG = _abi.SS_HIT, _abi.SS_NEW, _abi.SS_LOG
WIDTHS = (1, 3, 8, 9, 64, 65, 130)


def bit(m, d):
    return (int(m[d >> 6]) >> (d & 63)) & 1


def hit_slot(cs_clock, cs_mask, k, n, sct, sctm, D):
    """The slots of key k whose clock (and DC set) SCT is."""
    out = []
    for j in range(n):
        pres = [cs_mask is None or bit(cs_mask[k, j], d) for d in range(D)]
        if cs_mask is not None and not np.array_equal(cs_mask[k, j], sctm):
            continue
        if all(int(cs_clock[k, j, d]) == int(sct[d]) for d in range(D) if pres[d]):
            out.append(j)
    return out


def threshold_sources(a, out, k, D, sparse):
    """Per column: the kept slots whose present entry is the threshold's (an
    empty list: no kept clock has the DC)."""
    n = int(a["n"][k])
    src = []
    for d in range(D):
        have = [j for j in range(n) if not sparse or bit(a["mask"][k, j], d)]
        lo = min([int(a["clock"][k, j, d]) for j in have], default=0) if len(have) == n else 0
        assert int(out["thr"][k, d]) == lo, (k, d)
        if sparse:
            assert bit(out["thrm"][k], d) == (1 if have else 0), (k, d)
        src.append([j for j in have if int(a["clock"][k, j, d]) == lo] if len(have) == n else
                   (["absent"] if have else []))
    return src


@pytest.mark.parametrize("slots", ce.SLOTS)
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("D", WIDTHS)
def test_families_l_s(oracle_lib, D, sparse, slots):
    cs = ce.family_ls(D, slots, sparse)
    a, out = run_oracle(oracle_lib, cs)
    check_oracle_vs_model(cs, a, out)
    seen = set()
    for i, (name, e) in enumerate(zip(cs.names, cs.expect)):
        k, n0 = i, int(cs.n[i])
        assert int(out["status"][i]) == ce.STATUS[e["look"]], name
        if e["look"] == ce.HIT:
            f = e["f"]
            got = hit_slot(cs.clock, cs.mask, k, n0, out["sct"][i],
                           out["sctm"][i] if sparse else None, D)
            assert f in got, (name, got)
            assert int(out["base"][i]) == int(cs.value[k, f]), name
            assert int(out["first"][i]) == (1 if f == 0 else 0), name
            assert int(out["ign"][i]) == 0, name
            # no earlier slot is <= R
            R = vc(cs.R[i], cs.Rm[i] if sparse else None, D)
            for j in range(f):
                assert not po.vc_le(vc(cs.clock[k, j], cs.mask[k, j] if sparse else None, D), R), \
                    (name, j)
            seen.add(("hit", "first" if f == 0 else "last" if f == n0 - 1 else f))
            seen.add(("hit slot", f))
        else:
            assert int(out["ign"][i]) == 1 and int(out["base"][i]) == 0, name
            assert int(out["first"][i]) == (1 if e["look"] == ce.NEW else 0), name
            seen.add((e["look"],))
        n1 = max(n0, 1)
        assert int(a["n"][k]) == e["n"], (name, int(a["n"][k]), e["n"])
        assert int(out["prune"][k]) == (1 if e["prune"] else 0), name
        if not e["stored"]:
            assert e["n"] == n1 and not e["prune"], name
            for x in ("clock", "last_op", "value") + (("mask",) if sparse else ()):
                if n0:
                    assert np.array_equal(a[x][k, :n0], getattr(cs, x)[k, :n0]), (name, x)
        else:
            prepended = int(a["last_op"][k, 0]) == int(cs.hole[i]) and \
                int(a["value"][k, 0]) == int(cs.res_value[i])
            if prepended:
                assert np.array_equal(a["clock"][k, 0], cs.lastct[i]), name
            kept = e["n"] - (1 if prepended else 0)
            for x in ("clock", "last_op", "value"):
                assert np.array_equal(a[x][k, e["n"] - kept:e["n"]],
                                      getattr(cs, x)[k, :kept] if n0 else
                                      np.zeros_like(a[x][k, :kept])), (name, x)
            seen.add(("store", "prepend" if prepended else "keep", "collect" if e["prune"]
                      else "grow", e["n"] - n1))
            if "not prepended" in name:
                assert not prepended, name
            if ": prepended" in name or ", prepended" in name:
                assert prepended, name
        if e.get("thr"):
            src = threshold_sources(a, out, k, D, sparse)
            if e["thr"] == "rotate" and not (int(a["last_op"][k, 0]) == int(cs.hole[i])):
                assert all(len(s) == 1 for s in src), name
                assert len({s[0] for s in src}) == min(D, ce.KEEP), (name, src)
                seen.add(("thr", "rotate"))
            elif isinstance(e["thr"], tuple):
                kind, c = e["thr"]
                assert int(out["thr"][k, c]) == 0, name
                assert src[c] == (["absent"] if kind == "zero_set" else []), (name, src[c])
                assert bit(out["thrm"][k], c) == (1 if kind == "zero_set" else 0), name
                seen.add(("thr", kind))
    # every outcome class at this width
    want = {("new",), ("log",), ("hit", "first"), ("hit", "last"), ("hit slot", 1),
            ("hit slot", 7), ("hit slot", 8), ("hit slot", slots - 1),
            ("store", "prepend", "grow", 1), ("store", "keep", "grow", 0),
            ("store", "prepend", "collect", ce.KEEP - 9), ("store", "keep", "collect", 0),
            ("store", "keep", "collect", ce.KEEP - 9), ("store", "prepend", "collect", 1),
            ("thr", "rotate")}
    if sparse:
        want |= {("thr", "zero_set"), ("thr", "zero_clear")}
    assert want <= seen, sorted(want - seen, key=str)
    # the names the families must hold
    text = "\n".join(cs.names)
    for frag in ("status LOG", "number_of_ops = 0", "ERR_UNEXPECTED", "ERR_CORRUPTED",
                 "ERR_CAPACITY", "CT_IGNORE", "no NEWSS", "is_first = 0", "count 4", "count 5",
                 "hole - last_op = -1", "hole - last_op = 4", "hole - last_op = 5",
                 "hole - last_op = 4, GC read", "equals the head clock", "above the head in column",
                 "n = 8 -> 9", "n = 9, prepended", "n = 9, not prepended",
                 "GC read, n = 1,", "GC read, n = 9,", "clock equals R in every column",
                 "above R in all columns", "none: the last slot above R"):
        assert frag in text, frag
    if D > 1:
        assert "below the head in column 0" in text and "above R in column 0 only" in text
    if slots == ce.NSLOT:
        assert "n = 15, prepended" in text
    if sparse:
        for frag in ("absent from the head clock", "absent from R, head entry 0",
                     "absent from R, head entry 1", "all-absent last clock",
                     "only in LastOpCt, entry 1", "only in LastOpCt, entry 0",
                     "only in the head clock", "absent from one kept clock",
                     "absent from all kept clocks"):
            assert frag in text, frag


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("D", [1, 8, 64, 65, 130])
def test_family_g(oracle_lib, D, sparse):
    g = ce.family_g(D, sparse)
    nq = len(g["names"])
    wi, wf = np.zeros(nq, np.int32), np.zeros(nq, np.uint8)
    p = ce.ptr
    assert oracle_lib.oracle_select_base(D, nq, p(g["off"]), p(g["clocks"]), p(g["cm"]), p(g["R"]),
                                         p(g["Rm"]), p(wi), p(wf)) == 0
    for i, name in enumerate(g["names"]):
        a, b = int(g["off"][i]), int(g["off"][i + 1])
        lst = po.VectorOrddict([(vc(g["clocks"][c], g["cm"][c] if sparse else None, D), c - a)
                                for c in range(a, b)])
        found, first = lst.get_smaller(vc(g["R"][i], g["Rm"][i] if sparse else None, D))
        assert int(wi[i]) == (found[1] if found else -1), name
        assert bool(wf[i]) == first, name
        # the edge it was built for
        assert int(wi[i]) == int(g["idx"][i]) and int(wf[i]) == int(g["first"][i]), name
    lens = np.diff(g["off"].astype(np.int64))
    for n in ce.G_LENGTHS:
        sel = lens == n
        assert sel.any()
        if n:
            assert (wi[sel] == 0).any() and (wi[sel] == n - 1).any() and (wi[sel] == -1).any(), n
    assert ((wi == -1) & (wf == 1)).any() and ((wi == -1) & (wf == 0)).any()


def r_check(oracle_lib, r):
    m = ce.CacheMirror(oracle_lib, r.K, r.D, r.S, cache=r.cache)
    ls = ce.r_log_struct(r)
    o = m.read_batch(ls, r.keys, r.R, r.txid, r.gc)
    res = o["res"]
    seen = set()
    for k, (name, e) in enumerate(zip(r.names, r.expect)):
        n0 = int(r.cache["n"][k])
        assert int(o["status"][k]) == ce.STATUS[e["look"]], name
        if e["look"] == ce.HIT:
            got = hit_slot(r.cache["clock"], None, k, n0, o["sct"][k], None, r.D)
            assert got == [e["f"]], (name, got)
            assert int(o["first"][k]) == (1 if e["f"] == 0 else 0), name
        fl = int(res.flags[k])
        assert bool(fl & _abi.F_ERR_CORRUPTED) == e["corrupt"], name
        assert bool(fl & _abi.F_ERR_UNEXPECTED) == e["err"], name
        if e["err"]:
            pos = e["pattern"].index("E")
            off = int(r.log.key_off[k])
            assert int(res.err_pos[k]) == off + pos, name
        if e["count"] is not None:
            assert int(res.count[k]) == e["count"], (name, int(res.count[k]), e["count"])
        assert m.size(k) == e["n"], (name, m.size(k), e["n"])
        assert int(o["prune"][k]) == (1 if e["prune"] else 0), name
        prepended = m.size(k) > 0 and e["stored"] and \
            int(m.arr["last_op"][k, 0]) == int(res.hole[k]) and \
            np.array_equal(m.arr["clock"][k, 0], res.lastct[k])
        if e["stored"]:
            assert prepended == e["prepend"], name
            if not e["err"] and not e["corrupt"] and e["n0"]:
                assert int(res.hole[k]) - int(r.cache["last_op"][k, 0]) == e["gap"], name
        else:
            n1 = max(n0, 1)
            assert m.size(k) == n1, name
            if n0:
                assert np.array_equal(m.arr["clock"][k, :n0], r.cache["clock"][k, :n0]), name
        pat = e["pattern"]
        n = len(pat)
        for ch in "XPE":
            if pat.count(ch) == 1 and n in ce.R_LENGTHS:
                seen.add(("scan", n, ch, pat.index(ch), e["look"], e["f"]))
        if pat == "I" * n and n in ce.R_LENGTHS:
            seen.add(("scan", n, "I", None, e["look"], e["f"]))
        seen.add(("look", e["look"], e["f"]))
        if e["look"] == ce.HIT and np.array_equal(r.R[k], o["sct"][k]):
            seen.add(("R equals the hit clock", e["f"]))
        if e["stored"]:
            seen.add(("store", e["n0"], "prepend" if e["prepend"] else "keep",
                      "collect" if e["prune"] else "grow", e["gc"]))
        else:
            why = ("log" if e["look"] == ce.LOG else "nops" if not pat else
                   "corrupt" if e["corrupt"] else "err" if e["err"] else
                   "ct_ignore" if fl & _abi.F_CT_IGNORE else
                   "no_newss" if not fl & _abi.F_NEWSS else
                   "not_first" if not int(o["first"][k]) else
                   "count4" if int(res.count[k]) == ce.MIN_OPS - 1 else
                   f"gap{e['gap']}" if int(res.count[k]) >= ce.MIN_OPS else "count")
            seen.add(("nostore", why, e["gc"]))
        seen.add(("id0", e["id0"]))
        if e["stored"] and int(res.count[k]) == ce.MIN_OPS and not e["gc"]:
            seen.add(("count5",))
        if e["stored"] and e["gap"] == ce.MIN_OPS and e["n0"] and not e["gc"]:
            seen.add(("gap5",))
        if e["stored"] and e["gap"] == ce.MIN_OPS - 1 and e["gc"]:
            seen.add(("gap4 gc",))
        if "T" in pat:
            seen.add(("own txid", e["stored"], e["prepend"]))
    return m, o, seen


def r_required(D, slots):
    want = {("look", ce.NEW, None), ("look", ce.HIT, 0), ("look", ce.HIT, 8), ("look", ce.LOG, -1),
            ("id0", True), ("id0", False), ("count5",), ("gap5",), ("gap4 gc",),
            ("nostore", "log", 0), ("nostore", "log", 1), ("nostore", "nops", 0),
            ("nostore", "nops", 1), ("nostore", "corrupt", 0), ("nostore", "corrupt", 1),
            ("nostore", "err", 0), ("nostore", "err", 1), ("nostore", "ct_ignore", 0),
            ("nostore", "ct_ignore", 1), ("nostore", "no_newss", 0), ("nostore", "not_first", 0),
            ("nostore", "count4", 0), ("nostore", "gap-1", 0), ("nostore", "gap4", 0),
            ("store", 8, "prepend", "grow", 0), ("store", 9, "prepend", "collect", 0),
            ("store", 9, "keep", "grow", 0), ("store", 0, "prepend", "grow", 0),
            ("own txid", True, False), ("own txid", True, True)}
    for n in (1, 2, 3, 4, 9):
        want |= {("store", n, "prepend", "collect", 1), ("store", n, "keep", "collect", 1)}
    want |= {("R equals the hit clock", 0), ("R equals the hit clock", 8)}
    if slots >= ce.NSLOT:
        want |= {("store", 15, "prepend", "collect", 0), ("look", ce.HIT, 15),
                 ("R equals the hit clock", 15), ("nostore", "not_first", 0),
                 ("store", ce.NSLOT, "keep" if D == 1 else "prepend", "collect", 1),
                 ("store", ce.NSLOT, "keep", "collect", 1)}
    for n in ce.R_LENGTHS:
        for look, f in ((ce.NEW, None), (ce.HIT, 0), (ce.HIT, 8), (ce.LOG, -1)):
            want.add(("scan", n, "I", None, look, f))
            for p in ce.r_positions(n):
                for ch in "XPE":
                    want.add(("scan", n, ch, p, look, f))
    return want


@pytest.mark.parametrize("seg", [False, True], ids=["csr", "segments"])
@pytest.mark.parametrize("D", range(1, 9))
def test_family_r(oracle_lib, D, seg):
    r = ce.family_r(D, seg=seg)
    assert 200 < r.K < 500
    m, o, seen = r_check(oracle_lib, r)
    want = r_required(D, r.S)
    assert want <= seen, sorted(want - seen, key=str)
    if seg:
        return
    # oracle_materialize against the Python transcription, from the looked-up base
    req = EncodedRead(n_dcs=D, req_type=_abi.COUNTER_PN, keys=r.keys, R=r.R,
                      R_mask=np.zeros((r.K, 1), np.uint64), sct=o["sct"],
                      sct_mask=np.zeros((r.K, 1), np.uint64), sct_ignore=o["ign"], txid=r.txid,
                      base_value=o["base"], base_off=np.zeros(r.K + 1, np.uint64),
                      base_tag=np.zeros(0, np.uint32), base_tok=np.zeros(0, np.uint64))
    xc.SPARSE[0] = False
    for k, e in enumerate(r.expect):
        if e["corrupt"]:
            continue
        py = xc.py_run(r.log, req, k)
        c = xc.c_decode(r.log, req, o["res"], k, False)
        if py[0] == "error":
            assert c[0] == "error", r.names[k]
            continue
        assert c == py, (r.names[k], c, py)


def test_family_r_slots10(oracle_lib):
    r = ce.family_r(5, slots=10)
    _m, _o, seen = r_check(oracle_lib, r)
    want = r_required(5, 10)
    assert want <= seen, sorted(want - seen, key=str)


# ------------------------------------------------------------------ family B
def mirror_walk(lib, script, D, sparse):
    """The script on a one-key CacheMirror: per read (label, result, list
    size, log entries afterwards, the slot hit)."""
    m = ce.CacheMirror(lib, 1, D, ce.THRESHOLD, sparse)
    out, next_id = [], [1]
    for step in script.steps:
        if step[0] == "append":
            for oc, eff, mk in step[1]:
                m.append(0, oc, eff, next_id[0], 1000 + next_id[0], mk)
                next_id[0] += 1
            continue
        _x, R, rm, gc, label = step
        before = {x: a[0].copy() for x, a in m.arr.items()}
        g = m.read(0, R, rm, 0, gc)
        f = None
        if g["status"] == HIT:
            f = [j for j in range(int(before["n"])) if
                 np.array_equal(before["clock"][j], g["sct"])]
            f = f[0]
        out.append(dict(label=label, g=g, size=m.size(0), entries=len(m.entries[0]), f=f))
    return out


B_WIDTHS = (3, 5, 8, 9, 16, 17, 32, 33, 64)


# (the masked scripts are built for one mask word: D = 65 runs dense)
@pytest.mark.parametrize("D,sparse", [(D, sp) for D in B_WIDTHS for sp in (False, True)] +
                         [(65, False)])
def test_family_b(oracle_lib, D, sparse):
    sc = ce.scripts(D, sparse)
    w = {name: mirror_walk(oracle_lib, s, D, sparse) for name, s in sc.items()}
    grow = w["grow"]
    assert [x["size"] for x in grow] == [1, 2, 3, 4, 5, 6, 7, 8, 9, ce.KEEP]
    assert [x["g"]["status"] for x in grow] == [NEW] + [HIT] * 9
    assert [x["g"]["prune"] for x in grow] == [0] * 9 + [1]
    assert grow[-1]["entries"] < grow[-2]["entries"] == 40       # the log was pruned
    assert all(x["g"]["first"] for x in grow)
    assert [x["size"] for x in w["grow4"]] == [1, 2, 3, 3, 4, 5]
    assert w["grow4"][3]["g"]["count"] == 4 and w["grow4"][4]["g"]["count"] == 5
    deep = [x for x in w["deep"] if x["label"].startswith("deep")]
    assert [x["f"] for x in deep[:8]] == [8, 7, 6, 5, 4, 3, 2, 1]
    assert all(x["g"]["count"] == 2 and not x["g"]["first"] and x["size"] == 9
               for x in deep[:8])
    assert [x["f"] for x in deep[8:10]] == [7, 1] and all(x["g"]["count"] == 0 for x in deep[8:10])
    assert deep[10]["f"] == 5 and deep[10]["g"]["prune"] == 1 and deep[10]["size"] == ce.KEEP
    below = w["below"]
    assert [x["size"] for x in below[:10]] == [1, 2, 3, 4, 5, 6, 7, 8, 9, ce.KEEP]
    assert [x["g"]["status"] for x in below[10:13]] == [LOG] * 3
    assert all(x["size"] == ce.KEEP and x["g"]["prune"] == 0 for x in below[10:13])
    assert below[13]["g"]["status"] == HIT and below[13]["f"] == 0
    gt = w["gc_twice"]
    a, b = gt[5], gt[6]
    assert a["g"]["prune"] == 1 and a["size"] == ce.KEEP and a["g"]["count"] == 3
    assert b["g"]["prune"] == 1 and b["size"] == ce.KEEP and b["g"]["count"] == 0
    assert np.array_equal(a["g"]["lastct"], b["g"]["lastct"])       # LastOpCt = the head
    assert gt[7]["g"]["status"] == HIT and gt[7]["g"]["count"] == 1
    for x in w["invalid"][2:]:
        assert x["g"]["flags"] & _abi.F_ERR_UNEXPECTED and x["g"]["err_pos"] == 8, x["label"]
        assert x["size"] == 2 and x["g"]["prune"] == 0
    if sparse and D >= 3:
        full = (1 << D) - 1
        ops = [o for st in sc["mixed_sets"].steps if st[0] == "append" for o in st[1]]
        assert len({o[2] for o in ops}) > 1 and all(o[2] != full for o in ops)
        mx = w["mixed_sets"]
        # LastOpCt's DC set: SCT's united with the included ops'
        assert all(int(x["g"]["lastct_mask"][0]) == full for x in mx[1:])
        assert mx[4]["g"]["prune"] == 1 and mx[5]["g"]["count"] == 5
        un = w["uniform_set"]
        U = full & ~(1 << (D - 1))
        assert all(int(x["g"]["lastct_mask"][0]) == U for x in un[1:])
        assert un[-1]["g"]["prune"] == 1
        rl = w["r_lacks_dc"]
        assert rl[4]["g"]["status"] == HIT and rl[4]["f"] == 3 and rl[4]["g"]["count"] == 0
        assert rl[5]["g"]["prune"] == 1 and rl[5]["size"] == ce.KEEP
        assert [x["g"]["status"] for x in rl[6:8]] == [LOG, LOG]
        assert rl[8]["g"]["status"] == HIT and rl[8]["f"] == 0


# ------------------------------------------------------------------ determinism
def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[x], b[x]) for x in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def script_arrays(D, sparse):
    return {n: s.steps for n, s in ce.scripts(D, sparse).items()}


def r_arrays(D, seg):
    r = ce.family_r(D, seg=seg)
    lg = r.log
    return dict(cache=r.cache, R=r.R, tx=r.txid, gc=r.gc, key_len=r.key_len, key_off=lg.key_off,
                oc=lg.oc, op_id=lg.op_id, txid=lg.txid, eff=lg.eff, key_type=lg.key_type,
                names=r.names)


@pytest.mark.parametrize("build", [
    lambda: ce.family_ls(3, 10, False).all_arrays(), lambda: ce.family_ls(65, 16, True).all_arrays(),
    lambda: ce.family_ls(8, 9, True).all_arrays(), lambda: ce.family_g(130, True),
    lambda: ce.family_g(8, False), lambda: r_arrays(3, False), lambda: r_arrays(8, True),
    lambda: script_arrays(5, True), lambda: script_arrays(16, False)])
def test_deterministic(build):
    a, b = build(), build()
    assert same(a, b)
