"""The constructed edge cases of tests/edges.py without a GPU:

* the C oracle against the dict transcription (oracle/py_oracle.py) on every
  key of every family, GC against MaterializerVnode.prune_ops;
* attainment: from the inputs and the oracle's result, each named edge is
  really reached (the pattern's count, hole and error position, a chunk's
  token total and the matching token's index, the intended live size, a
  compaction, a straddling op, a segment start, the ring's token volume), so
  that a builder change that loses an edge fails here instead of passing
  vacuously on the GPU;
* determinism: building a family twice gives identical arrays."""
import ctypes as C

import numpy as np
import pytest

import edges
import test_oracle_crosscheck as xc
from antidote_amd import _abi
from antidote_amd.encode import alloc_result, log_struct, read_struct, result_struct
from oracle import py_oracle as po
from test_prune import oracle_prune

TAGS = (_abi.SET_AW, _abi.REGISTER_MV)
ALL = (_abi.COUNTER_PN,) + TAGS
ERR = _abi.F_ERR_UNEXPECTED


def run_oracle(oracle_lib, log, req, cap, sparse):
    res = alloc_result(req.n_req, log.n_dcs, sparse=True, cap_off=cap)
    ls, rs, os_ = log_struct(log), read_struct(req, sparse=bool(sparse)), result_struct(res)
    if not sparse:
        ls.oc_mask = None
    assert oracle_lib.oracle_materialize(C.byref(ls), C.byref(rs), C.byref(os_), 4) == 0
    return res


def crosscheck(oracle_lib, log, req, cap, names, sparse):
    """Every request through both restatements; returns the C oracle's result."""
    xc.SPARSE[0] = bool(sparse)
    res = run_oracle(oracle_lib, log, req, cap, sparse)
    for i in range(req.n_req):
        py = xc.py_run(log, req, i)
        if int(res.flags[i]) & _abi.F_ERR_CAPACITY:
            # no state written: the other fields and the state's size
            assert py[0] == "ok", names[i]
            n_py = sum(len(t) for _, t in py[1]) if log.crdt_type == _abi.SET_AW else len(py[1])
            assert n_py == int(res.out_n[i]), names[i]
            res.out_n[i] = 0
            c = xc.c_decode(log, req, res, i, True)
            res.out_n[i] = n_py
            assert c[2:] == py[2:], (names[i], c[2:], py[2:])
            continue
        c = xc.c_decode(log, req, res, i, True)
        if py[0] == "error":
            assert c[0] == "error", (names[i], py, c)
            k = int(req.keys[i])
            assert int(log.key_off[k]) <= c[1] < int(log.key_off[k + 1]), names[i]
            assert py[1][1] == ("invalid",), names[i]
            continue
        assert c == py, (names[i], c, py)
    return res


def expect_scan(log, req, i):
    """count, hole, err_pos of request i from its key's pattern alone."""
    k = int(req.keys[i])
    a, b = int(log.key_off[k]), int(log.key_off[k + 1])
    D = log.n_dcs
    if b == a:
        return 0, 0, None
    c = int(np.argmax(req.R[i] if log.oc_mask is None else
                      np.where(_bits(req.R_mask[i], D), req.R[i], 0)))
    ops = []  # (id, class) oldest first; classes from the clocks as built
    S = 1000 + (b - a) + 5
    for e in range(a, b):
        if ops and ops[-1][0] == int(log.op_id[e]):
            ops[-1][3].append(e)
            continue
        v = int(log.oc[e, c])
        cls = "X" if v > int(req.R[i, c]) else "I" if v > S else \
            "T" if int(log.txid[e]) == edges.READ_TXID else "P"
        ops.append((int(log.op_id[e]), cls, e, [e]))
    warm = not req.sct_ignore[i]
    incl = [o for o in ops if o[1] == "I" or (o[1] == "P" and not warm) or
            (o[1] == "T" and (not warm or int(req.txid[i]) == edges.READ_TXID))]
    excl = [o for o in ops if o[1] == "X"]
    hole = excl[0][0] - 1 if excl else ops[-1][0]
    bad = log.eff == _abi.EFFECT_INVALID if log.crdt_type == _abi.COUNTER_PN else \
        log.tag == _abi.TAG_INVALID
    count, err = 0, None
    for o in incl:
        hit = [e for e in o[3] if bad[e]]
        if hit:
            err = hit[0]
            break
        count += 1
    return count, hole, err


def _bits(row, D):
    return np.array([(int(row[d >> 6]) >> (d & 63)) & 1 for d in range(D)], bool)


def attain_scan(log, req, res, names):
    for i in range(req.n_req):
        count, hole, err = expect_scan(log, req, i)
        assert int(res.hole[i]) == hole, names[i]
        if err is None:
            assert not int(res.flags[i]) & ERR, names[i]
            assert int(res.count[i]) == count, names[i]
        else:
            assert int(res.flags[i]) & ERR and int(res.err_pos[i]) == err, names[i]


def pattern_counts(names):
    return {c: sum(f" {c}" in n for n in names) for c in "IXPTE"}


# ------------------------------------------------------------------ family A
A_CASES = [(crdt, D, sparse) for crdt in ALL
           for D, sparse in ((1, None), (3, None), (8, "uniform"), (5, "mixed"))]


@pytest.mark.parametrize("crdt,D,sparse", A_CASES)
def test_family_a(oracle_lib, crdt, D, sparse):
    log, req, cap, names = edges.family_a(crdt, D, sparse, identity=(D != 3))
    assert req.n_req == len(edges.family_a_patterns()) > 900
    res = crosscheck(oracle_lib, log, req, cap, names, sparse)
    attain_scan(log, req, res, names)
    lens = np.diff(log.key_off.astype(np.int64))
    assert set(lens.tolist()) == set(edges.LENGTHS)
    # every pattern class on every length's last lane, every column decides
    assert all(v > 100 for v in pattern_counts(names).values())
    assert {int(n.rsplit("col=", 1)[1]) for n in names} == set(range(D))
    # the two E at 63 and 64: the oldest included one is reported
    for i, n in enumerate(names):
        if " I63 E2" in n:
            k = int(req.keys[i])
            assert int(res.err_pos[i]) == int(log.key_off[k]) + 63, n
    if sparse == "mixed" and D >= 3:
        assert sum(edges.is_mixed(log, k) for k in range(log.n_keys)) > 800
    if sparse == "uniform":
        assert not any(edges.is_mixed(log, k) for k in range(log.n_keys))


# ------------------------------------------------------------------ family B
def key_effects(log, req, k):
    a, b = int(log.key_off[k]), int(log.key_off[k + 1])
    ro = log.rem_off
    rems = [log.rem_tok[int(ro[e]):int(ro[e + 1])].tolist() for e in range(a, b)]
    o0, o1 = int(req.base_off[k]), int(req.base_off[k + 1])
    base = list(zip(req.base_tag[o0:o1].tolist(), req.base_tok[o0:o1].tolist()))
    return base, log.tag[a:b], log.add_tok[a:b], rems


@pytest.mark.parametrize("crdt,D,sparse", [(c, D, s) for c in TAGS
                                           for D, s in ((2, None), (5, "mixed"), (8, "uniform"))])
def test_family_b(oracle_lib, crdt, D, sparse):
    log, req, cap, names, meta = edges.family_b(crdt, D, sparse)
    res = crosscheck(oracle_lib, log, req, cap, names, sparse)
    seen = set()
    for k, m in meta.items():
        if "err" in m:
            assert int(res.flags[k]) & ERR, names[k]
            assert int(res.err_pos[k]) == int(log.key_off[k]) + m["err"], names[k]
            base, tag, add, rems = key_effects(log, req, k)
            assert edges.model_used(crdt, base, tag[:m["err"]], add[:m["err"]],
                                    rems[:m["err"]])[1], names[k]
            continue
        assert int(res.out_n[k]) == m["L"], names[k]
        seen.add(m["L"])
        room = int(cap[k + 1] - cap[k])
        assert bool(int(res.flags[k]) & _abi.F_ERR_CAPACITY) == (room < m["L"]), names[k]
        if "room" in m:
            assert room == m["L"] - 1, names[k]
        base, tag, add, rems = key_effects(log, req, k)
        comp, ovf = edges.model_used(crdt, base, tag, add, rems)
        # alone, adds reach the slow pass past 256 pairs; a base past 192
        if "compacts" not in m and "overflow" not in m:
            assert ovf == (m["L"] > edges.FAST_CAP or len(base) > 192), names[k]
        if m.get("compacts"):
            assert comp >= 1, names[k]
        if m.get("overflow"):
            assert ovf, names[k]
            comp_s, ovf_s = edges.model_used(crdt, base, tag, add, rems, cap=edges.SLOW_CAP)
            assert not ovf_s, names[k]
            if m["L"] > 2000:
                assert comp_s >= 1, names[k]
        if m["L"] > edges.SLOW_CAP:
            assert edges.model_used(crdt, base, tag, add, rems, cap=edges.SLOW_CAP)[1], names[k]
    assert set(edges.LIVE_SIZES) <= seen
    # tokens descend in add order, many under one elem / value
    a, b = int(log.key_off[30]), int(log.key_off[31])
    assert b - a > 100 and (np.diff(log.add_tok[a:b].astype(np.int64)) < 0).all()
    assert len(set(log.tag[a:b].tolist())) == 3


@pytest.mark.parametrize("crdt,D,sparse", [(c, D, s) for c in TAGS
                                           for D, s in ((5, None), (8, "uniform"))])
def test_family_b300(oracle_lib, crdt, D, sparse):
    log, req, cap, names = edges.family_b300(crdt, D, sparse)
    res = crosscheck(oracle_lib, log, req, cap, names, sparse)
    assert req.n_req == 300 > 256
    assert (np.diff(req.base_off.astype(np.int64)) == 193).all()
    assert (res.out_n == 193 + np.arange(300) % 3).all()


# ------------------------------------------------------------------ family C
@pytest.mark.parametrize("crdt,D,sparse", [(c, D, s) for c in TAGS
                                           for D, s in ((2, None), (5, "mixed"), (8, "uniform"))])
def test_family_c(oracle_lib, crdt, D, sparse):
    log, req, cap, names, meta = edges.family_c(crdt, D, sparse)
    res = crosscheck(oracle_lib, log, req, cap, names, sparse)
    got_T, got_idx, kinds = set(), set(), set()
    for k, m in meta.items():
        a = int(log.key_off[k])
        ro = log.rem_off
        c0, c1 = int(ro[a + 64]), int(ro[a + 128])
        assert int(ro[a + 64]) == int(ro[a]), names[k]       # chunk 0 removes nothing
        assert c1 - c0 == m["T"], names[k]
        o, n = int(res.out_off[k]), int(res.out_n[k])
        live = set(res.out_tok[o:o + n].tolist())
        if m.get("span"):
            chunk = log.rem_tok[c0:c1].tolist()
            assert [chunk.index(t) for t in m["toks"]] == [63, 64, 129], names[k]
            own = a + 64 + 10
            assert (int(ro[own]) - c0, int(ro[own + 1]) - c0) == (30, 130), names[k]
            assert all(ro[e] == ro[e + 1] for e in (own - 1, own + 1)), names[k]
            assert all((t not in live) == m["dies"] for t in m["toks"]), names[k]
            continue
        assert int(log.rem_tok[c0 + m["idx"]]) == m["tok"], names[k]
        assert list(log.rem_tok[c0:c1]).count(m["tok"]) == 1, names[k]
        assert (m["tok"] not in live) == m["dies"], names[k]
        got_T.add(m["T"])
        got_idx.add(m["idx"])
        kinds.add((names[k].split("target=")[1], m["dies"]))
    assert got_T == set(edges.TOKEN_TOTALS)
    assert {0, 63, 64, 127, 128, 299} <= got_idx
    assert {("earlier chunk", True), ("earlier entry", True), ("same entry", False),
            ("later entry", False)} <= kinds
    if crdt == _abi.SET_AW:
        assert ("earlier chunk other elem", False) in kinds


# ------------------------------------------------------------------ family D
@pytest.mark.parametrize("D,sparse", [(2, None), (8, "uniform"), (5, "mixed")])
def test_family_d(oracle_lib, D, sparse):
    log, req, cap, names = edges.family_d(D, sparse)
    res = crosscheck(oracle_lib, log, req, cap, names, sparse)
    attain_scan(log, req, res, names)
    straddle = set()
    for k in range(log.n_keys):
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        ids = log.op_id[a:b]
        n_ops = 1 + int((ids[1:] != ids[:-1]).sum())
        assert n_ops < b - a, names[k]
        if "included" in names[k]:
            assert int(res.count[k]) == n_ops, names[k]
        for edge in (64, 128):
            if b - a > edge and ids[edge - 1] == ids[edge]:
                straddle.add(edge)
            if b - a > edge + 1 and ids[edge - 1] != ids[edge] == ids[edge + 1]:
                straddle.add(-edge)   # an op starting on a chunk's first lane
    assert straddle >= {64, 128, -64}


# ------------------------------------------------------------------ family F
@pytest.mark.parametrize("n_req,which", [(1, "all"), (1025, "all"), (1025, "first"),
                                         (2049, "last")])
def test_family_f_counter(oracle_lib, n_req, which):
    log, req, cap, names = edges.family_f_counter(n_req, which)
    res = crosscheck(oracle_lib, log, req, cap, names, "mixed")
    attain_scan(log, req, res, names)
    mixed = [k for k in range(n_req) if edges.is_mixed(log, k)]
    assert mixed == {"all": list(range(n_req)), "first": [0], "last": [n_req - 1]}[which]


def test_family_f_tags(oracle_lib):
    log, req, cap, names = edges.family_f_tags(_abi.SET_AW)
    res = crosscheck(oracle_lib, log, req, cap, names, "mixed")
    attain_scan(log, req, res, names)
    assert req.n_req > 8192 and all(edges.is_mixed(log, k) for k in range(req.n_req))


# ------------------------------------------------------------------ family E
def check_prune(oracle_lib, crdt, log, prune, thr, tm, names):
    """The C oracle's compaction against the ETS-tuple transcription; returns
    the kept entries per key."""
    arrs, flags, n_out = oracle_prune(oracle_lib, log, prune, thr, tm)
    D = log.n_dcs
    kept_n = np.diff(arrs["key_off"].astype(np.int64))
    for k in range(log.n_keys):
        ops = xc.key_ops(log, k, xc.TYPES[crdt])[::-1]
        got = arrs["op_id"][int(arrs["key_off"][k]):int(arrs["key_off"][k + 1])].tolist()
        if not prune[k]:
            assert got == [i for i, _ in ops] and flags[k] == 0, names[k]
            continue
        tup = po.EtsTuple(["k", (len(ops), len(ops) + 5), 0] + list(ops) + [0] * 6)
        threshold = xc.to_dict(thr[k], None if tm is None else tm[k], D)
        size, kept = po.MaterializerVnode.prune_ops(len(ops), tup, threshold)
        if all(el == 0 for _slot, el in kept):
            assert flags[k] == _abi.GC_ALL_PRUNED and got == [], names[k]
        else:
            assert flags[k] == 0 and got == [el[0] for _slot, el in kept], names[k]
            assert size == len(got), names[k]
    return arrs, flags, kept_n


@pytest.mark.parametrize("crdt,D,sparse", [(_abi.COUNTER_PN, 8, False), (_abi.COUNTER_PN, 3, True),
                                           (_abi.SET_AW, 5, False), (_abi.REGISTER_MV, 8, True),
                                           (_abi.REGISTER_LWW, 8, False)])
def test_family_e(oracle_lib, crdt, D, sparse):
    log, prune, thr, tm, names = edges.family_e(crdt, D, sparse)
    arrs, flags, kept_n = check_prune(oracle_lib, crdt, log, prune, thr, tm, names)
    seg = set()
    for k, name in enumerate(names):
        n = int(log.key_off[k + 1] - log.key_off[k])
        if name.startswith("filler"):
            continue
        if name.startswith("segment at"):
            off = int(name.split()[2])
            assert int(log.key_off[k]) % 32 == off, name
            seg.add(off)
        want = n
        if prune[k]:
            if "none kept" in name:
                want = 0
            elif "alternate" in name:
                want = (n + 1) // 2 if name.startswith("n=") else n // 2
            elif "one kept" in name:
                want = 1
            elif "drop" in name:
                want = n - int(name.rsplit(" ", 1)[1])
            assert (flags[k] == _abi.GC_ALL_PRUNED) == (want == 0), name
        assert int(kept_n[k]) == want, name
    assert seg == {0, 1, 31}
    assert (prune == 0).sum() > 20 and flags.any()


@pytest.mark.parametrize("crdt", TAGS)
def test_family_e_ring(oracle_lib, crdt):
    log, prune, thr, tm, names = edges.family_e_ring(crdt, 5)
    arrs, flags, kept_n = check_prune(oracle_lib, crdt, log, prune, thr, tm, names)
    longs = set()
    for k, name in enumerate(names):
        if not name.startswith("ring"):
            continue
        a = int(log.key_off[k])
        assert int(kept_n[k]) == 699, name
        lens = np.diff(log.rem_off[a:a + 701].astype(np.int64))
        moved = int(lens[1:].sum())
        assert moved > 2 * 512, name                    # the ring index wraps, twice
        short = lens[lens <= 4]
        assert short.min() == 1 and short.max() == 4, name
        longs |= set(lens[lens > 4].tolist())
    assert longs == {5, 64, 65, 200}


@pytest.mark.parametrize("n_keys", [1, 2, 3, 5, 7])
def test_family_e_small(oracle_lib, n_keys):
    log, prune, thr, tm, names = edges.family_e_small(n_keys)
    assert log.n_keys == n_keys
    check_prune(oracle_lib, _abi.COUNTER_PN, log, prune, thr, tm, names)


# ------------------------------------------------------------------ determinism
def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    if hasattr(a, "__dataclass_fields__"):
        return all(same(getattr(a, f), getattr(b, f)) for f in a.__dataclass_fields__)
    return a == b


@pytest.mark.parametrize("build", [
    lambda: edges.family_a(_abi.COUNTER_PN, 8, "mixed", lengths=(63, 64, 65)),
    lambda: edges.family_a(_abi.SET_AW, 17, None, identity=False, lengths=(127, 129)),
    lambda: edges.family_b(_abi.REGISTER_MV, 3, "mixed", sizes=(0, 65, 257)),
    lambda: edges.family_b300(_abi.SET_AW, 2),
    lambda: edges.family_c(_abi.SET_AW, 5, "uniform"),
    lambda: edges.family_d(8, "mixed"),
    lambda: edges.family_e(_abi.SET_AW, 5, True),
    lambda: edges.family_e_ring(_abi.REGISTER_MV, 2),
    lambda: edges.family_e_small(5),
    lambda: edges.family_f_counter(1025, "last"),
], ids=["a_counter", "a_set", "b", "b300", "c", "d", "e", "e_ring", "e_small", "f"])
def test_deterministic(build):
    assert same(build(), build())
