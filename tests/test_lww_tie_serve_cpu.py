"""The constructed timestamp ties of tests/lww_tie_serve_cases.py on the host
alone: every key reaches the branch it is named for, the label tables decide
against the id order, only the unlabelled keys are flagged, the script's store
points hold, and the reference transcription's vnode serves every labelled
read -- conditions on the inputs of tests/test_lww_tie_serve.py, checked on
tests/lww_order_model.py for every serve_dispatch shape, dense and masked, and
both tables, before anything reaches a GPU."""
import functools

import numpy as np
import pytest

import lww_order_model as om
import lww_tie_serve_cases as tc
from antidote_amd import _abi
from lww_model import opi

DS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 32, 33, 64]
SHAPES = [(D, m) for D in DS for m in (False, True) if D >= 2 or not m]
IDS = [f"D{d}-{'masked' if m else 'dense'}" for d, m in SHAPES]
WIDE = [(65, False), (129, True)]           # the sequence-only shapes test_lww_tie_serve also runs
TIE = _abi.F_TS_TIE


@functools.lru_cache(maxsize=None)
def run(D, masked):
    fam = tc.family(D, masked)
    return fam, {t: tc.script(fam, t) for t in tc.TABLES}


def test_shapes_are_every_serve_dispatch_row():
    assert len(SHAPES) == 27
    assert {opi(D) for D in DS} == {64, 32, 16, 8} and set(range(1, 9)) <= set(DS)
    assert {D for D in DS if D > 8} == {9, 16, 17, 32, 33, 64}


def test_tables():
    a, b = tc.TABLES["first"], tc.TABLES["reversed"]
    assert len(a) == len(b) == 8 and a[tc.UNL_IN] == b[tc.UNL_IN] == 0 and tc.UNL_PAST >= len(a)
    assert a[7] and b[7]                     # the zero lies inside the table
    la = [int(a[t]) for t in tc.TIED]
    assert len(set(la)) == 5 and sorted(la) == sorted(int(b[t]) for t in tc.TIED)
    ra = sorted(tc.TIED, key=lambda t: int(a[t]))
    rb = sorted(tc.TIED, key=lambda t: int(b[t]))
    assert ra == rb[::-1]                    # the second is the first one's order reversed
    for tab in (a, b):
        labs = [int(tab[t]) for t in tc.TIED]
        pairs = [(x, y) for x in labs for y in labs if x < y]
        assert any(x & 0xFFFFFFFF == y & 0xFFFFFFFF for x, y in pairs)      # differ above bit 32
        assert any(x >> 32 == y >> 32 for x, y in pairs)                    # ... only below
        assert sum(x >= tc.U63 for x in labs) == 2
    signed = lambda x: x - (1 << 64) if x >= tc.U63 else x  # noqa: E731
    for name, tab in tc.TABLES.items():
        # the value terms' order is the labels'
        ts = sorted(tc.TIED, key=lambda t: tc.value(name, t))
        assert ts == sorted(tc.TIED, key=lambda t: int(tab[t])), name
        # a wrong half, or a signed compare, changes the winner of some pair the family ties
        wrong = dict(low=lambda x: x & 0xFFFFFFFF, high=lambda x: x >> 32, signed=signed,
                     dropped=lambda x: 0)
        for how, f in wrong.items():
            hit = [(x, y) for x, y in tc.ALL_PAIRS
                   if max((int(tab[t]), t) for t in (x, y))[1] !=
                   max((f(int(tab[t])), t) for t in (x, y))[1]]
            assert hit or (how == "high" and name == "reversed"), (name, how)
    for how in ("low", "high"):
        f = (lambda x: x & 0xFFFFFFFF) if how == "low" else (lambda x: x >> 32)
        assert any(max((int(tab[t]), t) for t in p)[1] != max((f(int(tab[t])), t) for t in p)[1]
                   for tab in tc.TABLES.values() for p in tc.ALL_PAIRS), how
    # every tied pair: one table decides it against the id order
    for x, y in tc.ALL_PAIRS:
        w = {n: max((int(tab[t]), t) for t in (x, y))[1] for n, tab in tc.TABLES.items()}
        assert set(w.values()) == {x, y}, (x, y, w)
    # rewriting every label with the order kept (the GPU test's relabel)
    for tab in tc.TABLES.values():
        t3 = tab // np.uint64(3)
        assert (np.argsort(t3[1:6], kind="stable") == np.argsort(tab[1:6], kind="stable")).all()
        assert len(set(t3[[0, 1, 2, 3, 4, 5, 7]].tolist())) == 7 and t3[tc.UNL_IN] == 0
        assert t3[[0, 1, 2, 3, 4, 5, 7]].all()


def tied_set(fam, k, r):
    """The tags at TOP among the read's candidates, from the builder's own
    positions: the included tied ops, and the base pair."""
    s = fam.keys[k]
    T = {t for p, t in s["tied"].items() if r["incl"][p]}
    if r["base"] is not None and r["base"][1] == tc.TOP:
        T.add(r["base"][0])
    return T


@pytest.mark.parametrize("D,masked", SHAPES + WIDE, ids=IDS + ["D65-dense", "D129-masked"])
def test_geometry(D, masked):
    fam, runs = run(D, masked)
    o = fam.opi
    seen = set()
    for table, (out, _q) in runs.items():
        for k, s in enumerate(fam.keys):
            r, nm = out[k]["reads"][0], (table, s["name"])
            info, reach = r["info"], s["reach"]
            assert r["status"] == (_abi.SS_NEW if s["look"] == "new" else _abi.SS_HIT), nm
            assert r["out_n"] == 1 and r["pair"][1] == tc.TOP, nm
            T = tied_set(fam, k, r)
            assert info["nT"] == len(T), nm
            lanes = {}
            for p, t in s["tied"].items():
                if r["incl"][p]:
                    lanes.setdefault(p % o, []).append((p, t))
            if reach.get("across"):
                assert info["across_lanes"] and not info["in_lane"] and len(lanes) > 1, nm
                assert len({p // o for ps in lanes.values() for p, _t in ps}) == 1, nm
            if reach.get("in_lane"):
                assert info["in_lane"], nm
                two = [ps for ps in lanes.values() if len({t for _p, t in ps}) > 1]
                assert two and all(len({p // o for p, _t in ps}) > 1 for ps in two), nm
            if reach.get("base_tie"):
                assert info["base_tie"] and r["base"][1] == tc.TOP, nm
                assert s["prev"] >= 1 and not r["incl"][:s["prev"]].any(), nm
            if "lane0" in reach:
                on0 = all(p % o == 0 for p in s["tied"])
                assert on0 == bool(reach["lane0"]), nm
            if reach.get("last_iter"):
                p = max(s["tied"])
                assert p == s["n"] - 1 and p % o == 0 and p // o == (s["n"] - 1) // o >= 1, nm
            if reach.get("single"):
                assert info["nT"] == 1 and not info["flagged"], nm
            if "middle" in reach:
                ps = sorted(s["tied"])
                assert info["nT"] == 3 and ps[0] % o == ps[1] % o, nm
                if reach["middle"] == table:
                    assert r["pair"][0] == s["tied"][ps[1]], nm
            if s["case"] == "excluded":
                p = max(s["tied"])
                lw = max((int(tc.TABLES[table][t]), t) for t in s["tied"].values())[1]
                assert not r["incl"][p] and r["incl"][:p].all(), nm
                assert s["tied"][p] not in T and r["pair"][0] in T, nm
                if "wins" in reach:
                    assert r["pair"][0] == reach["wins"], nm
                    seen.add(("excluded winner", lw == s["tied"][p]))
            if s["case"] == "behind":
                assert s["tied"][1] not in T and not r["incl"][1] and len(T) == 2, nm
                if table == reach["table"]:     # ... it would have won under its table
                    every = list(s["tied"].values()) + [s["base"][0]]
                    assert max((int(tc.TABLES[table][t]), t) for t in every)[1] == s["tied"][1], nm
            if s["unl"]:
                assert info["flagged"] and not info["labelled"], nm
                assert info["past_table"] == (tc.UNL_PAST in T), nm
                seen.add(("unl", tc.UNL_IN in T, tc.UNL_PAST in T, bool(info["in_lane"]),
                          bool(info["across_lanes"]), bool(info["base_tie"])))
            seen.add((s["case"], s["look"], s["gc"]))
            seen.add(("length", s["case"], (s["n"] == o, s["n"] == o + 1)))
    assert ("excluded winner", True) in seen
    for case in ("lanes", "lane"):
        assert {(case, "hit", 0), (case, "new", 0), (case, "hit", 1), (case, "new", 1)} <= seen
        assert ("length", case, (False, True)) in seen
    assert ("length", "lanes", (True, False)) in seen
    # the three unlabelled forms, each in a lane and across lanes
    for u_in, u_past in ((True, False), (False, True)):
        assert ("unl", u_in, u_past, True, False, False) in seen
        assert ("unl", u_in, u_past, False, True, False) in seen
        assert any(x[:3] == ("unl", u_in, u_past) and x[5] for x in seen)


@pytest.mark.parametrize("D,masked", SHAPES, ids=IDS)
def test_winners_flags_counts_and_vnode(D, masked):
    fam, runs = run(D, masked)
    a, b = runs["first"][0], runs["reversed"][0]
    against = {}
    for k, s in enumerate(fam.keys):
        ra, rb = a[k]["reads"][0], b[k]["reads"][0]
        T = tied_set(fam, k, ra)
        assert T == tied_set(fam, k, rb)
        for table, r in (("first", ra), ("reversed", rb)):
            want = max((om.label(tc.TABLES[table], t), t) for t in T)[1]
            assert r["pair"] == (want, tc.TOP), (table, s["name"])
        if s["unl"]:
            continue
        if len(T) > 1:
            # the id-order winner is the wrong answer under one of the tables,
            # and the tables disagree
            idw = max(T)
            assert ra["pair"][0] != rb["pair"][0], s["name"]
            assert idw != ra["pair"][0] or idw != rb["pair"][0], s["name"]
            against.setdefault(s["case"], set()).update(
                t for t, r in (("first", ra), ("reversed", rb)) if r["pair"][0] != idw)
    # both tables decide against the id order in every case that ties
    assert set(against) == {"lanes", "lane", "three", "last", "base-lane0", "base-other",
                            "base-plus", "excluded", "behind"}
    assert all(v == {"first", "reversed"} for v in against.values()), against
    for table, (out, quirk) in runs.items():
        beats = loses = 0
        for k, s in enumerate(fam.keys):
            r1, r2, r3 = out[k]["reads"]
            nm = (table, s["name"])
            # flags: exactly the unlabelled keys (their later reads may stay flagged)
            assert bool(r1["flags"] & TIE) == s["unl"], nm
            if not s["unl"]:
                assert not (r2["flags"] | r3["flags"]) & TIE, nm
            assert not (r1["flags"] | r2["flags"] | r3["flags"]) & \
                (_abi.F_ERR_UNEXPECTED | _abi.F_ERR_CORRUPTED | _abi.F_ERR_CAPACITY), nm
            # counts: the constructed read stores, (a) hits it with count 0
            assert r1["count"] == s["upto"] - s["prev"] >= tc.MIN_OPS and r1["stored"], nm
            assert r1["pruned"] == (s["prev"] if s["gc"] else 0), nm
            assert r2["status"] == _abi.SS_HIT and r2["count"] == 0 and not r2["stored"], nm
            assert r2["pair"] == r1["pair"] == r2["base"], nm
            assert r3["status"] == _abi.SS_HIT and r3["base"] == r1["pair"], nm
            assert r3["count"] == 1 + s["n"] - s["upto"] and not r3["stored"], nm
            tag = out[k]["extra"][3]
            assert tag != r1["pair"][0] and tag in tc.TIED, nm
            if s["upto"] == s["n"]:
                beats += r3["pair"][0] == tag
                loses += r3["pair"][0] == r1["pair"][0]
            # the reference vnode serves every labelled read
            if not s["unl"]:
                for r in (r1, r2, r3):
                    assert r["vnode"] == (r["pair"][1], tc.value(table, r["pair"][0])), \
                        (nm, r["vnode"], r["pair"])
        assert quirk == set(), (table, quirk)
        assert beats >= fam.K // 4 and loses >= fam.K // 4, (table, beats, loses, fam.K)


@pytest.mark.parametrize("D,masked", WIDE, ids=["D65-dense", "D129-masked"])
def test_wide_shapes_hold_the_same_conditions(D, masked):
    """Beyond the fused kernel's widths the iterations are 4 and 2 ops: the
    reads that count five ops store, the others are served all the same."""
    fam, runs = run(D, masked)
    for table, (out, quirk) in runs.items():
        for k, s in enumerate(fam.keys):
            r1, r2, r3 = out[k]["reads"]
            assert bool(r1["flags"] & TIE) == s["unl"], s["name"]
            assert r1["stored"] == (r1["count"] >= tc.MIN_OPS or bool(s["gc"])), s["name"]
            if not s["unl"]:
                for r in (r1, r2, r3):
                    assert r["vnode"] == (r["pair"][1], tc.value(table, r["pair"][0])), s["name"]
        assert quirk == set()


def test_masked_ops_lack_dcs():
    fam = tc.family(5, True)
    full = int(fam.full[0])
    lack = sum(int((m[:, 0] != full).sum()) for m in fam.mask)
    total = sum(len(m) for m in fam.mask)
    assert lack > total // 2
    for k in range(fam.K):
        bad = fam.mask[k][:, 0] != full
        assert (fam.oc[k][bad] > np.uint64(1 << 60)).any(axis=1).all()
    w = tc.family(129, True)
    assert w.W == 3 and any((m != w.full).any() for m in w.mask)
    # the rows built at once are op_row's (which builds the follow-up op)
    for f in (fam, w, tc.family(8, False)):
        for k in (0, 1, f.K - 1):
            for q in range(f.keys[k]["n"]):
                oc, m = tc.op_row(f.D, k % f.D, q, f.masked)
                assert np.array_equal(oc, f.oc[k][q]), (f.D, k, q)
                assert m is None or np.array_equal(m, f.mask[k][q]), (f.D, k, q)


@pytest.mark.parametrize("D,masked", [(3, True), (8, False), (64, True)])
def test_building_twice_gives_identical_arrays(D, masked):
    f1, f2 = tc.family(D, masked), tc.family(D, masked)
    assert [s["name"] for s in f1.keys] == [s["name"] for s in f2.keys]
    for x in ("oc", "ts", "tag", "sct", "R") + (("mask",) if masked else ()):
        for u, v in zip(getattr(f1, x), getattr(f2, x)):
            assert u.dtype == v.dtype and np.array_equal(u, v), x
    s1, s2 = tc.script(f1, "first")[0], tc.script(f2, "first")[0]
    for u, v in zip(s1.values(), s2.values()):
        assert u["extra"][3] == v["extra"][3]
        for ru, rv in zip(u["reads"], v["reads"]):
            assert (ru["pair"], ru["flags"], ru["count"], ru["hole"]) == \
                (rv["pair"], rv["flags"], rv["count"], rv["hole"])
            assert np.array_equal(ru["lastct"], rv["lastct"])
