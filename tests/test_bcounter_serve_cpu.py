"""The fused counter_b cached read on the host: the path agn_read_cached takes
(agn_read_cached_path, no device), and the reach of the constructed cases
tests/test_bcounter_serve.py runs on the GPU -- every named edge is checked on
tests/bcounter_model.py and the C oracle's cache (oracle_ss_lookup ->
model -> oracle_ss_store) over the same arrays, so a builder that quietly
stops producing an edge goes red here."""
import numpy as np
import pytest

import bcounter_serve_cases as bc
from antidote_amd import _abi
from antidote_amd._lib import EngineError, set_knob
from antidote_amd.engine import read_cached_path
from test_lww_serve_cpu import FAKE, shapes

BC = _abi.COUNTER_B
LWW = _abi.REGISTER_LWW
SPLIT = 12288         # the bulk split api.hip carries for the type


def _others_unchanged():
    """Every answer tests/test_lww_serve_cpu.py's path table pins for the other
    types, assertion for assertion (its AGN_LWW_FUSED and
    AGN_READ_CACHED_SPLIT settings included); both are left unset."""
    set_knob("AGN_LWW_FUSED", None)
    set_knob("AGN_READ_CACHED_SPLIT", None)
    for D in (1, 8, 9, 64):
        assert read_cached_path(*shapes(LWW, D), 100) is True, D
    assert read_cached_path(*shapes(LWW, 65), 100) is False
    assert read_cached_path(*shapes(LWW, 256), 100) is False
    for D in (1, 8, 16, 64):
        assert read_cached_path(*shapes(LWW, D), (1 << 14) - 1) is True
        assert read_cached_path(*shapes(LWW, D), 1 << 14) is False
    set_knob("AGN_READ_CACHED_SPLIT", "0")        # 0: never
    assert read_cached_path(*shapes(LWW, 8), 1 << 20) is True
    set_knob("AGN_READ_CACHED_SPLIT", "100")
    assert read_cached_path(*shapes(LWW, 8), 99) is True
    assert read_cached_path(*shapes(LWW, 8), 100) is False
    set_knob("AGN_READ_CACHED_SPLIT", None)
    for D in (8, 16, 64):                          # a masked log over the dense-clock cache
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
    for kw in (dict(arena=False), dict(mask=True)):
        with pytest.raises(EngineError) as e:
            read_cached_path(*shapes(LWW, 8, **kw), 100)
        assert e.value.code == _abi.ENOTSUP
    for typ in (LWW, BC):
        c, log = shapes(typ, 8)
        log.n_keys = 17
        with pytest.raises(EngineError) as e:
            read_cached_path(c, log, 100)
        assert e.value.code == _abi.EINVAL
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


def test_path_table():
    try:
        set_knob("AGN_LWW_FUSED", None)
        set_knob("AGN_READ_CACHED_SPLIT", None)
        for knob in (None, "0"):            # off is the default
            set_knob("AGN_BCOUNTER_FUSED", knob)
            for D in (1, 8, 9, 64, 65, 256):
                assert read_cached_path(*shapes(BC, D), 100) is False, (knob, D)
        set_knob("AGN_BCOUNTER_FUSED", "1")
        for D in (1, 8, 9, 64):
            assert read_cached_path(*shapes(BC, D), 100) is True, D
        assert read_cached_path(*shapes(BC, 65), 100) is False
        assert read_cached_path(*shapes(BC, 256), 100) is False
        # the bulk split: measured at D = 8, used for every D <= 64
        for D in (1, 8, 16, 64):
            assert read_cached_path(*shapes(BC, D), SPLIT - 1) is True
            assert read_cached_path(*shapes(BC, D), SPLIT) is False
        set_knob("AGN_READ_CACHED_SPLIT", "0")        # 0: never
        assert read_cached_path(*shapes(BC, 8), 1 << 20) is True
        set_knob("AGN_READ_CACHED_SPLIT", "100")
        assert read_cached_path(*shapes(BC, 8), 99) is True
        assert read_cached_path(*shapes(BC, 8), 100) is False
        set_knob("AGN_READ_CACHED_SPLIT", None)
        # a masked log (oc_mask) over the dense-clock cache: the same path
        for D in (8, 16, 64):
            c, log = shapes(BC, D)
            log.oc_mask = FAKE
            assert read_cached_path(c, log, 100) is True, D
            assert read_cached_path(c, log, SPLIT) is False, D
        c, log = shapes(BC, 65)
        log.oc_mask = FAKE
        assert read_cached_path(c, log, 100) is False
        # the existing refusals
        for kw in (dict(arena=False), dict(mask=True)):
            with pytest.raises(EngineError) as e:
                read_cached_path(*shapes(BC, 8, **kw), 100)
            assert e.value.code == _abi.ENOTSUP
        # AGN_LWW_FUSED does not touch the type
        set_knob("AGN_LWW_FUSED", "0")
        assert read_cached_path(*shapes(BC, 8), 100) is True
        set_knob("AGN_LWW_FUSED", None)
        # the other types keep their answers with the knob on
        _others_unchanged()
        set_knob("AGN_BCOUNTER_FUSED", None)
        _others_unchanged()
    finally:
        set_knob("AGN_BCOUNTER_FUSED", None)
        set_knob("AGN_LWW_FUSED", None)
        set_knob("AGN_READ_CACHED_SPLIT", None)


def test_script_entries():
    """The scripts' entries: every slot, first appearing out of ascending
    order; amounts of 0 and of both signs; the invalid tag where asked."""
    ents = [bc.script_entry(t) for t in range(60)]
    assert {e[0] for e in ents} == set(bc.SCRIPT_SLOTS)
    first = []
    for t, _v in ents:
        if t not in first:
            first.append(t)
    assert first != sorted(first)
    assert any(v == 0 for _t, v in ents) and any(v >> 63 for _t, v in ents)
    assert bc.script_entry(3, True)[0] == _abi.TAG_INVALID
    import cache_edges as ce
    for D, sparse in ((3, False), (5, True)):
        sc = ce.scripts(D, sparse)
        for name in bc.SCRIPT_NAMES:
            steps = bc.bc_steps(sc[name])
            assert [st[0] for st in steps] == [st[0] for st in sc[name].steps]
            bad = [e for st in steps if st[0] == "append" for e in st[1]
                   if e[1][0] == _abi.TAG_INVALID]
            assert (len(bad) == 1) == (name == "invalid"), name


def _family(D, full, mask):
    return bc.masked_family(D, full) if mask else bc.family(D, full)


@pytest.mark.parametrize("D,full,mask", bc.FAMILIES, ids=bc.FAMILY_IDS)
def test_family_reaches_its_edges(oracle_lib, D, full, mask):
    fam = _family(D, full, mask)
    out = bc.chain(oracle_lib, fam)
    res, arrs = out["res"], out["arrs"]
    assert fam.K <= 64 and max(len(s["ops"]) for s in fam.specs) <= 304
    seen = dict(look=set(), store=set(), nafter=set(), flags=set(), base=set(), lens=set())
    unsorted_stored = 0
    for k, s in enumerate(fam.specs):
        nm, fl, st, inf = fam.names[k], int(res.flags[k]), int(out["status"][k]), out["info"][k]
        assert st == {"new": _abi.SS_NEW, "hit0": _abi.SS_HIT, "hit8": _abi.SS_HIT,
                      "log": _abi.SS_LOG}[s["look"]], nm
        if s["look"].startswith("hit"):
            assert int(out["first"][k]) == (1 if s["look"] == "hit0" else 0), nm
            # the planted base is what the fold starts from
            want_b = [(int(t), int(v) & bc.bm.M64) for t, v in (s["base"] or [])]
            assert out["bases"][k] == want_b, nm
            seen["base"].add(len(want_b))
        else:
            assert out["bases"][k] == [], nm
        seen["look"].add((s["look"], int(s["gc"])))
        if s["kind"] == "length":
            seen["lens"].add(len(s["ops"]))
        nb, na = int(out["n_before"][k]), int(arrs["n"][k])
        stored = out["handle"][k] != 0 and arrs["value"][k, 0] == out["handle"][k]
        if s["mistyped"] and s["ops"]:
            assert fl == _abi.F_ERR_CORRUPTED and not stored, nm
            seen["flags"].add("corrupted")
            continue
        if inf["err"]:
            assert fl & _abi.F_ERR_UNEXPECTED and not fl & _abi.F_ERR_CAPACITY and not stored, nm
            seen["flags"].add(("err", inf["err_at"], inf["overflow_then_err"]))
            continue
        if inf["invalid_excluded"]:
            seen["flags"].add("invalid excluded")
        if inf["overflow"]:
            assert fl & _abi.F_ERR_CAPACITY and int(res.out_n[k]) == 0 and not stored, nm
            seen["flags"].add(("overflow", bool(out["bases"][k])))
            continue
        if inf["no_room"]:
            assert fl & _abi.F_ERR_CAPACITY and int(res.out_n[k]) == inf["n_slots"] and not stored
            seen["flags"].add(("room", int(fam.cap_off[k + 1] - fam.cap_off[k])))
            continue
        if s["room"] is not None:
            assert int(fam.cap_off[k + 1] - fam.cap_off[k]) == inf["n_slots"], nm
            seen["flags"].add("room exact")
        seen["flags"].add(("slots", inf["n_slots"], bool(out["bases"][k])))
        for x in ("zero_sum", "wrapped", "dup_base"):
            if inf[x]:
                seen["flags"].add(x)
        if stored:
            seen["store"].add(("stored", int(s["gc"]), int(out["prune"][k])))
            state = out["states"][int(out["handle"][k])]
            tags = [t for t, _v in state]
            assert tags == sorted(tags) and len(set(tags)) == len(tags), nm
            table = bc.fold_order(s["ops"], out["bases"][k])
            assert sorted(table) == tags, nm
            unsorted_stored += table != tags
        seen["nafter"].add((nb, na))
        if s["name"] in ("count 4", "op-id gap 4", "hit 8 of 9", "LOG", "LOG, GC read"):
            assert not stored, nm
        if s["name"] in ("count 5", "op-id gap 5", "count 4, GC read", "list 8 -> 9",
                         "count 5 on an absent key"):
            assert stored, nm
        if s["name"] == "count 4 on an absent key":
            assert not stored and na == 1, nm
        if s["name"] == "list 8 -> 9":
            assert (nb, na) == (8, 9) and not out["prune"][k], nm
        if s["name"] in ("list 9 -> 10: collected", "list 9, GC read"):
            assert stored and (nb, na) == (9, bc.KEEP) and out["prune"][k] == 1, nm
        if s["name"] == "hit 8 of 9, GC read":
            assert out["prune"][k] == 1 and na <= bc.KEEP, nm
            assert bool(stored) == (D > 1), nm
    assert seen["look"] >= {(lk, g) for lk in ("new", "hit0", "log") for g in (0, 1)} | \
        {("hit8", 0), ("hit8", 1)}, seen["look"]
    assert seen["lens"] == set(bc.lengths(D))
    assert {("stored", 0, 0), ("stored", 1, 1), ("stored", 0, 1)} <= seen["store"], seen["store"]
    # a missing sort would show: some stored state's table order is not ascending
    assert unsorted_stored >= 3, unsorted_stored
    slots = {(x[1], x[2]) for x in seen["flags"] if isinstance(x, tuple) and x[0] == "slots"}
    assert {(1, False), (2, False), (64, False), (65, False), (256, False), (256, True)} <= slots
    assert {("overflow", False), ("overflow", True)} <= seen["flags"], seen["flags"]
    if full:
        assert {(255, False), (255, True), (4, True)} <= slots, slots
        assert {"zero_sum", "wrapped", "dup_base", "corrupted", "invalid excluded",
                "room exact", ("room", 0), ("room", 69), ("room", 1)} <= seen["flags"]
        errs = {x[1] for x in seen["flags"] if isinstance(x, tuple) and x[0] == "err"}
        assert {0, 63, 64, 129, 5, 300} <= errs, errs
        assert ("err", 300, True) in seen["flags"]
        assert seen["base"] >= {0, 1, 64, 65, 200}, seen["base"]


def test_masked_family_keeps_the_dense_outcomes(oracle_lib):
    """bc.masked: ops lack DCs (garbage above R in their place), and the chain
    agrees that nothing else changes."""
    D = 9
    fam, fm = bc.family(D, False), bc.masked_family(D, False)
    full = np.uint64((1 << D) - 1)
    lacking = fm.log.oc_mask[:, 0] != full
    assert lacking.sum() > fam.log.n_entries // 2
    assert (fm.log.oc[lacking] > np.uint64(1 << 60)).any(axis=1).all()
    a, b = bc.chain(oracle_lib, fam), bc.chain(oracle_lib, fm)
    for f in ("flags", "count", "hole", "out_n", "out_tag", "out_tok", "err_pos"):
        assert np.array_equal(getattr(a["res"], f), getattr(b["res"], f)), f
    # an absent DC does not enter LastOpCt (every op of the dense log names every DC)
    assert (b["res"].lastct <= a["res"].lastct).all()
    assert (b["res"].lastct < a["res"].lastct).any()
    assert np.array_equal(a["arrs"]["n"], b["arrs"]["n"])
    assert np.array_equal(a["prune"], b["prune"])
