"""antidote_crdt_counter_b without a GPU: the constants, descriptor validation,
agn_state_capacity, the host encoders, the known answers through the model and
through a literal update/2, the model's filter and per-slot sums against the C
oracle, and the reach of the cases tests/test_bcounter.py runs on the device."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import bcounter_model as bm
from antidote_amd import _abi
from antidote_amd import clocksi_materializer as cm
from antidote_amd import records
from antidote_amd._lib import load
from antidote_amd.encode import (ClocksiPayload, LogEncoder, ReadEncoder, alloc_result,
                                 bcounter_slot, log_struct, read_struct, result_struct,
                                 state_capacity)
from synth import random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BC = _abi.COUNTER_B
TYP = records.COUNTER_B
GPU_CASES = bm.gpu_cases()


@pytest.fixture(scope="module")
def lib():
    return load()


@functools.lru_cache(maxsize=None)
def case_model(idx):
    log, req, cap, sparse, D = bm.make_case(GPU_CASES[idx])
    want, incl, info = bm.model(log, req, sparse, cap)
    return log, req, cap, sparse, D, want, incl, info


def test_constants():
    hdr = open(os.path.join(ROOT, "include", "antidote_gpu.h")).read()
    assert re.search(r"#define AGN_COUNTER_B 6\b", hdr)
    assert re.search(r"#define AGN_BCOUNTER_SLOTS_MAX 256\b", hdr)
    assert re.search(r"#define AGN_ABI_VERSION 7\b", hdr)
    assert "5 is reserved" in hdr
    types = hdr[hdr.index("---- CRDT types"):hdr.index("#define AGN_TYPE_MIXED")]
    assert sorted(int(x) for x in re.findall(r"#define AGN_\w+ (\d+)\s", types)) == \
        [1, 2, 3, 4, 6, 256]
    assert _abi.COUNTER_B == 6 and _abi.BCOUNTER_SLOTS_MAX == 256 and _abi.ABI_VERSION == 7
    assert _abi.TYPE_NAMES[BC] == TYP == "antidote_crdt_counter_b"
    assert _abi.TYPE_IDS["antidote_crdt_counter_b"] == BC and 5 not in _abi.TYPE_NAMES
    assert cm.type_id(TYP) == BC
    assert cm.new(TYP) == ([], [])
    st = ([(("a", "a"), 3)], [("a", 1)])
    assert cm.value(TYP, st) == st
    nif = open(os.path.join(ROOT, "nif", "antidote_gpu_nif.erl")).read()
    assert re.search(r"-define\(COUNTER_B, 6\)", nif)
    assert re.search(r"type_id\(antidote_crdt_counter_b\) -> \?COUNTER_B", nif)
    # the per-call decode refuses a key past the slot limit (AGN_F_ERR_CAPACITY
    # = 0x10) before it would decode out_n = 0 as new()
    assert re.search(r"-define\(F_ERR_CAPACITY, 16#10\)", nif) and _abi.F_ERR_CAPACITY == 0x10
    clause = nif.index("F band ?F_ERR_CAPACITY =/= 0, TypeId =:= ?COUNTER_B -> {error, ecapacity};")
    dec = nif.index("decode(Type, TypeId, Dcs, D,")
    assert dec < clause < nif.index("?COUNTER_B -> decode_bcounter(")


def test_descriptors_validate_without_gpu(lib):
    """counter_b descriptors pass agn_* validation (checked before the device
    is touched: the NULL context is the only error), with and without rem_off;
    the missing arrays of the type are named; id 5 is still refused."""
    cases = [bm.bc_case(3, 5, lens=[0, 1, 8], base=0.5), bm.bc_case(4, 3, lens=[0, 0], base=1.0)]
    for log, req, cap in cases:
        res = alloc_result(req.n_req, log.n_dcs, sparse=True, cap_off=cap)
        for drop_rem in (False, True):
            ls, rs, os_ = log_struct(log), read_struct(req), result_struct(res)
            if drop_rem:
                ls.rem_off = ls.rem_tok = None
            assert lib.agn_materialize(None, C.byref(ls), C.byref(rs), C.byref(os_), None) == \
                _abi.EINVAL and lib.agn_last_error() == b"null context"
            assert lib.agn_materialize_host(None, C.byref(ls), C.byref(rs), C.byref(os_)) == \
                _abi.EINVAL and lib.agn_last_error() == b"null context"
    log, req, cap = cases[0]
    res = alloc_result(req.n_req, log.n_dcs, sparse=True, cap_off=cap)
    for name in ("tag", "add_tok"):
        ls, rs, os_ = log_struct(log), read_struct(req), result_struct(res)
        setattr(ls, name, None)
        assert lib.agn_materialize(None, C.byref(ls), C.byref(rs), C.byref(os_), None) == \
            _abi.EINVAL
        assert lib.agn_last_error() == b"counter_b log needs tag/add_tok"
    for name in ("out_off", "out_n", "out_tag", "out_tok"):
        ls, os_ = log_struct(log), result_struct(res)
        setattr(os_, name, None)
        assert lib.agn_materialize(None, C.byref(ls), C.byref(rs), C.byref(os_), None) == \
            _abi.EINVAL
        assert lib.agn_last_error() == b"counter_b result needs out_off/out_n/out_tag/out_tok"
    ls, os_ = log_struct(log), result_struct(res)
    ls.crdt_type = 5
    assert lib.agn_materialize(None, C.byref(ls), C.byref(rs), C.byref(os_), None) == _abi.EINVAL
    assert lib.agn_last_error() == b"unknown crdt_type 5"
    ls.crdt_type = 7
    assert lib.agn_materialize(None, C.byref(ls), C.byref(rs), C.byref(os_), None) == _abi.EINVAL
    assert lib.agn_last_error() == b"unknown crdt_type 7"


@pytest.mark.parametrize("segmented", [False, True], ids=["csr", "segmented"])
def test_prune_ops_needs_rem_off(lib, segmented):
    """agn_prune_ops takes a counter_b log as a tag-type log whose removal
    ranges are empty: tag, add_tok and rem_off are required, in both output
    forms, before the device is touched; id 5 is still unknown."""
    from test_prune import host_out_like, out_struct
    log, _req, _cap = bm.bc_case(17, 3, lens=[0, 3, 9], reps=2)
    thr = np.zeros((log.n_keys, 3), np.uint64)
    arrs = host_out_like(log)
    klen = np.zeros(log.n_keys, np.uint64)

    def call(drop_log=(), drop_out=(), crdt=BC):
        ls, os_ = log_struct(log), out_struct(log, arrs)
        ls.crdt_type = crdt
        if segmented:
            os_.key_len = klen.ctypes.data
        for name in drop_log:
            setattr(ls, name, None)
        for name in drop_out:
            setattr(os_, name, None)
        rc = lib.agn_prune_ops(None, C.byref(ls), None, thr.ctypes.data, None, C.byref(os_), None,
                               None, None)
        return rc, lib.agn_last_error()

    assert call() == (_abi.EINVAL, b"null context")
    for name in ("tag", "add_tok", "rem_off"):
        rc, msg = call(drop_log=(name,), drop_out=(name,))
        assert rc == _abi.EINVAL and b"needs" in msg and name.encode() in msg, (name, msg)
        rc, msg = call(drop_out=(name,))
        assert rc == _abi.EINVAL and msg == b"prune_ops: out lacks an array the log has"
    rc, msg = call(drop_log=("rem_off", "rem_tok"), drop_out=("rem_off", "rem_tok"))
    assert rc == _abi.EINVAL and b"rem_off" in msg
    assert call(crdt=5) == (_abi.EINVAL, b"prune_ops: unknown crdt_type 5")


def test_state_capacity(lib):
    """cap = the key's entries (whatever their amounts: 0 is a value) + the
    request's base pairs, through the CSR and through AGN_SS_STATE references."""
    log, req, cap = bm.bc_case(6, 4, lens=[0, 0, 0, 1, 2, 40], base=0.5, identity=False,
                               dup_base=True)
    assert (log.add_tok == 0).any()
    lens = np.diff(log.key_off.astype(np.int64))[req.keys.astype(np.int64)]
    nb = np.diff(req.base_off.astype(np.int64))
    assert np.array_equal(np.diff(cap.astype(np.int64)), lens + nb)
    assert (np.diff(cap.astype(np.int64)) == 0).any() and (nb[lens == 0] > 0).any()
    for r in (req, bm.as_state_refs(req)):
        got = np.zeros(req.n_req + 1, np.uint64)
        assert lib.agn_state_capacity(C.byref(log_struct(log)), C.byref(read_struct(r)),
                                      got.ctypes.data) == 0
        assert np.array_equal(got, cap)


def _payload(effect, t):
    return ClocksiPayload("k", TYP, effect, {"dc1": t - 1}, ("dc1", t), None)


def test_encoder_round_trip():
    """The three effect shapes: the orddict key interned into tag (P keys and D
    keys apart), the amount as two's complement in add_tok, no removals; any
    other effect, or an amount outside int64, is an invalid entry that keeps
    its term."""
    good = [(("increment", 10), "a"), (("decrement", 4), "a"), (("transfer", 5, "b"), "a"),
            (("increment", -(1 << 63)), "a"), (("decrement", (1 << 63) - 1), "b"),
            (("increment", 0), "b"), (("transfer", -1, "a"), "a")]
    bad = [(("increment", 1 << 63), "a"), (("decrement", -(1 << 63) - 1), "a"),
           (("increment", 1.5), "a"), (("increment", True), "a"), (("reset", 1), "a"),
           (("transfer", 1), "a"), (("increment", 1, 2, 3), "a"), "increment", 17,
           ("increment", 1, "a"), [("increment", 1), "a"], (("transfer", "x", "b"), "a")]
    enc = LogEncoder(BC, 1)
    k = enc.add_key([(i + 1, _payload(e, 10 + i)) for i, e in enumerate(good + bad)])
    log = enc.build()
    assert k == 0 and log.n_entries == len(good) + len(bad) and log.key_type[0] == BC
    assert np.array_equal(log.rem_off, np.zeros(log.n_entries + 1, np.uint32))
    slots = [("P", ("a", "a")), ("D", "a"), ("P", ("a", "b")), ("P", ("a", "a")), ("D", "b"),
             ("P", ("b", "b")), ("P", ("a", "a"))]
    for i, (e, s) in enumerate(zip(good, slots)):
        assert enc.tags.term(int(log.tag[i])) == s == bcounter_slot(e)[0]
        assert bm.i64(log.add_tok[i]) == e[0][1]
    assert log.tag[0] == log.tag[3] == log.tag[6] and log.tag[0] != log.tag[1]
    assert len({int(t) for t in log.tag[:len(good)]}) == 5
    for j, e in enumerate(bad):
        i = len(good) + j
        assert int(log.tag[i]) == _abi.TAG_INVALID and log.invalid_terms[i] == e
    st = ([(("a", "a"), 10), (("a", "b"), -2)], [("b", 1 << 62)])
    rd = ReadEncoder(enc)
    rd.add(0, {"dc1": 100}, base=cm._base_pairs(TYP, st))
    rd.add(0, {"dc1": 100}, base=cm._base_pairs(TYP, cm.new(TYP)))
    req = rd.build()
    assert list(req.base_off) == [0, 3, 3]
    assert [enc.tags.term(int(t)) for t in req.base_tag] == \
        [("P", ("a", "a")), ("P", ("a", "b")), ("D", "b")]
    assert [bm.i64(v) for v in req.base_tok] == [10, -2, 1 << 62]
    n = log.n_entries
    assert list(state_capacity(log, req)) == [0, n + 3, 2 * n + 3]
    # pairs -> {P, D}: the mirror's decode, each orddict in term order
    res = alloc_result(1, 1, sparse=True, cap_off=np.array([0, 4], np.uint64))
    tags = [enc.tags.id(("D", "b")), enc.tags.id(("P", ("b", "a"))), enc.tags.id(("P", ("a", "b"))),
            enc.tags.id(("D", "a"))]
    order = np.argsort(tags)
    res.out_n[0] = 4
    res.out_tag[:4] = np.array(tags, np.uint32)[order]
    res.out_tok[:4] = np.array([5, bm.M64, 7, 0], np.uint64)[order]
    assert cm._decode_state(TYP, enc, res, 0) == \
        ([(("a", "b"), 7), (("b", "a"), -1)], [("a", 0), ("b", 5)])


def _kat_through_model(ops, base=None):
    txid, R, resp = bm.kat_read(ops)
    enc = LogEncoder(BC, 1)
    k = enc.add_key(records.ops_oldest_first(resp.ops_list))
    rd = ReadEncoder(enc)
    rd.add(k, R, resp.snapshot_time, txid, cm._base_pairs(TYP, base or cm.new(TYP)))
    log, req = enc.build(), rd.build()
    res, _incl, _info = bm.model(log, req, True, state_capacity(log, req))
    assert not res.flags[0] & (_abi.F_ERR_UNEXPECTED | _abi.F_ERR_CAPACITY | _abi.F_ERR_CORRUPTED)
    assert int(res.count[0]) == len(ops)
    return cm._decode_state(TYP, enc, res, 0)


def _sequential(ops):
    st = ({}, {})
    for op in ops:
        st = bm.update(bm.kat_effect(op), st)
    return bm.as_orddicts(st)


@pytest.mark.parametrize("c", bm.kats()["cases"], ids=lambda c: c["name"])
def test_kats_through_model_and_update(c):
    """The suites' sequences: the model's state equals a literal sequential
    update/2, and permissions/1 is the pinned outcome -- for every size of the
    transfer the suites leave open."""
    variants = [c["ops"]]
    for v in c.get("transfer_range", []):
        ops = [list(o) for o in c["ops"]]
        ops[c["transfer_at"]][1] = v
        variants.append(ops)
    for ops in variants:
        got = _kat_through_model(ops)
        assert got == _sequential(ops)
        assert cm.permissions(got) == c["permissions"], ops
    if not c["ops"]:
        assert got == cm.new(TYP)


def test_kats_hold_the_issue_cases():
    k = bm.kats()
    by = {c["name"]: c["permissions"] for c in k["cases"]}
    assert by == {"new_bcounter_test": 0, "test_dec_success": 6, "test_dec_multi_success0": 5,
                  "test_dec_multi_success1": 5, "conditional_write_test_run": 7}
    for name in ("test_dec_multi_success0", "test_dec_multi_success1"):
        c = next(c for c in k["cases"] if c["name"] == name)
        assert c["ops"][c["transfer_at"]][:2] == ["transfer", 5]
        assert c["transfer_range"] == [5, 6, 7, 8, 9, 10]
    lp = k["local_permissions"]
    st = _kat_through_model(lp["ops"])
    assert lp["expect"] == {"dc1": 10, "dc2": 0}
    for ident, want in lp["expect"].items():
        assert cm.local_permissions(ident, st) == want
    # received less granted less decremented, own increments included
    st = _sequential([["increment", 10, "a"], ["transfer", 4, "b", "a"], ["decrement", 1, "a"],
                      ["transfer", 1, "a", "b"], ["decrement", 2, "b"]])
    assert cm.local_permissions("a", st) == 10 + 1 - 4 - 1
    assert cm.local_permissions("b", st) == 4 - 1 - 2
    assert cm.permissions(st) == 10 - 3


def _oracle_counter(oracle_lib, log, req, sparse, eff):
    """oracle_materialize on the same rows typed as a counter_pn log."""
    D, n = log.n_dcs, req.n_req
    ls, rs = log_struct(log), read_struct(req, sparse=sparse)
    eff = np.ascontiguousarray(eff, np.int64)
    kt = np.where(log.key_type == BC, _abi.COUNTER_PN, log.key_type).astype(np.uint8)
    ls.crdt_type, rs.req_type = _abi.COUNTER_PN, _abi.COUNTER_PN
    ls.eff, ls.key_type = eff.ctypes.data, kt.ctypes.data
    ls.tag = ls.add_tok = ls.rem_off = ls.rem_tok = None
    rs.base_value = rs.base_off = rs.base_tag = rs.base_tok = None
    if log.oc_mask is None:
        ls.oc_mask = None
    want = alloc_result(n, D, sparse=sparse)
    assert oracle_lib.oracle_materialize(C.byref(ls), C.byref(rs), C.byref(result_struct(want)),
                                         1) == 0
    return want


def _filter_fields_vs_oracle(oracle_lib, log, req, sparse, got, incl):
    """The model's hole, count, lastct (+ mask), NEWSS, CT_IGNORE and CORRUPTED
    against the oracle with unit effects."""
    D, n = log.n_dcs, req.n_req
    want = _oracle_counter(oracle_lib, log, req, sparse, np.ones(max(log.n_entries, 1), np.int64))
    keep = _abi.F_NEWSS | _abi.F_CT_IGNORE | _abi.F_ERR_CORRUPTED
    for i in range(n):
        fw = int(want.flags[i])
        assert int(got.flags[i]) & keep == fw & keep, i
        if fw & _abi.F_ERR_CORRUPTED:
            assert incl[i] is None
            continue
        assert int(got.hole[i]) == int(want.hole[i]), i
        assert int(got.count[i]) == int(want.count[i]) == int(incl[i].sum()), i
        assert int(want.value[i]) == int(want.count[i]), i
        if fw & _abi.F_CT_IGNORE:
            continue
        if sparse:
            assert np.array_equal(got.lastct_mask[i], want.lastct_mask[i]), i
            m = bm._bits(want.lastct_mask[i], D)
            assert np.array_equal(got.lastct[i][m], want.lastct[i][m]), i
        else:
            assert np.array_equal(got.lastct[i], want.lastct[i]), i


def _slot_sums_vs_oracle(oracle_lib, log, req, sparse, cap, got, max_slots=6):
    """For each slot, the model's sum less its base equals the oracle's counter
    value on the log with eff = amount where the tag matches, else 0.  (The
    oracle reserves INT64_MIN as an effect: such amounts are left to the
    literal fold of test_model_fold_is_sequential_update.)"""
    tags = [int(t) for t in np.unique(log.tag) if int(t) != _abi.TAG_INVALID][:max_slots]
    amt = log.add_tok.astype(np.int64)
    checked = 0
    for t in tags:
        eff = np.where(log.tag == t, amt, 0)
        if (eff == -(1 << 63)).any():
            continue
        want = _oracle_counter(oracle_lib, log, req, sparse, eff if len(eff) else np.zeros(1))
        for i in range(req.n_req):
            f = int(got.flags[i])
            if f & (_abi.F_ERR_CORRUPTED | _abi.F_ERR_UNEXPECTED | _abi.F_ERR_CAPACITY):
                continue
            o, n = int(cap[i]), int(got.out_n[i])
            st = dict(zip(got.out_tag[o:o + n].tolist(), got.out_tok[o:o + n].tolist()))
            o0, o1 = int(req.base_off[i]), int(req.base_off[i + 1])
            b = sum(int(v) for x, v in zip(req.base_tag[o0:o1], req.base_tok[o0:o1]) if int(x) == t)
            assert (st.get(t, 0) - b) & bm.M64 == int(want.value[i]) & bm.M64, (t, i)
            checked += 1
    return checked


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("D", [1, 5, 9, 70])
def test_model_matches_oracle(oracle_lib, D, sparse):
    """synth.random_case's counter_pn clocks (warm reads, reading txids,
    mismatched key types, permuted keys), given counter_b entries."""
    log, req, _ = random_case(40 + D, _abi.COUNTER_PN, 40, D, 30, sparse=sparse, warm=0.5,
                              txid=0.4, corrupt=0.05, identity=False)
    log.key_type = np.where(log.key_type == _abi.COUNTER_PN, BC, log.key_type).astype(np.uint8)
    log, req, cap = bm.attach_bc(log, req, D, invalid=0.1, base=0.4, dup_base=True)
    got, incl, _info = bm.model(log, req, sparse, cap)
    _filter_fields_vs_oracle(oracle_lib, log, req, sparse, got, incl)
    assert _slot_sums_vs_oracle(oracle_lib, log, req, sparse, cap, got) > 40
    assert (got.count > 0).any() and (got.flags & _abi.F_CT_IGNORE).any()


@pytest.mark.parametrize("idx", range(len(GPU_CASES)), ids=[c[0] for c in GPU_CASES])
def test_gpu_cases_match_oracle(oracle_lib, idx):
    """The very batches tests/test_bcounter.py runs on the device: the model's
    filter fields and (for a few slots of each) its sums against the C oracle."""
    log, req, cap, sparse, _D, got, incl, _info = case_model(idx)
    _filter_fields_vs_oracle(oracle_lib, log, req, sparse, got, incl)
    _slot_sums_vs_oracle(oracle_lib, log, req, sparse, cap, got, max_slots=3)


def test_model_fold_is_sequential_update():
    """The model's fold against a literal sequential update/2 over the included
    entries, on the value-domain batch (0, -1, INT64_MIN, wrapping sums)."""
    idx = [c[0] for c in GPU_CASES].index("D4-domain")
    log, req, cap, _sparse, _D, got, incl, _info = case_model(idx)
    n_ok = 0
    for i in range(req.n_req):
        if int(got.flags[i]) & (_abi.F_ERR_CORRUPTED | _abi.F_ERR_UNEXPECTED | _abi.F_ERR_CAPACITY):
            continue
        k = int(req.keys[i])
        a = int(log.key_off[k])
        st = ({}, {})
        for x in range(int(req.base_off[i]), int(req.base_off[i + 1])):
            st = bm.update((("increment", bm.i64(req.base_tok[x])), int(req.base_tag[x])), st)
        for p in np.nonzero(incl[i])[0]:
            st = bm.update((("increment", bm.i64(log.add_tok[a + p])), int(log.tag[a + p])), st)
        o, n = int(cap[i]), int(got.out_n[i])
        want = sorted((t, v & bm.M64) for (t, _), v in st[0].items())
        assert list(zip(got.out_tag[o:o + n].tolist(), got.out_tok[o:o + n].tolist())) == want, i
        n_ok += 1
    assert n_ok > 10


def test_gpu_cases_reach():
    """Every case class the device test names occurs in its batches."""
    hit = dict(corrupt=0, err=0, invalid_excluded=0, overflow=0, overflow_then_err=0, no_room=0,
               base_only=0, log_only=0, both=0, excluded_only=0, zero_sum=0, wrapped=0,
               dup_base=0, empty=0)
    err_at, slots, chunk_slots, lens, ds, amounts = set(), set(), set(), set(), set(), set()
    room0 = short1 = 0
    n_reqs, tot = set(), 0
    warm = cold = txr = masked = permuted = repeated = 0
    for idx, case in enumerate(GPU_CASES):
        log, req, cap, sparse, D, want, _incl, info = case_model(idx)
        assert bm.has_bases(case) == (len(req.base_tag) > 0), case[0]
        ds.add(D)
        n_reqs.add(req.n_req)
        tot += req.n_req
        lens |= set(np.diff(log.key_off.astype(np.int64)).tolist())
        masked += bool(sparse)
        keys = req.keys.astype(np.int64)
        permuted += bool(len(keys) > 1 and not np.array_equal(keys, np.arange(len(keys))))
        repeated += bool(len(set(keys.tolist())) < len(keys))
        warm += int((req.sct_ignore == 0).sum())
        cold += int((req.sct_ignore == 1).sum())
        txr += int((req.txid != 0).sum())
        room = np.diff(cap.astype(np.int64))
        for i, x in enumerate(info):
            for name in hit:
                hit[name] += bool(x[name])
            if x["err"]:
                err_at.add((x["err_at"], x["n"]))
            if not (x["corrupt"] or x["err"]):
                slots.add(x["n_slots"])
                chunk_slots.add(x["chunk_slots"])
                amounts |= x["amounts"]
            if x["no_room"]:
                room0 += room[i] == 0
                short1 += room[i] == x["n_slots"] - 1
    assert ds >= set(bm.DS) and lens >= {0, 1, 63, 64, 65, 128, 129}
    assert 1 in n_reqs and 5 in n_reqs and any(n % 4 == 0 for n in n_reqs)
    assert masked and permuted and repeated and warm * 20 >= tot and cold * 20 >= tot and txr > 0
    for name, n in hit.items():
        assert n > 0, name
    assert slots >= {0, 1, 2, 64, 65, 255, 256, 257} and chunk_slots >= {1, 2, 64}
    assert {p for p, _n in err_at} >= {0, 63, 64} and any(p == n - 1 for p, n in err_at)
    assert amounts >= {0, bm.M64, bm.I64_MIN}
    assert room0 > 0 and short1 > 0
    # 255 / 256 / 257 with and without base pairs making up the count
    idx = [c[0] for c in GPU_CASES].index("D8-slots")
    log, req, _cap, _sp, _D, want, _incl, info = case_model(idx)
    nb = np.diff(req.base_off.astype(np.int64))
    for total in (255, 256, 257):
        rows = [i for i, x in enumerate(info) if x["n_slots"] == total]
        assert any(nb[i] == 0 for i in rows) and any(nb[i] > 0 for i in rows), total
        for i in rows:
            assert bool(want.flags[i] & _abi.F_ERR_CAPACITY) == (total == 257)
            assert int(want.out_n[i]) == (0 if total == 257 else total)


def test_host_generator(lib):
    """agn_gen_host accepts the type: tag uniform in [0, n_elems), small signed
    amounts with 0 among them, empty removal ranges."""
    from antidote_amd.engine import free_gen_host, gen_host, host_view
    K, N, D, E = 50, 40, 3, 5
    cfg = _abi.AgnGenCfg(crdt_type=BC, n_dcs=D, n_keys=K, ops_per_key=N, n_elems=E, seed=77,
                         key_base=0, key_stride=1)
    log, req = gen_host(cfg)
    try:
        tag = host_view(log.tag, np.uint32, K * N).copy()
        amt = host_view(log.add_tok, np.uint64, K * N).copy().astype(np.int64)
        rem = host_view(log.rem_off, np.uint32, K * N + 1).copy()
        assert log.crdt_type == BC and log.n_entries == K * N and not log.eff
        assert req.req_type == BC
    finally:
        free_gen_host(log, req)
    assert set(tag.tolist()) == set(range(E)) and not rem.any()
    assert amt.min() >= -1000 and amt.max() <= 1000 and (amt < 0).any() and (amt > 0).any()
