"""antidote_crdt_register_lww without a GPU: the constants, descriptor
validation, agn_state_capacity, the host encoders, the known answers through
the model, the model's filter against the C oracle, and the reach of the cases
tests/test_lww.py runs on the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lww_model as lm
from antidote_amd import _abi
from antidote_amd import clocksi_materializer as cm
from antidote_amd import records
from antidote_amd._lib import load
from antidote_amd.encode import (ClocksiPayload, LogEncoder, ReadEncoder, alloc_result,
                                 log_struct, read_struct, result_struct, state_capacity,
                                 term_key)
from synth import random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LWW = _abi.REGISTER_LWW


@pytest.fixture(scope="module")
def lib():
    return load()


def test_constants():
    hdr = open(os.path.join(ROOT, "include", "antidote_gpu.h")).read()
    assert re.search(r"#define AGN_REGISTER_LWW 4\b", hdr)
    assert re.search(r"#define AGN_F_TS_TIE 0x40u", hdr)
    assert re.search(r"#define AGN_ABI_VERSION 7\b", hdr)
    assert _abi.REGISTER_LWW == 4 and _abi.F_TS_TIE == 0x40 and _abi.ABI_VERSION == 7
    assert _abi.TYPE_NAMES[LWW] == records.REGISTER_LWW == "antidote_crdt_register_lww"
    assert _abi.TYPE_IDS["antidote_crdt_register_lww"] == LWW
    assert cm.type_id(records.REGISTER_LWW) == LWW
    assert cm.new(records.REGISTER_LWW) == (0, b"")
    assert cm.value(records.REGISTER_LWW, (5, b"v")) == b"v"


def test_descriptors_validate_without_gpu(lib):
    """register_lww descriptors pass agn_* validation (checked before the
    device is touched: the NULL context is the only error), with and without
    rem_off; the missing arrays of the type are named."""
    cases = [lm.lww_case(3, 5, lens=[0, 1, 8], base=0.5),
             lm.lww_case(4, 3, lens=[0, 0], base=1.0)]
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
    ls, rs, os_ = log_struct(log), read_struct(req), result_struct(res)
    ls.add_tok = None
    assert lib.agn_materialize(None, C.byref(ls), C.byref(rs), C.byref(os_), None) == _abi.EINVAL
    assert b"tag/add_tok" in lib.agn_last_error()
    ls, os_ = log_struct(log), result_struct(res)
    os_.out_n = None
    assert lib.agn_materialize(None, C.byref(ls), C.byref(rs), C.byref(os_), None) == _abi.EINVAL
    assert b"out_off/out_n/out_tag/out_tok" in lib.agn_last_error()
    ls.crdt_type = 5
    assert lib.agn_materialize(None, C.byref(ls), C.byref(rs), C.byref(os_), None) == _abi.EINVAL
    assert lib.agn_last_error() == b"unknown crdt_type 5"


def test_state_capacity(lib):
    """One pair where the key has an entry or the request a base pair, through
    the CSR and through AGN_SS_STATE references; two base pairs are refused."""
    log, req, cap = lm.lww_case(6, 4, lens=[0, 0, 0, 1, 2, 40], base=0.5, identity=False)
    lens = np.diff(log.key_off.astype(np.int64))[req.keys.astype(np.int64)]
    nb = np.diff(req.base_off.astype(np.int64))
    assert np.array_equal(np.diff(cap.astype(np.int64)), ((lens > 0) | (nb > 0)).astype(np.int64))
    assert (np.diff(cap.astype(np.int64)) == 0).any() and (nb[lens == 0] > 0).any()
    for r in (req, lm.as_state_refs(req)):
        got = np.zeros(req.n_req + 1, np.uint64)
        assert lib.agn_state_capacity(C.byref(log_struct(log)), C.byref(read_struct(r)),
                                      got.ctypes.data) == 0
        assert np.array_equal(got, cap)
    req.base_off = np.arange(req.n_req + 1, dtype=np.uint64) * np.uint64(2)
    req.base_tag = np.zeros(2 * req.n_req, np.uint32)
    req.base_tok = np.ones(2 * req.n_req, np.uint64)
    got = np.zeros(req.n_req + 1, np.uint64)
    assert lib.agn_state_capacity(C.byref(log_struct(log)), C.byref(read_struct(req)),
                                  got.ctypes.data) == _abi.EINVAL
    with pytest.raises(ValueError):
        state_capacity(log, req)
    res = alloc_result(req.n_req, log.n_dcs, sparse=True, cap_off=cap)
    assert lib.agn_materialize_host(None, C.byref(log_struct(log)), C.byref(read_struct(req)),
                                    C.byref(result_struct(res))) == _abi.EINVAL
    assert b"more than one base pair" in lib.agn_last_error()


def _payload(effect, t):
    return ClocksiPayload("k", records.REGISTER_LWW, effect, {"dc1": t - 1}, ("dc1", t), None)


def test_encoder_round_trip():
    """{Ts, V}: the value interned into tag, the timestamp raw in add_tok, no
    removals; an effect that is not {integer Ts, V} with 1 <= Ts < 2^64 is an
    invalid entry that keeps its term."""
    good = [(1, b"a"), ((1 << 64) - 1, b"b"), (1 << 32, ("tuple", 1)), (7, b"a")]
    bad = [(0, b"zero"), (1 << 64, b"big"), (-1, b"neg"), (1.5, b"f"), (True, b"bool"),
           "atom", 17, (1, b"a", b"b"), [3, b"list"], ("ts", b"v")]
    enc = LogEncoder(LWW, 1)
    k = enc.add_key([(i + 1, _payload(e, 10 + i)) for i, e in enumerate(good + bad)])
    log = enc.build()
    assert k == 0 and log.n_entries == len(good) + len(bad) and log.key_type[0] == LWW
    assert np.array_equal(log.rem_off, np.zeros(log.n_entries + 1, np.uint32))
    for i, (ts, v) in enumerate(good):
        assert int(log.add_tok[i]) == ts and enc.tags.term(int(log.tag[i])) == v
    assert log.tag[0] == log.tag[3]
    for j, e in enumerate(bad):
        i = len(good) + j
        assert int(log.tag[i]) == _abi.TAG_INVALID and log.invalid_terms[i] == e
    rd = ReadEncoder(enc)
    rd.add(0, {"dc1": 100}, base=[(b"b", 1 << 63)])
    rd.add(0, {"dc1": 100}, base=[])
    req = rd.build()
    assert list(req.base_off) == [0, 1, 1]
    assert enc.tags.term(int(req.base_tag[0])) == b"b" and int(req.base_tok[0]) == 1 << 63
    assert list(state_capacity(log, req)) == [0, 1, 2]
    # the host mirror's state <-> pair mapping
    assert cm._base_pairs(records.REGISTER_LWW, (0, b"")) == []
    assert cm._base_pairs(records.REGISTER_LWW, (9, b"x")) == [(b"x", 9)]


def test_term_order_of_values():
    terms = [b"b", 3, "atom", (1, 2), b"a", [1], 2.5, (1,), b"ab", b""]
    assert sorted(terms, key=term_key) == [2.5, 3, "atom", (1,), (1, 2), [1], b"", b"a", b"ab", b"b"]


def _kat_through_model(c):
    txid, R, resp, want = lm.kat_read(c)
    enc = LogEncoder(LWW, 1)
    for v in cm._lww_values([(txid, R, resp)]):   # term order: the tag tie break is update/2's
        enc.tags.id(v)
    k = enc.add_key(records.ops_oldest_first(resp.ops_list))
    rd = ReadEncoder(enc)
    rd.add(k, R, resp.snapshot_time, txid,
           cm._base_pairs(records.REGISTER_LWW, resp.materialized_snapshot.value))
    log, req = enc.build(), rd.build()
    res, _incl, _info = lm.model(log, req, True, state_capacity(log, req))
    return cm._decode_state(records.REGISTER_LWW, enc, res, 0), res, want


@pytest.mark.parametrize("c", lm.kats(), ids=lambda c: c["name"])
def test_kats_through_model(c):
    got, res, want = _kat_through_model(c)
    assert got == want and cm.value(records.REGISTER_LWW, got) == lm._val(c["value"])
    assert int(res.count[0]) == c["count"] and int(res.hole[0]) == c["hole"]
    assert bool(res.flags[0] & _abi.F_TS_TIE) == (c["name"] == "equal_ts_larger_value_wins")
    assert not res.flags[0] & (_abi.F_ERR_UNEXPECTED | _abi.F_ERR_CAPACITY | _abi.F_ERR_CORRUPTED)


def test_kats_hold_the_issue_cases():
    names = {c["name"] for c in lm.kats()}
    assert {"pb_assign_then_read", "two_assigns_rising_ts", "two_assigns_falling_ts",
            "equal_ts_larger_value_wins", "snapshot_excludes_newest_assign",
            "warm_read_base_wins"} <= names
    held = [c for c in lm.kats() if c["origin"].startswith("reference")]
    assert [c["name"] for c in held] == ["pb_assign_then_read"]


def _filter_fields_vs_oracle(oracle_lib, log, req, sparse):
    """The model's hole, count, lastct (+ mask), NEWSS, CT_IGNORE and CORRUPTED
    against oracle_materialize on the same log recast as counter_pn, eff = 1."""
    D, n = log.n_dcs, req.n_req
    cap = state_capacity(log, req)
    got, incl, _info = lm.model(log, req, sparse, cap)
    ls, rs = log_struct(log), read_struct(req, sparse=sparse)
    eff = np.ones(max(log.n_entries, 1), np.int64)
    kt = np.where(log.key_type == LWW, _abi.COUNTER_PN, log.key_type).astype(np.uint8)
    ls.crdt_type, rs.req_type = _abi.COUNTER_PN, _abi.COUNTER_PN
    ls.eff, ls.key_type = eff.ctypes.data, kt.ctypes.data
    ls.tag = ls.add_tok = ls.rem_off = ls.rem_tok = None
    rs.base_value = rs.base_off = rs.base_tag = rs.base_tok = None
    if log.oc_mask is None:
        ls.oc_mask = None
    want = alloc_result(n, D, sparse=sparse)
    assert oracle_lib.oracle_materialize(C.byref(ls), C.byref(rs), C.byref(result_struct(want)),
                                         1) == 0
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
            m = lm._bits(want.lastct_mask[i], D)
            assert np.array_equal(got.lastct[i][m], want.lastct[i][m]), i
        else:
            assert np.array_equal(got.lastct[i], want.lastct[i]), i
    return got


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("D", [1, 5, 9, 70])
def test_model_filter_matches_oracle(oracle_lib, D, sparse):
    """synth.random_case's counter_pn clocks (warm reads, reading txids,
    mismatched key types, permuted keys), given register_lww entries."""
    log, req, _ = random_case(40 + D, _abi.COUNTER_PN, 40, D, 30, sparse=sparse, warm=0.5,
                              txid=0.4, corrupt=0.05, identity=False)
    log, req, _cap = lm.attach_lww(log, req, D, invalid=0.1, base=0.4)
    got = _filter_fields_vs_oracle(oracle_lib, log, req, sparse)
    assert (got.count > 0).any() and (got.flags & _abi.F_CT_IGNORE).any()


GPU_CASES = lm.gpu_cases()


@pytest.mark.parametrize("case", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_gpu_cases_filter_matches_oracle(oracle_lib, case):
    """The very batches tests/test_lww.py runs on the device: the model's
    filter fields against the C oracle."""
    _id, seed, D, sparse, kw = case
    log, req, _cap = lm.lww_case(seed, D, reps=lm.GPU_REPS, **kw)
    _filter_fields_vs_oracle(oracle_lib, log, req, sparse)


def test_gpu_cases_reach():
    """Over the device test's batches, each class the kernel can get wrong
    holds at least one request in twenty; every key length of the issue and
    every D is there."""
    tot = 0
    hit = dict(base_wins=0, last_chunk=0, tie=0, max_excluded=0, err=0, empty=0, corrupt=0,
               invalid_excluded=0)
    warm = cold = txr = 0
    for _id, seed, D, sparse, kw in GPU_CASES:
        log, req, cap = lm.lww_case(seed, D, reps=lm.GPU_REPS, **kw)
        lens = set(np.diff(log.key_off.astype(np.int64)).tolist())
        assert lens >= {0, 1, 63, 64, 65, 129} and (D != 256 or lens >= {2, 3})
        res, _incl, info = lm.model(log, req, sparse, cap)
        tot += req.n_req
        for x in info:
            for name in hit:
                hit[name] += bool(x[name])
        warm += int((req.sct_ignore == 0).sum())
        cold += int((req.sct_ignore == 1).sum())
        txr += int((req.txid != 0).sum())
    assert {c[2] for c in GPU_CASES} >= set(lm.DS)
    for name in ("base_wins", "last_chunk", "tie", "max_excluded", "err", "empty"):
        assert hit[name] * 20 >= tot, (name, hit[name], tot)
    assert hit["corrupt"] > 0 and hit["invalid_excluded"] > 0 and warm * 20 >= tot and cold * 20 >= tot and txr * 20 >= tot


def test_capacity_and_first_base_pair_in_model():
    """Room 0 with one live pair: AGN_F_ERR_CAPACITY and out_n = 1."""
    log, req, cap = lm.lww_case(9, 2, lens=[0, 3, 3, 3], reps=2, base=0.5)
    room0 = cap.copy()
    room0[1:] = 0
    res, _incl, info = lm.model(log, req, False, room0)
    live = np.array([not (x["empty"] or x["err"] or x["corrupt"]) for x in info])
    assert live.any() and not live.all()
    assert ((res.flags & _abi.F_ERR_CAPACITY) != 0).tolist() == live.tolist()
    assert res.out_n.tolist() == live.astype(int).tolist()


def test_host_generator(lib):
    """agn_gen_host accepts the type: tag uniform in [0, n_elems), add_tok the
    op's commit time plus a small jitter, empty removal ranges, the clocks
    those of the other types' generator at the same seed (its own draws come
    after the op's clock draws)."""
    from antidote_amd.engine import free_gen_host, gen_host, host_view
    K, N, D, E = 50, 20, 3, 5
    out = {}
    for crdt in (LWW, _abi.COUNTER_PN):
        cfg = _abi.AgnGenCfg(crdt_type=crdt, n_dcs=D, n_keys=K, ops_per_key=N, n_elems=E, seed=77,
                             key_base=0, key_stride=1)
        log, req = gen_host(cfg)
        try:
            out[crdt] = dict(oc=host_view(log.oc, np.uint64, K * N * D).reshape(K * N, D).copy(),
                             n=log.n_entries, crdt=log.crdt_type)
            if crdt == LWW:
                out["tag"] = host_view(log.tag, np.uint32, K * N).copy()
                out["ts"] = host_view(log.add_tok, np.uint64, K * N).copy()
                out["rem_off"] = host_view(log.rem_off, np.uint32, K * N + 1).copy()
                assert not log.eff and req.req_type == LWW
        finally:
            free_gen_host(log, req)
    assert out[LWW]["crdt"] == LWW and out[LWW]["n"] == K * N
    assert set(out["tag"].tolist()) == set(range(E))
    assert not out["rem_off"].any()
    # the commit DC's entry of the op's row is its commit time
    d = out["ts"].astype(np.int64)[:, None] - out[LWW]["oc"].astype(np.int64)
    ok = (d >= 0) & (d <= 15)
    assert ok.any(axis=1).all()
    assert len(set(np.where(ok, d, -1).max(axis=1).tolist())) > 8
    # the first op of every key draws the same clocks under either type
    first = np.arange(K) * N
    assert np.array_equal(out[LWW]["oc"][first], out[_abi.COUNTER_PN]["oc"][first])


@pytest.mark.parametrize("segmented", [False, True], ids=["csr", "segmented"])
@pytest.mark.parametrize("crdt", [_abi.COUNTER_PN, _abi.SET_AW, _abi.REGISTER_MV, LWW])
def test_prune_ops_needs_the_types_arrays(lib, crdt, segmented):
    """agn_prune_ops checks, before the device is touched (so the NULL context
    is a complete log's only error), that a log with entries carries its
    type's arrays and `out` the same; the CSR form and the one-pass segmented
    form (out.key_len) accept exactly the same inputs.  A register_lww log
    without rem_off, fine for agn_materialize, is refused here: the segmented
    kernel would take it for a counter log and read eff."""
    from test_prune import host_out_like, out_struct
    log, _req, _ = random_case(17 + crdt, crdt, 6, 3, 9, empty=0.2)
    assert log.n_entries > 0
    thr = np.zeros((log.n_keys, 3), np.uint64)
    arrs = host_out_like(log)
    klen = np.zeros(log.n_keys, np.uint64)
    needs = ("eff",) if crdt == _abi.COUNTER_PN else ("tag", "add_tok", "rem_off")

    def call(drop_log=(), drop_out=()):
        ls, os_ = log_struct(log), out_struct(log, arrs)
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
    for name in needs:
        rc, msg = call(drop_log=(name,), drop_out=(name,))
        assert rc == _abi.EINVAL and b"needs" in msg and name.encode() in msg, (name, msg)
        rc, msg = call(drop_log=(name,))
        assert rc == _abi.EINVAL and b"needs" in msg, (name, msg)
        rc, msg = call(drop_out=(name,))
        assert rc == _abi.EINVAL and msg == b"prune_ops: out lacks an array the log has", (name, msg)
    if crdt == LWW:   # what agn_materialize accepts for the type
        rc, msg = call(drop_log=("rem_off", "rem_tok"), drop_out=("rem_off", "rem_tok"))
        assert rc == _abi.EINVAL and b"rem_off" in msg
    # an empty log has no arrays to miss
    ls, os_ = log_struct(log), out_struct(log, arrs)
    ls.n_entries = 0
    for name in needs:
        setattr(ls, name, None)
    assert lib.agn_prune_ops(None, C.byref(ls), None, thr.ctypes.data, None, C.byref(os_), None,
                             None, None) == _abi.EINVAL and lib.agn_last_error() == b"null context"
    ls = log_struct(log)
    ls.crdt_type = 5
    assert lib.agn_prune_ops(None, C.byref(ls), None, thr.ctypes.data, None, C.byref(os_), None,
                             None, None) == _abi.EINVAL
    assert lib.agn_last_error() == b"prune_ops: unknown crdt_type 5"
