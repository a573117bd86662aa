"""antidote_crdt_register_lww in the two oracles, without a GPU.

oracle/oracle.c folds the included ops one after another (State =
max(Effect, State)); oracle/py_oracle.py applies update/2 to {Ts, Value}
terms; tests/lww_model.py takes the maximum over a candidate set.  The three
are written in three forms and must agree on the same logs: the batches
tests/test_lww.py runs on the device, fresh random ones at the widths where
the kernel shape changes, the domain-edge ones, and what synth.random_case
draws for the cross-type suites.  Plus: the known answers through both
oracles, the py oracle's term order against the encoder's, and the C oracle's
refusals (a type it has no fold for, a state of two pairs)."""
import ctypes as C

import numpy as np
import pytest

import lww_model as lm
import test_oracle_crosscheck as cc
from antidote_amd import _abi
from antidote_amd import clocksi_materializer as cm
from antidote_amd import records
from antidote_amd.encode import (LogEncoder, ReadEncoder, alloc_result, log_struct, read_struct,
                                 result_struct, state_capacity, term_key)
from oracle import py_oracle as po
from synth import random_case

LWW = _abi.REGISTER_LWW


def c_oracle(oracle_lib, log, req, sparse, cap, threads=2):
    res = alloc_result(req.n_req, log.n_dcs, sparse=True, cap_off=cap)
    res.err_pos[:] = lm.NO_POS
    ls, rs, os_ = log_struct(log), read_struct(req, sparse=sparse), result_struct(res)
    if log.oc_mask is None:
        ls.oc_mask = None
    ls.rem_off = ls.rem_tok = None      # the branch may not read them
    assert oracle_lib.oracle_materialize(C.byref(ls), C.byref(rs), C.byref(os_), threads) == 0
    return res


def three_way(oracle_lib, log, req, sparse, cap):
    """C oracle == model on every result field (AGN_F_TS_TIE included), and
    C oracle == py oracle on materialize/4's tuple."""
    D, n = log.n_dcs, req.n_req
    got = c_oracle(oracle_lib, log, req, sparse, cap)
    want, _incl, info = lm.model(log, req, sparse, cap)
    assert lm.compare_lww(D, got, want, sparse, n) == []
    live = [i for i in range(n) if not int(want.flags[i]) &
            (_abi.F_ERR_CORRUPTED | _abi.F_ERR_UNEXPECTED)]
    assert got.out_n[live].tolist() == want.out_n[live].tolist()
    cc.SPARSE[0] = sparse
    for i in range(n):
        py = cc.py_run(log, req, i)
        c = cc.c_decode(log, req, got, i, True)
        if py[0] == "error":
            k = int(req.keys[i])
            assert c[0] == "error" and py[1][1] == ("invalid",), (i, py, c)
            # apply_operations stops at the oldest included invalid entry
            assert int(log.key_off[k]) <= c[1] < int(log.key_off[k + 1])
            assert int(log.tag[c[1]]) == _abi.TAG_INVALID
            continue
        if sparse is False and c[0] == "ok" and c[3] != po.IGNORE:
            py = py[:3] + ({d: py[3].get(d, 0) for d in range(D)},) + py[4:]
        assert c == py, (i, c, py)
    return got, info


GPU_CASES = lm.gpu_cases()


@pytest.mark.parametrize("case", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_three_way_on_the_device_batches(oracle_lib, case):
    _id, seed, D, sparse, kw = case
    log, req, cap = lm.lww_case(seed, D, reps=lm.GPU_REPS, **kw)
    three_way(oracle_lib, log, req, sparse, cap)


@pytest.mark.parametrize("domain", [False, True], ids=["small", "domain"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "masked"])
@pytest.mark.parametrize("D", [1, 8, 33, 129])
def test_three_way_fresh(oracle_lib, D, sparse, domain):
    """Bases, warm requests, reading txids, invalid tags, mismatched key types
    and permuted requests; domain: timestamps and tags from TS_EDGE / TAG_EDGE."""
    lens = [0, 1, 2, 3, 7, 20, 40]
    log, req, cap = lm.lww_case(500 + 2 * D + sparse, D, lens=lens, reps=8, sparse=sparse, warm=0.5,
                                txid=0.4, corrupt=0.05, identity=False, invalid=0.2, base=0.5,
                                domain=domain)
    got, info = three_way(oracle_lib, log, req, sparse, cap)
    for name in ("base_wins", "tie", "err", "empty", "max_excluded"):
        assert any(x[name] for x in info), name
    assert (got.flags & _abi.F_TS_TIE).any()
    if domain:   # every edge of either domain wins somewhere or is at least carried
        assert set(log.add_tok.tolist()) == set(lm.TS_EDGE)
        assert set(log.tag.tolist()) - {_abi.TAG_INVALID} == set(lm.TAG_EDGE)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "masked"])
@pytest.mark.parametrize("D", [1, 8, 33, 129])
def test_three_way_random_case(oracle_lib, D, sparse):
    """synth.random_case's register_lww logs, as the cross-type suites draw
    them: half the keys at the domain edges, half with common ties."""
    log, req, cap = random_case(4000 + 10 * D + sparse, LWW, 40, D, 20, sparse=sparse, warm=0.4,
                                txid=0.3, invalid=0.05, corrupt=0.05, base=0.5, identity=False)
    assert not log.rem_off.any() and int(np.diff(req.base_off.astype(np.int64)).max()) == 1
    got, info = three_way(oracle_lib, log, req, sparse, cap)
    # random_case's read clocks include next to nothing at wide D (that is
    # test_three_way_fresh's part): ties are asked for where ops are included
    assert any(x["base_wins"] for x in info) and (D > 8 or any(x["tie"] for x in info))
    assert set(log.add_tok.tolist()) >= set(lm.TS_EDGE)


def test_capacity_keeps_the_tie_flag(oracle_lib):
    """No room: AGN_F_ERR_CAPACITY with out_n = 1 where a state exists, the
    tie flag as with room, nothing written."""
    log, req, cap = lm.lww_case(9, 2, lens=[0, 3, 3, 3, 12], reps=3, base=0.5)
    room0 = np.zeros_like(cap)
    roomy = c_oracle(oracle_lib, log, req, False, cap)
    got = c_oracle(oracle_lib, log, req, False, room0)
    want, _incl, _info = lm.model(log, req, False, room0)
    assert lm.compare_lww(2, got, want, False, req.n_req) == []
    capf = (got.flags & _abi.F_ERR_CAPACITY) != 0
    assert capf.any() and not capf.all()
    assert np.array_equal(got.flags & ~np.uint32(_abi.F_ERR_CAPACITY), roomy.flags)
    assert (got.flags[capf] & _abi.F_TS_TIE).any()
    assert np.array_equal(got.out_n, roomy.out_n) and set(got.out_n[capf].tolist()) == {1}


def _kat_encoded(c):
    txid, R, resp, want = lm.kat_read(c)
    enc = LogEncoder(LWW, 1)
    for v in cm._lww_values([(txid, R, resp)]):   # term order: the tag tie break is update/2's
        enc.tags.id(v)
    k = enc.add_key(records.ops_oldest_first(resp.ops_list))
    rd = ReadEncoder(enc)
    rd.add(k, R, resp.snapshot_time, txid,
           cm._base_pairs(records.REGISTER_LWW, resp.materialized_snapshot.value))
    return enc, enc.build(), rd.build(), want


@pytest.mark.parametrize("c", lm.kats(), ids=lambda c: c["name"])
def test_kats_through_both_oracles(oracle_lib, c):
    enc, log, req, want = _kat_encoded(c)
    res = c_oracle(oracle_lib, log, req, True, state_capacity(log, req), threads=1)
    assert cm._decode_state(records.REGISTER_LWW, enc, res, 0) == want
    assert int(res.count[0]) == c["count"] and int(res.hole[0]) == c["hole"]
    assert bool(res.flags[0] & _abi.F_TS_TIE) == (c["name"] == "equal_ts_larger_value_wins")
    assert not res.flags[0] & (_abi.F_ERR_UNEXPECTED | _abi.F_ERR_CAPACITY | _abi.F_ERR_CORRUPTED)
    txid, R, resp, want = lm.kat_read(c)
    r = po.materialize(po.REGISTER_LWW, txid, R, resp)
    assert r[0] == "ok" and r[1] == want and r[2] == c["hole"] and r[5] == c["count"]
    assert po.crdt_value(po.REGISTER_LWW, r[1]) == lm._val(c["value"])


def test_py_oracle_type():
    assert po.REGISTER_LWW == records.REGISTER_LWW
    assert po.crdt_new(po.REGISTER_LWW) == (0, b"") == cm.new(records.REGISTER_LWW)
    assert po.crdt_value(po.REGISTER_LWW, (5, b"v")) == b"v"
    up = lambda e, s: po.crdt_update(po.REGISTER_LWW, e, s)  # noqa: E731
    assert up((1, b"a"), (0, b"")) == (1, b"a")
    assert up((1, b"a"), (2, b"")) == (2, b"")
    assert up((7, b"a"), (7, b"b")) == (7, b"b") == up((7, b"b"), (7, b"a"))
    assert up((7, 3), (7, b"")) == (7, b"")          # number < binary
    assert up(((1 << 64) - 1, b"x"), (1 << 63, b"y")) == ((1 << 64) - 1, b"x")
    # what the encoder stores as an invalid entry raises, so update_snapshot
    # answers the error tuple (Ts = 0 is the encoder's own deviation: update/2
    # accepts it and the ABI carries it)
    bad = [(1 << 64, b"big"), (-1, b"neg"), (1.5, b"f"), (True, b"bool"), "atom", 17,
           (1, b"a", b"b"), [3, b"list"], ("ts", b"v"), ("invalid",)]
    for e in bad:
        assert po.update_snapshot(po.REGISTER_LWW, (3, b"s"), e) == \
            ("error", ("unexpected_operation", e, po.REGISTER_LWW)), e
    enc = LogEncoder(LWW, 1)
    pay = [(i + 1, records.ClocksiPayload("k", records.REGISTER_LWW, e, {"dc1": 9 + i},
                                          ("dc1", 10 + i), None)) for i, e in enumerate(bad)]
    enc.add_key(pay)
    assert (enc.build().tag == _abi.TAG_INVALID).all()
    assert po.materialize_eager(po.REGISTER_LWW, (0, b""), [(2, b"b"), (1, b"z")]) == (2, b"b")


def test_py_term_order_agrees_with_the_encoder():
    rng = np.random.default_rng(5)
    terms = [0, 1, -1, 255, 256, (1 << 64) - 1, -(1 << 70), b"", b"\x00", b"a", b"ab", b"b",
             b"\xff", b"a\x00"]
    terms += [int(x) for x in rng.integers(-1000, 1000, 20)]
    terms += [bytes(rng.integers(0, 256, int(n)).astype(np.uint8)) for n in rng.integers(0, 5, 20)]
    rng.shuffle(terms)
    assert sorted(terms, key=po._lww_term_key) == sorted(terms, key=term_key)
    for a in terms:   # pairwise, as update/2 compares {Ts, Value}
        for b in terms:
            want = (7, a) if term_key(a) > term_key(b) else (7, b)
            assert po.crdt_update(po.REGISTER_LWW, (7, a), (7, b)) == want


def test_c_oracle_refusals(oracle_lib):
    """A type the oracle has no fold for, as log type or as read type, and a
    register_lww state of two pairs: non-zero, instead of another type's fold."""
    log, req, cap = lm.lww_case(3, 2, lens=[0, 2, 5], reps=1, base=1.0)
    res = alloc_result(req.n_req, 2, sparse=True, cap_off=cap)

    def run(crdt=LWW, rtype=LWW, r=req):
        ls, rs, os_ = log_struct(log), read_struct(r), result_struct(res)
        ls.crdt_type, rs.req_type = crdt, rtype
        return oracle_lib.oracle_materialize(C.byref(ls), C.byref(rs), C.byref(os_), 1)

    assert run() == 0
    for bad in (0, 5, 0xFF):
        assert run(crdt=bad) != 0 and run(rtype=bad) != 0
    assert run(rtype=_abi.REGISTER_MV) == 0   # a known other type: corrupted_ops_cache per key
    assert (res.flags[np.diff(log.key_off.astype(np.int64))[req.keys.astype(np.int64)] > 0]
            == _abi.F_ERR_CORRUPTED).all()
    two = np.arange(req.n_req + 1, dtype=np.uint64)
    two[-1] += 1                                  # the last request: two base pairs
    req2 = lm.as_state_refs(req)                  # a copy of the request's arrays
    req2.base_value = np.zeros(req.n_req, np.int64)
    req2.base_off = two
    req2.base_tag = np.zeros(int(two[-1]), np.uint32)
    req2.base_tok = np.ones(int(two[-1]), np.uint64)
    assert run(r=req2) != 0


# ------------------------------------------------------------------ generators
def digest(*objs):
    """sha256 over every array (dtype, shape, bytes) of encoded logs / reads
    and plain arrays, in field order."""
    import hashlib
    h = hashlib.sha256()

    def feed(x):
        if x is None:
            h.update(b"N")
        elif isinstance(x, np.ndarray):
            h.update(str((x.dtype.str, x.shape)).encode())
            h.update(np.ascontiguousarray(x).tobytes())
        elif isinstance(x, (list, tuple)):
            for y in x:
                feed(y)
        elif hasattr(x, "__dataclass_fields__"):
            for f in x.__dataclass_fields__:
                h.update(f.encode())
                feed(getattr(x, f))
        else:
            h.update(repr(x).encode())
    feed(objs)
    return h.hexdigest()[:16]


# taken with the generators as they were before register_lww entered them
PARENT_DIGESTS = {
    "family_a-1": "022499ea9cc9ccf2", "family_a-2": "e82a210063b556c2",
    "family_a-3": "e511f8fab23c4806", "family_e-1": "a607ea2799c99940",
    "family_e-2": "2a81cec70bf1865e", "family_e-3": "97d229ab1396d8c3",
    "random-1-dense": "e0e853a5679bed7b", "random-1-masked": "a3f78dfcad6e72f9",
    "random-2-dense": "ce5ba95870b68662", "random-2-masked": "1abe7ea19b39e84c",
    "random-3-dense": "b2fe7e648b78eec3", "random-3-masked": "1e31ec85b1bf3653",
    "remap-1": "353b65f1fa5de1a9", "remap-2": "d884c606a29ff5e6", "remap-3": "3cfe540cc24a1003",
    "thresholds-1": "2bedc0159e148280", "thresholds-2": "745ee4eb5b2aa12b",
    "thresholds-3": "c714614f5a12d4e9"}


def test_other_types_generated_data_unchanged():
    """synth.random_case, the edges builders, domain.remap_payload and
    test_prune.thresholds give the three earlier types bit for bit what they
    gave before they learnt register_lww."""
    import domain
    import edges
    from test_prune import thresholds
    out = {}
    for crdt in (1, 2, 3):
        out[f"random-{crdt}-dense"] = digest(random_case(11 + crdt, crdt, 64, 8, 40, warm=0.3,
                                                         base=0.3))
        out[f"random-{crdt}-masked"] = digest(random_case(
            1000 * crdt + 171, crdt, 40, 17, 12, sparse=True, warm=0.4, txid=0.3, invalid=0.03,
            corrupt=0.05, multi=0.2 if crdt == 2 else 0.0, base=0.5, identity=False))
        out[f"family_e-{crdt}"] = digest(edges.family_e(crdt, 5, crdt == 3))
        out[f"family_a-{crdt}"] = digest(edges.family_a(crdt, 3, "mixed" if crdt == 2 else None,
                                                        lengths=(0, 1, 17, 65)))
        log, req, _ = random_case(5 + crdt, crdt, 20, 4, 30, base=0.4, txid=0.3)
        out[f"remap-{crdt}"] = digest(domain.remap_payload(log, req, "top", seed=3)[:2])
    for crdt, D, sp in ((1, 8, True), (2, 5, False), (3, 64, True)):
        log, _, _ = random_case(31 * D + crdt + sp, crdt, 30, D, 40, sparse=sp)
        out[f"thresholds-{crdt}"] = digest(thresholds(D + crdt, log, sp))
    assert out == PARENT_DIGESTS


def test_remap_payload_keeps_the_lww_result(oracle_lib):
    """domain.remap_payload's rank-preserving maps on a register_lww case:
    timestamps (add_tok / base_tok) and tags keep their order, so the result
    is the original's under the same maps."""
    import domain
    log, req, cap = random_case(77, LWW, 40, 4, 30, warm=0.3, txid=0.3, base=0.5, invalid=0.03)
    base = c_oracle(oracle_lib, log, req, False, cap)
    for mode in domain.MONOTONE_PAYLOAD:
        log2, req2, pm = domain.remap_payload(log, req, mode, seed=1)
        assert not log2.rem_off.any()
        got = c_oracle(oracle_lib, log2, req2, False, cap)
        want = domain.unmap_result(base, log, req, pm=pm, sparse=False)
        assert lm.compare_lww(4, got, want, False, req.n_req) == []
        assert (got.out_n == 1).any() and (got.flags & _abi.F_TS_TIE).any()


# ------------------------------------------------------------------ reach of the device rows
BIG_TS = set(lm.TS_EDGE) - {1}   # 0, 2^32 - 1 .. 2^64 - 1: no small-range key draws them


def gc_reach(oracle_lib, log, prune, thr, tm):
    """What a register_lww GC log must hold for its device row to mean
    something: the suites' own reach checks, every removal range empty, and
    kept entries at edge timestamps, a non-empty all-pruned key and a key of
    cut inside, longer than one 64-entry iteration (where the row's keys are
    at most 64 long: than the ops per iteration of the width's filter shape)."""
    from test_prune import oracle_prune
    arrs, flags, n_out = oracle_prune(oracle_lib, log, prune, thr, tm)
    assert log.crdt_type == LWW and not log.rem_off.any() and not arrs["rem_off"].any()
    assert flags.any() and (flags == 0).any()
    assert 0 < n_out < log.n_entries
    lens = np.diff(log.key_off.astype(np.int64))
    kept = np.diff(arrs["key_off"].astype(np.int64))
    step = 64 if lens.max() > 64 else lm.opi(log.n_dcs)
    hit = dict(edge_ts_kept=len(BIG_TS & set(arrs["add_tok"][:n_out].tolist())),
               all_pruned=int(((kept == 0) & (lens > 0) & (prune != 0)).sum()),
               long_key_cut=int(((lens > step) & (kept > 0) & (kept < lens)).sum()),
               untouched=int(((prune == 0) & (lens > 0)).sum()))
    assert all(hit.values()), hit
    # the staged 64-bit field carries both halves' edges out again
    assert {0, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1} <= \
        set(arrs["add_tok"][:n_out].tolist())
    return arrs, n_out


PRUNE_ROWS = [(LWW, 8, False), (LWW, 5, True), (LWW, 129, True)]


@pytest.mark.parametrize("crdt,D,sparse", PRUNE_ROWS)
@pytest.mark.parametrize("form", ["csr", "segmented"])
def test_reach_of_the_prune_rows(oracle_lib, form, crdt, D, sparse):
    """tests/test_prune.py's device rows (the seeds of test_prune_gpu_vs_oracle
    and of test_prune_segmented_gpu_vs_oracle)."""
    import test_prune as tp
    assert set(PRUNE_ROWS) <= set(tp.CASES)
    a, b, tx = (77, 3, 0.0) if form == "csr" else (91, 5, 0.3)
    log, _req, _ = random_case(a * D + crdt + sparse, crdt, 200, D, 150 if D <= 16 else 60,
                               sparse=sparse, multi=0.0, empty=0.1, txid=tx)
    prune, thr, tm = tp.thresholds(D * b + crdt, log, sparse)
    gc_reach(oracle_lib, log, prune, thr, tm)


def fold_reach(log, req, sparse):
    """A register_lww read batch for the device: a tie at the winning
    timestamp, a base pair that wins, a winner at an edge timestamp."""
    cap = state_capacity(log, req)
    res, _incl, info = lm.model(log, req, sparse, cap)
    hit = dict(tie=sum(x["tie"] for x in info), base_wins=sum(x["base_wins"] for x in info),
               edge_winner=sum(int(res.out_n[i]) == 1 and int(res.out_tok[int(cap[i])]) in BIG_TS
                               for i in range(req.n_req)
                               if not int(res.flags[i]) & (_abi.F_ERR_UNEXPECTED |
                                                           _abi.F_ERR_CORRUPTED)))
    return hit


def test_reach_of_the_oplog_rows(oracle_lib):
    """tests/test_oplog.py: the register_lww rows of CASES -- the log that is
    appended and pruned under every anchor, and the reads of the pruned log."""
    import test_oplog as to
    import test_prune as tp
    rows = [c for c in to.CASES if c[0] == LWW]
    assert [(D, sp) for _c, D, sp, _i in rows] == [(8, False), (13, True)]
    for crdt, D, sparse, init in rows:
        log, req, _ = random_case(9 * D + crdt + init, crdt, 60, D, 90, sparse=sparse, multi=0.0,
                                  empty=0.1)
        prune, thr, tm = tp.thresholds(D + crdt + 5, log, sparse)
        arrs, n_out = gc_reach(oracle_lib, log, prune, thr, tm)
        pruned = to.pruned_log(arrs, n_out, crdt, D, log.n_keys, sparse)
        hit = fold_reach(pruned, req, sparse)
        assert hit["tie"] and hit["edge_winner"], hit


def test_reach_of_the_edges_row(oracle_lib):
    """tests/test_edges.py GC_LOGS["lww8"] = edges.family_e(register_lww, 8)."""
    import edges
    log, prune, thr, tm, names = edges.family_e(LWW, 8)
    gc_reach(oracle_lib, log, prune, thr, tm)
    lens = np.diff(log.key_off.astype(np.int64))
    assert {0, 1, 63, 64, 65, 129, 257} <= set(lens.tolist())
    assert any("none kept" in n for n in names) and any("segment at 31" in n for n in names)


def test_reach_of_the_batcher_rows():
    """tests/test_batcher.py CASES: the reads the batcher coalesces."""
    import test_batcher as tb
    rows = [c for c in tb.CASES if c[0] == LWW]
    assert [(D, sp) for _c, D, sp in rows] == [(8, False), (6, True)]
    for crdt, D, sparse in rows:
        log, req, _ = random_case(17 * D + crdt, crdt, 300, D, 40, sparse=sparse, warm=0.4,
                                  txid=0.2, base=0.3, multi=0.0)
        hit = fold_reach(log, req, sparse)
        assert all(hit.values()), hit


def test_reach_of_the_load_rows(oracle_lib):
    """tests/test_oplog_load.py: the register_lww log every load test shares
    (constructed key lengths, edge timestamps in the copied 64-bit field), and
    the prunes of its VIEW_CASES / behaves-like-twin rows."""
    import test_oplog as to
    import test_oplog_load as tl
    import test_prune as tp
    assert LWW in tl.TYPES and (LWW, 8, False) in tl.VIEW_CASES
    for D, sparse, salt, more_seed in ((8, False, 3, None), (16, True, 9, 77)):
        log, _ = tl.case(LWW, D, sparse)
        assert np.diff(log.key_off.astype(np.int64)).tolist() == tl.LENGTHS
        assert set(log.add_tok.tolist()) >= BIG_TS and not log.rem_off.any()
        if more_seed is not None:
            more, _req, _ = random_case(more_seed + D + LWW, LWW, log.n_keys, D, 30, sparse=sparse,
                                        warm=0.3, txid=0.2, multi=0.0, empty=0.3)
            log = to.concat(log, more)
        prune, thr, tm = tp.thresholds(D + LWW + salt, log, sparse)
        arrs, _flags, n_out = tp.oracle_prune(oracle_lib, log, prune, thr, tm)
        assert 0 < n_out < log.n_entries
        assert len(BIG_TS & set(arrs["add_tok"][:n_out].tolist())) >= 5


def test_reach_of_the_state_workloads():
    """test_ss_states.TagWorkload / test_typed_partition.MixedWorkload for the
    type: even keys carry every edge timestamp an encoder accepts, odd keys
    repeat timestamps under different values (ties at the top timestamp)."""
    import test_ss_states as ts
    import test_typed_partition as ty
    for mk in (lambda: ts.TagWorkload(31 + LWW + 21, 16, LWW, 3),
               lambda: ty.MixedWorkload(101, 12, 4)):
        w = mk()
        seen = {}
        for s in range(1200):
            key = s % 8
            eff = w.op(key, LWW)[4] if isinstance(w, ty.MixedWorkload) else w.op(key)[4]
            assert po.crdt_update(po.REGISTER_LWW, eff, (0, b"")) == eff
            seen.setdefault(key, []).append(eff)
        for key, effs in seen.items():
            top = max(t for t, _v in effs)
            if key % 2 == 0:
                assert {t for t, _v in effs} == set(ts.LWW_TS_EDGE)
            else:
                assert top <= 8 and len({v for t, v in effs if t == top}) > 1
