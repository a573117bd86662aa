"""Every kernel over the full 64-bit value domain (include/antidote_gpu.h,
"Value domain").

The other parity tests draw clocks around 10^6, effects within +-1000 and
tokens, tags, ids and txids from small ranges, so a compare, max, shuffle or
readlane that drops or mixes up the upper 32 bits, a signed compare at 2^63, a
lost carry in the counter sum or an id sign-extended into `hole` would pass
them.  Here the same random cases are moved across those boundaries
(tests/domain.py: clocks per key by a strictly increasing map, payload values
by rank) and every kernel family runs them bit-exact against the C oracle
re-run on the remapped case.  tests/test_value_domain_cpu.py pins the remaps
and the oracle at these values without a GPU.
"""
import copy

import numpy as np
import pytest

import domain as dm
from antidote_amd import _abi
from antidote_amd.encode import state_capacity
from antidote_amd.engine import Batcher, OpLog
from synth import compare, random_case
from test_gpu_parity import COUNTER_IMPLS, _set_impl
from test_presence import IMPLS, presence_case

pytestmark = pytest.mark.gpu

TYPES3 = (_abi.COUNTER_PN, _abi.SET_AW, _abi.REGISTER_MV)
# `mixed` clocks (the mode by k % 5), with each single mode in turn: a family
# of ten or more cases runs all of them
CLOCKS = ("mixed", "carry32", "mixed", "sign64", "mixed", "hi32", "mixed", "top", "mixed", "zero")
PAYLOADS = tuple(dm.PAYLOAD_MODES)


def modes(i):
    return CLOCKS[i % len(CLOCKS)], PAYLOADS[i % len(PAYLOADS)]


def free(*ds):
    for d in ds:
        for b in (d.bufs.values() if hasattr(d, "bufs") else [d]):
            if b is not None:
                b.free()


def check(eng, oracle_lib, log, req, sparse, path, index=False, hints=0):
    """agn_materialize (host arrays, or device arrays with upload / fetch)
    against the oracle on the same case."""
    crdt, D = log.crdt_type, log.n_dcs
    cap = state_capacity(log, req) if crdt != _abi.COUNTER_PN else None
    want = dm.run_oracle(oracle_lib, log, req, cap, sparse=sparse)
    if path == "host":
        got = eng.materialize_host(log, req, sparse=sparse, cap_off=cap)
    else:
        dl, dr = eng.upload_log(log), eng.upload_read(req, sparse=sparse)
        dr.struct.hints = hints
        if index:
            eng.index_masks(dl)
        dres = eng.alloc_result(req.n_req, D, sparse=sparse, cap_off=cap)
        eng.materialize(dl, dr, dres)
        eng.sync()
        got = eng.fetch_result(dres)
        free(dl, dr, dres)
    bad = compare(crdt, D, got, want, sparse, req.n_req)
    assert not bad, bad[:10]
    return want


def wide(i, log, req, sparse=None, clock=None, payload=None):
    c, p = modes(i)
    log, req, _, _ = dm.remap_clocks(log, req, clock or c, sparse=sparse)
    log, req, _ = dm.remap_payload(log, req, payload or p, seed=i)
    return log, req


# ---------------------------------------------------------------- counter kernels
COUNTER = [(impl, D) for impl in COUNTER_IMPLS for D in (1, 3, 4, 8)]


@pytest.mark.parametrize("i,impl,D", [(i, *c) for i, c in enumerate(COUNTER)])
def test_counter_variants(eng, oracle_lib, monkeypatch, i, impl, D):
    """auto / glds / quad / quad2 / general, dense."""
    _set_impl(monkeypatch, impl)
    log, req, _ = dm.std_case(600 + i, _abi.COUNTER_PN, D, False)
    log, req = wide(i, log, req)
    check(eng, oracle_lib, log, req, False, "host" if i % 3 else "device")


MASKED = [(impl, path) for impl in ("split", "split_two", "split_cold", "split_mixed",
                                    "split_ctflag")
          for path in ("device_indexed", "device_no_index")]


@pytest.mark.parametrize("i,impl,path", [(i, *c) for i, c in enumerate(MASKED)])
def test_counter_masked_forms(eng, oracle_lib, monkeypatch, i, impl, path):
    """The masked D = 8 forms (test_presence's knobs), on a presence_case
    remapped after it is built: the present values move, the garbage in the
    absent columns stays."""
    monkeypatch.delenv("AGN_COUNTER_GLDS", raising=False)
    monkeypatch.delenv("AGN_COUNTER_IMPL", raising=False)
    monkeypatch.setenv("AGN_COUNTER_VARIANT", IMPLS[impl])
    monkeypatch.setenv("AGN_COUNTER_EARLY", "1")
    monkeypatch.setenv("AGN_Q8E_KM", "0")
    if impl == "split_cold":
        monkeypatch.delenv("AGN_Q8E_TWO", raising=False)
    else:
        monkeypatch.setenv("AGN_Q8E_TWO", "1" if impl == "split_two" else "0")
    log, req = presence_case(8000 + i, 130, 8, 150, txid=0.3, invalid=0.02, corrupt=0.03)
    before = log.oc.copy()
    log, req = wide(i, log, req, sparse=True)
    absent = ~dm.present_bits(log.oc_mask, log.n_entries, 8)
    assert np.array_equal(log.oc[absent], before[absent]) and absent.any()
    if impl == "split_cold":   # no SCT: the cold kernels
        req.sct = req.sct_mask = req.sct_ignore = None
    check(eng, oracle_lib, log, req, True, "device", index=(path == "device_indexed"),
          hints={"split_ctflag": _abi.HINT_CT_FLAG, "split_mixed": _abi.HINT_MIXED}.get(impl, 0))


GENERAL = [(D, sparse) for D in (12, 17, 64, 100, 256) for sparse in (False, True)]


@pytest.mark.parametrize("i,D,sparse", [(i, *c) for i, c in enumerate(GENERAL)])
def test_counter_general_wide_clocks(eng, oracle_lib, monkeypatch, i, D, sparse):
    _set_impl(monkeypatch, "general")
    log, req, _ = dm.std_case(700 + i, _abi.COUNTER_PN, D, sparse)
    log, req = wide(i, log, req)
    check(eng, oracle_lib, log, req, sparse, "host" if i % 3 else "device")


# ---------------------------------------------------------------- tag kernels
TAGS = [(crdt, D, sparse, None) for crdt in TYPES3[1:] for D in (3, 8) for sparse in (False, True)]
TAGS += [(crdt, D, False, dpl8) for crdt in TYPES3[1:] for D in (12, 16, 40, 64, 128)
         for dpl8 in ("0", "1")]
TAGS += [(crdt, D, True, None) for crdt in TYPES3[1:] for D in (16, 64)]


@pytest.mark.parametrize("i,crdt,D,sparse,dpl8", [(i, *c) for i, c in enumerate(TAGS)])
def test_tag_kernels(eng, oracle_lib, monkeypatch, i, crdt, D, sparse, dpl8):
    """set_aw / register_mv: D = 3, 8 sparse and dense, the dense
    contiguous-row shapes with and without AGN_TAGS_DPL8, the sparse forms at
    D = 16, 64."""
    if dpl8 == "1":
        monkeypatch.setenv("AGN_TAGS_DPL8", "1")
    else:
        monkeypatch.delenv("AGN_TAGS_DPL8", raising=False)
    log, req, _ = dm.std_case(800 + i, crdt, D, sparse)
    log, req = wide(i, log, req)
    check(eng, oracle_lib, log, req, sparse, "host" if i % 3 else "device")


@pytest.mark.parametrize("i,crdt", list(enumerate(TYPES3)))
def test_long_keys(eng, oracle_lib, i, crdt):
    """Keys far longer than a wave: 24 keys of up to 1500 ops, D = 8."""
    log, req, _ = random_case(99 + crdt, crdt, 24, 8, 1500, warm=0.3, base=0.3, n_elems=40,
                              empty=0.0)
    log, req = wide(2 * i, log, req)   # mixed clocks
    check(eng, oracle_lib, log, req, False, "device" if i == 1 else "host")


@pytest.mark.parametrize("crdt", TYPES3[1:])
def test_large_live_state_next_to_the_pad(eng, oracle_lib, crdt):
    """Live state beyond the fast table with `top` tokens (the last one is
    2^64 - 1) and `hi` tags (up to 0xFFFFFFFE): the bitonic pad (tag
    0xffffffff, tok ~0) meets real pairs next to it."""
    from test_value_domain_cpu import slow_path_case
    log, req = slow_path_case(crdt, 8)
    want = check(eng, oracle_lib, log, req, False, "host")
    assert int(want.out_n.max()) > 256  # the slow path really ran


# ---------------------------------------------------------------- agn_tune
def test_tune_top_clocks(eng, oracle_lib, monkeypatch):
    """agn_tune on a D = 8 counter batch whose clocks end at 2^64 - 2: the
    results it leaves and the later agn_materialize both equal the oracle's."""
    for k in ("AGN_COUNTER_GLDS", "AGN_COUNTER_VARIANT", "AGN_COUNTER_IMPL"):
        monkeypatch.delenv(k, raising=False)
    log, req, _ = dm.std_case(4243, _abi.COUNTER_PN, 8, False)
    log, req = wide(1, log, req, clock="top")
    want = dm.run_oracle(oracle_lib, log, req)
    dl, dr = eng.upload_log(log), eng.upload_read(req, sparse=False)
    res = eng.alloc_result(req.n_req, 8, sparse=False)
    choice, ms = eng.tune(dl, dr, res, rounds=2)
    assert choice in (0, 1, 2)
    bad = compare(_abi.COUNTER_PN, 8, eng.fetch_result(res), want, False, req.n_req)
    assert not bad, bad[:10]
    res2 = eng.alloc_result(req.n_req, 8, sparse=False)
    eng.materialize(dl, dr, res2)
    eng.sync()
    bad = compare(_abi.COUNTER_PN, 8, eng.fetch_result(res2), want, False, req.n_req)
    assert not bad, bad[:10]
    free(dl, dr, res, res2)


# ---------------------------------------------------------------- engine-owned log
@pytest.mark.parametrize("i,crdt,D,sparse", [(0, _abi.COUNTER_PN, 8, False),
                                             (1, _abi.SET_AW, 5, True),
                                             (2, _abi.REGISTER_MV, 8, False)])
def test_oplog_append_read_top_ids(eng, oracle_lib, monkeypatch, i, crdt, D, sparse):
    """The remapped entries appended to an agn_oplog whose per-key counters
    (agn_oplog_set_counter) make each key's newest op id 0xFFFFFFFE, so `hole`
    and the consecutive-id index see bit 31; read through agn_materialize over
    the flushed view, through agn_oplog_read and through a cached batcher
    (the fused read, AGN_READ6 = 1, and the batched kernels, 0)."""
    from test_batcher import gather
    from test_oplog import (append_ops, check_id_index, interleave, materialize_view, ops_of,
                            renumbered)
    rng = np.random.default_rng(50 + i)
    log, req, _ = dm.std_case(900 + i, crdt, D, sparse, K=80, nmax=70, corrupt=0.0, invalid=0.0)
    log, req, _, _ = dm.remap_clocks(log, req, "mixed")
    log, req, _ = dm.remap_payload(log, req, dict(dm.PAYLOAD_MODES[PAYLOADS[i]], ids=None), seed=i)
    ops = ops_of(log)
    n_ops = np.bincount([k for k, _, _ in ops], minlength=log.n_keys)
    with OpLog(eng, crdt, D, log.n_keys, sparse=sparse, init_slots=i) as ol:
        ol.set_counter(np.arange(log.n_keys), (0xFFFFFFFE - n_ops).astype(np.uint32))
        got = append_ops(ol, log, interleave(rng, ops), rng)
        log2 = renumbered(log, got)
        for k in range(log.n_keys):
            a, b = int(log.key_off[k]), int(log.key_off[k + 1])
            assert b == a or int(log2.op_id[b - 1]) == 0xFFFFFFFE
        view = ol.flush()
        check_id_index(eng, view, log.n_keys)
        assert not materialize_view(eng, oracle_lib, view, log2, req, sparse)
        cap = state_capacity(log2, req)
        want = dm.run_oracle(oracle_lib, log2, req, cap, sparse=sparse)
        assert int(want.hole.max()) >= 1 << 31
        dreq = eng.upload_read(req, sparse=sparse)
        dres = eng.alloc_result(req.n_req, D, sparse, cap_off=cap)
        ol.read(dreq, dres)
        bad = compare(crdt, D, eng.fetch_result(dres), want, sparse, req.n_req)
        assert not bad, bad[:10]
        free(dreq, dres)
        # read/6 through a cached batcher: the first read of a key finds no
        # snapshot, so it materializes from the empty base without SCT
        cold = copy.copy(req)
        cold.sct_ignore = np.ones(req.n_req, np.uint8)
        cold.base_value = np.zeros(req.n_req, np.int64)
        cold.base_off = np.zeros(req.n_req + 1, np.uint64)
        cold.base_tag, cold.base_tok = np.zeros(0, np.uint32), np.zeros(0, np.uint64)
        ccap = state_capacity(log2, cold)
        cwant = dm.run_oracle(oracle_lib, log2, cold, ccap, sparse=sparse)
        for read6 in ("1", "0"):
            monkeypatch.setenv("AGN_READ6", read6)
            with Batcher(ol, max_batch=8, cached=True) as bt:
                results = []
                for j in range(req.n_req):
                    kw = dict(R=cold.R[j], txid=int(cold.txid[j]))
                    if sparse:
                        kw["R_mask"] = cold.R_mask[j]
                    results.append(bt.read(int(cold.keys[j]), out_cap=int(ccap[j + 1] - ccap[j]),
                                           **kw))
            assert all(r["status"] == _abi.SS_NEW for r in results), read6
            bad = compare(crdt, D, gather(results, req.n_req, D, ccap), cwant, sparse, req.n_req)
            assert not bad, (read6, bad[:10])


# ---------------------------------------------------------------- GC
GC = [(crdt, D, sparse) for crdt in TYPES3 for D in (3, 8, 16) for sparse in (False, True)]


def gc_case(i, crdt, D, sparse):
    """200 keys with test_prune's thresholds, both pushed through the key's
    clock map (thresholds as further clock rows of the key)."""
    from test_prune import thresholds
    log, req, _ = dm.std_case(1000 + i, crdt, D, sparse, K=200, invalid=0.0, corrupt=0.0,
                              multi=0.2 if crdt == _abi.SET_AW else 0.0)
    prune, thr, tm = thresholds(3 * D + crdt, log, sparse)
    c, p = modes(i)
    log2, _, (thr2,), _ = dm.remap_clocks(log, req, c, extra=[(thr, np.arange(log.n_keys), tm)])
    thr2[thr2 == np.uint64(_abi.U64_MAX)] = np.uint64(dm.TOP)
    log2, _, _ = dm.remap_payload(log2, req, p, seed=i)
    return log2, prune, thr2, tm


@pytest.mark.parametrize("i,crdt,D,sparse", [(i, *c) for i, c in enumerate(GC)])
def test_prune_forms(eng, oracle_lib, monkeypatch, i, crdt, D, sparse):
    """agn_prune_ops in its CSR form and its segmented form (AGN_PRUNE_CT 0 /
    1, AGN_PRUNE_PF 2) against the oracle's prune."""
    from test_id_index import expected_index
    from test_prune import oracle_prune
    log, prune, thr, tm = gc_case(i, crdt, D, sparse)
    K = log.n_keys
    want, wflags, n_out = oracle_prune(oracle_lib, log, prune, thr, tm)
    assert 0 < n_out < log.n_entries and wflags.any()
    dlog = eng.upload_log(log)
    bp, bt = eng.upload(prune), eng.upload(thr)
    btm = eng.upload(tm) if tm is not None else None
    fl, tot = eng.empty(4 * K), eng.empty(16)
    # CSR
    dout = eng.alloc_log_like(log)
    eng.prune_ops(dlog, bp.ptr, bt.ptr, btm.ptr if btm else None, dout, fl.ptr, tot.ptr)
    eng.sync()
    totals = eng.download(tot, np.uint64, (2,))
    assert int(totals[0]) == n_out
    assert np.array_equal(eng.download(fl, np.uint32, (K,)), wflags)
    for name, (dt, shape) in dout.shapes.items():
        got, w = eng.download(dout.bufs[name], dt, shape), want[name]
        if name == "key_off":
            assert np.array_equal(got, w), name
        elif name == "rem_off":
            assert np.array_equal(got[:n_out + 1], w[:n_out + 1]), name
        elif name == "rem_tok":
            nr = int(totals[1])
            assert nr == int(want["rem_off"][n_out]) and np.array_equal(got[:nr], w[:nr]), name
        else:
            assert np.array_equal(got[:n_out], w[:n_out]), name
    free(dout)
    # segmented
    for ct in ("0", "1", "pf2"):
        monkeypatch.setenv("AGN_PRUNE_CT", ct if ct in ("0", "1") else "0")
        if ct.startswith("pf"):
            monkeypatch.setenv("AGN_PRUNE_PF", ct[2:])
        else:
            monkeypatch.delenv("AGN_PRUNE_PF", raising=False)
        dout = eng.alloc_log_like(log)
        kl, kid = eng.empty(8 * K), eng.empty(4 * K)
        dout.struct.key_len, dout.struct.key_id0 = kl.ptr, kid.ptr
        eng.prune_ops(dlog, bp.ptr, bt.ptr, btm.ptr if btm else None, dout, fl.ptr, tot.ptr)
        eng.sync()
        totals = eng.download(tot, np.uint64, (2,))
        assert int(totals[0]) == n_out, ct
        assert np.array_equal(eng.download(fl, np.uint32, (K,)), wflags), ct
        starts = eng.download(dout.bufs["key_off"], np.uint64, (K + 1,))[:K]
        lens = eng.download(kl, np.uint64, (K,))
        assert np.array_equal(starts, log.key_off[:K]), ct
        assert np.array_equal(lens, np.diff(want["key_off"])), ct
        got = {n: eng.download(dout.bufs[n], *dout.shapes[n]) for n in dout.shapes}
        for k in range(K):
            a, b = int(starts[k]), int(starts[k]) + int(lens[k])
            wa, wb = int(want["key_off"][k]), int(want["key_off"][k + 1])
            for name in ("oc", "oc_mask", "op_id", "txid", "eff", "tag", "add_tok"):
                if name in got:
                    assert np.array_equal(got[name][a:b], want[name][wa:wb]), (ct, k, name)
            if log.rem_off is not None:
                ro, wro = got["rem_off"], want["rem_off"]
                for e, we in zip(range(a, b), range(wa, wb)):
                    assert np.array_equal(got["rem_tok"][int(ro[e]):int(ro[e + 1])],
                                          want["rem_tok"][int(wro[we]):int(wro[we + 1])]), (ct, k, e)
        assert np.array_equal(eng.download(kid, np.uint32, (K,)),
                              expected_index(starts, lens, got["op_id"])), ct
        free(dout, kl, kid)
    free(dlog, bp, bt, fl, tot)
    if btm is not None:
        btm.free()


@pytest.mark.parametrize("i,crdt,D,sparse", [(i, *c) for i, c in enumerate(GC)])
def test_oplog_prune(eng, oracle_lib, i, crdt, D, sparse):
    """agn_oplog_prune on the appended remapped entries (ids ending at
    0xFFFFFFFE) leaves per key the oracle's prune output."""
    from test_oplog import (append_ops, check_id_index, csr_key, interleave, ops_of, renumbered,
                            segments)
    from test_prune import oracle_prune
    rng = np.random.default_rng(70 + i)
    log, prune, thr, tm = gc_case(i + 5, crdt, D, sparse)   # the clock modes shifted
    K, tags, W = log.n_keys, crdt != _abi.COUNTER_PN, (D + 63) // 64
    ops = ops_of(log)
    n_ops = np.bincount([k for k, _, _ in ops], minlength=K)
    with OpLog(eng, crdt, D, K, sparse=sparse, init_slots=i % 3) as ol:
        ol.set_counter(np.arange(K), (0xFFFFFFFE - n_ops).astype(np.uint32))
        log2 = renumbered(log, append_ops(ol, log, interleave(rng, ops), rng, max_batch=400))
        want, wflags, n_out = oracle_prune(oracle_lib, log2, prune, thr, tm)
        bp, bt = eng.upload(prune), eng.upload(thr)
        btm = eng.upload(tm) if tm is not None else None
        fl = eng.empty(4 * K)
        ol.prune(bp.ptr, bt.ptr, btm.ptr if btm else None, fl.ptr)
        assert np.array_equal(eng.download(fl, np.uint32, (K,)), wflags)
        assert ol.stats()["entries"] == n_out
        view = ol.flush()
        check_id_index(eng, view, K)
        segs = segments(eng, view, K, D, W, tags, sparse)
        for k in range(K):
            for name, v in csr_key(want, k, tags).items():
                g = segs[k][name]
                if name == "rems":
                    assert g == v, (k, name)
                else:
                    assert np.array_equal(np.asarray(g), np.asarray(v)), (k, name)
        free(bp, bt, fl)
        if btm is not None:
            btm.free()


# ---------------------------------------------------------------- rows compared across partitions
@pytest.mark.parametrize("mode", ["carry32", "sign64"])
@pytest.mark.parametrize("D", [2, 8, 64, 130])
def test_select_base(eng, oracle_lib, D, mode):
    """test_select_base_vs_oracle's generator, the rows pushed through one map
    per column (rows of different requests are compared)."""
    rng = np.random.default_rng(3 + D)
    n = 500
    lens = rng.integers(0, 11, n)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    M = int(off[-1])
    W = (D + 63) // 64
    clocks = rng.integers(0, 100, (M, D)).astype(np.uint64)
    cm = rng.integers(0, 2 ** 62, (M, W)).astype(np.uint64)
    R = rng.integers(50, 150, (n, D)).astype(np.uint64)
    Rm = rng.integers(0, 2 ** 62, (n, W)).astype(np.uint64) | np.uint64(0x5555)
    clocks, R = dm.remap_columns([clocks, R], [cm, Rm], mode)
    both = np.concatenate([clocks[dm.present_bits(cm, M, D)], R[dm.present_bits(Rm, n, D)]])
    side = both >> np.uint64(63 if mode == "sign64" else 32)
    assert len(np.unique(side)) == 2 and 0.25 < (side == side.max()).mean() < 0.75
    wi, wf = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    oracle_lib.oracle_select_base(D, n, off.ctypes.data, clocks.ctypes.data, cm.ctypes.data,
                                  R.ctypes.data, Rm.ctypes.data, wi.ctypes.data, wf.ctypes.data)
    assert len(np.unique(wf)) == 2 and (D > 8 or len(np.unique(wi)) > 3)
    bufs = [eng.upload(x) for x in (off, clocks, cm, R, Rm)]
    oi, of = eng.empty(n * 4), eng.empty(n)
    eng.select_base(D, n, *[b.ptr for b in bufs], oi.ptr, of.ptr)
    assert np.array_equal(eng.download(oi, np.int32, (n,)), wi)
    assert np.array_equal(eng.download(of, np.uint8, (n,)), wf)
    free(*bufs, oi, of)


@pytest.mark.parametrize("mode", ["carry32", "sign64"])
@pytest.mark.parametrize("D,sparse", [(1, False), (3, True), (8, False), (64, True), (256, False),
                                      (300, True)])
def test_dep_check(eng, oracle_lib, D, sparse, mode):
    from test_next_rows import dep_case, dep_oracle
    n = 500
    deps, dmask, origin, part, pc, pm = dep_case(D * 13 + n, D, n, 16, sparse)
    deps, pc = dm.remap_columns([deps, pc], [dmask, pm], mode)
    want = dep_oracle(oracle_lib, D, deps, dmask, origin, part, pc, pm)
    assert D == 1 or 0 < want.mean() < 1
    bufs = [eng.upload(x) if x is not None else None for x in (deps, dmask, origin, part, pc, pm)]
    out = eng.empty(n)
    eng.dep_check(D, n, *[b.ptr if b is not None else None for b in bufs[:4]], pc.shape[0],
                  bufs[4].ptr, bufs[5].ptr if bufs[5] is not None else None, out.ptr)
    assert np.array_equal(eng.download(out, np.uint8, (n,)), want)
    free(*[b for b in bufs if b is not None], out)


@pytest.mark.parametrize("mode", ["carry32", "sign64"])
@pytest.mark.parametrize("D,p_absent", [(1, 0.0), (5, 0.3), (256, 0.0), (300, 0.5)])
def test_gst_scalar(eng, oracle_lib, D, p_absent, mode):
    from test_next_rows import gst_case, ptr
    E = 500
    v = gst_case(D + E, D, E, p_absent)
    absent = v[:, :D] == np.uint64(_abi.U64_MAX)
    mask = np.zeros((E, (D + 63) // 64), np.uint64)
    for d in range(D):
        mask[:, d >> 6] |= (~absent[:, d]).astype(np.uint64) << np.uint64(d & 63)
    v[:, :D] = dm.remap_columns([np.ascontiguousarray(v[:, :D])], [mask], mode)[0]
    assert (v[:, :D][absent] == np.uint64(_abi.U64_MAX)).all()
    want, wg = v.copy(), np.zeros(E, np.uint64)
    oracle_lib.oracle_gst_scalar(D, E, ptr(want), ptr(wg))
    dv, dg = eng.upload(v), eng.empty(E * 8)
    eng.gst_scalar(D, E, dv.ptr, dg.ptr)
    assert np.array_equal(eng.download(dv, np.uint64, (E, D + 1)), want)
    assert np.array_equal(eng.download(dg, np.uint64, (E,)), wg)
    free(dv, dg)


# ---------------------------------------------------------------- snapshot cache
def wide_cache_case(seed, K, D, sparse, mode):
    """test_ss_cache's Case with the cache clocks, R and LastOpCt remapped per
    key (only a key's live slots are clock entries)."""
    from test_ss_cache import S, Case
    cs = Case(seed, K, D, sparse, n_req=K // 2)
    nr, W = len(cs.keys), cs.W
    live = (np.arange(S)[None, :] < cs.n[:, None]).reshape(K * S)
    cp = dm.present_bits(cs.mask.reshape(K * S, W) if sparse else None, K * S, D) & live[:, None]
    groups = [(cs.clock.reshape(K * S, D), np.repeat(np.arange(K), S), cp),
              (cs.R, cs.keys, dm.present_bits(cs.Rm, nr, D)),
              (cs.lastct, cs.keys, dm.present_bits(cs.lastct_mask, nr, D))]
    clock, cs.R, cs.lastct = dm.remap_rows(groups, K, mode)
    cs.clock = clock.reshape(K, S, D)
    side = cs.clock.reshape(K * S, D)[cp] >> np.uint64(63 if mode == "sign64" else 32)
    if mode == "top":
        assert (cs.clock.reshape(K * S, D)[cp] == np.uint64(dm.TOP)).sum() + \
            (cs.R == np.uint64(dm.TOP)).sum() + (cs.lastct == np.uint64(dm.TOP)).sum() > K // 2
    else:
        assert 0.25 < (side == side.max()).mean() < 0.75 and len(np.unique(side)) == 2
    return cs


@pytest.mark.parametrize("mode", ["carry32", "sign64", "top"])
@pytest.mark.parametrize("D,sparse", [(3, True), (8, False), (16, False)])
def test_cache_lookup_store(eng, oracle_lib, D, sparse, mode):
    """agn_ss_lookup / agn_ss_store against the oracle, as
    test_cache_gpu_vs_oracle, at 2000 keys."""
    from test_ss_cache import S, run_oracle
    K = 2000
    cs = wide_cache_case(7 * D + K, K, D, sparse, mode)
    want_a, want = run_oracle(oracle_lib, cs)
    assert len(np.unique(want["status"])) > 1 and want["prune"].any()
    nr, W = len(cs.keys), cs.W
    dev = {n: eng.upload(x) for n, x in cs.arrays().items()}
    c = _abi.AgnSsCache()
    c.n_dcs, c.slots, c.n_keys = D, S, K
    c.n, c.clock, c.last_op, c.value = (dev[x].ptr for x in ("n", "clock", "last_op", "value"))
    c.clock_mask = dev["mask"].ptr if sparse else None
    up = lambda x: eng.upload(x) if x is not None else None  # noqa: E731
    keys, R, Rm = up(cs.keys), up(cs.R), up(cs.Rm)
    o = {"sct": eng.empty(nr * D * 8), "sctm": eng.empty(nr * W * 8), "ign": eng.empty(nr),
         "base": eng.empty(nr * 8), "first": eng.empty(nr), "status": eng.empty(nr)}
    eng.ss_lookup(c, nr, keys.ptr, R.ptr, Rm.ptr if Rm else None, o["sct"].ptr,
                  o["sctm"].ptr if sparse else None, o["ign"].ptr, o["base"].ptr,
                  o["first"].ptr, o["status"].ptr)
    for n, dt in (("status", np.uint8), ("first", np.uint8), ("base", np.int64), ("ign", np.uint8)):
        assert np.array_equal(eng.download(o[n], dt, (nr,)), want[n]), n
    hit = want["status"] == _abi.SS_HIT
    assert np.array_equal(eng.download(o["sct"], np.uint64, (nr, D))[hit], want["sct"][hit])
    if sparse:
        assert np.array_equal(eng.download(o["sctm"], np.uint64, (nr, W))[hit], want["sctm"][hit])
    log = _abi.AgnLog()
    log.n_keys, log.n_dcs = K, D
    ko = up(cs.key_off)
    log.key_off = ko.ptr
    res = _abi.AgnResult()
    rb = {n: up(getattr(cs, n)) for n in ("res_value", "hole", "lastct", "lastct_mask", "count",
                                          "flags")}
    res.value, res.hole, res.lastct = rb["res_value"].ptr, rb["hole"].ptr, rb["lastct"].ptr
    res.lastct_mask = rb["lastct_mask"].ptr if sparse else None
    res.count, res.flags = rb["count"].ptr, rb["flags"].ptr
    gcb = up(cs.gc)
    pr, th, thm = eng.empty(K), eng.empty(K * D * 8), eng.empty(K * W * 8)
    eng.ss_store(c, log, nr, keys.ptr, o["first"].ptr, o["status"].ptr, gcb.ptr, res, None,
                 pr.ptr, th.ptr, thm.ptr if sparse else None)
    assert np.array_equal(eng.download(pr, np.uint8, (K,)), want["prune"])
    sel = want["prune"] == 1
    assert np.array_equal(eng.download(th, np.uint64, (K, D))[sel], want["thr"][sel])
    if sparse:
        assert np.array_equal(eng.download(thm, np.uint64, (K, W))[sel], want["thrm"][sel])
    gn = eng.download(dev["n"], np.uint32, (K,))
    assert np.array_equal(gn, want_a["n"])
    live = np.arange(S)[None, :] < gn[:, None]
    for name, dt, shape in (("clock", np.uint64, (K, S, D)), ("last_op", np.int64, (K, S)),
                            ("value", np.int64, (K, S))) + \
            ((("mask", np.uint64, (K, S, W)),) if sparse else ()):
        assert np.array_equal(eng.download(dev[name], dt, shape)[live], want_a[name][live]), name
    free(*dev.values(), keys, R, *o.values(), ko, *[b for b in rb.values() if b is not None],
         gcb, pr, th, thm)
    if Rm is not None:
        Rm.free()


@pytest.mark.parametrize("split,np_", [("0", "1"), ("1", "")], ids=["fused", "batched"])
@pytest.mark.parametrize("D", [3, 8])
def test_read_cached_rounds(eng, oracle_lib, monkeypatch, D, split, np_):
    """agn_read_cached (fused and batched) over three rounds of reads on a
    `mixed`-remapped counter case with wide effects: every round equals the
    oracle's lookup -> materialize -> store chain on a host cache (results,
    status, prune flags, thresholds, cache contents)."""
    from antidote_amd.encode import EncodedRead, log_struct
    from test_ss_cache import S, oracle_read_cached, ptr
    monkeypatch.setenv("AGN_READ_CACHED_SPLIT", split)
    monkeypatch.setenv("AGN_READ6_NP", np_)
    K, rounds = 601, 3
    log, req, _ = random_case(501 + D, _abi.COUNTER_PN, K, D, 150, txid=0.2, empty=0.05)
    rng = np.random.default_rng(D)
    # the rounds' reads (R a little ahead of the case's) as one request list,
    # so that the key's map covers them
    nrs = [301 + 100 * r for r in range(rounds)]
    keys = np.concatenate([rng.permutation(K)[:n] for n in nrs]).astype(np.uint64)
    ki = keys.astype(np.int64)
    n_all = len(keys)
    jit = np.concatenate([rng.integers(0, 3 if r < 2 else 40, (n, D)) for r, n in enumerate(nrs)])
    allreq = EncodedRead(n_dcs=D, req_type=_abi.COUNTER_PN, keys=keys,
                         R=np.ascontiguousarray(req.R[ki] + jit.astype(np.uint64)),
                         R_mask=np.zeros((n_all, 1), np.uint64), sct=None, sct_mask=None,
                         sct_ignore=None, txid=req.txid[ki].copy(),
                         base_value=np.zeros(n_all, np.int64), base_off=np.zeros(n_all + 1, np.uint64),
                         base_tag=np.zeros(0, np.uint32), base_tok=np.zeros(0, np.uint64))
    log, allreq = wide(0, log, allreq, sparse=False, clock="mixed", payload="lowsame")
    ls = log_struct(log)
    ls.oc_mask = None
    dlog = eng.upload_log(log)
    hcache = {"n": np.zeros(K, np.uint32), "clock": np.zeros((K, S, D), np.uint64),
              "last_op": np.zeros((K, S), np.int64), "value": np.zeros((K, S), np.int64)}
    hc = _abi.AgnSsCache()
    hc.n_dcs, hc.slots, hc.n_keys = D, S, K
    hc.n, hc.clock, hc.last_op, hc.value = (ptr(hcache[x]) for x in ("n", "clock", "last_op",
                                                                     "value"))
    bufs = {"n": eng.upload(np.zeros(K, np.uint32)), "clock": eng.empty(8 * K * S * D),
            "last_op": eng.empty(8 * K * S), "value": eng.empty(8 * K * S)}
    c = _abi.AgnSsCache()
    c.n_dcs, c.slots, c.n_keys = D, S, K
    c.n, c.clock, c.last_op, c.value = (bufs[x].ptr for x in ("n", "clock", "last_op", "value"))
    at, seen_hit, seen_prune = 0, False, False
    for rnd, nr in enumerate(nrs):
        k_r, R_r = keys[at:at + nr].copy(), np.ascontiguousarray(allreq.R[at:at + nr])
        tx = allreq.txid[at:at + nr].copy()
        at += nr
        gc = (rng.random(nr) < (0.0 if rnd == 0 else 0.3)).astype(np.uint8)
        want, wst, wpr, wthr = oracle_read_cached(oracle_lib, hc, ls, k_r, R_r, tx, gc, D)
        dk, dR, dtx, dgc = (eng.upload(x) for x in (k_r, R_r, tx, gc))
        res = eng.alloc_result(nr, D, sparse=False)
        st, pr, thr = eng.empty(nr), eng.empty(nr), eng.empty(K * D * 8)
        eng.read_cached(c, dlog, nr, dk.ptr, dR.ptr, dtx.ptr, dgc.ptr, res, st.ptr, pr.ptr, thr.ptr)
        eng.sync()
        bad = compare(_abi.COUNTER_PN, D, eng.fetch_result(res), want, False, nr)
        assert not bad, (rnd, bad[:10])
        assert np.array_equal(eng.download(st, np.uint8, (nr,)), wst), rnd
        gp = eng.download(pr, np.uint8, (nr,))
        kr = k_r.astype(np.int64)
        assert np.array_equal(gp, wpr[kr]), rnd
        pk = kr[gp == 1]
        assert np.array_equal(eng.download(thr, np.uint64, (K, D))[pk], wthr[pk]), rnd
        n = eng.download(bufs["n"], np.uint32, (K,))
        assert np.array_equal(n, hcache["n"]), rnd
        live = np.arange(S)[None, :] < n[:, None]
        for name, dt, shape in (("clock", np.uint64, (K, S, D)), ("last_op", np.int64, (K, S)),
                                ("value", np.int64, (K, S))):
            assert np.array_equal(eng.download(bufs[name], dt, shape)[live],
                                  hcache[name][live]), (rnd, name)
        seen_hit |= bool((wst == _abi.SS_HIT).any())
        seen_prune |= bool(wpr.any())
        free(dk, dR, dtx, dgc, res, st, pr, thr)
    assert seen_hit and seen_prune
    assert int(hcache["clock"].max()) >= 1 << 63 and (np.abs(hcache["value"]) > 1 << 40).any()
    free(dlog, *bufs.values())


@pytest.mark.parametrize("typ", [_abi.SET_AW, _abi.REGISTER_MV])
def test_read_cached_states_lowsame_tokens(eng, typ):
    """agn_read_cached with cached set / register states, as
    test_read_cached_states_vs_reference: tokens (t << 32) | 1 -- every low
    word the same -- and clocks across a 2^32 boundary, against the
    reference's transcription."""
    from oracle import py_oracle as po
    from test_ss_states import (D, PTYPE, TagWorkload, append_entry, placeholder, state_of, vc)
    K, rounds = 64, 2
    w = TagWorkload(91 + typ, K, typ)
    vn = po.MaterializerVnode()
    S = _abi.SNAPSHOT_THRESHOLD
    off = dm.B32 - 1150            # the workload's clocks start at 1000 and pass 1150 early

    def tk(t):
        return (int(t) << 32) | 1 if t else 0

    def clk(row):
        return np.asarray(row, np.int64).astype(np.uint64) + np.uint64(off)

    def eff_of(eff):
        if typ == _abi.SET_AW:
            return [(e, [tk(t) for t in add], [tk(t) for t in obs]) for e, add, obs in eff]
        if eff[0] == "reset":
            return ("reset", [tk(t) for t in eff[1]])
        return (eff[0], tk(eff[1]), [tk(t) for t in eff[2]])

    with OpLog(eng, typ, D, K) as ol:
        bufs = {"n": eng.empty(4 * K), "clock": eng.empty(8 * K * S * D),
                "last_op": eng.empty(8 * K * S), "value": eng.empty(8 * K * S),
                "ctl": eng.empty(32), "status": eng.empty(K), "prune": eng.empty(K),
                "thr": eng.empty(8 * K * D)}
        eng.lib.agn_memset_d(eng.ctx, bufs["n"].ptr, 0, 4 * K, None)
        eng.lib.agn_memset_d(eng.ctx, bufs["ctl"].ptr, 0, 32, None)
        cap = 1 << 14
        arena = [eng.empty(4 * cap), eng.empty(8 * cap)]
        c = _abi.AgnSsCache()
        c.n_dcs, c.slots, c.n_keys = D, S, K
        c.n, c.clock, c.last_op, c.value = (bufs[x].ptr for x in ("n", "clock", "last_op", "value"))
        c.state_tag, c.state_tok, c.state_cap, c.state_ctl = arena[0].ptr, arena[1].ptr, cap, \
            bufs["ctl"].ptr
        keys = eng.upload(np.arange(K, dtype=np.uint64))
        quirk, s, checked, below = set(), 0, 0, 0
        for rnd in range(rounds):
            for _ in range(3 * K):
                key = int(w.rng.integers(0, K))
                c_, ss, ct, oc, eff, entry = w.op(key)
                s += 1
                below += int((clk(oc) < np.uint64(dm.B32)).any())
                try:
                    vn.update(key, po.Payload(key, PTYPE[typ], eff_of(eff), vc(clk(ss)),
                                              (c_, ct + off), s))
                except po.BadMatch:
                    quirk.add(key)
                tag, add, rems = entry
                append_entry(ol, key, clk(oc), (tag, tk(add), [tk(t) for t in rems]), s)
                if placeholder(vn, key):
                    quirk.add(key)
            view = ol.flush()
            ln, _, _ = ol.key_meta()
            cap_off = np.zeros(K + 1, np.uint64)
            cap_off[1:] = np.cumsum(ln.astype(np.uint64) + np.uint64(512))
            dres = eng.alloc_result(K, D, sparse=False, cap_off=cap_off)
            R = clk(w.read_clock(lag=300))
            dR = eng.upload(np.tile(R, (K, 1)))
            gc = (w.rng.random(K) < 0.2).astype(np.uint8)
            dgc = eng.upload(gc)
            eng.read_cached(c, view, K, keys.ptr, dR.ptr, None, dgc.ptr, dres, bufs["status"].ptr,
                            bufs["prune"].ptr, bufs["thr"].ptr)
            res = eng.fetch_result(dres)
            status = eng.download(bufs["status"], np.uint8, (K,))
            for k in range(K):
                if k in quirk:
                    continue
                try:
                    want = vn.internal_read(k, PTYPE[typ], vc(R), po.IGNORE, bool(gc[k]))
                except NotImplementedError:
                    assert status[k] == _abi.SS_LOG, (rnd, k)
                    continue
                except po.BadMatch:
                    quirk.add(k)
                    continue
                assert status[k] in (_abi.SS_HIT, _abi.SS_NEW), (rnd, k, status[k])
                o, m = int(res.out_off[k]), int(res.out_n[k])
                got = state_of(typ, res.out_tag[o:o + m], res.out_tok[o:o + m])
                assert want == ("ok", got), (rnd, k, want, got)
                checked += 1
                if placeholder(vn, k):
                    quirk.add(k)
            ol.prune(bufs["prune"].ptr, bufs["thr"].ptr)
            ctl = eng.download(bufs["ctl"], np.uint64, (4,))
            assert ctl[2] == 0, "state arena overflow"
            free(dR, dgc, dres)
        assert len(quirk) < K // 2 and checked > K and 0 < below < s
        free(keys, *arena, *bufs.values())
