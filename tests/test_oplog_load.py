"""agn_oplog_load (recovery): a device log loaded into a pristine engine-owned
op log is indistinguishable from a twin -- a fresh log of the same parameters
that received the same entries key by key through agn_oplog_append (same_op
for an id equal to its predecessor's, agn_oplog_set_counter(k, id - 1) before
an id that is not counter + 1) -- right after the load and after the same
later appends, flushes, reads, prunes and cached-batcher reads.  Physical slot
numbers may differ; everything else is compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from antidote_amd import _abi
from antidote_amd._lib import EngineError
from antidote_amd.engine import Batcher, OpLog
from oplog_load_util import LENGTHS, take, twin_steps, with_lengths
from synth import random_case
from test_oplog import (append_ops, concat, dl, interleave, materialize_view, ops_of, pruned_log,
                        renumbered, segments)
from test_prune import oracle_prune, thresholds

pytestmark = pytest.mark.gpu

TYPES = [_abi.COUNTER_PN, _abi.SET_AW, _abi.REGISTER_MV, _abi.REGISTER_LWW]
INIT = 4


@functools.lru_cache(maxsize=None)
def case(crdt, D, sparse, lengths=tuple(LENGTHS)):
    """A log with the constructed key lengths (read-only: shared by the tests)."""
    donors, req, _ = random_case(1000 * crdt + 10 * D + sparse, crdt, 20, D, 220, sparse=sparse,
                                 warm=0.3, txid=0.2, multi=0.25 if crdt == _abi.SET_AW else 0.0,
                                 empty=0.0)
    log, req = with_lengths(donors, req, list(lengths))
    K = log.n_keys
    # ids: random with gaps (and equal neighbours for set_aw) from the donors;
    # one key without any gap, one consecutive from 5 (key_id0 = 5)
    for k, first in ((6, 1), (10, 5)):
        if k < K:
            a, b = int(log.key_off[k]), int(log.key_off[k + 1])
            log.op_id[a:b] = first + np.arange(b - a)
    if sparse:
        # even keys: one DC set for every entry; odd keys keep differing sets
        full = np.zeros(log.oc_mask.shape[1], np.uint64)
        for d in range(D):
            full[d >> 6] |= np.uint64(1 << (d & 63))
        for k in range(0, K, 2):
            log.oc_mask[int(log.key_off[k]):int(log.key_off[k + 1])] = full
    for a in (log.oc, log.op_id, log.txid, log.key_off):
        a.setflags(write=False)
    return log, req


def upload_src(eng, log):
    """The CSR device log; an array that upload_log drops because it is empty
    (an all-empty log) is still present, as agn_oplog_load requires."""
    d = eng.upload_log(log)
    tags = log.crdt_type != _abi.COUNTER_PN
    need = ["oc", "op_id", "txid"] + (["tag", "add_tok", "rem_off"] if tags else ["eff"]) + \
        (["oc_mask"] if log.oc_mask is not None else [])
    for name in need:
        if not getattr(d.struct, name):
            d.bufs[name] = eng.empty(8)
            setattr(d.struct, name, d.bufs[name].ptr)
    return d


def free(d):
    for b in d.bufs.values():
        b.free()


def twin_fill(ol, log):
    """The defining twin: log's entries key by key through agn_oplog_append."""
    tags = log.crdt_type != _abi.COUNTER_PN
    for k in range(log.n_keys):
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        steps = twin_steps(log.op_id[a:b])
        e = a
        while e < b:
            if steps[e - a][0] is not None:
                ol.set_counter(k, steps[e - a][0])
            f = e + 1
            while f < b and steps[f - a][0] is None:
                f += 1
            es = np.arange(e, f)
            kw = dict(oc=log.oc[es], txid=log.txid[es],
                      same_op=np.array([steps[x - a][1] for x in es], np.uint8))
            if log.oc_mask is not None:
                kw["oc_mask"] = log.oc_mask[es]
            if tags:
                ro = (log.rem_off[e:f + 1] - log.rem_off[e]).astype(np.uint32)
                kw.update(tag=log.tag[es], add_tok=log.add_tok[es], rem_off=ro,
                          rem_tok=log.rem_tok[int(log.rem_off[e]):int(log.rem_off[f])])
            else:
                kw["eff"] = log.eff[es]
            ids, _ = ol.append(np.full(f - e, k, np.uint64), **kw)
            assert np.array_equal(ids, log.op_id[e:f]), k
            e = f


def observe(eng, ol, log_params):
    """Every observable of the log but its physical slot numbers."""
    crdt, D, sparse, K = log_params
    W, tags = (D + 63) // 64, crdt != _abi.COUNTER_PN
    view = ol.flush()
    ln, ll, ct = ol.key_meta()
    st = ol.stats()
    obs = {"segments": segments(eng, view, K, D, W, tags, sparse),
           "key_len": dl(eng, view.key_len, np.uint64, K),
           "key_id0": dl(eng, view.key_id0, np.uint32, K),
           "length": ln, "list_len": ll, "counter": ct,
           "gc_due": ol.gc_due(np.arange(K, dtype=np.uint64)) if K else np.zeros(0, bool),
           "entries": st["entries"], "tokens": st["tokens"]}
    if sparse and D <= 64:
        assert view.key_mask
        obs["key_mask"] = dl(eng, view.key_mask, np.uint64, K)
        # the keys the batcher counts as mixed (non-empty, no shared DC set)
        obs["mixed"] = int(np.sum((obs["key_mask"] == 0) & (obs["key_len"] != 0)))
    else:
        assert not view.key_mask
    return view, obs, st


def assert_same(a, b):
    assert a.keys() == b.keys()
    for name in a:
        if name == "segments":
            for k, (sa, sb) in enumerate(zip(a[name], b[name])):
                assert sa.keys() == sb.keys()
                for f in sa:
                    if f == "rems":
                        assert sa[f] == sb[f], (k, f)
                    else:
                        assert np.array_equal(sa[f], sb[f]), (k, f)
        else:
            assert np.array_equal(np.asarray(a[name]), np.asarray(b[name])), name


def check_twin(eng, log, sparse, src, init=INIT):
    """Loads `src` (whose contents are `log`) and compares with the twin."""
    crdt, D, K = log.crdt_type, log.n_dcs, log.n_keys
    params = (crdt, D, sparse, K)
    with OpLog(eng, crdt, D, K, sparse=sparse, init_slots=init) as lo, \
            OpLog(eng, crdt, D, K, sparse=sparse, init_slots=init) as tw:
        lo.load(src)
        twin_fill(tw, log)
        _, a, st = observe(eng, lo, params)
        _, b, _ = observe(eng, tw, params)
        assert_same(a, b)
        # the contents are the log's, the ListLen is init doubled up to Length
        lens = (log.key_off[1:] - log.key_off[:-1]).astype(np.int64)
        assert np.array_equal(a["key_len"].astype(np.int64), lens)
        want_ll = np.zeros(K, np.int64)
        for k in range(K):
            if lens[k]:
                c = init if init else _abi.OPS_THRESHOLD
                while c < lens[k]:
                    c *= 2
                want_ll[k] = c
        assert np.array_equal(a["list_len"].astype(np.int64), want_ll)
        # arenas of exactly the laid-out size
        assert st["slots"] == int(np.sum(want_ll[lens > 0] + 1))
        assert st["entries"] == log.n_entries


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("D", [1, 3, 8, 16, 65])
@pytest.mark.parametrize("crdt", TYPES)
def test_load_csr_equals_twin(eng, crdt, D, sparse):
    log, _ = case(crdt, D, sparse)
    src = upload_src(eng, log)
    try:
        check_twin(eng, log, sparse, src)
    finally:
        free(src)


@pytest.mark.parametrize("lengths", [(0, 0, 0, 0, 0), (65,), (0,), (129, 0)],
                         ids=["all-empty", "one-key", "one-empty-key", "long-then-empty"])
@pytest.mark.parametrize("crdt,D,sparse", [(_abi.COUNTER_PN, 3, True), (_abi.SET_AW, 8, False),
                                           (_abi.REGISTER_LWW, 5, True)])
def test_load_small_logs(eng, crdt, D, sparse, lengths):
    log, _ = case(crdt, D, sparse, lengths)
    src = upload_src(eng, log)
    try:
        check_twin(eng, log, sparse, src, init=0 if len(lengths) == 1 else INIT)
    finally:
        free(src)


VIEW_CASES = [(_abi.COUNTER_PN, 3, True), (_abi.COUNTER_PN, 8, False), (_abi.SET_AW, 16, True),
              (_abi.REGISTER_MV, 65, False), (_abi.REGISTER_LWW, 8, False)]


@pytest.mark.parametrize("crdt,D,sparse", VIEW_CASES)
def test_load_view_after_prune_equals_twin(eng, oracle_lib, crdt, D, sparse):
    """src = another op log's flushed view after a prune: segmented (key_len),
    live ranges advanced past the dropped entries, ids with gaps."""
    rng = np.random.default_rng(7 * D + crdt)
    log, _ = case(crdt, D, sparse)
    with OpLog(eng, crdt, D, log.n_keys, sparse=sparse, init_slots=2) as donor:
        got = append_ops(donor, log, interleave(rng, ops_of(log)), rng)
        log2 = renumbered(log, got)
        prune, thr, tm = thresholds(D + crdt + 3, log2, sparse)
        want, _, n_out = oracle_prune(oracle_lib, log2, prune, thr, tm)
        bufs = [eng.upload(prune), eng.upload(thr)] + ([eng.upload(tm)] if tm is not None else [])
        donor.prune(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr if tm is not None else None)
        view = donor.flush()
        assert view.key_len
        check_twin(eng, pruned_log(want, n_out, crdt, D, log.n_keys, sparse), sparse, view)
        for b in bufs:
            b.free()


@pytest.mark.parametrize("crdt,D,sparse", [(_abi.COUNTER_PN, 8, False), (_abi.COUNTER_PN, 3, True),
                                           (_abi.SET_AW, 5, True), (_abi.REGISTER_MV, 16, False),
                                           (_abi.REGISTER_LWW, 16, True)])
def test_loaded_log_behaves_like_twin(eng, oracle_lib, crdt, D, sparse):
    """The same appends, flush, materialize, prune and cached-batcher reads
    (GC reads included) on the loaded log and on the twin."""
    log, _ = case(crdt, D, sparse)
    K = log.n_keys
    params = (crdt, D, sparse, K)
    more, req, _ = random_case(77 + D + crdt, crdt, K, D, 30, sparse=sparse, warm=0.3, txid=0.2,
                               multi=0.25 if crdt == _abi.SET_AW else 0.0, empty=0.3)
    src = upload_src(eng, log)
    with OpLog(eng, crdt, D, K, sparse=sparse, init_slots=INIT) as lo, \
            OpLog(eng, crdt, D, K, sparse=sparse, init_slots=INIT) as tw:
        lo.load(src)
        twin_fill(tw, log)
        ops = interleave(np.random.default_rng(5), ops_of(more))
        gots = [append_ops(ol, more, ops, np.random.default_rng(6)) for ol in (lo, tw)]
        assert gots[0] == gots[1]
        both = concat(log, renumbered(more, gots[0]))
        views = []
        for ol in (lo, tw):
            view, obs, _ = observe(eng, ol, params)
            assert not materialize_view(eng, oracle_lib, view, both, req, sparse)
            views.append(obs)
        assert_same(*views)
        prune, thr, tm = thresholds(D + crdt + 9, both, sparse)
        want, wflags, n_out = oracle_prune(oracle_lib, both, prune, thr, tm)
        bufs = [eng.upload(prune), eng.upload(thr)] + ([eng.upload(tm)] if tm is not None else [])
        fl = eng.empty(4 * K)
        after = []
        for ol in (lo, tw):
            ol.prune(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr if tm is not None else None, fl.ptr)
            assert np.array_equal(eng.download(fl, np.uint32, (K,)), wflags)
            after.append(observe(eng, ol, params)[1])
            assert after[-1]["entries"] == n_out
        assert_same(*after)
        if crdt == _abi.COUNTER_PN:
            rng = np.random.default_rng(8)
            with Batcher(lo, max_batch=8, cached=True) as ba, \
                    Batcher(tw, max_batch=8, cached=True) as bb:
                for _ in range(60):
                    k = int(rng.integers(0, K))
                    gc = bool(rng.random() < 0.3)
                    kw = dict(R=req.R[k], R_mask=req.R_mask[k] if sparse else None, gc=gc)
                    ra, rb = ba.read(k, **kw), bb.read(k, **kw)
                    for f in ra:
                        assert np.array_equal(np.asarray(ra[f]), np.asarray(rb[f])), (k, f)
            assert_same(observe(eng, lo, params)[1], observe(eng, tw, params)[1])
        for b in bufs + [fl]:
            b.free()
    free(src)


def pristine_then_loads(eng, ol, log, sparse, src):
    """After a refusal: nothing in the log, and the load then succeeds."""
    K = log.n_keys
    ln, ll, ct = ol.key_meta()
    assert not ln.any() and not ll.any() and not ct.any()
    assert ol.stats() == {"entries": 0, "slots": 0, "tokens": 0}
    ol.load(src)
    assert ol.stats()["entries"] == log.n_entries
    assert np.array_equal(ol.key_meta()[0].astype(np.int64),
                          (log.key_off[1:] - log.key_off[:-1]).astype(np.int64))
    assert K == log.n_keys


def refused(ol, src, code=_abi.EINVAL):
    with pytest.raises(EngineError) as ei:
        ol.load(src)
    assert ei.value.code == code, ei.value


@pytest.mark.parametrize("crdt,D,sparse", [(_abi.COUNTER_PN, 3, True), (_abi.SET_AW, 8, False)])
def test_load_refusals(eng, crdt, D, sparse):
    log, _ = case(crdt, D, sparse, (5, 0, 9, 1, 17))
    K, tags = log.n_keys, crdt != _abi.COUNTER_PN
    src = upload_src(eng, log)
    one = dict(oc=log.oc[:1], txid=log.txid[:1], oc_mask=log.oc_mask[:1] if sparse else None)
    if tags:
        one.update(tag=log.tag[:1], add_tok=log.add_tok[:1], rem_off=np.zeros(2, np.uint32),
                   rem_tok=np.zeros(1, np.uint64))
    else:
        one["eff"] = log.eff[:1]
    mk = lambda: OpLog(eng, crdt, D, K, sparse=sparse, init_slots=INIT)  # noqa: E731
    # a target that is not pristine: a staged entry, a flushed one, only a counter
    for how in ("append", "flush", "counter"):
        with mk() as ol:
            if how == "counter":
                ol.set_counter(K - 1, 3)
            else:
                ol.append(np.array([2], np.uint64), **one)
                if how == "flush":
                    ol.flush()
            before = ol.key_meta()
            refused(ol, src)
            assert all(np.array_equal(x, y) for x, y in zip(before, ol.key_meta()))
            if how == "counter":
                ol.set_counter(K - 1, 0)
                pristine_then_loads(eng, ol, log, sparse, src)
    # descriptor mismatches, then bad ids found on the device
    with mk() as ol:
        def variant(**kw):
            s = _abi.AgnLog()
            C.pointer(s)[0] = src.struct
            for name, v in kw.items():
                setattr(s, name, v)
            return s
        other = next(t for t in TYPES if t != crdt)
        bad = [variant(crdt_type=other), variant(n_dcs=D + 1), variant(n_keys=K - 1),
               variant(oc_mask=None) if sparse else variant(oc_mask=src.struct.oc)]
        bad += [variant(tag=None), variant(add_tok=None), variant(rem_off=None)] if tags else \
            [variant(eff=None)]
        for s in bad:
            refused(ol, s)
        ol.flush()  # an empty flush leaves the log pristine; its own view is refused
        v = ol.flush()
        refused(ol, v)
        a = int(log.key_off[2])
        for pos, val in ((a, 0), (a + 3, _abi.ID0_NONE), (a + 4, int(log.op_id[a + 3]) - 1),
                         (int(log.key_off[4]) + 16, 0)):
            ids = log.op_id.copy()
            ids[pos] = val
            b = eng.upload(ids)
            refused(ol, variant(op_id=b.ptr))
            b.free()
        pristine_then_loads(eng, ol, log, sparse, src)
        refused(ol, src)  # loaded: no longer pristine
    free(src)


def test_load_refuses_2_32_slots(eng):
    """Five one-entry keys with init_slots 2^30 want 5 (2^30 + 1) slots:
    AGN_ENOTSUP from the lengths alone, nothing allocated."""
    log, _ = case(_abi.COUNTER_PN, 8, False, (1, 1, 1, 1, 1))
    src = upload_src(eng, log)
    with OpLog(eng, _abi.COUNTER_PN, 8, 5, init_slots=1 << 30) as ol:
        refused(ol, src, _abi.ENOTSUP)
        ln, ll, ct = ol.key_meta()
        assert not ln.any() and not ll.any() and not ct.any()
        assert ol.stats() == {"entries": 0, "slots": 0, "tokens": 0}
    with OpLog(eng, _abi.COUNTER_PN, 8, 5, init_slots=INIT) as ol:
        ol.load(src)
        assert ol.stats() == {"entries": 5, "slots": 5 * (INIT + 1), "tokens": 0}
    free(src)


@pytest.mark.parametrize("crdt,init", [(_abi.COUNTER_PN, 0), (_abi.SET_AW, 1), (_abi.SET_AW, 4)])
def test_load_arena_sizing(eng, crdt, init):
    """Slots = the sum of ListLen + 1 over the non-empty keys, not doubled."""
    log, _ = case(crdt, 8, False)
    src = upload_src(eng, log)
    with OpLog(eng, crdt, 8, log.n_keys, init_slots=init) as ol:
        ol.load(src)
        ln, ll, _ = ol.key_meta()
        assert ol.stats()["slots"] == int(np.sum(ll[ln > 0].astype(np.int64) + 1))
        first = init if init else _abi.OPS_THRESHOLD
        for n, c in zip(ln, ll):
            assert c == 0 if n == 0 else (c >= n and c >= first and (c == first or c // 2 < n))
    free(src)
