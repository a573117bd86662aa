"""register_lww's timestamp ties in term order on the device: agn_oplog_read
over an engine-owned log with a value-order table (agn_oplog_tag_order), exact
against tests/lww_order_model.py on the constructed keys whose reach
tests/test_lww_order_cpu.py checks, and on lww_model's random logs."""
import functools

import numpy as np
import pytest

import lww_model as lm
import lww_order_model as om
from antidote_amd import _abi
from antidote_amd._lib import EngineError
from antidote_amd.engine import OpLog
from test_lww import append_all, oplog_read, renumber, run_dev

pytestmark = pytest.mark.gpu

LWW = _abi.REGISTER_LWW
SHAPES = [(D, sparse) for D in om.DS for sparse in (False, True)]


@functools.lru_cache(maxsize=None)
def case(D, sparse):
    """The constructed keys and the model's answers per label table, once."""
    log, req, cap = om.tie_case(D, sparse)
    want = {name: om.model(log, req, sparse, cap, order=o)[0] for name, o in om.ORDERS.items()}
    want[None] = lm.model(log, req, sparse, cap)[0]
    return log, req, cap, want


def fill(eng, log, seed):
    ol = OpLog(eng, LWW, log.n_dcs, log.n_keys, sparse=log.oc_mask is not None)
    append_all(ol, log, np.random.default_rng(seed))
    return ol


@pytest.mark.parametrize("D,sparse", SHAPES, ids=[f"D{d}-{'masked' if s else 'dense'}"
                                                  for d, s in SHAPES])
def test_oplog_read_ties_in_label_order(eng, D, sparse):
    log, req, cap, want = case(D, sparse)
    n = req.n_req
    o = cap[:-1].astype(np.int64)

    def read(ol):
        return oplog_read(eng, ol, req, cap, D, sparse)

    with fill(eng, log, D) as ol:
        # no table yet: the larger id, flagged (what the parent computes)
        got = read(ol)
        assert not lm.compare_lww(D, got, want[None], sparse, n)
        # labels against the id order: the model's winner, never flagged
        ol.tag_order(0, om.ORDERS["against"])
        got = read(ol)
        bad = lm.compare_lww(D, got, want["against"], sparse, n)
        assert not bad, bad[:8]
        assert not (got.flags & _abi.F_TS_TIE).any()
        tied = want[None].flags & _abi.F_TS_TIE != 0
        assert tied.sum() == 10 and (got.out_tag[o][tied] != want[None].out_tag[o][tied]).all()
        # every label rewritten, the order kept: identical results
        ol.tag_order(0, om.ORDERS["against-rewritten"])
        again = read(ol)
        for f in ("flags", "out_n", "out_tag", "out_tok", "count", "hole", "lastct"):
            assert np.array_equal(getattr(again, f), getattr(got, f)), f
        # the reversed order: the other winner
        ol.tag_order(0, om.ORDERS["reversed"])
        rev = read(ol)
        assert not lm.compare_lww(D, rev, want["reversed"], sparse, n)
        assert (rev.out_tag[o][tied] != got.out_tag[o][tied]).all()
        assert not (rev.flags & _abi.F_TS_TIE).any()
        # one tag unlabelled (a rewrite in the middle of the table)
        ol.tag_order(0, om.ORDERS["against"])
        ol.tag_order(2, np.zeros(1, np.uint64))
        unl = read(ol)
        bad = lm.compare_lww(D, unl, want["tag2-unlabelled"], sparse, n)
        assert not bad, bad[:8]
        assert (unl.flags & _abi.F_TS_TIE).any()
    # one tag past the table: a fresh log whose table ends below tag 3
    with fill(eng, log, D + 100) as ol:
        ol.tag_order(0, om.ORDERS["tag3-past"])
        past = read(ol)
        bad = lm.compare_lww(D, past, want["tag3-past"], sparse, n)
        assert not bad, bad[:8]
        fl = past.flags & _abi.F_TS_TIE != 0
        assert fl.any() and (tied & ~fl).any()
        # labels set piecewise, upwards and past the first allocation: as one call
        ol.tag_order(3, om.ORDERS["against"][3:])
        ol.tag_order(5000, np.array([9], np.uint64))
        got = read(ol)
        assert not lm.compare_lww(D, got, want["against"], sparse, n)


def test_caller_arrays_do_not_see_the_table(eng):
    """agn_materialize on caller arrays, and a flushed view of a labelled log,
    behave as before: the larger id, flagged."""
    D, sparse = 8, False
    log, req, cap, want = case(D, sparse)
    with fill(eng, log, 3) as ol:
        ol.tag_order(0, om.ORDERS["against"])
        got = run_dev(eng, log, req, cap, sparse)
        assert not lm.compare_lww(D, got, want[None], sparse, req.n_req)
        view = ol.flush()
        dreq = eng.upload_read(req, sparse=sparse)
        dres = eng.alloc_result(req.n_req, D, sparse, cap_off=cap)
        eng.materialize(view, dreq, dres)
        eng.sync()
        got = eng.fetch_result(dres)
        assert not lm.compare_lww(D, got, want[None], sparse, req.n_req)
        for d in (dreq, dres):
            for b in d.bufs.values():
                b.free()
        # a recovery load does not copy the table: the loader sets it again
        with OpLog(eng, LWW, D, log.n_keys) as ol2:
            ol2.load(view)
            got = oplog_read(eng, ol2, req, cap, D, sparse)
            assert not lm.compare_lww(D, got, want[None], sparse, req.n_req)
            ol2.tag_order(0, om.ORDERS["against"])
            got = oplog_read(eng, ol2, req, cap, D, sparse)
            assert not lm.compare_lww(D, got, want["against"], sparse, req.n_req)


@pytest.mark.parametrize("D,sparse,load", [(8, False, "early"), (8, True, "late"),
                                           (3, True, "early"), (6, False, "late"),
                                           (33, True, "early"), (129, False, "late")])
def test_random_logs_with_labels(eng, monkeypatch, D, sparse, load):
    """lww_model's random logs (excluded newest assigns, invalid tags, base
    pairs, warm reads, reading txids) under a table that labels three of the
    four values against the id order: both orders of the ts / tag loads."""
    monkeypatch.setenv("AGN_LWW_LOAD", load)
    log, req, cap = lm.lww_case(900 + D, D, reps=3, sparse=sparse, warm=0.4, txid=0.3, base=0.5,
                                invalid=0.1, n_vals=4, ts_max=5)
    log = renumber(log)
    order = np.array([40, 30, 0, 10], np.uint64)
    want, _incl, info = om.model(log, req, sparse, cap, order=order)
    idw = lm.model(log, req, sparse, cap)[0]
    assert (want.flags & _abi.F_TS_TIE).any() and any(i and i["nT"] > 1 and not i["flagged"]
                                                      for i in info)
    assert not np.array_equal(want.out_tag, idw.out_tag)
    with fill(eng, log, D) as ol:
        ol.tag_order(0, order)
        got = oplog_read(eng, ol, req, cap, D, sparse)
        # err_pos is the failing entry's slot: in the log's arena here, in the CSR there
        bad = [b for b in lm.compare_lww(D, got, want, sparse, req.n_req) if b[1] != "err_pos"]
        assert not bad, bad[:8]
        errs = want.flags & _abi.F_ERR_UNEXPECTED != 0
        assert ((got.err_pos != lm.NO_POS) == errs).all()


def test_tag_order_refusals(eng):
    with OpLog(eng, _abi.SET_AW, 3, 4) as ol:
        with pytest.raises(EngineError) as e:
            ol.tag_order(0, np.array([1, 2], np.uint64))
        assert e.value.code == _abi.EINVAL
    with OpLog(eng, _abi.COUNTER_PN, 3, 4) as ol:
        with pytest.raises(EngineError) as e:
            ol.tag_order(0, np.array([1], np.uint64))
        assert e.value.code == _abi.EINVAL
    with OpLog(eng, LWW, 3, 4) as ol:
        ol.tag_order(7, np.zeros(0, np.uint64))       # nothing to set
        assert eng.lib.agn_oplog_tag_order(ol.h, 0, 2, None) == _abi.EINVAL
        assert eng.lib.agn_oplog_tag_order(None, 0, 0, None) == _abi.EINVAL
        with pytest.raises(EngineError) as e:         # AGN_TAG_INVALID is no value id
            ol.tag_order(0xFFFFFFFE, np.array([1, 2], np.uint64))
        assert e.value.code == _abi.EINVAL
