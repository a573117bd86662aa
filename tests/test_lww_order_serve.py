"""register_lww's timestamp ties through the cached batcher: the snapshot a
tied read stores is the term-order winner, so every later read that hits it is
exact and unflagged.  Twin partitions, one on the fused kernel (k_lww_serve)
and one on the kernel sequence (AGN_LWW_FUSED=0), are compared with each other
bit for bit and with two models: the reference transcription's vnode (lookup,
fold, store: oracle/py_oracle.py, whose update/2 is max(Effect, State) in term
order) for every served value, and a model chain for every other result field
(flags, hole, count, LastOpCt, the pair): tests/lww_order_model.py's fold over
the key's log from the snapshot the script's earlier read stored -- the base
pair and its clock as SCT, which is what the lookup hands the fold.  The chain
follows the script's own store points (the first read of six ops, the GC
read), each confirmed by the next read's status and count; it stops at the GC
read, whose prune changes the log under the last read (that one is held to
the vnode and to the other arm).

Values are binaries whose term order is the reverse of their id order, so the
id-order winner is always the wrong answer."""
import threading

import numpy as np
import pytest

import cache_edges as ce
import lww_order_model as om
from antidote_amd import _abi
from antidote_amd.encode import EncodedLog, EncodedRead
from antidote_amd.engine import TagOrder
from oracle import py_oracle as po
from test_lww_serve import ERRS, same_result, twins
from test_ss_states import vc

pytestmark = pytest.mark.gpu

PT = po.REGISTER_LWW
LWW = _abi.REGISTER_LWW
TOP = 1 << 40            # the tied timestamp
N_TAGS = 5


def value(tag):
    """The value behind a tag id: descending in term order."""
    return bytes([ord("z") - tag]) + b"-val"


class Pair:
    """Twin partitions with one label table, and the reference vnode."""

    def __init__(self, eng, monkeypatch, D, K, **bk):
        self.D = D
        self.pa, self.pb = twins(eng, monkeypatch, D, False, K, **bk)
        self.order = TagOrder()
        for tag in range(N_TAGS):       # arrival order: every insert goes to the front
            self.order.insert_term(tag, value(tag))
        assert [self.order.at(i) for i in range(N_TAGS)] == list(range(N_TAGS - 1, -1, -1))
        self.upload(1)
        self.vn, self.tx, self.lock = po.MaterializerVnode(), 0, threading.Lock()
        self.ents = [[] for _ in range(K)]      # per key: (oc row, ts, tag), op ids 1..
        self.snap = [None] * K                  # per key: ((tag, ts), clock) of the cached snapshot

    def upload(self, scale):
        """The whole table, every label divided by `scale` (order-preserving:
        neighbours are 2^58 apart or more)."""
        labels = self.order.labels(0, N_TAGS) // np.uint64(scale)
        assert len(set(labels.tolist())) == N_TAGS and labels.all()
        self.labels = labels
        for p in (self.pa, self.pb):
            p.ol.tag_order(0, labels)

    def close(self):
        self.pa.close()
        self.pb.close()
        self.order.close()

    def append(self, k, clk, ts, tag):
        c, oc = clk.op()
        for p in (self.pa, self.pb):
            p.append(k, oc.astype(np.uint64), ts, tag, None)
        self.ents[k].append((oc.astype(np.uint64), int(ts), int(tag)))
        ss = oc.copy()
        ss[c] = int(oc[c]) - 1
        with self.lock:
            self.tx += 1
            self.vn.update(k, po.Payload(k, PT, (int(ts), value(tag)), vc(ss), (c, int(oc[c])),
                                         self.tx))

    def read(self, k, R, gc, ctx):
        ga, gb = self.pa.read(k, R, None, gc), self.pb.read(k, R, None, gc)
        same_result(ga, gb, ctx)
        ka = np.array([k], np.uint64)
        ma, mb = self.pa.ol.key_meta(ka), self.pb.ol.key_meta(ka)
        assert all(np.array_equal(x, y) for x, y in zip(ma, mb)), (ctx, "key_meta")
        with self.lock:
            want = self.vn.internal_read(k, PT, vc(R), po.IGNORE, bool(gc))
        assert want[0] == "ok" and not ga["flags"] & (ERRS | _abi.F_TS_TIE), (ctx, want, ga)
        assert ga["status"] in (_abi.SS_HIT, _abi.SS_NEW) and ga["out_n"] == 1, (ctx, ga)
        got = (int(ga["out_tok"][0]), value(int(ga["out_tag"][0])))
        assert got == want[1], (ctx, got, want)
        return ga

    def chain(self, k, R, g, ctx, stores):
        """The model chain for one read: the fold over the key's whole log from
        the cached snapshot (none: a NEW read), every result field."""
        D, ents, snap = self.D, self.ents[k], self.snap[k]
        n = len(ents)
        assert g["status"] == (_abi.SS_HIT if snap else _abi.SS_NEW), (ctx, g["status"])
        log = EncodedLog(crdt_type=LWW, n_dcs=D, key_off=np.array([0, n], np.uint64),
                         key_type=np.full(1, LWW, np.uint8),
                         oc=np.array([e[0] for e in ents], np.uint64).reshape(n, D), oc_mask=None,
                         op_id=np.arange(1, n + 1, dtype=np.uint32), txid=np.zeros(n, np.uint64),
                         tag=np.array([e[2] for e in ents], np.uint32),
                         add_tok=np.array([e[1] for e in ents], np.uint64),
                         rem_off=np.zeros(n + 1, np.uint32), rem_tok=np.zeros(1, np.uint64))
        sct = np.zeros((1, D), np.uint64) if snap is None else snap[1].reshape(1, D)
        req = EncodedRead(n_dcs=D, req_type=LWW, keys=np.zeros(1, np.uint64),
                          R=np.asarray(R, np.uint64).reshape(1, D), R_mask=None, sct=sct,
                          sct_mask=None, sct_ignore=np.array([snap is None], np.uint8),
                          txid=np.zeros(1, np.uint64), base_value=None, base_off=None,
                          base_tag=None, base_tok=None)
        cap = np.array([0, 1], np.uint64)
        w, _incl, _info = om.model(log, req, False, cap, bases=[snap[0] if snap else None],
                                   order=self.labels)
        fl = int(w.flags[0])
        assert g["flags"] == fl and g["count"] == int(w.count[0]), (ctx, g, fl, int(w.count[0]))
        assert g["hole"] == int(w.hole[0]), (ctx, g["hole"], int(w.hole[0]))
        if not fl & _abi.F_CT_IGNORE:
            assert np.array_equal(g["lastct"], w.lastct[0]), (ctx, g["lastct"], w.lastct[0])
        assert g["out_n"] == int(w.out_n[0]) == 1, ctx
        pair = (int(w.out_tag[0]), int(w.out_tok[0]))
        assert (int(g["out_tag"][0]), int(g["out_tok"][0])) == pair, (ctx, pair)
        if stores:
            self.snap[k] = (pair, w.lastct[0].copy())


def script(P, k, a, b, c, relabel=None):
    """One key.  Tags a and b tie at TOP inside the log; the read that folds
    them stores a snapshot; a later read with no new op returns the stored
    pair; then an op with tag c ties with the cached base pair."""
    clk = ce.Clock(P.D)
    best = lambda *tags: max(value(t) for t in tags)  # noqa: E731  (bytewise: the term order)
    for x in range(6):
        tie = {1: a, 4: b}.get(x)
        P.append(k, clk, TOP if tie is not None else 10 + x, tie if tie is not None else x % N_TAGS)
    g = P.read(k, clk.R(), False, (k, "tie read"))
    assert g["status"] == _abi.SS_NEW and g["count"] == 6, g      # >= MIN_OP_STORE_SS: stored
    P.chain(k, clk.R(), g, (k, "tie read"), stores=True)
    assert value(int(g["out_tag"][0])) == best(a, b) and int(g["out_tok"][0]) == TOP
    if relabel is not None:
        relabel()
    g = P.read(k, clk.R() + np.uint64(7), False, (k, "later clock, no new op"))
    P.chain(k, clk.R() + np.uint64(7), g, (k, "later clock, no new op"), stores=False)
    assert g["status"] == _abi.SS_HIT and g["count"] == 0, g      # the stored pair alone
    assert value(int(g["out_tag"][0])) == best(a, b) and int(g["out_tok"][0]) == TOP
    P.append(k, clk, TOP, c)
    g = P.read(k, clk.R(), False, (k, "op ties with the cached pair"))
    P.chain(k, clk.R(), g, (k, "op ties with the cached pair"), stores=False)
    assert g["status"] == _abi.SS_HIT and g["count"] == 1, g
    assert value(int(g["out_tag"][0])) == best(a, b, c)
    for x in range(5):
        P.append(k, clk, 20 + x, (x + k) % N_TAGS)
    g = P.read(k, clk.R(), True, (k, "GC read"))                   # stores again
    P.chain(k, clk.R(), g, (k, "GC read"), stores=True)
    assert g["count"] == 6 and value(int(g["out_tag"][0])) == best(a, b, c)
    g = P.read(k, clk.R() + np.uint64(3), False, (k, "second stored pair"))
    assert g["status"] == _abi.SS_HIT and g["count"] == 0
    assert value(int(g["out_tag"][0])) == best(a, b, c) and int(g["out_tok"][0]) == TOP


# (a, b, c): the tie inside the log either way round; c beats the cached pair,
# loses to it, or repeats its tag
TAGS = [(1, 3, 0), (3, 1, 4), (0, 4, 2), (4, 0, 0), (2, 3, 1), (3, 2, 3), (1, 0, 4), (4, 2, 3)]


@pytest.mark.parametrize("D", [8, 64])
def test_stored_snapshot_is_the_term_order_winner(eng, monkeypatch, D):
    P = Pair(eng, monkeypatch, D, len(TAGS), max_batch=8)
    try:
        for k, (a, b, c) in enumerate(TAGS):
            script(P, k, a, b, c)
        pa, pb = P.pa.bt.path_stats(), P.pb.bt.path_stats()
        assert pa["sequence"] == 0 and pa["fused"] > 0 and pb["fused"] == 0, (pa, pb)
    finally:
        P.close()


@pytest.mark.parametrize("D", [8, 64])
def test_same_script_from_eight_threads(eng, monkeypatch, D):
    """Each key's script on its own thread, the reads meeting in shared
    batches; thread 0 rewrites every label in the middle (order kept), which
    takes both logs exclusively against the others' read batches."""
    P = Pair(eng, monkeypatch, D, len(TAGS), max_batch=8, max_wait_us=2000)
    errs = []

    def run(k):
        try:
            a, b, c = TAGS[k]
            script(P, k, a, b, c, relabel=(lambda: P.upload(3)) if k == 0 else None)
        except Exception as e:  # noqa: BLE001
            errs.append((k, e))
    try:
        ths = [threading.Thread(target=run, args=(k,)) for k in range(len(TAGS))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errs, errs[0]
        st, ps = P.pa.bt.stats(), P.pa.bt.path_stats()
        assert st["reads"] == 5 * len(TAGS) and ps["fused"] == st["batches"], (st, ps)
    finally:
        P.close()


def test_unlabelled_tie_is_flagged_labelled_is_exact(eng, monkeypatch):
    """Without labels the tie read is flagged on both paths and the larger id
    wins (what the parent does); once the labels are set, the same tie on a
    fresh key is exact and unflagged."""
    D = 8
    pa, pb = twins(eng, monkeypatch, D, False, 2, max_batch=4)
    try:
        clk = ce.Clock(D)
        for x in range(6):
            _c, oc = clk.op()
            for p in (pa, pb):
                p.append(0, oc.astype(np.uint64), TOP if x in (1, 4) else 10 + x, x % N_TAGS, None)
        ga, gb = pa.read(0, clk.R()), pb.read(0, clk.R())
        same_result(ga, gb, "unlabelled")
        assert ga["flags"] & _abi.F_TS_TIE and int(ga["out_tag"][0]) == 4      # ids 1 and 4
        labels = np.array([50, 40, 30, 20, 10], np.uint64)
        for p in (pa, pb):
            p.ol.tag_order(0, labels)
        clk2 = ce.Clock(D)
        for x in range(6):
            _c, oc = clk2.op()
            for p in (pa, pb):
                p.append(1, oc.astype(np.uint64), TOP if x in (1, 4) else 10 + x, x % N_TAGS, None)
        ga, gb = pa.read(1, clk2.R()), pb.read(1, clk2.R())
        same_result(ga, gb, "labelled")
        assert not ga["flags"] & _abi.F_TS_TIE and int(ga["out_tag"][0]) == 1
    finally:
        pa.close()
        pb.close()
