"""The NIF's register_lww partition over the C ABI (helper, no tests): the
same calls nif/antidote_gpu_nif.c makes for the type -- an op log with presence
masks, its cached batcher, a value interner, an agn_tagorder whose labels go to
the log (agn_oplog_tag_order) before the op that names a new value is
appended, op_insert_gc's GC read, the log fallback with agn_batcher_store --
in test_typed_partition.TypedPartition's sequence.  Values are terms; the
comparator is encode.term_key where the NIF uses enif_compare."""
from __future__ import annotations

import numpy as np

from antidote_amd import _abi
from antidote_amd import clocksi_materializer as cm
from antidote_amd.engine import Batcher, Interner, OpLog, TagOrder
from antidote_amd.records import IGNORE
from oracle import py_oracle as po
from test_ss_states import LWW_NEW, log_response, vc

LWW = _abi.REGISTER_LWW
TYPE = po.REGISTER_LWW
ERRS = _abi.F_ERR_UNEXPECTED | _abi.F_ERR_CORRUPTED | _abi.F_ERR_CAPACITY


def valid_effect(eff):
    """{Ts, V} with integer 1 =< Ts < 2^64."""
    return isinstance(eff, tuple) and len(eff) == 2 and isinstance(eff[0], int) and \
        not isinstance(eff[0], bool) and 1 <= eff[0] < 1 << 64


class LwwPartition:
    def __init__(self, eng, d, K, **bk):
        self.d, self.K = d, K
        self.full = np.uint64((1 << d) - 1)
        self.ol = OpLog(eng, LWW, d, K, sparse=True)
        self.bt = Batcher(self.ol, max_batch=8, cached=True, **bk)
        self.vals = Interner(first_id=0, max_ids=(1 << 32) - 1)
        self.terms = []          # tag id -> value term
        self.order = TagOrder()
        self.bad = {}            # (key, op id) -> the effect term of an invalid entry
        self.disk = []           # the logging_vnode's committed payloads
        self.log_reads = self.log_gc = self.relabels = self.gc_reads = 0
        self.flags_seen = 0

    def close(self):
        self.bt.close()
        self.ol.close()
        self.order.close()
        self.vals.close()

    # ---- terms <-> ids
    def tag_of(self, v):
        """The value's id; on its first intern its place in the term order is
        found, labelled and uploaded -- before any op names it."""
        tag, new = self.vals.intern(repr(v).encode())
        if new:
            assert tag == len(self.terms)
            self.terms.append(v)
            self.relabels += self.order.insert_term(tag, v, self.ol)
        return tag

    def decode(self, key, g):
        self.flags_seen |= g["flags"]
        if g["flags"] & _abi.F_ERR_CORRUPTED:
            raise po.CorruptedOpsCache()
        if g["flags"] & _abi.F_ERR_UNEXPECTED:
            return ("error", ("unexpected_operation", self.bad[(key, g["err_pos"])], TYPE))
        if g["flags"] & _abi.F_TS_TIE:       # cannot happen: every value is labelled
            return ("error", "ts_tie")
        if not g["out_n"]:
            return ("ok", LWW_NEW)
        return ("ok", (int(g["out_tok"][0]), self.terms[int(g["out_tag"][0])]))

    # ---- the log fallback (antidote_gpu_nif.erl read/5)
    def from_log(self, key, R_dict, gc):
        resp = log_response(self.disk, key, R_dict, LWW_NEW)
        if resp.number_of_ops == 0:
            return ("ok", LWW_NEW)
        r = cm.materialize(TYPE, IGNORE, R_dict, resp)   # the per-call path: values sorted per call
        if r[0] != "ok":
            return r
        _, value, hole, ct, _newss, count = r
        if gc and ct != IGNORE:
            row, m = np.zeros(self.d, np.uint64), 0
            for dc, t in ct.items():
                row[dc] = t
                m |= 1 << dc
            pairs = [] if value == LWW_NEW else [(self.tag_of(value[1]), value[0])]
            self.bt.store(key, row, clock_mask=np.uint64(m), last_op=hole, count=count,
                          tags=[p[0] for p in pairs], toks=[p[1] for p in pairs], gc=True)
            self.log_gc += 1
        return ("ok", value)

    def _read(self, key, R, gc):
        return self.bt.read(key, R=np.asarray(R, np.uint64), R_mask=np.array([self.full]), gc=gc,
                            out_cap=4)

    # ---- update/2 and read/6
    def update(self, key, pay, oc, txid):
        self.disk.append(pay)                       # logged before the materializer
        if self.ol.gc_due(key)[0]:                  # op_insert_gc's GC read at the op's dict
            row = np.zeros(self.d, np.uint64)
            for dc, t in pay.snapshot_time.items():
                row[dc] = t
            g = self._read(key, row, True)
            self.gc_reads += 1
            self.flags_seen |= g["flags"]
            if g["status"] == _abi.SS_LOG:
                self.from_log(key, pay.snapshot_time, True)
        eff = pay.op_param
        tag, ts = (self.tag_of(eff[1]), eff[0]) if valid_effect(eff) else (_abi.TAG_INVALID, 0)
        ids, _ = self.ol.append(np.array([key], np.uint64),
                                np.asarray(oc, np.uint64).reshape(1, self.d),
                                oc_mask=np.array([[self.full]], np.uint64),
                                tag=np.array([tag], np.uint32), add_tok=np.array([ts], np.uint64),
                                txid=np.array([txid], np.uint64))
        if tag == _abi.TAG_INVALID:
            self.bad[(key, int(ids[0]))] = eff

    def read(self, key, R):
        g = self._read(key, R, False)
        if g["status"] == _abi.SS_LOG:
            self.log_reads += 1
            return self.from_log(key, vc(R), False), g
        return self.decode(key, g), g
