"""Helpers of the agn_oplog_load tests (no GPU needed to import): the twin's
call derivation and logs with constructed key lengths."""
import numpy as np

from antidote_amd import _abi
from antidote_amd.encode import EncodedLog, EncodedRead

# key lengths around the copy kernel's paths (a head / tail of one 16-byte
# unit, one unit, 4 G units for G = 4 / 16 / 64) with empty keys first, in the
# middle and last
LENGTHS = [0, 0, 1, 3, 4, 5, 8, 9, 0, 63, 64, 65, 128, 129, 0, 0, 2, 7, 16, 17, 31, 32, 33, 50,
           51, 100, 0, 1, 1, 4, 64, 12, 6, 10, 20, 40, 3, 129, 5, 0]


def twin_steps(ids):
    """For one key's op ids (oldest first) the calls that make agn_oplog_append
    assign them: per entry (counter to set before it, or None; same_op)."""
    out, counter, prev = [], 0, None
    for i in ids:
        i = int(i)
        if prev is not None and i == prev:
            out.append((None, 1))
        else:
            out.append((None if i == counter + 1 else i - 1, 0))
            counter = i
        prev = i
    return out


def take(log, req, picks):
    """A log (and its reads) whose key j is the first n entries of log's key
    d, for picks[j] = (d, n)."""
    tags = log.crdt_type != _abi.COUNTER_PN
    es, key_off = [], [0]
    for d, n in picks:
        a = int(log.key_off[d])
        assert a + n <= int(log.key_off[d + 1])
        es.extend(range(a, a + n))
        key_off.append(len(es))
    es = np.array(es, np.int64)
    K = len(picks)
    out = EncodedLog(crdt_type=log.crdt_type, n_dcs=log.n_dcs,
                     key_off=np.array(key_off, np.uint64),
                     key_type=np.full(K, log.crdt_type, np.uint8), oc=log.oc[es].copy(),
                     oc_mask=None if log.oc_mask is None else log.oc_mask[es].copy(),
                     op_id=log.op_id[es].copy(), txid=log.txid[es].copy())
    if tags:
        out.tag, out.add_tok = log.tag[es].copy(), log.add_tok[es].copy()
        ro, toks = [0], []
        for e in es:
            toks.extend(log.rem_tok[int(log.rem_off[e]):int(log.rem_off[e + 1])].tolist())
            ro.append(len(toks))
        out.rem_off = np.array(ro, np.uint32)
        out.rem_tok = np.array(toks if toks else [0], np.uint64)
    else:
        out.eff = log.eff[es].copy()
    ds = np.array([d for d, _ in picks], np.int64)
    assert not len(req.base_tag)
    r = EncodedRead(n_dcs=req.n_dcs, req_type=req.req_type, keys=np.arange(K, dtype=np.uint64),
                    R=req.R[ds].copy(), R_mask=req.R_mask[ds].copy(), sct=req.sct[ds].copy(),
                    sct_mask=req.sct_mask[ds].copy(), sct_ignore=req.sct_ignore[ds].copy(),
                    txid=req.txid[ds].copy(), base_value=req.base_value[ds].copy(),
                    base_off=np.zeros(K + 1, np.uint64), base_tag=req.base_tag[:0],
                    base_tok=req.base_tok[:0])
    return out, r


def with_lengths(log, req, lengths):
    """take() with, per wanted length, the first donor key that is long enough."""
    have = (log.key_off[1:] - log.key_off[:-1]).astype(np.int64)
    picks = []
    for j, n in enumerate(lengths):
        ok = np.nonzero(have >= n)[0]
        assert len(ok), n
        picks.append((int(ok[j % len(ok)]), n))
    return take(log, req, picks)
