"""Randomised SoA logs for differential tests (engine vs C oracle).

Unlike the bench generator (agn_gen_*), these exercise every corner the
reference's semantics has: ragged and empty keys, sparse clocks (DCs missing
from op clocks, from the read snapshot and from SCT), warm reads (SCT set),
reading-transaction matches (TxId == op.txid), invalid effects, keys whose
ops have another type, multi-entry ops and base states.

random_case's batches are warm-capable (the SCT arrays are always there) and
read every key once; cold() drops the SCT arrays and rekey() turns the key map
into a subset or into repeated keys with a row of their own per request.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from antidote_amd import _abi
from antidote_amd.encode import EncodedLog, EncodedRead, n_words, state_capacity


def _mask_rows(rng, n, D, p_absent):
    W = n_words(D)
    m = np.zeros((n, W), np.uint64)
    present = rng.random((n, D)) >= p_absent
    for d in range(D):
        m[:, d >> 6] |= present[:, d].astype(np.uint64) << np.uint64(d & 63)
    return m, present


LWW_VALS, LWW_TS_MAX = 3, 8   # the small range of register_lww values / timestamps


def _lww_entries(rng, log, invalid):
    """register_lww entries for a log of clocks: tag = value id, add_tok =
    timestamp, every removal range empty.  About half the keys draw both from
    the edges of their domains (lww_model.TS_EDGE / TAG_EDGE: 0, 2^32 +- 1,
    2^63, 2^64 - 1 travel through whatever stages the 64-bit field), the rest
    from a small range, so ties at the winning timestamp, base wins and an
    excluded newest assign are common.  Returns the per-key edge choice."""
    from lww_model import TAG_EDGE, TS_EDGE
    K, E = log.n_keys, log.n_entries
    edge_key = rng.random(K) < 0.5
    edge = np.repeat(edge_key, np.diff(log.key_off.astype(np.int64)))
    tag = np.where(edge, rng.choice(np.array(TAG_EDGE, np.uint32), E),
                   rng.integers(0, LWW_VALS, E).astype(np.uint32)).astype(np.uint32)
    ts = np.where(edge, rng.choice(np.array(TS_EDGE, np.uint64), E),
                  rng.integers(1, LWW_TS_MAX + 1, E).astype(np.uint64)).astype(np.uint64)
    tag[rng.random(E) < invalid] = _abi.TAG_INVALID
    log.tag, log.add_tok = tag, ts
    log.rem_off, log.rem_tok = np.zeros(E + 1, np.uint32), np.zeros(1, np.uint64)
    return edge_key


def random_case(seed, crdt, K, D, nmax, *, sparse=False, warm=0.0, txid=0.0, invalid=0.0,
                corrupt=0.0, multi=0.0, base=0.0, n_elems=6, empty=0.1, identity=True,
                lens=None):
    """lens: the keys' lengths, given (then nmax and empty choose nothing; the
    generator's draws stay where they were)."""
    rng = np.random.default_rng(seed)
    W = n_words(D)
    drawn = rng.integers(0, nmax + 1, K)
    drawn[rng.random(K) < empty] = 0
    lens = drawn if lens is None else np.asarray(lens, np.int64).copy()
    assert len(lens) == K and (lens >= 0).all()
    key_off = np.zeros(K + 1, np.uint64)
    key_off[1:] = np.cumsum(lens)
    E = int(key_off[-1])
    base_t = 1_000_000
    # op clocks: per key a random walk so that reads include a prefix-ish subset
    oc = np.zeros((E, D), np.uint64)
    op_id = np.zeros(E, np.uint32)
    txids = np.zeros(E, np.uint64)
    R = np.zeros((K, D), np.uint64)
    sct = np.zeros((K, D), np.uint64)
    sct_ign = np.ones(K, np.uint8)
    rtx = np.zeros(K, np.uint64)
    for k in range(K):
        a, b = int(key_off[k]), int(key_off[k + 1])
        clk = base_t + rng.integers(0, 50, D)
        ids = np.sort(rng.choice(np.arange(1, 4 * (b - a) + 2), b - a, replace=False)) \
            if b > a else []
        snaps = []
        for j, e in enumerate(range(a, b)):
            c = rng.integers(0, D)
            clk = clk.copy()
            clk[c] += rng.integers(1, 20)
            row = clk - rng.integers(0, 30, D)
            row[c] = clk[c]
            oc[e] = row
            op_id[e] = ids[j]
            txids[e] = rng.integers(1, 6)
            snaps.append(row)
        cut = rng.integers(0, (b - a) + 1)
        Rk = (np.max(np.array(snaps[:cut]), axis=0) if cut else clk - 10) + rng.integers(-4, 16, D)
        R[k] = np.maximum(Rk, 1)
        if rng.random() < warm:
            c2 = rng.integers(0, cut + 1)
            sct[k] = (np.max(np.array(snaps[:c2]), axis=0) if c2 else clk - 40) + \
                rng.integers(-5, 6, D)
            sct_ign[k] = 0
        if rng.random() < txid:
            rtx[k] = rng.integers(1, 6)
    # multi-entry ops: copy the previous entry's id/clock/txid
    if multi and E:
        for k in range(K):
            a, b = int(key_off[k]), int(key_off[k + 1])
            for e in range(a + 1, b):
                if rng.random() < multi:
                    op_id[e], oc[e], txids[e] = op_id[e - 1], oc[e - 1], txids[e - 1]
    log = EncodedLog(crdt_type=crdt, n_dcs=D, key_off=key_off,
                     key_type=np.full(K, crdt, np.uint8), oc=oc, oc_mask=None, op_id=op_id,
                     txid=txids)
    log.key_type[rng.random(K) < corrupt] = _abi.TYPE_MIXED
    if sparse:
        log.oc_mask, present = _mask_rows(rng, E, D, 0.25)
        # the commit DC (max entry) is always present in OpSSCommit
        for e in range(E):
            d = int(np.argmax(oc[e]))
            log.oc_mask[e, d >> 6] |= np.uint64(1 << (d & 63))
        # multi-entry ops share the mask too
        for k in range(K):
            a, b = int(key_off[k]), int(key_off[k + 1])
            for e in range(a + 1, b):
                if op_id[e] == op_id[e - 1]:
                    log.oc_mask[e] = log.oc_mask[e - 1]
    if crdt == _abi.COUNTER_PN:
        eff = rng.integers(-1000, 1001, E).astype(np.int64)
        eff[rng.random(E) < invalid] = _abi.EFFECT_INVALID
        log.eff = eff
    elif crdt == _abi.REGISTER_LWW:
        edge_key = _lww_entries(rng, log, invalid)
    else:
        tag = rng.integers(0, n_elems, E).astype(np.uint32)
        add = np.zeros(E, np.uint64)
        rem_off = np.zeros(E + 1, np.uint32)
        rem = []
        tok_ctr = 1
        for k in range(K):
            a, b = int(key_off[k]), int(key_off[k + 1])
            live: dict = {}
            allt = []
            for e in range(a, b):
                t = int(tag[e])
                if crdt == _abi.REGISTER_MV and rng.random() < 0.1:
                    tag[e] = 0
                    add[e] = 0
                    obs = [x for v in live.values() for x in v]
                    live = {}
                elif rng.random() < 0.7:
                    tok = (k << 24) | tok_ctr
                    tok_ctr += 1
                    add[e] = tok
                    key = t if crdt == _abi.SET_AW else 0
                    cur = live.get(key, [])
                    if rng.random() < 0.25:
                        obs = []
                        live[key] = cur + [tok]
                    else:
                        obs = list(cur)
                        live[key] = [tok]
                    allt.append(tok)
                else:
                    key = t if crdt == _abi.SET_AW else 0
                    obs = list(live.get(key, []))
                    live[key] = []
                # stale / foreign tokens in removal lists (must be no-ops or order-aware)
                if allt and rng.random() < 0.2:
                    obs = obs + [int(rng.choice(allt))]
                rem.extend(obs)
                rem_off[e + 1] = len(rem)
            tok_ctr += 0
        tag[rng.random(E) < invalid] = _abi.TAG_INVALID
        log.tag, log.add_tok, log.rem_off = tag, add, rem_off
        log.rem_tok = np.array(rem if rem else [0], np.uint64)
    Rm = Sm = None
    if sparse:
        Rm, _ = _mask_rows(rng, K, D, 0.03)
        Sm, _ = _mask_rows(rng, K, D, 0.2)
    else:
        Rm = np.zeros((K, W), np.uint64)
        Sm = np.zeros((K, W), np.uint64)
    boff = np.zeros(K + 1, np.uint64)
    btag, btok = [], []
    if crdt == _abi.REGISTER_LWW:
        from lww_model import TAG_EDGE, TS_EDGE
        for k in range(K):   # at most one pair: a state is one {Ts, Value}
            if rng.random() < base:
                if edge_key[k]:
                    btag.append(int(rng.choice(TAG_EDGE)))
                    btok.append(int(rng.choice(np.array(TS_EDGE, np.uint64))))
                else:
                    btag.append(int(rng.integers(0, LWW_VALS)))
                    btok.append(int(rng.integers(1, LWW_TS_MAX + 3)))
            boff[k + 1] = len(btag)
    elif crdt != _abi.COUNTER_PN:
        for k in range(K):
            if rng.random() < base:
                pairs = [(int(rng.integers(0, n_elems)), (1 << 60) | (k << 8) | (x + 1))
                         for x in range(int(rng.integers(1, 5)))]
                # the reference's states are ordered: set_aw orddict by elem (tokens in
                # list order), register_mv sorted by {Value, Token}
                pairs.sort(key=(lambda p: p[0]) if crdt == _abi.SET_AW else None)
                for t, tk in pairs:
                    btag.append(t)
                    btok.append(tk)
            boff[k + 1] = len(btag)
    keys = np.arange(K, dtype=np.uint64)
    if not identity:
        keys = rng.permutation(K).astype(np.uint64)
        R, Rm, sct, Sm, sct_ign, rtx = R[keys], Rm[keys], sct[keys], Sm[keys], sct_ign[keys], \
            rtx[keys]
    req = EncodedRead(n_dcs=D, req_type=crdt, keys=keys, R=np.ascontiguousarray(R),
                      R_mask=np.ascontiguousarray(Rm), sct=np.ascontiguousarray(sct),
                      sct_mask=np.ascontiguousarray(Sm), sct_ignore=sct_ign, txid=rtx,
                      base_value=rng.integers(-50, 50, K).astype(np.int64), base_off=boff,
                      base_tag=np.array(btag, np.uint32), base_tok=np.array(btok, np.uint64))
    cap = state_capacity(log, req) if crdt != _abi.COUNTER_PN else None
    return log, req, cap


def cold(req):
    """The same requests without SCT (sct == NULL: the cold kernels)."""
    return dataclasses.replace(req, sct=None, sct_mask=None, sct_ignore=None)


REPEAT_RUN = 9   # rekey "repeat": one key fills this many consecutive requests


def rekey(log, req, mode, seed, hot=0):
    """(req2, cap2): the requests of `req` (one per key, any order) under a key
    map that is no permutation.

    "subset": about K/3 distinct keys in random order, each with its row of
    `req` as it is.
    "repeat": n_req = 2K + 1, keys drawn with replacement from all but
    ceil(K/4) keys, which are never requested (hot > 0: half of the draws go to
    the first `hot` keys of the pool); one key fills the REPEAT_RUN requests
    from a multiple of 8 on, a whole aligned group of 8 and both halves of a
    pair.  Every request has a row of its own: the key's R plus a jitter in
    [-3, 4) per column, floored at 1, a txid and a base_value of its own, with
    SCT arrays an SCT (the key's plus the same kind of jitter, floored at 0)
    and an sct_ignore of its own, and for the state types a base of its own: a
    subsequence of the key's base pairs (which keeps their order)."""
    rng = np.random.default_rng(seed)
    K, D = log.n_keys, log.n_dcs
    assert req.n_req == K and len(set(req.keys.tolist())) == K
    row_of = np.zeros(K, np.int64)
    row_of[req.keys.astype(np.int64)] = np.arange(K)
    if mode == "subset":
        keys = rng.permutation(K)[:max(1, K // 3)]
    elif mode == "repeat":
        pool = rng.permutation(K)[:K - (K + 3) // 4]
        n = 2 * K + 1
        keys = pool[rng.integers(0, len(pool), n)]
        if hot:
            h = rng.random(n) < 0.5
            keys[h] = pool[rng.integers(0, hot, int(h.sum()))]
        at = 8 * int(rng.integers(0, (n - REPEAT_RUN) // 8 + 1))
        keys[at:at + REPEAT_RUN] = pool[0]
    else:
        raise KeyError(mode)
    n = len(keys)
    src = row_of[keys]
    rep = mode == "repeat"
    R = req.R[src]
    txid, bv = req.txid[src], req.base_value[src]
    if rep:
        assert int(R.max()) < 1 << 62
        R = np.maximum(R.astype(np.int64) + rng.integers(-3, 4, (n, D)), 1).astype(np.uint64)
        txid = np.where(rng.random(n) < 0.3, rng.integers(1, 6, n), 0).astype(np.uint64)
        bv = rng.integers(-50, 50, n).astype(np.int64)
    sct = sm = si = None
    if req.sct is not None:
        sct, sm, si = req.sct[src], req.sct_mask[src], req.sct_ignore[src]
        if rep:
            sct = np.maximum(sct.astype(np.int64) + rng.integers(-3, 4, (n, D)), 0).astype(np.uint64)
            si = np.where(rng.random(n) < 0.25, 1 - si, si).astype(np.uint8)
    boff = np.zeros(n + 1, np.uint64)
    btag, btok = [], []
    for i, j in enumerate(src):
        a, b = int(req.base_off[j]), int(req.base_off[j + 1])
        keep = rng.random(b - a) < 0.7 if rep else np.ones(b - a, bool)
        btag += req.base_tag[a:b][keep].tolist()
        btok += req.base_tok[a:b][keep].tolist()
        boff[i + 1] = len(btag)
    req2 = EncodedRead(n_dcs=D, req_type=req.req_type, keys=keys.astype(np.uint64),
                       R=np.ascontiguousarray(R), R_mask=np.ascontiguousarray(req.R_mask[src]),
                       sct=None if sct is None else np.ascontiguousarray(sct),
                       sct_mask=None if sm is None else np.ascontiguousarray(sm),
                       sct_ignore=None if si is None else np.ascontiguousarray(si),
                       txid=np.ascontiguousarray(txid), base_value=np.ascontiguousarray(bv),
                       base_off=boff, base_tag=np.array(btag, np.uint32),
                       base_tok=np.array(btok, np.uint64))
    cap2 = state_capacity(log, req2) if log.crdt_type != _abi.COUNTER_PN else None
    return req2, cap2


def compare(crdt, D, a, b, sparse, n):
    """Field-by-field bit-exact comparison of two ResultArrays; returns a list
    of mismatching request indices (empty = identical)."""
    bad = []
    for i in range(n):
        fa, fb = int(a.flags[i]), int(b.flags[i])
        if fa != fb:
            bad.append((i, "flags", fa, fb))
            continue
        if fa & (_abi.F_ERR_CORRUPTED | _abi.F_ERR_UNEXPECTED):
            if int(a.err_pos[i]) != int(b.err_pos[i]):
                bad.append((i, "err_pos", int(a.err_pos[i]), int(b.err_pos[i])))
            continue
        if int(a.hole[i]) != int(b.hole[i]):
            bad.append((i, "hole", int(a.hole[i]), int(b.hole[i])))
        if int(a.count[i]) != int(b.count[i]):
            bad.append((i, "count", int(a.count[i]), int(b.count[i])))
        if not (fa & _abi.F_CT_IGNORE):
            if sparse:
                if not np.array_equal(a.lastct_mask[i], b.lastct_mask[i]):
                    bad.append((i, "lastct_mask"))
                m = [(int(a.lastct_mask[i][d >> 6]) >> (d & 63)) & 1 for d in range(D)]
                va = [int(x) for x, keep in zip(a.lastct[i], m) if keep]
                vb = [int(x) for x, keep in zip(b.lastct[i], m) if keep]
                if va != vb:
                    bad.append((i, "lastct"))
            elif not np.array_equal(a.lastct[i], b.lastct[i]):
                bad.append((i, "lastct"))
        if crdt == _abi.COUNTER_PN:
            if int(a.value[i]) != int(b.value[i]):
                bad.append((i, "value", int(a.value[i]), int(b.value[i])))
        elif not (fa & _abi.F_ERR_CAPACITY):
            if int(a.out_n[i]) != int(b.out_n[i]):
                bad.append((i, "out_n", int(a.out_n[i]), int(b.out_n[i])))
                continue
            o, k = int(a.out_off[i]), int(a.out_n[i])
            if not (np.array_equal(a.out_tag[o:o + k], b.out_tag[o:o + k]) and
                    np.array_equal(a.out_tok[o:o + k], b.out_tok[o:o + k])):
                bad.append((i, "state"))
    return bad
