"""register_lww's tie rule with value-order labels (include/antidote_gpu.h,
AGN_F_TS_TIE; mat_lww.hip), over a candidate set, and the constructed cases the
CPU and GPU tests share.

Candidates are the base pair (if any) plus every included entry with a valid
tag.  wts is the largest ts among them, T the set of distinct tags at wts,
label(tag) = order[tag] if tag is below the table's length, else 0.  The winner
is the tag of T with the largest (label(tag), tag), unsigned and
lexicographic; AGN_F_TS_TIE iff |T| > 1 and some tag of T has label 0.  With
no table every label is 0 and the rule is tests/lww_model.py's.

The snapshot filter and every other result field are lww_model.model's.
"""
from __future__ import annotations

import numpy as np

import lww_model as lm
from antidote_amd import _abi
from antidote_amd.encode import EncodedLog, EncodedRead

LWW = _abi.REGISTER_LWW


def label(order, tag):
    return int(order[tag]) if order is not None and tag < len(order) else 0


def settle(cands, order=None):
    """cands: iterable of (ts, tag).  -> (wts, winner tag, flagged, |T|)."""
    ts = np.array([c[0] for c in cands], np.uint64)
    tg = np.array([c[1] for c in cands], np.uint32)
    wts = ts.max()
    T = np.unique(tg[ts == wts])
    labs = np.array([label(order, int(t)) for t in T], np.uint64)
    # the largest (label, tag): the largest tag among those at the largest label
    win = int(T[labs == labs.max()].max())
    return int(wts), win, bool(len(T) > 1 and (labs == 0).any()), len(T)


def candidates(log, req, incl_all, i, bases=None):
    """The candidate set of request i, base pair first, and where each sits:
    -1 for the base pair, else the entry's position in its key."""
    k = int(req.keys[i])
    a = int(log.key_off[k])
    if bases is not None:
        base = bases[i]
    else:
        o0, o1 = int(req.base_off[i]), int(req.base_off[i + 1])
        base = (int(req.base_tag[o0]), int(req.base_tok[o0])) if o1 > o0 else None
    cands, pos = [], []
    if base is not None:
        cands.append((base[1], base[0]))
        pos.append(-1)
    incl = incl_all[i]
    for p in np.nonzero(incl)[0] if incl is not None else []:
        t = int(log.tag[a + int(p)])
        if t != _abi.TAG_INVALID:
            cands.append((int(log.add_tok[a + int(p)]), t))
            pos.append(int(p))
    return cands, pos


def model(log, req, sparse, cap_off, bases=None, order=None):
    """lww_model.model with the fold's winner and AGN_F_TS_TIE by the rule
    above.  -> (result, per-entry inclusion, per-request branch info)."""
    res, incl_all, _info = lm.model(log, req, sparse, cap_off, bases=bases)
    info = []
    for i in range(req.n_req):
        fl = int(res.flags[i])
        if fl & (_abi.F_ERR_CORRUPTED | _abi.F_ERR_UNEXPECTED) or not int(res.out_n[i]):
            info.append(None)
            continue
        cands, pos = candidates(log, req, incl_all, i, bases)
        wts, win, flagged, nT = settle(cands, order)
        fl = (fl & ~_abi.F_TS_TIE) | (_abi.F_TS_TIE if flagged else 0)
        res.flags[i] = fl
        if not fl & _abi.F_ERR_CAPACITY:
            o = int(cap_off[i])
            res.out_tag[o], res.out_tok[o] = win, wts
        at = [(p, t) for (ts, t), p in zip(cands, pos) if ts == wts]
        step = lm.opi(log.n_dcs)     # ops per filter iteration: lane = position % step at LPO 1
        lanes = {}
        for p, t in at:
            lanes.setdefault(-1 if p < 0 else p % step, set()).add(t)
        info.append(dict(
            nT=nT, flagged=flagged,
            labelled=all(label(order, t) for _p, t in at),
            past_table=any(order is not None and t >= len(order) for _p, t in at),
            in_lane=any(ln >= 0 and len(ts_) > 1 for ln, ts_ in lanes.items()),
            across_lanes=len({ln for ln in lanes if ln >= 0}) > 1 and
            len({t for p, t in at if p >= 0}) > 1,
            base_tie=nT > 1 and any(p < 0 for p, _t in at)))
    return res, incl_all, info


# ------------------------------------------------------------------ constructed keys
LENS = [1, 2, 63, 64, 65, 129]
DS = [1, 8, 9, 33, 64, 65]     # LPO 1, 1, 2, 8, 8 and the general shape
TS_TOP = 1000                  # the tied timestamp; every other entry is below it


def tie_keys():
    """(name, length, {position: tag} at TS_TOP, base (tag, ts) or None).
    Tags 1..3 tie; every other entry carries tag 0 at a smaller ts."""
    out = [(f"len{n}", n, {n - 1: 1}, None) for n in LENS]          # |T| = 1
    out += [("lane-0-64", 65, {0: 1, 64: 2}, None),                 # one lane at LPO 1
            ("lane-0-64-long", 129, {0: 2, 64: 1, 128: 2}, None),
            ("lanes-3-40", 64, {3: 1, 40: 2}, None),                # different lanes
            ("lanes-3-40-odd", 63, {3: 2, 40: 1}, None),
            ("base-op", 2, {1: 1}, (2, TS_TOP)),                    # the base pair and one op
            ("base-op-long", 65, {64: 2}, (1, TS_TOP)),
            ("three-way", 129, {5: 1, 69: 2, 100: 3}, None),        # lane 5 twice, then another
            ("three-way-base", 64, {0: 1, 63: 2}, (3, TS_TOP)),
            ("lanes-7-50", 64, {7: 1, 50: 3}, None),                # a tie without tag 2
            ("base-below", 2, {0: 1, 1: 2}, (3, TS_TOP - 1)),       # a base pair that loses
            ("same-tag-twice", 65, {0: 2, 64: 2}, None)]            # |T| = 1, two candidates
    return out


def tie_case(D, sparse):
    """The keys of tie_keys() as one log whose every entry every read includes
    (R at the clocks' ceiling, no base snapshot time), dense or masked.  Masked:
    each entry carries its own DC set, R every DC."""
    ks = tie_keys()
    K = len(ks)
    lens = [k[1] for k in ks]
    key_off = np.zeros(K + 1, np.uint64)
    key_off[1:] = np.cumsum(lens)
    E = int(key_off[-1])
    rng = np.random.default_rng(D * 2 + int(sparse))
    oc = rng.integers(1, 100, (E, D)).astype(np.uint64)
    W = (D + 63) // 64
    ocm = None
    if sparse:
        ocm = np.zeros((E, W), np.uint64)
        present = rng.random((E, D)) < 0.7
        present[np.arange(E), rng.integers(0, D, E)] = True
        for e, d in zip(*np.nonzero(present)):
            ocm[e, d >> 6] |= np.uint64(1 << (int(d) & 63))
    tag = np.zeros(E, np.uint32)
    ts = rng.integers(1, TS_TOP - 1, E).astype(np.uint64)
    op_id = np.zeros(E, np.uint32)
    boff, btag, btok = np.zeros(K + 1, np.uint64), [], []
    for k, (_name, n, tied, base) in enumerate(ks):
        a = int(key_off[k])
        op_id[a:a + n] = np.arange(1, n + 1)
        for p, t in tied.items():
            tag[a + p], ts[a + p] = t, TS_TOP
        if base is not None:
            btag.append(base[0])
            btok.append(base[1])
        boff[k + 1] = len(btag)
    log = EncodedLog(crdt_type=LWW, n_dcs=D, key_off=key_off, key_type=np.full(K, LWW, np.uint8),
                     oc=oc, oc_mask=ocm, op_id=op_id, txid=np.zeros(E, np.uint64), tag=tag,
                     add_tok=ts, rem_off=np.zeros(E + 1, np.uint32), rem_tok=np.zeros(1, np.uint64))
    full = np.zeros((K, W), np.uint64)
    for d in range(D):
        full[:, d >> 6] |= np.uint64(1 << (d & 63))
    req = EncodedRead(n_dcs=D, req_type=LWW, keys=np.arange(K, dtype=np.uint64),
                      R=np.full((K, D), 100, np.uint64), R_mask=full,
                      sct=np.zeros((K, D), np.uint64), sct_mask=np.zeros((K, W), np.uint64),
                      sct_ignore=np.ones(K, np.uint8), txid=np.zeros(K, np.uint64),
                      base_value=np.zeros(K, np.int64), base_off=boff,
                      base_tag=np.array(btag, np.uint32), base_tok=np.array(btok, np.uint64))
    cap = np.arange(K + 1, dtype=np.uint64)
    return log, req, cap


U62 = 1 << 62
# label tables over tag ids 0..3 (tag 0 is the filler below TS_TOP)
ORDERS = {
    # against the id order: the id-order winner is the wrong answer
    "against": np.array([7, 3 * U62, 2 * U62, 5], np.uint64),
    # the same order in other numbers
    "against-rewritten": np.array([400, 300, 200, 100], np.uint64),
    # the reverse of it: the other winner
    "reversed": np.array([1, 2, 3, (1 << 64) - 2], np.uint64),
    # one tag unlabelled
    "tag2-unlabelled": np.array([7, 3 * U62, 0, 5], np.uint64),
    # tag 3 past the table
    "tag3-past": np.array([7, 3 * U62, 2 * U62], np.uint64),
}
