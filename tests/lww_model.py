"""antidote_crdt_register_lww on the host: a numpy restatement of the per-key
snapshot filter (filter.hpp) plus the type's fold, and
the cases the CPU and GPU tests share.

The fold (include/antidote_gpu.h, AGN_REGISTER_LWW): candidates are the base
pair, if present, plus every included entry whose tag is valid; the winner is
the maximum by (ts, tag), unsigned and lexicographic; AGN_F_TS_TIE iff another
candidate carries the winner's ts under a different tag.  Everything but the
sequential assign is parity-unpinned (antidote_crdt 0.1.2 is restated, not
held): the model is this project's statement of it, not the reference's.
"""
from __future__ import annotations

import numpy as np

from antidote_amd import _abi
from antidote_amd.encode import (EncodedLog, EncodedRead, alloc_result, n_words,
                                 state_capacity)
from synth import _mask_rows

LWW = _abi.REGISTER_LWW
NO_POS = 0xFFFFFFFF


def opi(D):
    """Ops per filter iteration of the kernel shape that serves D (filter.hpp)."""
    return 64 if D <= 8 else 32 if D <= 16 else 16 if D <= 32 else 8 if D <= 64 else \
        4 if D <= 128 else 2


def _bits(row, D):
    d = np.arange(D)
    return ((np.asarray(row, np.uint64)[d >> 6] >> (d & 63).astype(np.uint64)) & np.uint64(1)) != 0


def _pack(present, D):
    m = np.zeros(n_words(D), np.uint64)
    for d in np.nonzero(present)[0]:
        m[int(d) >> 6] |= np.uint64(1 << (int(d) & 63))
    return m


def model(log, req, sparse, cap_off, bases=None):
    """Every result field of a register_lww batch, the per-entry inclusion of
    each request, and what the reach test classifies.  `sparse`: the masks of
    `req` are passed (read_struct(sparse)); log.oc_mask None reads as dense.
    `bases`: per request None or (tag, ts), instead of req.base_off."""
    D, n = log.n_dcs, req.n_req
    res = alloc_result(n, D, sparse=True, cap_off=cap_off)
    res.err_pos[:] = NO_POS
    full, none = np.ones(D, bool), np.zeros(D, bool)
    incl_all, info = [], []
    for i in range(n):
        k = int(req.keys[i])
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        cls = dict(corrupt=False, base_wins=False, last_chunk=False, tie=False,
                   max_excluded=False, err=False, empty=False, invalid_excluded=False)
        info.append(cls)
        if b > a and log.key_type is not None and int(log.key_type[k]) != req.req_type:
            res.flags[i] = _abi.F_ERR_CORRUPTED
            cls["corrupt"] = True
            incl_all.append(None)
            continue
        R = req.R[i]
        rp = _bits(req.R_mask[i], D) if sparse and req.R_mask is not None else full
        sct_ign = req.sct is None or (req.sct_ignore is not None and bool(req.sct_ignore[i]))
        sp = none if sct_ign else \
            (_bits(req.sct_mask[i], D) if sparse and req.sct_mask is not None else full)
        s = np.where(sp, req.sct[i], np.uint64(0)) if req.sct is not None else np.zeros(D, np.uint64)
        ct, ctdef = s.copy(), sp.copy()
        txr = int(req.txid[i]) if req.txid is not None else 0
        use_tx = txr != 0 and log.txid is not None
        incl = np.zeros(b - a, bool)
        first_excl = first_err = -1
        for p in range(b - a):
            e = a + p
            op = _bits(log.oc_mask[e], D) if log.oc_mask is not None else full
            oc = log.oc[e]
            ok_r = bool(np.all(~op | (rp & (oc <= R))))      # a DC missing in R excludes
            le_s = bool(np.all(~op | (oc <= s)))             # a DC missing in SCT reads 0
            nip = sct_ign or not le_s or (use_tx and int(log.txid[e]) == txr)
            if nip and not ok_r and first_excl < 0:
                first_excl = p
            if nip and ok_r:
                incl[p] = True
                ct = np.where(op, np.maximum(ct, oc), ct)
                ctdef = ctdef | op
                if first_err < 0 and int(log.tag[e]) == _abi.TAG_INVALID:
                    first_err = p
        incl_all.append(incl)
        cnt = int(incl.sum())
        res.count[i] = cnt
        res.hole[i] = (int(log.op_id[a + first_excl]) - 1 if first_excl >= 0 else
                       int(log.op_id[b - 1]) if b > a else 0)
        fl = _abi.F_NEWSS if cnt else 0
        if sct_ign and cnt == 0:
            fl |= _abi.F_CT_IGNORE
        else:
            res.lastct[i] = np.where(ctdef, ct, np.uint64(0))
            res.lastct_mask[i] = _pack(ctdef, D)
        # ---- the fold
        if bases is not None:
            base = bases[i]
        else:
            o0, o1 = int(req.base_off[i]), int(req.base_off[i + 1])
            base = (int(req.base_tag[o0]), int(req.base_tok[o0])) if o1 > o0 else None
        cands = [] if base is None else [(base[1], base[0], -1)]
        cands += [(int(log.add_tok[a + p]), int(log.tag[a + p]), p) for p in range(b - a)
                  if incl[p] and int(log.tag[a + p]) != _abi.TAG_INVALID]
        valid = [(int(log.add_tok[a + p]), p) for p in range(b - a)
                 if int(log.tag[a + p]) != _abi.TAG_INVALID]
        if valid:
            top = max(t for t, _ in valid)
            cls["max_excluded"] = any(t == top and not incl[p] for t, p in valid)
        cls["invalid_excluded"] = first_err < 0 and any(
            int(log.tag[a + p]) == _abi.TAG_INVALID for p in range(b - a))
        if first_err >= 0:
            fl |= _abi.F_ERR_UNEXPECTED
            res.err_pos[i] = a + first_err
            cls["err"] = True
        elif cands:
            ts, tag = max((c[0], c[1]) for c in cands)
            tie = any(c[0] == ts and c[1] != tag for c in cands)
            if tie:
                fl |= _abi.F_TS_TIE
            res.out_n[i] = 1
            o = int(cap_off[i])
            if int(cap_off[i + 1]) - o == 0:
                fl |= _abi.F_ERR_CAPACITY
            else:
                res.out_tag[o], res.out_tok[o] = tag, ts
            wins = [c[2] for c in cands if (c[0], c[1]) == (ts, tag)]
            cls["tie"] = tie
            cls["base_wins"] = -1 in wins
            step = opi(D)
            tail = ((b - a) // step) * step
            cls["last_chunk"] = (b - a) % step != 0 and any(p >= tail for p in wins)
        else:
            cls["empty"] = True
        res.flags[i] = fl
    return res, incl_all, info


# ------------------------------------------------------------------ cases
def clocks_case(seed, D, lens, *, sparse=False, warm=0.0, txid=0.0, corrupt=0.0,
                identity=True):
    """synth.random_case's clocks for explicit key lengths: per key a random
    walk, a read snapshot that includes a prefix-ish subset, optionally a base
    snapshot time and a reading txid.  Sparse: DCs missing from op clocks, R
    and SCT (the absence rates shrink with D, so wide clocks still include)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    K, W = len(lens), n_words(D)
    key_off = np.zeros(K + 1, np.uint64)
    key_off[1:] = np.cumsum(lens)
    E = int(key_off[-1])
    oc, op_id, txids = np.zeros((E, D), np.uint64), np.zeros(E, np.uint32), np.zeros(E, np.uint64)
    R, sct = np.zeros((K, D), np.uint64), np.zeros((K, D), np.uint64)
    sct_ign, rtx = np.ones(K, np.uint8), np.zeros(K, np.uint64)
    for k in range(K):
        a, b = int(key_off[k]), int(key_off[k + 1])
        clk = 1_000_000 + rng.integers(0, 50, D)
        ids = np.sort(rng.choice(np.arange(1, 4 * (b - a) + 2), b - a, replace=False)) \
            if b > a else []
        snaps = []
        for j, e in enumerate(range(a, b)):
            c = rng.integers(0, D)
            clk = clk.copy()
            clk[c] += rng.integers(1, 20)
            row = clk - rng.integers(0, 30, D)
            row[c] = clk[c]
            oc[e], op_id[e], txids[e] = row, ids[j], rng.integers(1, 6)
            snaps.append(row)
        cut = rng.integers(0, (b - a) + 1)
        Rk = (np.max(np.array(snaps[:cut]), axis=0) if cut else clk - 10) + \
            rng.integers(-4 if D <= 16 else 0, 16, D)
        R[k] = np.maximum(Rk, 1)
        if rng.random() < warm:
            c2 = rng.integers(0, cut + 1)
            sct[k] = (np.max(np.array(snaps[:c2]), axis=0) if c2 else clk - 40) + \
                rng.integers(-5, 6, D)
            sct_ign[k] = 0
        if rng.random() < txid:
            rtx[k] = rng.integers(1, 6)
    log = EncodedLog(crdt_type=LWW, n_dcs=D, key_off=key_off, key_type=np.full(K, LWW, np.uint8),
                     oc=oc, oc_mask=None, op_id=op_id, txid=txids)
    log.key_type[rng.random(K) < corrupt] = _abi.TYPE_MIXED
    Rm, Sm = np.zeros((K, W), np.uint64), np.zeros((K, W), np.uint64)
    if sparse:
        log.oc_mask, _ = _mask_rows(rng, E, D, 0.25)
        for e in range(E):  # the commit DC (max entry) is always present in OpSSCommit
            d = int(np.argmax(oc[e]))
            log.oc_mask[e, d >> 6] |= np.uint64(1 << (d & 63))
        Rm, _ = _mask_rows(rng, K, D, min(0.03, 0.25 / D))
        Sm, _ = _mask_rows(rng, K, D, 0.2)
    keys = np.arange(K, dtype=np.uint64)
    if not identity:
        keys = rng.permutation(K).astype(np.uint64)
        R, Rm, sct, Sm, sct_ign, rtx = R[keys], Rm[keys], sct[keys], Sm[keys], sct_ign[keys], \
            rtx[keys]
    req = EncodedRead(n_dcs=D, req_type=LWW, keys=keys, R=np.ascontiguousarray(R),
                      R_mask=np.ascontiguousarray(Rm), sct=np.ascontiguousarray(sct),
                      sct_mask=np.ascontiguousarray(Sm), sct_ignore=sct_ign, txid=rtx,
                      base_value=np.zeros(K, np.int64), base_off=np.zeros(K + 1, np.uint64),
                      base_tag=np.zeros(0, np.uint32), base_tok=np.zeros(0, np.uint64))
    return log, req


TS_EDGE = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1]
TAG_EDGE = [0, 1, 0xFFFFFFFE]


def attach_lww(log, req, seed, *, invalid=0.0, base=0.0, n_vals=3, ts_max=8, domain=False):
    """Give a log of clocks its register_lww entries and the requests their
    base pairs.  Timestamps come from a small range, so ties, base wins and an
    excluded newest assign are all common; `invalid`: the share of keys a third
    of whose entries carry AGN_TAG_INVALID; `domain`: timestamps and tags from
    the edges of their domains (TS_EDGE, TAG_EDGE) instead."""
    rng = np.random.default_rng(seed + 7919)
    K, E = log.n_keys, log.n_entries
    if domain:
        tag = rng.choice(np.array(TAG_EDGE, np.uint32), E)
        ts = rng.choice(np.array(TS_EDGE, np.uint64), E).astype(np.uint64)
    else:
        tag = rng.integers(0, n_vals, E).astype(np.uint32)
        ts = rng.integers(1, ts_max + 1, E).astype(np.uint64)
    for k in np.nonzero(rng.random(K) < invalid)[0]:
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        tag[a:b][rng.random(b - a) < 0.34] = _abi.TAG_INVALID
    log.crdt_type = LWW
    log.key_type = np.where(log.key_type == _abi.TYPE_MIXED, log.key_type, LWW).astype(np.uint8)
    log.eff = None
    log.tag, log.add_tok = tag, ts
    log.rem_off, log.rem_tok = np.zeros(E + 1, np.uint32), np.zeros(1, np.uint64)
    n = req.n_req
    boff, btag, btok = np.zeros(n + 1, np.uint64), [], []
    for i in range(n):
        if rng.random() < base:
            if domain:
                btag.append(int(rng.choice(TAG_EDGE)))
                btok.append(int(rng.choice(np.array(TS_EDGE, np.uint64))))
            else:
                btag.append(int(rng.integers(0, n_vals)))
                btok.append(int(rng.integers(1, ts_max + 3)))
        boff[i + 1] = len(btag)
    req.req_type = LWW
    req.base_off, req.base_tag, req.base_tok = boff, np.array(btag, np.uint32), \
        np.array(btok, np.uint64)
    return log, req, state_capacity(log, req)


LENS = [0, 1, 63, 64, 65, 129]           # chunk edges of the one-lane-per-op shapes
LENS_WIDE = [0, 1, 2, 3, 63, 64, 65, 129]  # + 2, 3: a chunk is two ops at D = 256
DS = [1, 3, 8, 9, 16, 33, 64, 129, 256]    # every LPO shape
GPU_REPS = 3                                # keys of each length in a device batch


def lww_case(seed, D, lens=None, reps=6, **kw):
    """A register_lww batch: clocks_case over `reps` keys of each length, then
    attach_lww.  kw: sparse, warm, txid, corrupt, identity | invalid, base,
    domain, ts_max, n_vals."""
    lens = (LENS_WIDE if D == 256 else LENS) if lens is None else lens
    ck = {x: kw.pop(x) for x in ("sparse", "warm", "txid", "corrupt", "identity") if x in kw}
    log, req = clocks_case(seed, D, list(lens) * reps, **ck)
    return attach_lww(log, req, seed, **kw)


def gpu_cases():
    """(id, seed, D, sparse, kwargs): what tests/test_lww.py runs through
    agn_materialize and tests/test_lww_cpu.py checks the reach of."""
    out = []
    for j, D in enumerate(DS):
        out.append((f"D{D}-dense-cold", 100 + j, D, False,
                    dict(invalid=0.15, base=0.4, txid=0.3, corrupt=0.05)))
        out.append((f"D{D}-masked-warm", 200 + j, D, True,
                    dict(sparse=True, warm=0.6, invalid=0.15, base=0.4, txid=0.3,
                         identity=False)))
    out.append(("D8-dense-warm-perm", 300, 8, False,
                dict(warm=0.7, base=0.5, txid=0.5, identity=False, invalid=0.1)))
    out.append(("D3-masked-cold", 301, 3, True, dict(sparse=True, base=0.3, invalid=0.1)))
    short = [0, 1, 1, 2, 2, 3, 63, 64, 65, 129]   # few candidates: every edge value wins somewhere
    out.append(("D4-domain", 302, 4, False, dict(domain=True, base=0.5, warm=0.3, lens=short)))
    out.append(("D33-domain-masked", 303, 33, True,
                dict(sparse=True, domain=True, base=0.5, lens=short)))
    return out


def as_state_refs(req):
    """The same bases through AGN_SS_STATE references (base_off NULL): the
    pairs sit in an arena with a gap in front of each, base_value names them."""
    n = req.n_req
    bv = np.zeros(n, np.int64)
    tags, toks = [0xDEAD], [0xDEAD]
    for i in range(n):
        o0, o1 = int(req.base_off[i]), int(req.base_off[i + 1])
        if o1 > o0:
            bv[i] = _abi.ss_state(len(tags), 1)
            tags += [int(req.base_tag[o0]), 0xBEEF]
            toks += [int(req.base_tok[o0]), 0xBEEF]
        else:
            bv[i] = _abi.ss_state(len(tags), 0)
    return EncodedRead(n_dcs=req.n_dcs, req_type=req.req_type, keys=req.keys, R=req.R,
                       R_mask=req.R_mask, sct=req.sct, sct_mask=req.sct_mask,
                       sct_ignore=req.sct_ignore, txid=req.txid, base_value=bv,
                       base_off=np.zeros(0, np.uint64), base_tag=np.array(tags, np.uint32),
                       base_tok=np.array(toks, np.uint64))


def compare_lww(D, got, want, sparse, n):
    """synth.compare for the type, plus what it leaves out: out_n under
    AGN_F_ERR_CAPACITY (1: the room to come back with) and under
    AGN_F_ERR_CORRUPTED (0)."""
    from synth import compare
    bad = compare(LWW, D, got, want, sparse, n)
    for i in range(n):
        f = int(want.flags[i])
        if f & (_abi.F_ERR_CAPACITY | _abi.F_ERR_CORRUPTED) and \
                int(got.out_n[i]) != int(want.out_n[i]):
            bad.append((i, "out_n", int(got.out_n[i]), int(want.out_n[i])))
    return bad


# ------------------------------------------------------------------ known answers
LWW_TYPE = "antidote_crdt_register_lww"


def kats():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "lww_kats.json")) as f:
        return json.load(f)["cases"]


def _val(s):
    return s.encode("latin1")


def kat_read(c):
    """(TxId, MinSnapshotTime, #snapshot_get_response{}) of a known answer, and
    the state {Ts, Value} it must give."""
    from antidote_amd.records import (IGNORE, ClocksiPayload, MaterializedSnapshot,
                                      SnapshotGetResponse)
    ops = [(i + 1, ClocksiPayload("k", LWW_TYPE, (ts, _val(v)), {"dc1": t - 1}, ("dc1", t), None))
           for i, (t, ts, v) in enumerate(c["ops"])]
    base = (0, b"") if c["base"] is None else (c["base"][0], _val(c["base"][1]))
    sct = IGNORE if c["sct"] is None else {"dc1": c["sct"]}
    resp = SnapshotGetResponse(ops[::-1], len(ops), MaterializedSnapshot(0, base), sct, True)
    return IGNORE, {"dc1": c["read"]}, resp, (c["state"][0], _val(c["state"][1]))
