"""antidote_crdt_counter_b on the host: a numpy restatement of the per-key
snapshot filter (filter.hpp) plus the type's fold, and
the cases the CPU and GPU tests share.

The fold (include/antidote_gpu.h, AGN_COUNTER_B): the state is a set of
(slot, sum) pairs.  A slot is present iff a base pair or an included entry
with a valid tag names it; its sum is the base sums (duplicate base tags add
up) plus the included amounts mod 2^64.  Result pairs come out in ascending
tag order.  More than AGN_BCOUNTER_SLOTS_MAX distinct slots: AGN_F_ERR_CAPACITY
with out_n = 0; room smaller than the state: the flag with out_n = the size;
an included invalid entry: AGN_F_ERR_UNEXPECTED alone.  Everything but the
permissions/1 outcomes of the two bcountermgr_SUITEs is parity-unpinned
(antidote_crdt 0.1.2 is restated, not held): the model is this project's
statement of the type, not the reference's.
"""
from __future__ import annotations

import numpy as np

from antidote_amd import _abi
from antidote_amd.encode import (EncodedLog, EncodedRead, alloc_result, n_words,
                                 state_capacity)
from lww_model import _bits, _pack, clocks_case, opi

BC = _abi.COUNTER_B
NO_POS = 0xFFFFFFFF
SLOTS_MAX = _abi.BCOUNTER_SLOTS_MAX
M64 = (1 << 64) - 1
I64_MIN = 1 << 63           # INT64_MIN's bits
AMT_EDGE = [0, M64, I64_MIN, 1, (1 << 63) - 1, I64_MIN + 1]   # 0, -1, INT64_MIN, 1, MAX, MIN+1


def i64(bits):
    bits = int(bits) & M64
    return bits - (1 << 64) if bits >> 63 else bits


def model(log, req, sparse, cap_off, bases=None):
    """Every result field of a counter_b batch, the per-entry inclusion of
    each request, and what the reach test classifies.  `sparse`: the masks of
    `req` are passed (read_struct(sparse)); log.oc_mask None reads as dense.
    `bases`: per request a list of (tag, tok) pairs, instead of req.base_off."""
    D, n = log.n_dcs, req.n_req
    res = alloc_result(n, D, sparse=True, cap_off=cap_off)
    res.err_pos[:] = NO_POS
    full, none = np.ones(D, bool), np.zeros(D, bool)
    incl_all, info = [], []
    for i in range(n):
        k = int(req.keys[i])
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        cls = dict(corrupt=False, err=False, err_at=None, invalid_excluded=False, overflow=False,
                   overflow_then_err=False, no_room=False, n_slots=0, base_only=False,
                   log_only=False, both=False, excluded_only=False, zero_sum=False, wrapped=False,
                   dup_base=False, chunk_slots=0, empty=False, amounts=set(), n=b - a)
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
        # ---- the fold: a dict slot -> sum, in arrival order (base first)
        if bases is not None:
            base = list(bases[i] or [])
        else:
            o0, o1 = int(req.base_off[i]), int(req.base_off[i + 1])
            base = [(int(req.base_tag[x]), int(req.base_tok[x])) for x in range(o0, o1)]
        st: dict = {}
        true_sum: dict = {}
        for t, v in base:
            st[t] = (st.get(t, 0) + v) & M64
            true_sum[t] = true_sum.get(t, 0) + i64(v)
        base_tags = {t for t, _ in base}
        cls["dup_base"] = len(base_tags) < len(base)
        log_tags, excl_tags = set(), set()
        over_at = -1 if len(st) <= SLOTS_MAX else 0
        step = opi(D)
        for p in range(b - a):
            t, v = int(log.tag[a + p]), int(log.add_tok[a + p])
            if t == _abi.TAG_INVALID:
                continue
            if not incl[p]:
                excl_tags.add(t)
                continue
            log_tags.add(t)
            cls["amounts"].add(v)
            st[t] = (st.get(t, 0) + v) & M64
            true_sum[t] = true_sum.get(t, 0) + i64(v)
            if over_at < 0 and len(st) > SLOTS_MAX:
                over_at = p
        for c0 in range(0, b - a, step):
            cls["chunk_slots"] = max(cls["chunk_slots"], len(
                {int(log.tag[a + p]) for p in range(c0, min(c0 + step, b - a))
                 if incl[p] and int(log.tag[a + p]) != _abi.TAG_INVALID}))
        cls["invalid_excluded"] = first_err < 0 and any(
            int(log.tag[a + p]) == _abi.TAG_INVALID for p in range(b - a))
        cls["n_slots"] = len(st)
        cls["base_only"] = bool(base_tags - log_tags)
        cls["log_only"] = bool(log_tags - base_tags)
        cls["both"] = bool(log_tags & base_tags)
        cls["excluded_only"] = bool(excl_tags - log_tags - base_tags)
        cls["zero_sum"] = any(v == 0 for v in st.values())
        cls["wrapped"] = any(i64(st[t]) != true_sum[t] for t in st)
        cls["empty"] = not st
        if first_err >= 0:
            fl |= _abi.F_ERR_UNEXPECTED
            res.err_pos[i] = a + first_err
            cls["err"], cls["err_at"] = True, first_err
            cls["overflow_then_err"] = 0 <= over_at < first_err
        elif len(st) > SLOTS_MAX:
            fl |= _abi.F_ERR_CAPACITY       # the engine's limit: out_n = 0
            cls["overflow"] = True
        else:
            res.out_n[i] = len(st)
            o = int(cap_off[i])
            if int(cap_off[i + 1]) - o < len(st):
                fl |= _abi.F_ERR_CAPACITY   # out_n = the room to come back with
                cls["no_room"] = True
            else:
                for j, t in enumerate(sorted(st)):
                    res.out_tag[o + j], res.out_tok[o + j] = t, st[t]
        res.flags[i] = fl
    return res, incl_all, info


# ------------------------------------------------------------------ cases
def attach_bc(log, req, seed, *, invalid=0.0, base=0.0, n_slots=4, own=False, dup_base=False,
              domain=False, n_base=3):
    """Give a log of clocks its counter_b entries and the requests their base
    pairs.  Slots come from `n_slots` ids per key (own: entry p names slot
    p mod n_slots, so a chunk's lanes all differ); amounts are small and
    signed, 0 included, with a +a / -a pair planted now and then so that sums
    of 0 occur; `domain`: amounts from AMT_EDGE, tags from the edges of u32;
    `invalid`: the share of keys a third of whose entries carry
    AGN_TAG_INVALID; `base`: the share of requests with up to n_base base
    pairs, drawn from n_slots + 2 ids (so some are in the base only), with a
    repeated tag when dup_base."""
    rng = np.random.default_rng(seed + 104729)
    K, E = log.n_keys, log.n_entries
    pos = np.concatenate([np.arange(int(b - a)) for a, b in
                          zip(log.key_off[:-1], log.key_off[1:])] + [np.zeros(0, np.int64)])
    ids = np.array([0, 1, 0xFFFFFFFE, 7, 0x80000000, 2], np.uint32)
    if own:
        tag = (pos % n_slots).astype(np.uint32)
    else:
        tag = rng.integers(0, n_slots, E).astype(np.uint32)
    if domain:
        tag = ids[tag % len(ids)]
        amt = rng.choice(np.array(AMT_EDGE, np.uint64), E).astype(np.uint64)
    else:
        amt = rng.integers(-5, 6, E).astype(np.int64)
        flip = np.nonzero((rng.random(E) < 0.3) & (pos > 0))[0]
        same = tag[flip] == tag[flip - 1]
        amt[flip[same]] = -amt[flip[same] - 1]
        amt = amt.astype(np.uint64)
    for k in np.nonzero(rng.random(K) < invalid)[0]:
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        tag[a:b][rng.random(b - a) < 0.34] = _abi.TAG_INVALID
    log.crdt_type = BC
    log.key_type = np.where(log.key_type == _abi.TYPE_MIXED, log.key_type, BC).astype(np.uint8)
    log.eff = None
    log.tag, log.add_tok = tag, amt
    log.rem_off, log.rem_tok = np.zeros(E + 1, np.uint32), np.zeros(1, np.uint64)
    n = req.n_req
    boff, btag, btok = np.zeros(n + 1, np.uint64), [], []
    for i in range(n):
        if rng.random() < base:
            nb = int(rng.integers(1, n_base + 1))
            ts = rng.choice(np.arange(min(n_slots, 250) + 2), min(nb, n_slots + 2), replace=False)
            ts = [int(x) for x in ts]
            if dup_base:
                ts.append(ts[0])
            for t in ts:
                btag.append(int(ids[t % len(ids)]) if domain else t)
                btok.append(int(rng.choice(np.array(AMT_EDGE, np.uint64))) if domain
                            else int(rng.integers(-5, 6)) & M64)
        boff[i + 1] = len(btag)
    req.req_type = BC
    req.base_off, req.base_tag, req.base_tok = boff, np.array(btag, np.uint32), \
        np.array(btok, np.uint64)
    return log, req, state_capacity(log, req)


LENS = [0, 1, 63, 64, 65, 128, 129]         # chunk edges of the one-lane-per-op shapes
DS = [1, 3, 8, 9, 16, 33, 64, 65, 130]      # every LPO shape
GPU_REPS = 2                                 # keys of each length in a device batch


def bc_case(seed, D, lens=None, reps=6, **kw):
    """A counter_b batch: clocks_case over `reps` keys of each length, then
    attach_bc.  kw: sparse, warm, txid, corrupt, identity | attach_bc's."""
    lens = LENS if lens is None else lens
    ck = {x: kw.pop(x) for x in ("sparse", "warm", "txid", "corrupt", "identity") if x in kw}
    log, req = clocks_case(seed, D, list(lens) * reps, **ck)
    req.req_type = BC
    return attach_bc(log, req, seed, **kw)


def built_case(D, specs, n_copies=1):
    """A batch with every inclusion decided by hand.  specs: per key a dict
    ops=[(tag, amount bits, included)], base=[(tag, tok)], room=None | int
    (the request's room instead of the capacity bound), mistyped=bool.  Dense,
    cold: entry p's clock is 100 + p in every column against R = 10^6, an
    excluded entry's column 0 is 2 * 10^6.  The whole list is repeated
    n_copies times (so a batch spans more than one block)."""
    specs = list(specs) * n_copies
    K = len(specs)
    lens = [len(s["ops"]) for s in specs]
    key_off = np.zeros(K + 1, np.uint64)
    key_off[1:] = np.cumsum(lens)
    E = int(key_off[-1])
    oc, op_id = np.zeros((E, D), np.uint64), np.zeros(E, np.uint32)
    tag, amt = np.zeros(E, np.uint32), np.zeros(E, np.uint64)
    boff, btag, btok = [0], [], []
    e = 0
    for s in specs:
        for p, (t, v, inc) in enumerate(s["ops"]):
            oc[e] = 100 + p
            if not inc:
                oc[e, 0] = 2_000_000
            op_id[e], tag[e], amt[e] = 2 * p + 1, t, int(v) & M64
            e += 1
        for t, v in s.get("base", []):
            btag.append(t)
            btok.append(int(v) & M64)
        boff.append(len(btag))
    kt = np.array([_abi.SET_AW if s.get("mistyped") else BC for s in specs], np.uint8)
    log = EncodedLog(crdt_type=BC, n_dcs=D, key_off=key_off, key_type=kt, oc=oc, oc_mask=None,
                     op_id=op_id, txid=np.zeros(E, np.uint64), tag=tag, add_tok=amt,
                     rem_off=np.zeros(E + 1, np.uint32), rem_tok=np.zeros(1, np.uint64))
    W = n_words(D)
    req = EncodedRead(n_dcs=D, req_type=BC, keys=np.arange(K, dtype=np.uint64),
                      R=np.full((K, D), 1_000_000, np.uint64), R_mask=np.zeros((K, W), np.uint64),
                      sct=np.zeros((K, D), np.uint64), sct_mask=np.zeros((K, W), np.uint64),
                      sct_ignore=np.ones(K, np.uint8), txid=np.zeros(K, np.uint64),
                      base_value=np.zeros(K, np.int64), base_off=np.array(boff, np.uint64),
                      base_tag=np.array(btag, np.uint32), base_tok=np.array(btok, np.uint64))
    room = np.diff(state_capacity(log, req).astype(np.int64))
    for i, s in enumerate(specs):
        if s.get("room") is not None:
            room[i] = s["room"]
    cap = np.concatenate([[0], np.cumsum(room)]).astype(np.uint64)
    return log, req, cap


def _distinct(n, first=1000, amount=1, inc=True):
    return [(first + p, amount, inc) for p in range(n)]


def slot_specs():
    """The distinct-slot counts of the issue: 1, 2, 64, 65, and 255 / 256 / 257
    from the log alone and with base pairs making up the count."""
    sp = [dict(ops=[(7, 3, True)] * 64),                                  # 1: all lanes one slot
          dict(ops=[(7, 3, True)] * 129),
          dict(ops=[(p & 1, p, True) for p in range(130)]),               # 2
          dict(ops=_distinct(64)),                                         # 64: every lane its own
          dict(ops=_distinct(65)),                                         # 65
          dict(ops=_distinct(64) + _distinct(64, amount=-1) + [(1000, 5, True)])]
    for total in (255, 256, 257):
        sp.append(dict(ops=_distinct(total)))                              # the log alone
        sp.append(dict(ops=_distinct(129), base=[(5000 + x, x) for x in range(total - 129)]))
        sp.append(dict(ops=_distinct(57, first=50), base=[(50 + x, -x) for x in range(200)]
                       + [(9000 + x, 1) for x in range(total - 200)]))    # the log's 57 are in the base
    # in the base only / the log only / both; excluded-only: absent; sums of 0; duplicates
    sp.append(dict(ops=[(1, 5, True), (2, 6, True), (3, 7, False), (2, -6, True)],
                   base=[(0, 9), (1, -5), (0, 1), (4, 0)]))
    sp.append(dict(ops=[], base=[(3, 1), (3, 2), (3, 3), (1, 0)]))
    sp.append(dict(ops=[], base=[]))
    # sums wrapping past +-2^63; amounts 0, -1, INT64_MIN
    big = (1 << 63) - 1
    sp.append(dict(ops=[(1, big, True), (1, 1, True), (2, I64_MIN, True), (2, -1, True),
                        (3, 0, True), (4, -1, True), (5, I64_MIN, True), (5, I64_MIN, True)],
                   base=[(1, big), (6, I64_MIN)]))
    return sp


def error_specs():
    """Invalid entries included at 0 / 63 / 64 / n - 1 and excluded; after the
    overflow point; room 0 and one short; a key_type mismatch."""
    INV = _abi.TAG_INVALID
    n = 130
    sp = []
    for at in (0, 63, 64, n - 1):
        ops = [(p % 3, 1, True) for p in range(n)]
        ops[at] = (INV, 0, True)
        sp.append(dict(ops=ops))
    ops = [(p % 3, 1, True) for p in range(n)]
    ops[5] = ops[70] = (INV, 0, True)                                      # the oldest is named
    sp.append(dict(ops=ops))
    ops = [(p % 3, 1, True) for p in range(n)]
    ops[0] = ops[64] = ops[n - 1] = (INV, 9, False)                        # excluded: no error
    sp.append(dict(ops=ops))
    sp.append(dict(ops=_distinct(300) + [(INV, 0, True)] + _distinct(3)))  # overflow, then invalid
    sp.append(dict(ops=_distinct(300) + [(INV, 0, False)]))                # overflow alone
    sp.append(dict(ops=_distinct(70), room=0))
    sp.append(dict(ops=_distinct(70), room=69))
    sp.append(dict(ops=[(1, 1, True)], base=[(2, 2)], room=1))
    sp.append(dict(ops=_distinct(70), room=70))
    sp.append(dict(ops=_distinct(5), mistyped=True))
    sp.append(dict(ops=[], mistyped=True))                                 # an empty key is never corrupt
    return sp


def gpu_cases():
    """(id, kind, args): what tests/test_bcounter.py runs through
    agn_materialize and tests/test_bcounter_cpu.py checks the reach of.
    kind "rand": (seed, D, sparse, kwargs) for bc_case; kind "built":
    (D, specs, copies) for built_case."""
    out = []
    for j, D in enumerate(DS):
        out.append((f"D{D}-dense-cold", "rand",
                    (100 + j, D, False, dict(invalid=0.15, base=0.5, txid=0.3, corrupt=0.05,
                                             n_slots=3 + j % 3))))
        out.append((f"D{D}-masked-warm", "rand",
                    (200 + j, D, True, dict(sparse=True, warm=0.6, invalid=0.15, base=0.5,
                                            txid=0.3, identity=False, n_slots=2 + j % 4,
                                            dup_base=True))))
    out.append(("D8-dense-warm-perm", "rand",
                (300, 8, False, dict(warm=0.7, base=0.5, txid=0.5, identity=False, invalid=0.1))))
    out.append(("D3-masked-cold", "rand", (301, 3, True, dict(sparse=True, base=0.3, invalid=0.1))))
    out.append(("D8-own-slots", "rand", (302, 8, False, dict(own=True, n_slots=70, base=0.5,
                                                             n_base=6))))
    out.append(("D16-own-slots-masked", "rand",
                (303, 16, True, dict(sparse=True, own=True, n_slots=40, warm=0.4, base=0.5))))
    out.append(("D4-domain", "rand", (304, 4, False, dict(domain=True, n_slots=6, base=0.5,
                                                          warm=0.3, dup_base=True))))
    out.append(("D33-domain-masked", "rand",
                (305, 33, True, dict(sparse=True, domain=True, n_slots=6, base=0.5))))
    out.append(("D8-one-request", "rand", (306, 8, False, dict(lens=[65], reps=1, base=1.0))))
    out.append(("D5-five-requests", "rand", (307, 5, False, dict(lens=[0, 1, 64, 65, 129], reps=1,
                                                                 base=0.5, identity=False))))
    out.append(("D8-repeated-keys", "rand", (308, 8, False, dict(base=0.5, repeat=True))))
    out.append(("D8-slots", "built", (8, slot_specs(), 1)))
    out.append(("D9-slots", "built", (9, slot_specs(), 1)))
    out.append(("D8-errors", "built", (8, error_specs(), 2)))
    out.append(("D65-errors", "built", (65, error_specs(), 1)))
    return out


def has_bases(case):
    """Does a gpu_cases() row give some request base pairs?"""
    _id, kind, args = case
    if kind == "built":
        return any(s.get("base") for s in args[1])
    return args[3].get("base", 0.0) > 0.0


def make_case(case):
    """(log, req, cap, sparse, D) of one gpu_cases() row."""
    _id, kind, args = case
    if kind == "built":
        D, specs, copies = args
        log, req, cap = built_case(D, specs, copies)
        return log, req, cap, False, D
    seed, D, sparse, kw = args
    kw = dict(kw)
    repeat = kw.pop("repeat", False)
    reps = kw.pop("reps", GPU_REPS)
    log, req, cap = bc_case(seed, D, reps=reps, **kw)
    if repeat:  # every key read twice, the second time under its neighbour's snapshot
        req = repeat_keys(req)
        cap = state_capacity(log, req)
    return log, req, cap, sparse, D


def repeat_keys(req):
    n = req.n_req
    idx = np.concatenate([np.arange(n), np.arange(n)])
    rot = np.concatenate([np.arange(n), np.roll(np.arange(n), 1)])
    nb = np.diff(req.base_off.astype(np.int64))[idx]
    btag = np.concatenate([req.base_tag, req.base_tag])
    btok = np.concatenate([req.base_tok, req.base_tok])
    return EncodedRead(n_dcs=req.n_dcs, req_type=req.req_type, keys=req.keys[idx],
                       R=np.ascontiguousarray(req.R[rot]),
                       R_mask=np.ascontiguousarray(req.R_mask[rot]),
                       sct=np.ascontiguousarray(req.sct[rot]),
                       sct_mask=np.ascontiguousarray(req.sct_mask[rot]),
                       sct_ignore=np.ascontiguousarray(req.sct_ignore[rot]),
                       txid=np.ascontiguousarray(req.txid[idx]),
                       base_value=np.zeros(2 * n, np.int64),
                       base_off=np.concatenate([[0], np.cumsum(nb)]).astype(np.uint64),
                       base_tag=btag, base_tok=btok)


def as_state_refs(req):
    """The same bases through AGN_SS_STATE references (base_off NULL): the
    pairs sit in an arena with a gap in front of each, base_value names them."""
    n = req.n_req
    bv = np.zeros(n, np.int64)
    tags, toks = [0xDEAD], [0xDEAD]
    for i in range(n):
        o0, o1 = int(req.base_off[i]), int(req.base_off[i + 1])
        bv[i] = _abi.ss_state(len(tags), o1 - o0)
        tags += [int(x) for x in req.base_tag[o0:o1]] + [0xBEEF]
        toks += [int(x) for x in req.base_tok[o0:o1]] + [0xBEEF]
    return EncodedRead(n_dcs=req.n_dcs, req_type=req.req_type, keys=req.keys, R=req.R,
                       R_mask=req.R_mask, sct=req.sct, sct_mask=req.sct_mask,
                       sct_ignore=req.sct_ignore, txid=req.txid, base_value=bv,
                       base_off=np.zeros(0, np.uint64), base_tag=np.array(tags, np.uint32),
                       base_tok=np.array(toks, np.uint64))


def compare_bc(D, got, want, sparse, n):
    """synth.compare for the type, plus what it leaves out: out_n under
    AGN_F_ERR_CAPACITY (the size needed, or 0 past the engine's limit) and
    under AGN_F_ERR_CORRUPTED (0)."""
    from synth import compare
    bad = compare(BC, D, got, want, sparse, n)
    for i in range(n):
        f = int(want.flags[i])
        if f & (_abi.F_ERR_CAPACITY | _abi.F_ERR_CORRUPTED) and \
                int(got.out_n[i]) != int(want.out_n[i]):
            bad.append((i, "out_n", int(got.out_n[i]), int(want.out_n[i])))
    return bad


# ------------------------------------------------------------------ known answers
BC_TYPE = "antidote_crdt_counter_b"


def kats():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "bcounter_kats.json")) as f:
        return json.load(f)


def kat_effect(op):
    """A KAT op ["increment", V, Id] / ["decrement", V, Id] / ["transfer", V,
    To, From] as the update/2 effect term."""
    if op[0] == "transfer":
        return (("transfer", op[1], op[2]), op[3])
    return ((op[0], op[1]), op[2])


def update(effect, state):
    """antidote_crdt_counter_b:update/2, literally, on dict states {P, D}."""
    P, D = dict(state[0]), dict(state[1])
    op, ident = effect
    if op[0] == "increment":
        P[(ident, ident)] = P.get((ident, ident), 0) + op[1]
    elif op[0] == "decrement":
        D[ident] = D.get(ident, 0) + op[1]
    elif op[0] == "transfer":
        P[(ident, op[2])] = P.get((ident, op[2]), 0) + op[1]
    else:
        raise ValueError(effect)
    return P, D


def as_orddicts(state):
    from antidote_amd.encode import term_key
    return (sorted(state[0].items(), key=lambda kv: term_key(kv[0])),
            sorted(state[1].items(), key=lambda kv: term_key(kv[0])))


def kat_read(ops):
    """(TxId, MinSnapshotTime, #snapshot_get_response{}) applying every op of
    a known answer to new()."""
    from antidote_amd.records import (IGNORE, ClocksiPayload, MaterializedSnapshot,
                                      SnapshotGetResponse)
    pl = [(i + 1, ClocksiPayload("k", BC_TYPE, kat_effect(op), {"dc1": 2 * i}, ("dc1", 2 * i + 1),
                                 None)) for i, op in enumerate(ops)]
    resp = SnapshotGetResponse(pl[::-1], len(pl), MaterializedSnapshot(0, ([], [])), IGNORE, True)
    return IGNORE, {"dc1": 2 * len(ops) + 1}, resp
