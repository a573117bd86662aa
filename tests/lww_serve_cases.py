"""Constructed cases for the fused register_lww cached read (k_lww_serve):
helper, no tests.  Nothing is drawn: building a case twice gives identical
arrays.

  script_entry / lww_steps   the (ts, tag) entries behind cache_edges.scripts'
                             scripted effects, for the batcher tests
  family(D)                  one agn_read_cached batch of constructed keys:
                             the log, a prebuilt cache with its state arena,
                             one request per key, and per key the edge it was
                             built for (`expect`), which
                             tests/test_lww_serve_cpu.py checks on the host
                             model and the C oracle.
"""
from __future__ import annotations

import numpy as np

from antidote_amd import _abi
from antidote_amd.encode import EncodedLog, EncodedRead
from lww_model import LWW, opi
from test_ss_states import LWW_TS_EDGE

THRESHOLD, KEEP, MIN_OPS = _abi.SNAPSHOT_THRESHOLD, _abi.SNAPSHOT_MIN, _abi.MIN_OP_STORE_SS
SLOTS = THRESHOLD
TS_POOL = [5, 6, 7, 8] + LWW_TS_EDGE      # a window of 4 values plus the domain's edges
N_TAGS = 5


def script_entry(t, bad=False):
    """The (ts, tag) of a script's op number t: both walk their small pools at
    different strides, so equal timestamps under different tags (ties), and
    the edge timestamps, occur within every few ops."""
    if bad:
        return TS_POOL[t % len(TS_POOL)], _abi.TAG_INVALID
    return TS_POOL[(t // 2 + 4 * (t // 7)) % len(TS_POOL)], (2 * t + t // 3) % N_TAGS


def lww_steps(script):
    """cache_edges.Script steps with every scripted effect replaced by its
    entry: ("append", [(oc row, (ts, tag), DC set or None)]) | the read steps."""
    out, t = [], 0
    for st in script.steps:
        if st[0] != "append":
            out.append(st)
            continue
        ops = []
        for oc, eff, mk in st[1]:
            ops.append((oc, script_entry(t, eff == _abi.EFFECT_INVALID), mk))
            t += 1
        out.append(("append", ops))
    return out


# ------------------------------------------------------------------ agn_read_cached family
LOOKS = ("new", "hit0", "hit8", "log")
# (cached entries, hole - head.last_op, GC read) of the keys that hit slot 0
HIT0_STORES = ((2, 5, 0), (2, 4, 0), (3, 5, 1), (8, 5, 0), (9, 5, 0), (4, 4, 1), (1, 5, 1))
C0 = 100          # every clock column's floor
TOP = 1000        # the winner's timestamp where a key places one


class Family:
    pass


def lengths(D):
    o = opi(D)
    return (0, 1, o - 1, o, o + 1, 2 * o - 1, 2 * o, 2 * o + 1)


def family(D):
    """One key per spec.  Key k's ops commit at column c = k mod D: op p (from
    0) has clock C0 everywhere and C0 + p + 1 at c.  `prev` leading ops belong
    to the hit snapshot (SCT[c] = C0 + prev), the read includes ops up to
    `upto` (R[c] = C0 + upto, R = C0 + 500 elsewhere)."""
    o = opi(D)
    specs = []

    def add(name, n, ts, tag, look="hit0", ncache=2, gap=MIN_OPS, gc=0, prev=0, upto=None,
            base=None, cap=4, corrupt=False, own_tx=False, **expect):
        if look == "new":
            ncache, base = 0, None
        if look == "hit8":
            ncache = 9
        assert len(ts) == n and len(tag) == n, name
        specs.append(dict(name=name, n=n, ts=list(ts), tag=list(tag), look=look, ncache=ncache,
                          gap=gap, gc=gc, prev=prev, upto=n if upto is None else upto, base=base,
                          cap=cap, corrupt=corrupt, own_tx=own_tx, expect=expect))

    def flat(n, at=None, top=TOP):
        """Timestamps 10, 11, ... with `top` at position `at`; tags cycle."""
        ts = [10 + (p % 7) for p in range(n)]
        if at is not None:
            ts[at] = top
        return ts, [p % N_TAGS for p in range(n)]

    # key lengths x winner positions, the cache states / GC / store recipes in rotation
    x = 0
    for n in lengths(D):
        for at in sorted({p for p in (0, o - 1, o, n - 1) if 0 <= p < n}) or [None]:
            ts, tag = flat(n, at)
            for look in LOOKS:
                kw = dict(win=at, length=n)
                if look == "hit0":
                    nc, gap, gc = HIT0_STORES[x % len(HIT0_STORES)]
                    add(f"n={n} winner at {at}", n, ts, tag, look, nc, gap, gc,
                        base=(1, 3), **kw)
                elif look == "log":
                    add(f"n={n} winner at {at}", n, ts, tag, look, (1, 3, 9)[x % 3],
                        gc=(x // 4) % 2, **kw)
                else:
                    add(f"n={n} winner at {at}", n, ts, tag, look, gc=(x // 4) % 2,
                        base=(2, 4), **kw)
                x += 1
    # ties
    n = 2 * o + 1
    for gc in (0, 1):
        for a, b, nm in ((1, 2, "same chunk"), (1, o + 1, "another chunk")):
            if b >= n or a == b:
                continue
            for ta, tb in ((1, 3), (3, 1)):
                ts, tag = flat(n)
                ts[a] = ts[b] = TOP
                tag[a], tag[b] = ta, tb
                add(f"tie {nm}, tags {ta}/{tb}", n, ts, tag, gc=gc, tie="ops", win_tag=3)
        for bt, ot in ((4, 2), (2, 4)):
            ts, tag = flat(n, o)
            tag[o] = ot
            add(f"tie base/op, base tag {bt}, op tag {ot}", n, ts, tag, gc=gc, base=(bt, TOP),
                tie="base", win_tag=4, base_wins=bt == 4)
        ts, tag = flat(n, o)
        add("the base pair beats every op", n, ts, tag, gc=gc, base=(2, 5 * TOP), base_wins=True,
            win_tag=2)
        ts, tag = flat(n, o)
        add("every op excluded: the base, count 0", n, ts, tag, gc=gc, upto=0, base=(3, 7),
            base_wins=True, count=0, win_tag=3)
        # errors
        ts, tag = flat(o + 1, 0)
        tag[o] = _abi.TAG_INVALID
        add("invalid tag, included", o + 1, ts, tag, gc=gc, err=True)
        add("invalid tag, excluded", o + 1, ts, tag, gc=gc, upto=o, err=False, win=0)
        ts, tag = flat(5, 2)
        add("empty out_off range, key with a state", 5, ts, tag, gc=gc, base=(1, 3), cap=0,
            capacity=True)
        add("key of another type", 5, ts, tag, gc=gc, corrupt=True)
        add("key of another type, absent from the cache", 5, ts, tag, "new", gc=gc, corrupt=True)
        # the reader's own TxId: ops of the hit snapshot come back in
        ts, tag = flat(6, 1)
        add("own TxId: the snapshot's ops included", 6, ts, tag, gc=gc, prev=6, own_tx=True,
            count=6, win=1, prepend=False)
        add("ops of the snapshot, another TxId", 6, ts, tag, gc=gc, prev=6, count=0, base=(1, 3),
            base_wins=True, prepend=False)
    # store outcomes
    for cnt in (4, 5):
        ts, tag = flat(cnt, 0)
        add(f"count {cnt}", cnt, ts, tag, count=cnt, stored=cnt >= MIN_OPS)
        add(f"count {cnt}, GC read", cnt, ts, tag, gc=1, count=cnt, stored=True)
        add(f"count {cnt} on an absent key", cnt, ts, tag, "new", count=cnt, stored=cnt >= MIN_OPS)
    ts, tag = flat(6, 3)
    for gap in (4, 5):
        add(f"op-id gap {gap}", 6, ts, tag, gap=gap, stored=gap >= MIN_OPS)
        add(f"op-id gap {gap}, GC read", 6, ts, tag, gap=gap, gc=1, stored=True)
    add("list 8 -> 9", 6, ts, tag, ncache=8, stored=True, n_after=9, prune=False)
    add("list 9 -> 10: collects, keeps 3", 6, ts, tag, ncache=9, stored=True, n_after=KEEP,
        prune=True)
    add("list 9, GC read", 6, ts, tag, ncache=9, gc=1, stored=True, n_after=KEEP, prune=True)
    add("not prepended: LastOpCt = head, GC read", 6, ts, tag, ncache=4, gc=1, prev=6,
        base=(1, 3), stored=True, prepend=False, n_after=KEEP, prune=True)
    add("hit 8 of 9, count 6", 6, ts, tag, "hit8", base=(1, 3), stored=False)
    # (D = 1: the head is above LastOpCt in the only column, so nothing is prepended)
    add("hit 8 of 9, GC read", 6, ts, tag, "hit8", gc=1, base=(1, 3), stored=D > 1,
        **({} if D > 1 else dict(prepend=False)))
    add("LOG, GC read", 6, ts, tag, "log", gc=1, stored=False)
    if len(specs) % 2 == 0:     # an odd batch
        add("one more", 3, [1, 2, 3], [0, 1, 2], "new")

    K = len(specs)
    lens = np.array([s["n"] for s in specs], np.int64)
    key_off = np.zeros(K + 1, np.uint64)
    key_off[1:] = np.cumsum(lens)
    E = int(key_off[-1])
    oc = np.full((E, D), C0, np.uint64)
    op_id, txid = np.zeros(E, np.uint32), np.zeros(E, np.uint64)
    tag, tok = np.zeros(E, np.uint32), np.zeros(E, np.uint64)
    R = np.full((K, D), C0 + 500, np.uint64)
    rtx, gc = np.zeros(K, np.uint64), np.zeros(K, np.uint8)
    key_type = np.full(K + 3, LWW, np.uint8)
    n_arr = np.zeros(K, np.uint32)
    clock = np.full((K, SLOTS, D), 0xDEAD0000, np.uint64)     # rows past n: nothing reads them
    last_op = np.full((K, SLOTS), -777, np.int64)
    value = np.full((K, SLOTS), _abi.ss_state(0, 0), np.int64)
    st_tag, st_tok = [0xDEAD], [0xDEAD]                        # the arena, a gap in front
    cap_off = np.zeros(K + 1, np.uint64)
    for k, s in enumerate(specs):
        c, a, n = k % D, int(key_off[k]), s["n"]
        id0 = 5 + (k % 3)
        for p in range(n):
            oc[a + p, c] = C0 + p + 1
            op_id[a + p] = id0 + p * (1 + k % 2)        # odd keys: ids two apart
            txid[a + p] = 77 if s["own_tx"] else 1 + p % 5
            tag[a + p], tok[a + p] = s["tag"][p], s["ts"][p]
        R[k, c] = C0 + s["upto"]
        rtx[k] = 77 if s["own_tx"] else 0
        gc[k] = s["gc"]
        if s["corrupt"]:
            key_type[k] = _abi.SET_AW
        cap_off[k + 1] = cap_off[k] + s["cap"]
        # the read's NewLastOp: the op before the first excluded one
        upto = s["upto"]
        hole = (int(op_id[a + upto]) - 1 if upto < n else int(op_id[a + n - 1])) if n else 0
        nc, look = s["ncache"], s["look"]
        n_arr[k] = nc
        sct = np.full(D, C0, np.uint64)
        sct[c] = C0 + s["prev"]
        xc = (c + 1) % D
        f = {"new": None, "hit0": 0, "hit8": 8, "log": -1}[look]
        for j in range(nc):
            if look == "hit0":
                row = sct.copy() if j == 0 else np.full(D, C0 - j, np.uint64)
            elif look == "hit8":
                row = sct.copy()
                if j < 8:
                    row[xc] = R[k, xc] + np.uint64(8 - j)
            else:
                row = sct.copy()
                row[xc] = R[k, xc] + np.uint64(nc - j)
            clock[k, j] = row
            last_op[k, j] = (hole - s["gap"]) - 6 * j
            ref = _abi.ss_state(len(st_tag), 0)
            if s["base"] is not None and j == (f if f is not None and f >= 0 else 0):
                ref = _abi.ss_state(len(st_tag), 1)
                st_tag += [s["base"][0], 0xBEEF]
                st_tok += [s["base"][1], 0xBEEF]
            elif j % 2:     # other slots hold states too: they are released when dropped
                ref = _abi.ss_state(len(st_tag), 1)
                st_tag += [0, 0xBEEF]
                st_tok += [1, 0xBEEF]
            value[k, j] = ref
        s["expect"].update(look=look, f=f, hole=hole)
    fam = Family()
    fam.D, fam.K, fam.S, fam.opi = D, K, SLOTS, o
    fam.names = [f"k={k} {s['look']} n={s['ncache']} gap={s['gap']} gc={s['gc']} {s['name']}"
                 for k, s in enumerate(specs)]
    fam.specs, fam.expect = specs, [s["expect"] for s in specs]
    fam.log = EncodedLog(crdt_type=LWW, n_dcs=D, key_off=key_off, key_type=key_type, oc=oc,
                         oc_mask=None, op_id=op_id, txid=txid)
    fam.log.tag, fam.log.add_tok = tag, tok
    fam.log.rem_off, fam.log.rem_tok = np.zeros(E + 1, np.uint32), np.zeros(1, np.uint64)
    fam.keys = np.arange(K, dtype=np.uint64)
    fam.R, fam.txid, fam.gc, fam.cap_off = R, rtx, gc, cap_off
    fam.cache = {"n": n_arr, "clock": clock, "last_op": last_op, "value": value}
    used = len(st_tag)
    fam.arena_cap = used + K + 64          # room for every store of the batch
    fam.state_tag = np.array(st_tag + [0] * (fam.arena_cap - used), np.uint32)
    fam.state_tok = np.array(st_tok + [0] * (fam.arena_cap - used), np.uint64)
    fam.ctl = np.array([used, 0, 0, 0], np.uint64)
    return fam


def masked(fam):
    """fam with presence masks on its log (oc_mask; D >= 2): two ops in three
    lack one DC other than their own, and hold garbage far above every read
    clock there -- taken for present, the column would exclude the op.  Cache,
    read clocks and results stay dense: the form a masked partition's log has
    over a dense-clock cache."""
    import copy
    D = fam.D
    assert D >= 2
    out = copy.copy(fam)
    log = copy.copy(fam.log)
    E = log.n_entries
    log.oc = fam.log.oc.copy()
    log.oc_mask = np.full((E, 1), (1 << D) - 1, np.uint64)
    for k in range(fam.K):
        a, b, c = int(log.key_off[k]), int(log.key_off[k + 1]), k % D
        for p in range(b - a):
            if p % 3 == 0:
                continue
            d = (c + 1 + p % 2) % D
            if d == c:
                continue
            log.oc_mask[a + p, 0] &= np.uint64(~(1 << d) & ((1 << 64) - 1))
            log.oc[a + p, d] = np.uint64((1 << 61) | (977 * p + d))
    out.log = log
    return out


def orders(K):
    """All K keys (an odd batch), and the first K - 1 in reverse."""
    assert K % 2 == 1
    return [("all", np.arange(K)), ("reversed", np.arange(K - 1)[::-1].copy())]


def requests(fam, order):
    """(EncodedRead with the lookup's outputs still empty, cap_off) of a batch
    of fam's keys in `order`; one output range per request."""
    ks = fam.keys[order]
    n = len(ks)
    caps = np.diff(fam.cap_off.astype(np.int64))[order]
    co = np.zeros(n + 1, np.uint64)
    co[1:] = np.cumsum(caps)
    req = EncodedRead(n_dcs=fam.D, req_type=LWW, keys=np.ascontiguousarray(ks),
                      R=np.ascontiguousarray(fam.R[order]), R_mask=None,
                      sct=np.zeros((n, fam.D), np.uint64), sct_mask=None,
                      sct_ignore=np.zeros(n + 8, np.uint8),
                      txid=np.ascontiguousarray(fam.txid[order]),
                      base_value=np.zeros(n, np.int64), base_off=np.zeros(n + 1, np.uint64),
                      base_tag=np.zeros(0, np.uint32), base_tok=np.zeros(0, np.uint64))
    return req, co, np.ascontiguousarray(fam.gc[order])


def decode_states(value, n, state_tag, state_tok):
    """Every live slot's state through its AGN_SS_STATE reference:
    {(key, slot): (tag, ts) or None}."""
    out = {}
    for k in range(len(n)):
        for j in range(int(n[k])):
            start, pairs = _abi.ss_state_unpack(int(value[k, j]))
            assert pairs <= 1, (k, j, pairs)
            out[(k, j)] = (int(state_tag[start]), int(state_tok[start])) if pairs else None
    return out
