"""Constructed timestamp ties for the fused register_lww cached read
(k_lww_serve) under a value-order table: helper, no tests, nothing drawn.

One family per D, in units of o = lww_model.opi(D) (ops per filter iteration:
position p sits on lane p % o of iteration p // o; the base pair is taken by
lane 0).  The clock layout is lww_serve_cases.family's: key k commits at column
c = k mod D, op p has clock C0 everywhere and C0 + p + 1 at c; `prev` leading
ops lie behind the planted snapshot (SCT[c] = C0 + prev), the read includes ops
up to `upto` (R[c] = C0 + upto, C0 + 500 elsewhere).  Fillers carry tag 0 at
small timestamps, tied entries tags 1..5 (or an unlabelled tag) at TOP.

  keys(D)            the key records: length, {position: tag} at TOP, planted
                     base pair, prev, upto, GC read, cache state, and what the
                     key was built to reach (`reach`)
  family(D, masked)  the records with their per-key arrays (clocks, presence
                     masks, entries, SCT and R rows)
  TABLES             two label tables over tags 0..7, the second the first
                     one's order reversed; value(table, tag) is a binary whose
                     term order is the table's label order
  script(fam, table) the whole run on the host: per key the planted snapshot,
                     the constructed read, (a) a read at a later clock with no
                     new op, (b) one more op at TOP and a read -- each read's
                     every result field from tests/lww_order_model.py's fold
                     over the key's log from the cached snapshot (lookup, store
                     and GC prune restated after cache_dev.hpp), and the served
                     state of the reference transcription's vnode
                     (oracle/py_oracle.py) fed the same ops alone.
"""
from __future__ import annotations

import functools

import numpy as np

import lww_order_model as om
from antidote_amd import _abi
from antidote_amd.encode import EncodedLog, EncodedRead, n_words
from lww_model import LWW, opi
from lww_serve_cases import C0, KEEP, MIN_OPS, THRESHOLD
from oracle import py_oracle as po

TOP = (1 << 40) + 5          # the tied timestamp (above 2^32); every filler is far below
U63 = 1 << 63
UNL_IN, UNL_PAST = 6, 9      # label 0 inside the table | an id past the table's end
TIED = (1, 2, 3, 4, 5)

# Label order, largest first: 3 > 5 > 1 > 2 > 4.  Labels 3 and 5 are >= 2^63 (a
# signed compare puts them below the rest), 1 and 2 differ only above bit 32
# (a low-half compare sees them equal: the larger id, 2, would win), 2 and 4
# differ only below bit 32 (a high-half compare: 4 would win).
_FIRST = {3: U63 + (1 << 40) + 7, 5: U63 + 5, 1: (3 << 32) + 9, 2: (2 << 32) + 9, 4: (2 << 32) + 4}
_RANK = [3, 5, 1, 2, 4]


def _table(of):
    t = np.zeros(8, np.uint64)
    t[0], t[UNL_IN], t[7] = 1 << 20, 0, 77
    for tag, lab in of.items():
        t[tag] = lab
    return t


TABLES = {
    "first": _table(_FIRST),
    # the same labels in the reverse order: 4 > 2 > 1 > 5 > 3
    "reversed": _table({_RANK[4 - r]: _FIRST[_RANK[r]] for r in range(5)}),
}
# tag pairs the first table settles against the id order, and the second
A_PAIRS = [(3, 4), (1, 2), (2, 4)]
B_PAIRS = [(2, 5), (1, 5)]
ALL_PAIRS = A_PAIRS + B_PAIRS


@functools.lru_cache(maxsize=None)
def value(table, tag):
    """The value term behind a tag id under a table: a binary whose bytewise
    (= Erlang term) order is the order of the labels."""
    labs = TABLES[table]
    assert tag < len(labs) and labs[tag], ("no term for an unlabelled tag", tag)
    rank = sorted(int(x) for x in labs if x).index(int(labs[tag]))
    return bytes([ord("a") + rank]) + b"-val"


# ------------------------------------------------------------------ the keys
def keys(D, repeats=True):
    """The key records of one D.  repeats=False leaves out the n = o, o + 1
    repeats (never a tie geometry).  A key of n = o or o + 1 ops cannot hold
    positions 1 and o + 1, so the one-lane repeat is {0, o} at n = o + 1: lane
    0 in two iterations, the second one partial.  Where an iteration is two ops
    (D > 128) the two lanes are positions 0 and 1 and the keys are four
    iterations and one op long."""
    o = opi(D)
    n2 = 2 * o + 1 if o >= 4 else 4 * o + 1      # an odd number of iterations' worth + 1
    last = n2 - 1                                 # the lone op of the last iteration, lane 0
    other = o + min(3, o - 1)                     # second iteration, a lane other than 0
    l1, l2 = (1, 2) if o >= 3 else (0, 1)        # two lanes of one iteration
    out, x = [], [0]

    def add(case, tied, n=n2, base=None, prev=0, upto=None, gc=0, look="hit", unl=False, **reach):
        assert all(0 <= p < n for p in tied) and prev <= (n if upto is None else upto)
        k = len(out)
        if look == "new":
            base, prev = None, 0
        elif base is None and k % 2:
            base = (0, 3)                         # a planted pair that loses to every op
        out.append(dict(case=case, n=n, tied=dict(tied), base=base, prev=prev,
                        upto=n if upto is None else upto, gc=gc, look=look, unl=unl, reach=reach,
                        name=f"{case} n={n} {sorted(tied.items())} base={base} prev={prev} "
                             f"upto={upto} gc={gc} {look}"))

    def two(case, pa, pb, pairs=None, **kw):
        """{pa: a, pb: b} for an A pair and a B pair (or `pairs`), both ways round."""
        if pairs is None:
            pairs = [A_PAIRS[x[0] % 3], B_PAIRS[x[0] % 2]]
            x[0] += 1
        for a, b in pairs:
            add(case, {pa: a, pb: b}, **kw)
            add(case, {pa: b, pb: a}, **kw)

    two("lanes", l1, l2, ALL_PAIRS, across=True)
    two("lane", 1, o + 1, ALL_PAIRS, in_lane=True)
    third = 2 * o - 1 if 2 * o - 1 not in (1, o + 1) else 2 * o + 1
    add("three", {1: 1, o + 1: 3, third: 2}, in_lane=True, middle="first")
    add("three", {1: 5, o + 1: 2, third: 3}, in_lane=True, middle="reversed")
    two("last", 0, last, in_lane=True, lane0=True, last_iter=True)
    for case, p in (("base-lane0", o), ("base-other", other)):
        pairs = [A_PAIRS[x[0] % 3], B_PAIRS[x[0] % 2]]
        x[0] += 1
        for a, b in pairs:
            for bt, ot in ((a, b), (b, a)):
                add(case, {p: ot}, base=(bt, TOP), prev=1, base_tie=True, lane0=p % o == 0)
    add("base-plus", {1: 1, o + 1: 2}, base=(3, TOP), prev=1, base_tie=True, in_lane=True)
    add("base-plus", {1: 4, o + 1: 5}, base=(3, TOP), prev=1, base_tie=True, in_lane=True)
    # the label-winner is the one op R excludes: the log's label-loser wins
    add("excluded", {1: 4, last: 3}, upto=last, wins=4, single=True)        # first: 3 > 4
    add("excluded", {1: 5, last: 2}, upto=last, wins=5, single=True)        # reversed: 2 > 5
    add("excluded", {l1: 1, l2: 2, last: 3}, upto=last, across=True)
    add("excluded", {l1: 5, l2: 2, last: 4}, upto=last, across=True)
    # the label-winner lies behind the snapshot, whose pair carries another tag
    add("behind", {1: 3, o + 1: 1}, base=(2, TOP), prev=3, base_tie=True, table="first")
    add("behind", {1: 4, o + 1: 2}, base=(5, TOP), prev=3, base_tie=True, table="reversed")
    for a in (3, 2):
        add("no-tie", {1: a, o + 1: a}, single=True)
        add("no-tie", {o: a}, base=(a, TOP), prev=1, single=True)
    if repeats:
        two("lanes", l1, l2, n=o, across=True)
        two("lanes", l1, l2, n=o + 1, across=True)
        two("lane", 0, o, n=o + 1, in_lane=True, lane0=True, last_iter=True)
    for look, gc in (("new", 0), ("hit", 1), ("new", 1)):
        two("lanes", l1, l2, look=look, gc=gc, across=True)
        two("lane", 1, o + 1, look=look, gc=gc, in_lane=True)
    # one tag without a label: the only keys that may carry AGN_F_TS_TIE
    for u in (UNL_IN, UNL_PAST):
        for a, b in ((u, 3), (2, u)):
            add("unlabelled", {l1: a, l2: b}, unl=True, across=True)
            add("unlabelled", {1: a, o + 1: b}, unl=True, in_lane=True)
        add("unlabelled-base", {o: 3}, base=(u, TOP), prev=1, unl=True, base_tie=True, lane0=True)
        add("unlabelled-base", {other: 4}, base=(u, TOP), prev=1, unl=True, base_tie=True)
    add("unlabelled", {l1: UNL_IN, l2: UNL_PAST}, unl=True, across=True)
    add("unlabelled", {1: UNL_PAST, o + 1: UNL_IN}, unl=True, in_lane=True)
    return out


class Family:
    pass


def full_mask(D):
    m = np.zeros(n_words(D), np.uint64)
    for d in range(D):
        m[d >> 6] |= np.uint64(1 << (d & 63))
    return m


def op_row(D, c, p, masked):
    """Op p of a key on column c: its clock row and presence words.  Masked
    (D >= 2), after lww_serve_cases.masked: two ops in three lack one DC other
    than their own and hold garbage far above every read clock there.  Every
    fiftieth op keeps every DC: its snapshot time is the clock of the
    reference's own GC read (op_insert_gc), which must find the planted
    snapshot rather than fall back to the disk log."""
    oc = np.full(D, C0, np.uint64)
    oc[c] = C0 + p + 1
    if not masked:
        return oc, None
    m = full_mask(D)
    d = (c + 1 + p % 2) % D
    if p % 3 and p % po.OPS_THRESHOLD != po.OPS_THRESHOLD - 1 and d != c:
        m[d >> 6] &= np.uint64(~(1 << (d & 63)) & ((1 << 64) - 1))
        oc[d] = np.uint64((1 << 61) | (977 * p + d))
    return oc, m


def op_rows(D, c, n, masked):
    """op_row for p = 0 .. n - 1 at once: (n, D) clocks, (n, W) words or None."""
    p = np.arange(n)
    oc = np.full((n, D), C0, np.uint64)
    oc[:, c] = C0 + p + 1
    if not masked:
        return oc, None
    m = np.tile(full_mask(D), (n, 1))
    d = (c + 1 + p % 2) % D
    rows = np.flatnonzero((p % 3 != 0) & (p % po.OPS_THRESHOLD != po.OPS_THRESHOLD - 1) & (d != c))
    dr = d[rows]
    m[rows, dr >> 6] &= ~(np.uint64(1) << (dr & 63).astype(np.uint64))
    oc[rows, dr] = (np.uint64(1) << np.uint64(61)) | (977 * rows + dr).astype(np.uint64)
    return oc, m


def family(D, masked=False, repeats=True):
    assert D >= 2 or not masked
    fam = Family()
    fam.D, fam.W, fam.masked, fam.opi = D, n_words(D), masked, opi(D)
    fam.full = full_mask(D)
    fam.keys = keys(D, repeats)
    fam.K = len(fam.keys)
    fam.oc, fam.mask, fam.ts, fam.tag, fam.sct, fam.R = [], [], [], [], [], []
    for k, s in enumerate(fam.keys):
        c, n = k % D, s["n"]
        oc, m = op_rows(D, c, n, masked)
        fam.oc.append(oc)
        fam.mask.append(m)
        ts = np.array([10 + p % 7 for p in range(n)], np.uint64)
        tag = np.zeros(n, np.uint32)
        for p, t in s["tied"].items():
            ts[p], tag[p] = TOP, t
        fam.ts.append(ts)
        fam.tag.append(tag)
        sct = np.full(D, C0, np.uint64)
        sct[c] = C0 + s["prev"]
        R = np.full(D, C0 + 500, np.uint64)
        R[c] = C0 + s["upto"]
        fam.sct.append(sct)
        fam.R.append(R)
    return fam


def later(fam, k, R):
    """R at a later clock with no new op: every column but the key's own."""
    out = R.copy()
    c = k % fam.D
    out[np.arange(fam.D) != c] += np.uint64(7)
    return out


def followup_tag(table, stored, k):
    """Follow-up (b)'s tag: beats the stored pair's on even keys and loses to it
    on odd ones (the other way round where the stored tag is the table's top
    or bottom, or has no label)."""
    labs = TABLES[table]
    order = sorted(TIED, key=lambda t: int(labs[t]))           # ascending
    lab = om.label(labs, stored)
    above = [t for t in order if int(labs[t]) > lab and t != stored]
    below = [t for t in order if int(labs[t]) < lab and t != stored]
    want = above if k % 2 == 0 else below
    pick = want or above or below
    return pick[-1] if pick is above else pick[0]


# ------------------------------------------------------------------ the run on the host
def _le(a, am, b, bm, D):
    """vectorclock:le(A, B) with presence words (None: every DC); missing = 0."""
    for d in range(D):
        if am is not None and not (int(am[d >> 6]) >> (d & 63)) & 1:
            continue
        bv = int(b[d]) if bm is None or (int(bm[d >> 6]) >> (d & 63)) & 1 else 0
        if int(a[d]) > bv:
            return False
    return True


class KeyChain:
    """One key of one partition on the host: its log, its cached snapshots
    (newest first: pair or None, clock, presence words, last op id), and the
    read after get_from_snapshot_cache / materialize / materialize_snapshot as
    cache_dev.hpp restates them."""

    def __init__(self, D, masked, labels):
        self.D, self.W, self.masked, self.labels = D, n_words(D), masked, labels
        self.full = full_mask(D)
        self.ents, self.snaps, self.next_id = [], [], 1

    def plant(self, pair, clock, last_op):
        """Batcher.store(gc=True) on a key with no op and no snapshot."""
        assert not self.snaps and not self.ents
        self.snaps = [(pair, clock.copy(), self.full.copy() if self.masked else None, last_op)]

    def append(self, oc, mask, ts, tag):
        self.ents.append((oc, mask, int(ts), int(tag), self.next_id))
        self.next_id += 1

    def read(self, R, gc):
        D, W, ents = self.D, self.W, self.ents
        n = len(ents)
        # the lookup
        if not self.snaps:
            self.snaps = [(None, np.zeros(D, np.uint64),
                           np.zeros(W, np.uint64) if self.masked else None, 0)]
            status, first, ign, snap = _abi.SS_NEW, True, True, self.snaps[0]
        else:
            hit = [j for j, s in enumerate(self.snaps) if _le(s[1], s[2], R, None, D)]
            assert hit, "the script never reads below every snapshot"
            status, first, ign, snap = _abi.SS_HIT, hit[0] == 0, False, self.snaps[hit[0]]
        # the fold
        log = EncodedLog(crdt_type=LWW, n_dcs=D, key_off=np.array([0, n], np.uint64),
                         key_type=np.full(1, LWW, np.uint8),
                         oc=np.array([e[0] for e in ents], np.uint64).reshape(n, D),
                         oc_mask=np.array([e[1] for e in ents], np.uint64).reshape(n, W)
                         if self.masked else None,
                         op_id=np.array([e[4] for e in ents], np.uint32),
                         txid=np.ones(n, np.uint64),
                         tag=np.array([e[3] for e in ents], np.uint32),
                         add_tok=np.array([e[2] for e in ents], np.uint64),
                         rem_off=np.zeros(n + 1, np.uint32), rem_tok=np.zeros(1, np.uint64))
        req = EncodedRead(n_dcs=D, req_type=LWW, keys=np.zeros(1, np.uint64),
                          R=np.asarray(R, np.uint64).reshape(1, D),
                          R_mask=self.full.reshape(1, W) if self.masked else None,
                          sct=snap[1].reshape(1, D),
                          sct_mask=snap[2].reshape(1, W) if self.masked else None,
                          sct_ignore=np.array([ign], np.uint8), txid=np.zeros(1, np.uint64),
                          base_value=None, base_off=None, base_tag=None, base_tok=None)
        w, incl, info = om.model(log, req, self.masked, np.array([0, 1], np.uint64),
                                 bases=[snap[0]], order=self.labels)
        fl, cnt, hole = int(w.flags[0]), int(w.count[0]), int(w.hole[0])
        out_n = int(w.out_n[0])
        pair = (int(w.out_tag[0]), int(w.out_tok[0])) if out_n else None
        ct = w.lastct[0].copy()
        ctm = w.lastct_mask[0].copy() if self.masked else None
        r = dict(status=status, flags=fl, count=cnt, hole=hole, out_n=out_n, pair=pair, lastct=ct,
                 lastct_mask=ctm, info=info[0], incl=incl[0], n=n, base=snap[0], stored=False,
                 pruned=0)
        # the store
        errs = _abi.F_ERR_UNEXPECTED | _abi.F_ERR_CORRUPTED | _abi.F_ERR_CAPACITY
        if n == 0 or fl & errs or fl & _abi.F_CT_IGNORE:
            return r
        refresh = bool(fl & _abi.F_NEWSS) and first and cnt >= MIN_OPS
        if not (refresh or gc):
            return r
        ns = len(self.snaps)
        if not (hole - self.snaps[0][3] >= MIN_OPS or gc):
            return r
        prepend = not _le(ct, ctm, self.snaps[0][1], self.snaps[0][2], D)
        collect = ns + int(prepend) >= THRESHOLD or bool(gc)
        kept = self.snaps if not collect else self.snaps[:KEEP - 1 if prepend else KEEP]
        self.snaps = ([(pair, ct, ctm, hole)] if prepend else []) + list(kept)
        r["stored"] = prepend
        if collect:       # prune_ops below vectorclock:min of the kept clocks (missing = 0)
            thr = np.zeros(D, np.uint64)
            for d in range(D):
                vals = [int(s[1][d]) if s[2] is None or (int(s[2][d >> 6]) >> (d & 63)) & 1 else 0
                        for s in self.snaps]
                thr[d] = min(vals)
            keep = [e for e in ents if not _le(e[0], e[1], thr, None, D)]
            assert keep, "the script never collects a whole key"
            r["pruned"] = n - len(keep)
            self.ents = keep
        return r


class Vnode:
    """The reference transcription's vnode fed one table's values."""

    def __init__(self, table, D):
        self.vn, self.table, self.D = po.MaterializerVnode(), table, D
        self.tx, self.quirk = 0, set()

    def vc(self, row, mask=None):
        row = row.tolist()
        if mask is None:
            return dict(enumerate(row))
        bits = sum(int(w) << (64 * x) for x, w in enumerate(mask))
        return {d: row[d] for d in range(self.D) if (bits >> d) & 1}

    def plant(self, k, pair, clock, last_op):
        state = po.crdt_new(po.REGISTER_LWW) if pair is None else \
            (pair[1], value(self.table, pair[0]))
        self.vn.internal_store_ss(k, po.MaterializedSnapshot(last_op, state), self.vc(clock), False)

    def update(self, k, c, oc, mask, ts, tag):
        ss = oc.copy()
        ss[c] = int(oc[c]) - 1
        self.tx += 1
        pay = po.Payload(k, po.REGISTER_LWW, (int(ts), value(self.table, int(tag))),
                         self.vc(ss, mask), (c, int(oc[c])), self.tx)
        try:
            self.vn.update(k, pay)
        except (po.BadMatch, NotImplementedError):
            self.quirk.add(k)

    def read(self, k, R, gc):
        try:
            r = self.vn.internal_read(k, po.REGISTER_LWW, self.vc(R), po.IGNORE, bool(gc))
        except (po.BadMatch, NotImplementedError):
            self.quirk.add(k)
            return None
        assert r[0] == "ok", r
        return r[1]


READS = ("constructed", "later clock, no new op", "one more op at TOP")


def script(fam, table, ks=None):
    """The whole run of one family (or its keys `ks`) under one table on the
    host.  Per key:
    reads = [the three reads' expected results, in READS' order], each with
    "R", "gc" and, for a labelled key, "vnode": the reference's served state;
    extra = follow-up (b)'s op (oc, mask, ts, tag).  -> ({key: ...}, vnode
    quirk set)."""
    D, labels = fam.D, TABLES[table]
    vn = Vnode(table, D)
    out = {}
    for k in range(fam.K) if ks is None else ks:
        s = fam.keys[k]
        c, ref = k % D, not s["unl"]
        ch = KeyChain(D, fam.masked, labels)
        if s["look"] == "hit":
            ch.plant(s["base"], fam.sct[k], s["prev"])
            if ref:
                vn.plant(k, s["base"], fam.sct[k], s["prev"])
        for p in range(s["n"]):
            m = fam.mask[k][p] if fam.masked else None
            ch.append(fam.oc[k][p], m, fam.ts[k][p], fam.tag[k][p])
            if ref:
                vn.update(k, c, fam.oc[k][p], m, fam.ts[k][p], fam.tag[k][p])
        reads = []

        def read(R, gc):
            r = ch.read(R, gc)
            r["R"], r["gc"] = R, gc
            if ref:
                r["vnode"] = vn.read(k, R, gc)
            reads.append(r)
            return r
        r1 = read(fam.R[k], s["gc"])
        read(later(fam, k, fam.R[k]), 0)
        stored = ch.snaps[0][0] if ch.snaps[0][0] is not None else r1["pair"]
        tag = followup_tag(table, stored[0], k)
        p = s["n"]
        oc, m = op_row(D, c, p, fam.masked)
        ch.append(oc, m, TOP, tag)
        if ref:
            vn.update(k, c, oc, m, TOP, tag)
        Rb = later(fam, k, fam.R[k])
        Rb[c] = C0 + p + 1
        read(Rb, 0)
        out[k] = dict(reads=reads, extra=(oc, m, TOP, tag))
    return out, vn.quirk
