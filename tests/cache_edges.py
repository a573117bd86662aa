"""Constructed snapshot caches, store inputs, logs and batcher scripts that sit
on the device snapshot cache's slot and policy edges (helper, no tests).

The randomised cache tests draw their shapes; the builders here place one
named edge per key instead: a cached clock equal to the read clock, above it
in one column only (column 0, the last column, the last column of a 64-bit
mask word), the hit in the first / second / last / ninth slot, a list of 8 /
9 / 10 entries, a snapshot of exactly 4 / 5 ops, an op-id gap of 4 / 5 to the
head snapshot, LastOpCt equal to / above / concurrent with the head clock, a
GC read that keeps min(n, 2) + 1 or min(n, 3) snapshots, a GC threshold whose
minimum comes from a different kept snapshot per column.  Nothing is drawn:
building a family twice gives identical arrays.

  Family L  lookup_cases / family_ls   agn_ss_lookup (get_smaller)
  Family S  family_ls                  agn_ss_store with synthetic results
  Family R  family_r                   agn_read_cached on real logs, D <= 8
  Family B  scripts + CacheMirror      the cached read batcher
  Family G  family_g                   agn_select_base

Every key carries a name (for assertion messages) and an `expect` dict: the
outcome the key was built for, which tests/test_cache_edges_cpu.py checks on
the oracle's outputs (a builder that misses its edge fails there).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from antidote_amd import _abi
from antidote_amd.encode import EncodedLog, alloc_result, log_struct, n_words, result_struct
from edges import READ_TXID, _garbage, from_patterns, one_at, pack_mask

THRESHOLD, KEEP, MIN_OPS = _abi.SNAPSHOT_THRESHOLD, _abi.SNAPSHOT_MIN, _abi.MIN_OP_STORE_SS
NSLOT = 16          # the most slots the fused read looks at
SLOTS = (9, 10, 16)
NEW, HIT, LOG = "new", "hit", "log"
STATUS = {NEW: _abi.SS_NEW, HIT: _abi.SS_HIT, LOG: _abi.SS_LOG}


def ptr(a):
    return None if a is None else a.ctypes.data


def word_cols(D):
    """Column 0, the last column and the last column of every full mask word."""
    return sorted({0, D - 1} | set(range(63, D, 64)))


def hit_slots(n):
    return sorted({f for f in (0, 1, n - 2, n - 1, 7, 8) if 0 <= f < n})


def ladder(n, D):
    """n clocks, newest first, every column of slot j above slot j + 1's."""
    j = np.arange(n, dtype=np.int64)[:, None]
    return 1000 + 100 * (n - 1 - j) + np.arange(D, dtype=np.int64)[None, :]


# ------------------------------------------------------------------ family L: lookup edges
def lookup_cases(D, sizes, sparse):
    """(name, clocks [n, D], present [n, D], R [D], R present [D], f): the
    list of one key, its read clock and the slot get_smaller returns (-1:
    none, None: the key is absent)."""
    full = lambda n: np.ones((n, D), bool)  # noqa: E731
    out = []
    for n in sizes:
        if n == 0:
            out.append(("n=0 absent key", np.zeros((0, D), np.int64), full(0),
                        np.full(D, 500, np.int64), np.ones(D, bool), None))
            continue
        base = ladder(n, D)
        for f in hit_slots(n):
            out.append((f"n={n} hit {f}: clock equals R in every column", base, full(n),
                        base[f].copy(), np.ones(D, bool), f))
            out.append((f"n={n} hit {f}: earlier slots above R in all columns", base, full(n),
                        base[f] + 1, np.ones(D, bool), f))
            for c in word_cols(D) if f else ():
                cl = base.copy()
                for j in range(f):
                    cl[j] = base[f]
                    cl[j, c] = base[f, c] + (f - j)
                out.append((f"n={n} hit {f}: earlier slots above R in column {c} only", cl,
                            full(n), base[f].copy(), np.ones(D, bool), f))
        for c in word_cols(D):
            R = base[n - 1].copy()
            R[c] -= 1
            out.append((f"n={n} none: the last slot above R by 1 in column {c} only", base,
                        full(n), R, np.ones(D, bool), -1))
        if not sparse:
            continue
        for c in word_cols(D):
            # a DC the cached clock lacks is ignored (its column holds garbage above R)
            p = full(n)
            p[0, c] = False
            R = base[0].copy()
            R[c] = 0
            out.append((f"n={n} mask: DC {c} absent from the head clock, R[{c}] = 0", base, p, R,
                        np.ones(D, bool), 0))
            # a DC R lacks reads 0: a cached 0 passes, a cached 1 does not
            for v in (0, 1):
                cl = base.copy()
                cl[0, c] = v
                p = full(n)
                Rp = np.ones(D, bool)
                Rp[c] = False
                f = 0
                if v:
                    f = -1
                    if n >= 2:      # ...and falls through to the last slot, which lacks the DC
                        p[n - 1, c] = False
                        f = n - 1
                R = base[0].copy()
                if f > 0:
                    cl[1:n - 1, c] = 1
                out.append((f"n={n} mask: DC {c} absent from R, head entry {v}", cl, p, R, Rp, f))
        # vectorclock:new() as the last slot: any R hits it
        p = full(n)
        p[n - 1] = False
        out.append((f"n={n} mask: all-absent last clock, R = 0", base, p, np.zeros(D, np.int64),
                    np.ones(D, bool), n - 1 if n > 1 else 0))
        out.append((f"n={n} mask: all-absent last clock, R all absent", base, p,
                    base[0].copy(), np.zeros(D, bool), n - 1 if n > 1 else 0))
    return out


class CacheCase:
    """A cache in host arrays, one request per key and the fields of the
    materialize result the store consumes: the attributes of
    test_ss_cache.Case (its run_oracle / py_model take either), with
    names[i] and expect[i] per request."""

    def __init__(self, D, slots, sparse):
        self.D, self.W, self.S, self.sparse = D, n_words(D), slots, sparse
        self.rows, self.names, self.expect = [], [], []

    def key(self, name, clocks, pres, R, Rp, expect, *, nops=3, flags=0, count=0, gap=0, gc=0,
            ct=None, ctp=None, last_op=None):
        clocks = np.asarray(clocks, np.int64).reshape(-1, self.D)
        n = len(clocks)
        assert n <= self.S, (name, n, self.S)
        pres = np.ones((n, self.D), bool) if pres is None else np.asarray(pres, bool)
        if not self.sparse:
            assert pres.all() and (Rp is None or np.all(Rp)) and (ctp is None or np.all(ctp)), name
        self.rows.append(dict(
            clocks=clocks, pres=pres, R=np.asarray(R, np.int64),
            Rp=np.ones(self.D, bool) if Rp is None else np.asarray(Rp, bool), nops=nops,
            flags=flags, count=count, gap=gap, gc=gc,
            ct=np.zeros(self.D, np.int64) if ct is None else np.asarray(ct, np.int64),
            ctp=np.ones(self.D, bool) if ctp is None else np.asarray(ctp, bool),
            last_op=last_op))
        self.names.append(name)
        self.expect.append(expect)

    def pack(self):
        K, D, W, S = len(self.rows), self.D, self.W, self.S
        self.K = K
        self.n = np.array([len(r["clocks"]) for r in self.rows], np.uint32)
        # rows past n hold garbage: nothing may read them
        self.clock = _garbage((K, S, D), 11)
        pres = np.ones((K, S, D), bool)
        self.last_op = (np.arange(K * S, dtype=np.int64).reshape(K, S) * 7919) % 100003 - 50000
        self.value = (np.arange(K * S, dtype=np.int64).reshape(K, S) * 104729) % 1000003 - 500000
        self.R = np.zeros((K, D), np.uint64)
        Rp = np.ones((K, D), bool)
        self.lastct = np.zeros((K, D), np.uint64)
        ctp = np.ones((K, D), bool)
        self.key_off = np.zeros(K + 1, np.uint64)
        self.flags, self.count = np.zeros(K, np.uint32), np.zeros(K, np.uint32)
        self.hole, self.gc = np.zeros(K, np.int64), np.zeros(K, np.uint8)
        self.res_value = (np.arange(K, dtype=np.int64) * 15485863) % 2000003 - 1000001
        for k, r in enumerate(self.rows):
            n = int(self.n[k])
            self.clock[k, :n] = r["clocks"].astype(np.uint64)
            pres[k, :n] = r["pres"]
            head = 10 * n if r["last_op"] is None else r["last_op"]
            self.last_op[k, :n] = head - 6 * np.arange(n)
            self.R[k], Rp[k] = r["R"].astype(np.uint64), r["Rp"]
            self.lastct[k], ctp[k] = r["ct"].astype(np.uint64), r["ctp"]
            self.key_off[k + 1] = self.key_off[k] + np.uint64(r["nops"])
            self.flags[k], self.count[k], self.gc[k] = r["flags"], r["count"], r["gc"]
            self.hole[k] = (head if n else 0) + r["gap"]
        self.keys = np.arange(K, dtype=np.uint64)
        self.mask = self.Rm = self.lastct_mask = None
        if self.sparse:
            self.clock[~pres] = _garbage(int((~pres).sum()), 12)
            self.R[~Rp] = _garbage(int((~Rp).sum()), 13)
            self.lastct[~ctp] = _garbage(int((~ctp).sum()), 14)
            self.mask = pack_mask(pres.reshape(K * S, D)).reshape(K, S, W)
            self.mask[np.arange(S)[None, :] >= self.n[:, None]] = 0
            self.Rm, self.lastct_mask = pack_mask(Rp), pack_mask(ctp)
        return self

    # test_ss_cache.run_oracle's view of a case
    def arrays(self):
        a = {"n": self.n.copy(), "clock": self.clock.copy(), "last_op": self.last_op.copy(),
             "value": self.value.copy()}
        if self.sparse:
            a["mask"] = self.mask.copy()
        return a

    def cache_struct(self, arrs):
        return cache_struct(self.D, self.S, self.K, arrs, ptr)

    def all_arrays(self):
        names = ("n", "clock", "mask", "last_op", "value", "keys", "R", "Rm", "key_off", "flags",
                 "count", "hole", "res_value", "lastct", "lastct_mask", "gc")
        return {x: getattr(self, x) for x in names}


def cache_struct(D, S, K, arrs, addr):
    """An agn_ss_cache over arrs (host arrays with addr = ptr, or device
    buffers with addr = lambda b: b.ptr)."""
    c = _abi.AgnSsCache()
    c.n_dcs, c.slots, c.n_keys = D, S, K
    c.n, c.clock, c.last_op, c.value = (addr(arrs[x]) for x in ("n", "clock", "last_op", "value"))
    c.clock_mask = addr(arrs["mask"]) if arrs.get("mask") is not None else None
    return c


def lookup_sizes(slots):
    return (0, 1, 2, 3, 8, 9, slots)


def policy(n, prepend, gc):
    """(entries afterwards, prune) of a store that reaches insert_bigger."""
    n1 = n + (1 if prepend else 0)
    collect = n1 >= THRESHOLD or bool(gc)
    return (min(n1, KEEP) if collect else n1), collect


def family_ls(D, slots, sparse):
    """Families L and S in one cache (names start with "L " / "S ")."""
    cs = CacheCase(D, slots, sparse)
    for name, clocks, pres, R, Rp, f in lookup_cases(D, sorted(set(lookup_sizes(slots))), sparse):
        n = len(clocks)
        look = NEW if f is None else HIT if f >= 0 else LOG
        cs.key("L " + name, clocks, pres, R, Rp,
               dict(look=look, f=f, stored=False, n=max(n, 1), prune=False))
    NS, ones = _abi.F_NEWSS, np.ones(D, bool)

    def s(name, n=2, look=HIT, f=0, want=None, ct="above", clocks=None, pres=None, ctp=None,
          thr=None, **kw):
        """One store edge: want = (entries afterwards, prune) or None (nothing
        is stored).  ct: LastOpCt against the head clock."""
        cl = ladder(n, D) if clocks is None else np.asarray(clocks, np.int64)
        pr = np.ones((n, D), bool) if pres is None else pres
        if look == HIT:
            R = cl[f].copy()
        elif look == LOG:
            R = cl[n - 1].copy()
            R[0] -= 1
        else:
            R = np.full(D, 500, np.int64)
        head = cl[0] if n else np.zeros(D, np.int64)
        cp = ones.copy() if ctp is None else ctp
        if ct == "above":
            lct = head + 1
        elif ct == "equal":
            lct = head.copy()
        elif ct[0] == "one":        # above the head in one column only
            lct = head.copy()
            lct[ct[1]] += 1
        elif ct[0] == "mixed":      # below it in one column, above it in another
            lct = head.copy()
            lct[0] -= 1
            lct[D - 1] += 1
        else:                       # ("set", column, value): the others equal
            lct = head.copy()
            lct[ct[1]] = ct[2]
        kw.setdefault("flags", NS)
        kw.setdefault("count", MIN_OPS)
        kw.setdefault("gap", MIN_OPS)
        n_after = max(n, 1)
        e = dict(look=look, f=f if look == HIT else (None if look == NEW else -1),
                 stored=want is not None, n=want[0] if want else n_after,
                 prune=bool(want and want[1]), thr=thr)
        cs.key("S " + name, cl, pr, R, None, e, ct=lct, ctp=cp, **kw)

    s("stores: 2 -> 3", want=(3, False))
    s("status LOG", look=LOG)
    s("status LOG, GC read", look=LOG, gc=1)
    s("number_of_ops = 0", nops=0)
    s("number_of_ops = 0, GC read", nops=0, gc=1)
    for fl, nm in ((_abi.F_ERR_UNEXPECTED, "ERR_UNEXPECTED"), (_abi.F_ERR_CORRUPTED,
                   "ERR_CORRUPTED"), (_abi.F_ERR_CAPACITY, "ERR_CAPACITY"),
                   (_abi.F_CT_IGNORE, "CT_IGNORE")):
        s(nm, flags=NS | fl)
        s(nm + ", GC read", flags=NS | fl, gc=1)
    s("no NEWSS", flags=0)
    s("no NEWSS, GC read", flags=0, gc=1, want=(3, True))
    s("absent key (NEW): 0 -> 1 -> 2", n=0, look=NEW, want=(2, False))
    s("is_first = 0, count 7", n=3, f=1, count=7)
    s("is_first = 0, count 7, GC read", n=3, f=1, count=7, gc=1, want=(3, True))
    s("count 4", count=4)
    s("count 5", count=5, want=(3, False))
    s("count 4, GC read", count=4, gc=1, want=(3, True))
    s("hole - last_op = -1", gap=-1)
    s("hole - last_op = 4", gap=4)
    s("hole - last_op = 5", gap=5, want=(3, False))
    s("hole - last_op = 4, GC read", gap=4, gc=1, want=(3, True))
    s("LastOpCt equals the head clock: not prepended", ct="equal", want=(2, False))
    for c in word_cols(D):
        s(f"LastOpCt above the head in column {c} only", ct=("one", c), want=(3, False))
    if D >= 2:
        s("LastOpCt below the head in column 0, above it in the last", ct=("mixed",),
          want=(3, False))
    if sparse:
        for c in word_cols(D):
            p = np.ones((2, D), bool)
            p[0, c] = False
            s(f"DC {c} only in LastOpCt, entry 1: prepended", pres=p, ct=("set", c, 1),
              want=(3, False))
            s(f"DC {c} only in LastOpCt, entry 0: not prepended", pres=p, ct=("set", c, 0),
              want=(2, False))
            cp = ones.copy()
            cp[c] = False
            s(f"DC {c} only in the head clock: not prepended", ct="equal", ctp=cp, want=(2, False))
    s("n = 8 -> 9: no collect", n=8, want=(9, False))
    s("n = 9, prepended -> 10: collects", n=9, want=(KEEP, True))
    s("n = 9, not prepended: no collect", n=9, ct="equal", want=(9, False))
    if slots >= NSLOT:
        s("n = 15, prepended: collects", n=15, want=(KEEP, True))
    for n in (1, 2, 3, 4, 9):
        s(f"GC read, n = {n}, prepended", n=n, gc=1, want=(min(n, KEEP - 1) + 1, True))
        s(f"GC read, n = {n}, not prepended", n=n, gc=1, ct="equal", want=(min(n, KEEP), True))
    # the threshold: column-wise min over the kept clocks
    d = np.arange(D)
    rot = np.stack([2000 + 10 * ((j + d) % 3) + j for j in range(4)])
    s("GC threshold: the min in a different kept slot per column", n=4, gc=1, ct="equal",
      clocks=rot, want=(KEEP, True), thr="rotate")
    s("GC threshold: the same, LastOpCt prepended", n=4, gc=1, clocks=rot, want=(KEEP, True),
      thr="rotate")
    if sparse:
        for c in word_cols(D):
            p = np.ones((4, D), bool)
            p[1, c] = False
            s(f"GC threshold: DC {c} absent from one kept clock", n=4, gc=1, ct="equal",
              clocks=rot, pres=p, want=(KEEP, True), thr=("zero_set", c))
            p = np.ones((4, D), bool)
            p[:KEEP, c] = False
            cp = ones.copy()
            cp[c] = False
            s(f"GC threshold: DC {c} absent from all kept clocks", n=4, gc=1, ct="equal",
              clocks=rot, pres=p, ctp=cp, want=(KEEP, True), thr=("zero_clear", c))
    return cs.pack()


# ------------------------------------------------------------------ family G: select_base
G_LENGTHS = (0, 1, 2, 10)


def family_g(D, sparse):
    """agn_select_base's CSR lists: lengths 0 / 1 / 2 / 10, the match at the
    first entry, the last or nowhere, and Family L's clock and mask edges."""
    cases = lookup_cases(D, G_LENGTHS, sparse)
    W, nq = n_words(D), len(cases)
    off = np.zeros(nq + 1, np.uint64)
    off[1:] = np.cumsum([len(c[1]) for c in cases])
    M = int(off[-1])
    clocks, pres = np.zeros((M, D), np.uint64), np.ones((M, D), bool)
    R, Rp = np.zeros((nq, D), np.uint64), np.ones((nq, D), bool)
    for i, (_, cl, p, r, rp, _f) in enumerate(cases):
        a = int(off[i])
        clocks[a:a + len(cl)], pres[a:a + len(cl)] = cl.astype(np.uint64), p
        R[i], Rp[i] = r.astype(np.uint64), rp
    cm = Rm = None
    if sparse:
        clocks[~pres] = _garbage(int((~pres).sum()), 21)
        R[~Rp] = _garbage(int((~Rp).sum()), 22)
        cm, Rm = pack_mask(pres), pack_mask(Rp)
        if cm.shape[0] == 0:
            cm = np.zeros((1, W), np.uint64)
    idx = np.array([-1 if c[5] is None else c[5] for c in cases], np.int32)
    first = np.array([1 if (c[5] is None or c[5] == 0) else 0 for c in cases], np.uint8)
    return dict(D=D, off=off, clocks=clocks, cm=cm, R=R, Rm=Rm, idx=idx, first=first,
                names=[c[0] for c in cases])


# ------------------------------------------------------------------ family R: real logs
R_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)
R_POSITIONS = (0, 63, 64)


def r_positions(n):
    return sorted({p for p in R_POSITIONS + (n - 1,) if 0 <= p < n})


def r_scan_patterns():
    """Every length with all ops included, and with the one excluded op (X),
    the one op of the previous snapshot (P) and the one invalid effect (E) at
    0 / 63 / 64 / n - 1."""
    pats = []
    for n in R_LENGTHS:
        pats.append("I" * n)
        for p in r_positions(n):
            pats += [one_at(n, p, "X", "I"), one_at(n, p, "P", "I"), one_at(n, p, "E", "I")]
    return pats


LOOKS = ("new", "hit0", "hit8", "log")
# (cached entries, hole - head.last_op, GC read) of the keys that hit slot 0
HIT0_STORES = ((1, 5, 0), (2, 4, 0), (3, 5, 1), (8, 5, 0), (9, 5, 0), (4, 4, 1), (2, -1, 0),
               (9, 50, 1), (3, 50, 0), (1, 5, 1), (2, 5, 1), (15, 5, 0))


def segmented(log, K):
    """The same keys as segments with slack (key_off = segment starts,
    key_len = entries in use); the slack entries hold garbage."""
    lens = np.diff(log.key_off.astype(np.int64))
    pad = 1 + (np.arange(K) % 3) * 2
    start = np.zeros(K + 1, np.int64)
    start[1:] = np.cumsum(lens + pad)
    E2, D = int(start[-1]), log.n_dcs
    src = np.concatenate([np.arange(lens[k]) + int(log.key_off[k]) for k in range(K)] or
                         [np.zeros(0, np.int64)]).astype(np.int64)
    dst = np.concatenate([np.arange(lens[k]) + start[k] for k in range(K)] or
                         [np.zeros(0, np.int64)]).astype(np.int64)
    oc = _garbage((E2, D), 31)
    op_id = np.full(E2, 0xFFFFFFF0, np.uint32)
    txid = np.full(E2, READ_TXID, np.uint64)
    eff = np.full(E2, 99999, np.int64)
    oc[dst], op_id[dst], txid[dst], eff[dst] = log.oc[src], log.op_id[src], log.txid[src], \
        log.eff[src]
    seg = EncodedLog(crdt_type=log.crdt_type, n_dcs=D, key_off=start.astype(np.uint64),
                     key_type=log.key_type, oc=oc, oc_mask=None, op_id=op_id, txid=txid, eff=eff)
    return seg, lens.astype(np.uint64)


class RCase:
    """Family R for one D: the log (CSR, or segments with key_len), the
    prebuilt cache, one request per key and what each key was built for."""


def family_r(D, slots=NSLOT, seg=False):
    """One key per (log pattern, lookup outcome, store recipe): the log from
    edges.from_patterns (its R and SCT per key), the cache prebuilt around
    that SCT so that the lookup ends as NEW, a hit at slot 0, a hit at slot 8
    of 9 or LOG, the head's last_op placed `gap` below the read's NewLastOp.
    Even keys have consecutive op ids, odd keys ids three apart.  (A counter
    read cannot end in ERR_CAPACITY: that row of Family S has no key here.)"""
    specs = []   # (pattern, look, cached entries, gap, gc, label, corrupt, R = SCT)

    def add(pat, look, n=2, gap=MIN_OPS, gc=0, label="", corrupt=False, eq=False):
        if look == "hit8":
            n = 9
        if look == "new":
            n = 0
        if look == "hit15":
            n = NSLOT
        elif n > slots - 1:
            n = 9
        assert not eq or set(pat) <= {"P"}, pat
        specs.append((pat, look, n, gap, gc, label, corrupt, eq))

    x = 0
    for pat in r_scan_patterns():
        for look in LOOKS:
            if look == "hit0":
                n, gap, gc = HIT0_STORES[x % len(HIT0_STORES)]
                add(pat, look, n, gap, gc)
            elif look == "log":
                add(pat, look, (1, 3, 9)[x % 3], MIN_OPS, x % 2)
            else:
                add(pat, look, gc=(x // 2) % 2)
            x += 1
    I5, I4 = "I" * 5, "I" * 4
    add(I4, "hit0", label="count 4")
    add(I5, "hit0", label="count 5")
    add("PP" + I4, "hit0", label="count 4 after two ops of the snapshot")
    add(I4, "hit0", gc=1, label="count 4, GC read")
    for gap in (-1, 4, 5):
        add(I5, "hit0", gap=gap, label=f"hole - last_op = {gap}")
    add(I5, "hit0", gap=4, gc=1, label="hole - last_op = 4, GC read")
    add("PPP", "hit0", label="no NEWSS")
    add("PPP", "hit0", n=4, gc=1, label="no NEWSS, GC read: LastOpCt = head")
    add("XXX", "new", label="CT_IGNORE")
    add("XXX", "new", gc=1, label="CT_IGNORE, GC read")
    add("XXX", "log", gc=1, label="status LOG, CT_IGNORE, GC read")
    add(I5, "log", n=3, label="status LOG, count 5")
    add("IIEII", "hit0", label="ERR_UNEXPECTED")
    add("IIEII", "hit0", gc=1, label="ERR_UNEXPECTED, GC read")
    add("IIEII", "new", label="ERR_UNEXPECTED on an absent key")
    add(I5, "new", corrupt=True, label="ERR_CORRUPTED, key absent from the cache")
    add(I5, "hit0", corrupt=True, label="ERR_CORRUPTED, key present")
    add(I5, "hit0", gc=1, corrupt=True, label="ERR_CORRUPTED, key present, GC read")
    add(I5, "hit8", gc=1, corrupt=True, label="ERR_CORRUPTED, hit 8, GC read")
    add("", "new", label="no ops, absent")
    add("", "hit0", gc=1, label="no ops, GC read")
    add(I5, "hit8", label="is_first = 0, count 5")
    add(I5, "hit8", gc=1, label="is_first = 0, count 5, GC read")
    add(I5, "new", label="absent key, count 5: 0 -> 1 -> 2")
    add(I4, "new", label="absent key, count 4: 0 -> 1")
    add(I5, "hit0", n=8, label="n = 8 -> 9")
    add(I5, "hit0", n=9, label="n = 9 -> 10: collects")
    add("TTTTT", "hit0", n=9, label="n = 9, own TxId, LastOpCt = head: no collect")
    add("TTTTT", "hit0", n=2, label="own TxId, count 5, LastOpCt = head")
    add("PTPTI", "hit0", n=2, gc=1, label="own TxId between ops of the snapshot, GC read")
    add(I5, "hit0", n=15, label="n = 15, prepended")
    for n in (1, 2, 3, 4, 9):
        add("II", "hit0", n=n, gc=1, label=f"GC read, n = {n}, prepended")
        add("PP", "hit0", n=n, gc=1, label=f"GC read, n = {n}, not prepended")
    # the hit clock equal to R in every column (the patterns' R is above SCT in one)
    add("PPP", "hit0", n=3, eq=True, label="R equals the hit clock")
    add("PPP", "hit0", n=3, gc=1, eq=True, label="R equals the hit clock, GC read")
    add("", "hit8", eq=True, label="R equals the hit clock, no ops")
    add("PPP", "hit8", gc=1, eq=True, label="R equals the hit clock, GC read")
    if slots >= NSLOT:   # the last slot the fused read looks at
        add(I5, "hit15", label="hit 15 of 16")
        add(I5, "hit15", gc=1, label="hit 15 of 16, GC read")
        add("PPP", "hit15", gc=1, eq=True, label="hit 15 of 16, R equals the hit clock, GC read")
        add("X" + I5, "hit15", gc=1, label="hit 15 of 16, the oldest op excluded, GC read")
    pats = [sp[0] for sp in specs]
    K = len(pats)
    col = [(k * 5 + k // 7) % D for k in range(K)]
    log, req, _, labels = from_patterns(_abi.COUNTER_PN, D, pats, col=col)
    # op ids: even keys consecutive (key_id0 serves NewLastOp), odd keys with gaps
    for k in range(0, K, 2):
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        log.op_id[a:b] = 5 + np.arange(b - a)
    clock = _garbage((K, slots, D), 41)
    n_arr = np.zeros(K, np.uint32)
    last_op = (np.arange(K * slots, dtype=np.int64).reshape(K, slots) * 7919) % 100003 - 50000
    value = (np.arange(K * slots, dtype=np.int64).reshape(K, slots) * 104729) % 1000003 - 500000
    gc = np.zeros(K, np.uint8)
    expect, names = [], []
    d = np.arange(D)
    for k, (pat, look, n, gap, g, label, corrupt, eq) in enumerate(specs):
        c = col[k]
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        ids = log.op_id[a:b].astype(np.int64)
        if eq:
            req.R[k] = req.sct[k]
        sct, R = req.sct[k].astype(np.int64), req.R[k].astype(np.int64)
        xc = (c + 1) % D
        if look == "hit0":      # slot 0 = SCT; deeper slots around it, none compared
            for j in range(n):
                clock[k, j] = (sct + (10 * (((j + d) % 3) - 1) + j if j else 0)).astype(np.uint64)
            f = 0
        elif look in ("hit8", "hit15"):   # the slots before above R in column xc only
            f = 8 if look == "hit8" else NSLOT - 1
            for j in range(f):
                row = sct.copy()
                row[xc] = R[xc] + (f - j)
                clock[k, j] = row.astype(np.uint64)
            clock[k, f] = sct.astype(np.uint64)
        elif look == "log":     # every slot above R in column xc only
            for j in range(n):
                row = sct.copy()
                row[xc] = R[xc] + (n - j)
                clock[k, j] = row.astype(np.uint64)
            f = -1
        else:
            f = None
        n_arr[k], gc[k] = n, g
        nI, nP, nT = pat.count("I"), pat.count("P"), pat.count("T")
        has_e, has_x = "E" in pat, "X" in pat
        incl = nI + nT + (0 if f is not None and f >= 0 else nP) + pat.count("E")
        hole = (int(ids[pat.index("X")]) - 1 if has_x else int(ids[-1])) if pat else 0
        if n:
            last_op[k, :n] = (hole - gap) - 6 * np.arange(n)
        if corrupt:
            log.key_type[k] = _abi.SET_AW
        # the store this key was built for
        n1 = max(n, 1)
        first = f is None or f == 0
        gate = f != -1 and len(pat) > 0 and not has_e and not corrupt
        ct_ign = (f is None or f < 0) and incl == 0
        refresh = incl > 0 and first and incl >= MIN_OPS
        head_gap = gap if n else hole
        stored = bool(gate and not ct_ign and (refresh or g) and (head_gap >= MIN_OPS or g))
        # LastOpCt: SCT (or nothing) with column c raised by the included I / E ops
        if look in ("hit8", "hit15"):
            prepend = (nI > 0 or has_e) and D > 1      # D = 1: the head is above it
        else:
            prepend = nI > 0 or (f is None and incl > 0)
        want_n, want_pr = policy(n1, prepend, g) if stored else (n1, False)
        expect.append(dict(look=HIT if f is not None and f >= 0 else (NEW if f is None else LOG),
                           f=f, count=None if (has_e or corrupt) else incl, stored=stored,
                           n=want_n, prune=want_pr, prepend=bool(stored and prepend),
                           corrupt=corrupt, err=has_e and not corrupt,
                           id0=k % 2 == 0 and len(pat) > 0, gc=g, gap=head_gap, n0=n,
                           pattern=pat))
        names.append(f"k={k} {look} n={n} gap={gap} gc={g} {label or labels[k]}")
    r = RCase()
    r.D, r.S, r.K, r.names, r.expect = D, slots, K, names, expect
    r.log, r.key_len = log, None
    if seg:
        r.log, r.key_len = segmented(log, K)
    r.keys = np.arange(K, dtype=np.uint64)
    r.R, r.txid, r.gc = req.R.copy(), req.txid.copy(), gc
    r.cache = {"n": n_arr, "clock": clock, "last_op": last_op, "value": value}
    return r


def r_log_struct(r):
    """(agn_log over r's host arrays, keep-alive)."""
    ls = log_struct(r.log)
    ls.oc_mask = None
    if r.key_len is not None:
        ls.key_len = ptr(r.key_len)
    return ls


# ------------------------------------------------------------------ the mirror
class CacheMirror:
    """What the device cache and a cached batcher must compute: host arrays
    for the cache, per-key entry lists for the log, and read/6 as the C
    oracle's chain oracle_ss_lookup -> oracle_materialize -> oracle_ss_store,
    then oracle_prune_ops of a key whose read collected.  The oracle keeps
    zero entries when every op is pruned, as the engine does."""

    def __init__(self, lib, K, D, slots=THRESHOLD, sparse=False, cache=None):
        self.lib, self.K, self.D, self.S, self.sparse = lib, K, D, slots, sparse
        self.W = W = n_words(D)
        self.arr = {"n": np.zeros(K, np.uint32), "clock": np.zeros((K, slots, D), np.uint64),
                    "last_op": np.zeros((K, slots), np.int64),
                    "value": np.zeros((K, slots), np.int64)}
        if sparse:
            self.arr["mask"] = np.zeros((K, slots, W), np.uint64)
        if cache is not None:
            for x, a in cache.items():
                self.arr[x] = a.copy()
        self.entries = [[] for _ in range(K)]   # (oc row, mask row or None, op id, txid, eff)

    def append(self, k, oc, eff, op_id, txid, mask=None):
        self.entries[k].append((np.asarray(oc, np.uint64).copy(),
                                None if mask is None else np.atleast_1d(
                                    np.asarray(mask, np.uint64)).copy(),
                                int(op_id), int(txid), int(eff)))

    def key_log(self, k):
        ents, D, W = self.entries[k], self.D, self.W
        n = len(ents)
        log = EncodedLog(
            crdt_type=_abi.COUNTER_PN, n_dcs=D, key_off=np.array([0, n], np.uint64),
            key_type=np.full(4, _abi.COUNTER_PN, np.uint8),
            oc=np.array([e[0] for e in ents], np.uint64).reshape(n, D),
            oc_mask=(np.array([e[1] for e in ents], np.uint64).reshape(n, W)
                     if self.sparse else None),
            op_id=np.array([e[2] for e in ents], np.uint32),
            txid=np.array([e[3] for e in ents], np.uint64),
            eff=np.array([e[4] for e in ents], np.int64))
        return log

    def chain(self, c, ls, n_keys, keys, R, Rm, tx, gc):
        """read/6 of a batch on cache struct c and log struct ls."""
        lib, D, W, sp = self.lib, self.D, self.W, self.sparse
        nr = len(R)
        sct, ign = np.zeros((nr, D), np.uint64), np.zeros(nr + 8, np.uint8)
        sctm = np.zeros((nr, W), np.uint64) if sp else None
        base, first, status = np.zeros(nr, np.int64), np.zeros(nr + 8, np.uint8), \
            np.zeros(nr + 8, np.uint8)
        assert lib.oracle_ss_lookup(C.byref(c), nr, ptr(keys), ptr(R), ptr(Rm), ptr(sct),
                                    ptr(sctm), ptr(ign), ptr(base), ptr(first), ptr(status)) == 0
        rq = _abi.AgnRead()
        rq.n_req, rq.keys, rq.R, rq.R_mask = nr, ptr(keys), ptr(R), ptr(Rm)
        rq.sct, rq.sct_mask, rq.sct_ignore, rq.txid = ptr(sct), ptr(sctm), ptr(ign), ptr(tx)
        rq.req_type, rq.base_value = _abi.COUNTER_PN, ptr(base)
        res = alloc_result(nr, D, sparse=sp)
        rs = result_struct(res)
        assert lib.oracle_materialize(C.byref(ls), C.byref(rq), C.byref(rs), 1) == 0
        prune, thr = np.zeros(n_keys + 8, np.uint8), np.zeros((n_keys, D), np.uint64)
        thrm = np.zeros((n_keys, W), np.uint64) if sp else None
        assert lib.oracle_ss_store(C.byref(c), C.byref(ls), nr, ptr(keys), ptr(first),
                                   ptr(status), ptr(gc), C.byref(rs), None, ptr(prune), ptr(thr),
                                   ptr(thrm)) == 0
        return dict(res=res, status=status[:nr], first=first[:nr], prune=prune[:n_keys], thr=thr,
                    thrm=thrm, sct=sct, sctm=sctm, ign=ign[:nr], base=base)

    def read_batch(self, ls, keys, R, tx, gc, Rm=None):
        """A batch over the whole cache and a caller's log (Family R)."""
        c = cache_struct(self.D, self.S, self.K, self.arr, ptr)
        return self.chain(c, ls, self.K, keys, R, Rm, tx, gc)

    def read(self, k, R, Rm=None, txid=0, gc=False):
        """One read/6 of key k on its entry list; returns every
        agn_key_result field (err_pos as the op's id) + prune."""
        from test_prune import oracle_prune
        one = {x: a[k:k + 1].copy() for x, a in self.arr.items()}
        c = cache_struct(self.D, self.S, 1, one, ptr)
        log = self.key_log(k)
        ls = log_struct(log)
        if not self.sparse:
            ls.oc_mask = None
        R = np.ascontiguousarray(R, np.uint64).reshape(1, self.D)
        Rm = None if (Rm is None or not self.sparse) else \
            np.ascontiguousarray(np.atleast_1d(Rm), np.uint64).reshape(1, self.W)
        if self.sparse and Rm is None:
            Rm = pack_mask(np.ones((1, self.D), bool))
        o = self.chain(c, ls, 1, None, R, Rm, np.array([txid], np.uint64),
                       np.array([1 if gc else 0] + [0] * 7, np.uint8))
        for x, a in one.items():
            self.arr[x][k] = a[0]
        res = o["res"]
        fl, ep = int(res.flags[0]), int(res.err_pos[0])
        if fl & _abi.F_ERR_UNEXPECTED and ep != 0xFFFFFFFF:
            ep = int(log.op_id[ep])
        out = dict(status=int(o["status"][0]), value=int(res.value[0]), hole=int(res.hole[0]),
                   count=int(res.count[0]), flags=fl, err_pos=ep, lastct=res.lastct[0].copy(),
                   lastct_mask=res.lastct_mask[0].copy() if self.sparse else None,
                   prune=int(o["prune"][0]), first=int(o["first"][0]), thr=o["thr"][0].copy(),
                   sct=o["sct"][0].copy())
        if out["prune"] and len(self.entries[k]):
            arrs, _fl, n_out = oracle_prune(self.lib, log, np.array([1, 0, 0, 0], np.uint8),
                                            o["thr"], o["thrm"])
            self.entries[k] = [(arrs["oc"][e].copy(),
                                arrs["oc_mask"][e].copy() if self.sparse else None,
                                int(arrs["op_id"][e]), int(arrs["txid"][e]), int(arrs["eff"][e]))
                               for e in range(n_out)]
        return out

    def size(self, k):
        return int(self.arr["n"][k])




# ------------------------------------------------------------------ family B: batcher scripts
class Clock:
    """Causal hand-built clocks: the script's op number t commits at DC
    dcs[t mod len(dcs)], one tick after everything before it."""

    def __init__(self, D, dcs=None):
        self.D, self.now, self.t = D, np.full(D, 100, np.int64), 0
        self.dcs = list(range(D)) if dcs is None else list(dcs)

    def op(self):
        c = self.dcs[self.t % len(self.dcs)]
        oc = self.now.copy()
        self.now[c] += 1
        oc[c] = self.now[c]
        self.t += 1
        return c, oc

    def R(self):
        return self.now.astype(np.uint64)


class Script:
    """One key's steps: ("append", [(oc row, effect, DC set or None)]) and
    ("read", R, R's DC set or None, gc, label)."""

    def __init__(self, D, sparse, dcs=None):
        self.D, self.sparse, self.clk, self.steps = D, sparse, Clock(D, dcs), []
        self.full = (1 << D) - 1

    def append(self, m, masks=None, bad_at=None):
        out = []
        for x in range(m):
            c, oc = self.clk.op()
            oc = oc.astype(np.uint64)
            eff = _abi.EFFECT_INVALID if x == bad_at else 3 + 7 * self.clk.t
            mk = None
            if self.sparse:
                mk = self.full if masks is None else masks(self.clk.t - 1, c)
                assert (mk >> c) & 1
                for d in range(self.D):     # absent columns hold garbage
                    if not (mk >> d) & 1:
                        oc[d] = np.uint64((1 << 61) | (977 * self.clk.t + d))
            out.append((oc, eff, mk))
        self.steps.append(("append", out))
        return self

    def read(self, label, R=None, rm=None, gc=False):
        self.steps.append(("read", self.clk.R() if R is None else R.copy(),
                           rm if self.sparse else None, gc, label))
        return self

    def rounds(self, k, m=5, **kw):
        for _ in range(k):
            self.append(m, **kw).read(f"round of {m}")
        return self


def scripts(D, sparse):
    """{name: Script}.  Every script starts with a read of the still absent
    key (NEW, one entry: the empty snapshot)."""
    sc = {}
    # grow: 1, then eight rounds of five ops -> 2..9, the tenth read collects to 3
    sc["grow"] = Script(D, sparse).read("absent").rounds(9)
    # a round of four ops stores nothing in that round
    s = Script(D, sparse).read("absent").rounds(2)
    sc["grow4"] = s.append(4).read("round of 4").append(1).read("one more op").rounds(1)
    # deep: nine entries, then reads at clocks between the earlier rounds
    s = Script(D, sparse).read("absent")
    mids, ends = [], [s.clk.R()]
    for r in range(8):
        s.append(2)
        mids.append(s.clk.R())
        s.append(3).read(f"round {r + 1}")
        ends.append(s.clk.R())
    s.append(2)
    for j in range(8):       # mids[j] lies between snapshots j and j + 1: slot 8 - j
        s.read(f"deep {8 - j}: between rounds {j} and {j + 1}", R=mids[j])
    for j in (1, 7):
        s.read(f"deep {8 - j}: equal to round {j}'s clock", R=ends[j])
    s.read("deep 5 as a GC read", R=mids[3], gc=True)
    sc["deep"] = s
    # below: after a collect, a read below every kept snapshot
    s = Script(D, sparse).read("absent")
    zero = s.clk.R()
    s.rounds(2)
    early = s.clk.R()
    s.rounds(7)
    s.read("below the kept snapshots", R=early).read("below, GC read", R=early, gc=True)
    s.read("at the initial clock, GC read", R=zero, gc=True).read("now")
    sc["below"] = s
    # gc_twice: the second GC read's LastOpCt is the head
    s = Script(D, sparse).read("absent").rounds(4).append(3)
    s.read("GC read", gc=True).read("GC read again", gc=True).append(1).read("now")
    sc["gc_twice"] = s
    # invalid: an included op with an invalid effect
    s = Script(D, sparse).read("absent").rounds(1).append(6, bad_at=2)
    s.read("invalid effect").read("invalid effect, GC read", gc=True)
    sc["invalid"] = s
    if sparse and D >= 3:
        full = (1 << D) - 1
        # ops with different DC sets (each holds its own DC)
        mixed = lambda t, c: full & ~(1 << ((c + 1 + t % 2) % D))  # noqa: E731
        s = Script(D, True).read("absent").rounds(3, masks=mixed).append(2, masks=mixed)
        sc["mixed_sets"] = s.read("GC read", gc=True).append(5, masks=mixed).read("now")
        # one DC set U inside R's: no op commits at the last DC
        U = full & ~(1 << (D - 1))
        s = Script(D, True, dcs=range(D - 1)).read("absent").rounds(3, masks=lambda t, c: U)
        sc["uniform_set"] = s.append(2, masks=lambda t, c: U).read("GC read", gc=True)
        # R lacks a DC the head snapshot holds above 0
        s = Script(D, True).read("absent").rounds(3)
        s.read("R lacks DC 0: the empty snapshot, deep", rm=full & ~1)
        s.append(5).read("GC read: the empty snapshot leaves", gc=True)
        s.read("R lacks the last DC: LOG", rm=full & ~(1 << (D - 1)))
        s.read("R lacks DC 0, GC read: LOG", rm=full & ~1, gc=True).append(5).read("now")
        sc["r_lacks_dc"] = s
    return sc
