"""Constructed inputs for the log ingest (agn_log_ingest), the stable-time
kernels (agn_gst_min / agn_gst_finalize / agn_gst_scalar) and the dependency
check (agn_dep_check) that sit on those kernels' edges (helper, no tests).

Like tests/edges.py nothing is drawn from a library generator: a small
congruential sequence with fixed seeds shapes the filler, so building a case
twice gives identical arrays.  Every case carries `edges`, the names of the
edges it is built to reach; tests/test_small_kernels_cpu.py asserts that each
is reached and tests/test_small_kernels.py runs the cases through the HIP
kernels, bit for bit against the C oracle.

The slot function, the table size, the GST launch plan and the dependency
check's group widths below mirror antidote_amd/csrc/ingest.hip and gst.hip:
they only steer the builders towards an edge and name it; what the kernels
must compute is always the oracle's result.
"""
from __future__ import annotations

import numpy as np

import domain
from antidote_amd import _abi
from edges import _garbage, pack_mask
from test_ingest import Records

U64 = (1 << 64) - 1
TOP = U64 - 1
M64 = 1 << 64


class Seq:
    """x -> (a x + c) mod 2^31, the high bits taken."""

    def __init__(self, seed):
        self.s = (seed * 2654435761 + 12345) % (1 << 31)

    def __call__(self, m):
        self.s = (self.s * 1103515245 + 12345) % (1 << 31)
        return (self.s >> 8) % m


# ====================================================================== ingest
GOLD = 0x9E3779B97F4A7C15            # ingest.hip slot_of
GOLD_INV = pow(GOLD, -1, M64)


def table_size(n_commits):
    """ingest.hip table_mask + 1."""
    T = 16
    while T < n_commits + n_commits // 2 + 1:
        T <<= 1
    return T


def slot_of(t, T):
    return ((t * GOLD % M64) >> 20) & (T - 1)


def txid_in_slot(s, j):
    """A txid (distinct per (s, j), 1 <= j < 2^20) whose slot is s in every
    table of at most 2^20 slots."""
    assert 0 < j < (1 << 20)
    return (((s << 20) | (j << 40) | j) * GOLD_INV) % M64


class IngestCase(Records):
    """test_ingest.Records' arrays (its struct / out_arrays and oracle_ingest
    apply) from an explicit record list: ("u", txid, key) / ("c", txid) /
    ("o", txid), in log order."""

    def __init__(self, name, edges, recs, K, D, crdt=_abi.COUNTER_PN, sparse=False,
                 commit_dc=None, rem_len=None, meta=None):
        n, W = len(recs), (D + 63) // 64
        self.name, self.edges, self.meta = name, list(edges), dict(meta or {})
        self.K, self.D, self.W, self.crdt, self.sparse, self.n = K, D, W, crdt, sparse, n
        self.kind = np.array([{"u": 1, "c": 2, "o": 0}[r[0]] for r in recs], np.uint8)
        self.txid = np.array([r[1] for r in recs], np.uint64)
        self.key = np.array([r[2] if len(r) > 2 else 0 for r in recs], np.uint64)
        x = np.arange(n, dtype=np.int64)
        d = np.arange(D, dtype=np.int64)
        cds = commit_dc if commit_dc is not None else [(3 * i + 1) % D for i in range(7)]
        self.commit_dc = np.array([cds[i % len(cds)] for i in range(n)], np.uint32)
        self.ss = (1_000_000 + ((x * 37) % 1500)[:, None] + ((d * 11) % 300)[None, :]).astype(
            np.uint64)
        self.commit_time = (self.ss.max(axis=1) if n else np.zeros(0, np.uint64)) + \
            (1 + x % 50).astype(np.uint64)
        self.ss_mask = None
        if sparse:
            pres = ((x[:, None] * 5 + d[None, :] * 3) % 4) != 0
            self.ss_mask = pack_mask(pres) if n else np.zeros((0, W), np.uint64)
            self.ss[~pres] = _garbage(int((~pres).sum()), 11)
        if crdt == _abi.COUNTER_PN:
            self.eff = ((x * 37) % 2001 - 1000).astype(np.int64)
            self.tag = self.add_tok = self.rem_off = self.rem_tok = None
        else:
            self.eff = None
            self.tag = ((x * 7) % 5).astype(np.uint32)
            self.add_tok = np.where(x % 10 < 7, x + 1, 0).astype(np.uint64)
            lens = np.array([(rem_len(i) if rem_len else (i * 5 + 3) % 4) for i in range(n)],
                            np.int64)
            self.rem_off = np.zeros(n + 1, np.uint32)
            self.rem_off[1:] = np.cumsum(lens)
            tot = int(self.rem_off[-1])
            owner = np.repeat(x, lens)
            self.rem_tok = (((owner + 1) << 20) | (np.arange(tot) % (1 << 20) + 1)).astype(
                np.uint64) if tot else np.array([0], np.uint64)
        self.max_t = self.max_m = None

    def with_max(self, refuse_all=False):
        """Even keys admit every commit; odd keys a share of them; in the masked
        form every fourth key's Max lacks a DC (it reads 0 there)."""
        K, D = self.K, self.D
        k = np.arange(K, dtype=np.int64)[:, None]
        d = np.arange(D, dtype=np.int64)[None, :]
        t = np.where(k % 2 == 0, 1800 + 0 * d, 600 + (k * 13) % 900 + (d * 11) % 300)
        if refuse_all:
            t = 0 * t - 1_000_000 + 5
        self.max_t = (1_000_000 + t).astype(np.uint64)
        if self.sparse:
            pres = np.ones((K, D), bool) | (d < 0)
            pres &= ~((k % 4 == 1) & ((k * 3 + d) % 19 == 0))
            self.max_m = pack_mask(pres)
            self.max_t[~pres] = _garbage(int((~pres).sum()), 12)
        return self

    def commits(self):
        return np.flatnonzero(self.kind == _abi.REC_COMMIT)

    def table(self):
        """(T, slot per commit record) of the kernel's commit table."""
        c = self.commits()
        T = table_size(len(c))
        return T, [slot_of(int(self.txid[x]), T) for x in c]


def mixed_log(n, K, seed=1, txid_of=lambda t: 1000 + 7 * t, n_open=4, foreign=0, commit=8):
    """Exactly n records: n_open transactions in flight, 1..4 updates each,
    then a commit (commit / 10 of them), an abort or nothing."""
    q = Seq(seed)
    recs, t_next = [], 0
    live = []
    while len(recs) < n:
        while len(live) < n_open:
            live.append([txid_of(t_next), 1 + q(4), q(10)])
            t_next += 1
        i = q(len(live))
        tx = live[i]
        if tx[1] > 0:
            key = K + q(50) if foreign and q(100) < foreign else q(K)
            recs.append(("u", tx[0], key))
            tx[1] -= 1
        else:
            if tx[2] < commit:
                recs.append(("c", tx[0]))
            elif tx[2] == commit:
                recs.append(("o", tx[0]))
            live.pop(i)
    return recs[:n]


def _interleave(streams, seed=3):
    """One log of the streams, each keeping its order."""
    q = Seq(seed)
    pos = [0] * len(streams)
    live = [i for i, s in enumerate(streams) if s]
    out = []
    while live:
        i = live[q(len(live))]
        out.append(streams[i][pos[i]])
        pos[i] += 1
        if pos[i] == len(streams[i]):
            live.remove(i)
    return out


def case_slot_chain(crdt=_abi.COUNTER_PN, D=3, sparse=False):
    """100 commit records (a 256-slot table): 40 txids in slot 5, 40 in the
    last slot (their chain wraps to slot 0), 10 each in slots 100 and 101
    (two chains that merge); uncommitted and aborted transactions in the same
    chains probe to their ends.  Updates first, commits in reverse order."""
    K = 64
    groups = [(5, 40), (255, 40), (100, 10), (101, 10)]
    assert table_size(sum(g[1] for g in groups)) == 256
    ups, cms, j = [], [], 1
    for s, m in groups:
        for _ in range(m):
            t = txid_in_slot(s, j)
            ups.append([("u", t, (j * 5 + i) % K) for i in range(1 + j % 3)])
            cms.append(("c", t))
            j += 1
    loose = []
    for s in (5, 255, 100):
        for _ in range(6):
            t = txid_in_slot(s, j)
            loose.append([("u", t, j % K)] + ([("o", t)] if j % 2 else []))
            j += 1
    recs = _interleave(ups + loose) + cms[::-1]
    return IngestCase(f"slot_chain-{crdt}-D{D}", ["slot_chain"], recs, K, D, crdt, sparse)


TOP_TXIDS = (U64, U64 - 1, 1, 1 << 63, 1 << 32)


def case_txid_top(crdt=_abi.COUNTER_PN, D=5, sparse=False):
    """Txids 2^64-1, 2^64-2, 1, 2^63 and 2^32, and six more in the slot of
    2^64-1 (11 commit records, a 32-slot table)."""
    K = 16
    T = table_size(len(TOP_TXIDS) + 6)
    s = slot_of(U64, T)
    tx = list(TOP_TXIDS) + [txid_in_slot(s, j) for j in range(1, 7)]
    streams = [[("u", t, (i * 3 + m) % K) for m in range(3)] + [("c", t)]
               for i, t in enumerate(tx)]
    return IngestCase(f"txid_top-{crdt}-D{D}", ["txid_top"], _interleave(streams, 5), K, D, crdt,
                      sparse, meta=dict(alias_slot=s, T=T))


def case_txid_reuse(crdt=_abi.COUNTER_PN, D=4, sparse=False):
    """A txid with more than one commit record: each update belongs to the
    first later commit of its txid (handle_commit erases the transaction)."""
    K = 12
    a, b, c, d, e = 501, 502, 503, 504, 505
    streams = [
        # u c u c
        [("u", a, 0), ("u", a, 1), ("c", a), ("u", a, 0), ("u", a, 2), ("c", a)],
        # u c c u c, and an update after the last commit (never emitted)
        [("u", b, 3), ("c", b), ("c", b), ("u", b, 3), ("u", b, 4), ("c", b), ("u", b, 5)],
        # a commit before any update of its txid, then updates, then a commit
        [("c", c), ("u", c, 6), ("u", c, 0), ("u", c, 7), ("c", c)],
        # two commits with no update between them, after an abort-like record
        [("u", d, 8), ("o", d), ("u", d, 9), ("c", d), ("c", d), ("u", d, 8)],
        # an ordinary transaction over several keys
        [("u", e, 0), ("u", e, 3), ("u", e, 6), ("u", e, 10), ("c", e)],
    ]
    return IngestCase(f"txid_reuse-{crdt}-D{D}", ["txid_reuse"], _interleave(streams, 7), K, D,
                      crdt, sparse)


def case_order(crdt=_abi.COUNTER_PN, D=3, sparse=False):
    """Commit order against first-update order on one key, many updates of
    one key inside a transaction, two transactions committing a key back to
    back."""
    a, b, c, d = 11, 12, 13, 14
    recs = [("u", a, 0), ("u", b, 0), ("u", c, 0), ("u", a, 1), ("u", b, 0),
            ("c", c), ("c", b), ("u", d, 0), ("c", a), ("c", d)]
    recs += [("u", 20, 2)] * 9 + [("u", 21, 2)] * 3 + [("c", 21), ("c", 20)]
    recs += [("u", 30, 3), ("u", 31, 3), ("c", 30), ("c", 31)]
    return IngestCase(f"order-{crdt}-D{D}", ["order"], recs, 5, D, crdt, sparse)


SIZES_N = (0, 1, 2, 255, 256, 257, 4095, 4096, 4097)
SIZES_K = (1, 2, 255, 256, 257)


def cases_sizes():
    out = []
    for i, n in enumerate(SIZES_N):
        crdt = (_abi.COUNTER_PN, _abi.SET_AW, _abi.REGISTER_MV)[i % 3]
        out.append(IngestCase(f"sizes-n{n}", ["sizes", f"n={n}"], mixed_log(n, 37, seed=n + 1),
                              37, 3 + i % 3, crdt, sparse=bool(i % 2)))
    out.append(IngestCase("sizes-n0-set", ["sizes", "n=0"], [], 5, 3, _abi.SET_AW, True))
    one = [("c", 9)]
    out.append(IngestCase("sizes-n1-commit", ["sizes", "n=1"], one, 3, 2))
    out.append(IngestCase("sizes-n2-uc", ["sizes", "n=2"], [("u", 9, 1), ("c", 9)], 3, 2))
    for K in SIZES_K:
        out.append(IngestCase(f"sizes-K{K}", ["sizes", f"n_keys={K}"],
                              mixed_log(900, K, seed=K), K, 4, sparse=bool(K % 2)).with_max())
    out.append(IngestCase("sizes-no-commit", ["sizes", "no_commit"],
                          mixed_log(300, 20, seed=5, commit=-1), 20, 3, _abi.SET_AW))
    out.append(IngestCase("sizes-only-commits", ["sizes", "only_commits"],
                          [("c", 100 + i // 2) for i in range(300)], 20, 3))
    out.append(IngestCase("sizes-all-foreign", ["sizes", "all_foreign"],
                          mixed_log(300, 20, seed=6, foreign=100), 20, 3, _abi.REGISTER_MV, True))
    out.append(IngestCase("sizes-all-refused", ["sizes", "all_refused"],
                          mixed_log(300, 20, seed=7), 20, 3, sparse=False).with_max(True))
    return out


def cases_key_gaps():
    K = 2000

    def on(keys, seed):
        recs = mixed_log(600, len(keys), seed=seed)
        return [(r[0], r[1], keys[r[2]]) if r[0] == "u" else r for r in recs]
    return [
        IngestCase("key_gaps-first", ["key_gaps", "only_key_0"], on([0], 1), K, 3),
        IngestCase("key_gaps-last", ["key_gaps", "only_last_key"], on([K - 1], 2), K, 3,
                   _abi.SET_AW),
        IngestCase("key_gaps-97", ["key_gaps", "every_97th"], on(list(range(0, K, 97)), 3), K, 3),
        IngestCase("key_gaps-run", ["key_gaps", "run_of_1000"],
                   on(list(range(0, 500)) + list(range(1500, K)), 4), K, 3, sparse=True),
    ]


REM_LENS = (0, 1, 63, 64, 65, 128, 129, 300)


def case_rem_lists(crdt, empty=False):
    """Removal lists of REM_LENS tokens on emitted updates, lists on updates
    that are not emitted (uncommitted, foreign) and on commit records."""
    K = 9
    streams = []
    for i, _ in enumerate(REM_LENS * 2):
        t = 700 + i
        streams.append([("u", t, i % K), ("u", t, (i + 4) % K), ("c", t)])
    streams.append([("u", 900, 1), ("u", 900, 2)])               # never committed
    streams.append([("u", 901, K + 3), ("c", 901)])               # foreign
    recs = _interleave(streams, 9)
    ups = [x for x, r in enumerate(recs) if r[0] == "u" and r[1] < 900]
    lens = {x: REM_LENS[j % len(REM_LENS)] for j, x in enumerate(ups)}
    for x, r in enumerate(recs):
        if r[0] == "c":
            lens[x] = 70 + x % 3
        elif r[1] >= 900:
            lens[x] = 100
    name = f"rem_lists-{crdt}" + ("-empty" if empty else "")
    return IngestCase(name, ["rem_lists", "all_empty" if empty else "long_lists"], recs, K, 3, crdt,
                      rem_len=(lambda x: 0) if empty else lens.__getitem__)


DC_WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)
COMMIT_DCS = (0, 62, 63, 64, 127, 128)


def case_dc_words(D, sparse):
    """D over the mask-word edges, the commit DC on bits 62..64 / 127 / 128 /
    D-1.  Masked: key 1's Max lacks DC `a`; transaction 801's commit carries
    `a` = 0 (admitted), 802's carries it non-zero (refused), 803's lacks it
    (admitted, garbage in the column)."""
    K = 8
    cds = sorted({c for c in COMMIT_DCS + (D - 1,) if c < D})
    recs = mixed_log(150, K, seed=D, n_open=3)
    special = []
    for t in (801, 802, 803):
        special += [("u", t, 1), ("u", t, 2), ("c", t)]
    recs = recs + special
    case = IngestCase(f"dc_words-D{D}-{'sparse' if sparse else 'dense'}", ["dc_words", f"D={D}"],
                      recs, K, D, _abi.COUNTER_PN if D % 2 else _abi.SET_AW, sparse,
                      commit_dc=cds)
    case.with_max()
    if sparse:
        a = D - 1
        base = len(recs) - 9
        cx = [base + 2, base + 5, base + 8]                       # the three commits
        for c in cx:                                              # small clocks: Max admits them
            case.ss[c] = 1_000_001
            case.ss_mask[c] = pack_mask(np.ones((1, D), bool))[0]
            case.commit_time[c] = 1_000_500
            case.commit_dc[c] = 0
        pres = np.ones((K, D), bool)
        pres[1, a] = False
        case.max_t[1] = 1_000_900
        case.max_t[2] = 1_000_900
        case.max_m[1] = pack_mask(pres[1:2])[0]
        case.max_m[2] = pack_mask(np.ones((1, D), bool))[0]
        case.max_t[1, a] = _garbage(1, 13)[0]
        case.ss[cx[0], a] = 0
        if D > 1:                                                 # D = 1: DC 0 is the only one
            m = np.ones((1, D), bool)
            m[0, a] = False
            case.ss_mask[cx[2]] = pack_mask(m)[0]
            case.ss[cx[2], a] = _garbage(1, 14)[0]
        else:
            case.ss[cx[2], a] = 0
        case.meta.update(absent_dc=a, commits=cx)
    return case


WIDE_MODES = domain.CLOCK_MODES


def widen(case, mode):
    """The case's values moved to the limits of the header's value domain: one
    increasing map over every present clock entry (snapshot times, commit
    times, Max), so the order of any two is kept; effects, tags and tokens by
    position.  The oracle runs on the widened case."""
    c = IngestCase.__new__(IngestCase)
    c.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v)
                       for k, v in case.__dict__.items()})
    c.name, c.edges = f"{case.name}/wide-{mode}", ["wide", mode] + list(case.edges)
    n, D = c.n, c.D
    sp = domain.present_bits(c.ss_mask, n, D)
    iscommit = (c.kind == _abi.REC_COMMIT)[:, None]
    sp = sp & iscommit
    mp = domain.present_bits(c.max_m, c.K, D) if c.max_t is not None else None
    vals = [c.ss[sp], c.commit_time[iscommit[:, 0]]] + ([c.max_t[mp]] if mp is not None else [])
    allv = np.concatenate(vals) if vals else np.zeros(0, np.uint64)
    if allv.size:
        mn, mx = int(allv.min()), int(allv.max())
        med = int(np.sort(c.ss[sp])[sp.sum() // 2]) if sp.any() else mn

        def f(v):
            v = v.astype(np.uint64)
            with np.errstate(over="ignore"):
                if mode == "hi32":
                    dlt = v - np.uint64(mn)
                    return (dlt << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - dlt)
                off = {"carry32": domain.B32 - med, "sign64": domain.B63 - med,
                       "top": domain.TOP - mx, "zero": -mn}[mode]
                return v + np.uint64(off % M64)
        assert mx - mn < (1 << 31)
        c.ss = np.where(sp, f(c.ss), c.ss)
        c.commit_time = np.where(iscommit[:, 0], f(c.commit_time), c.commit_time)
        if mp is not None:
            c.max_t = np.where(mp, f(c.max_t), c.max_t)
    x = np.arange(n, dtype=np.int64)
    if c.eff is not None:
        pool = np.array([domain.INT64_MAX, domain.INT64_MIN + 1, (1 << 32) + 3, -(1 << 32) - 3,
                         (1 << 31), -(1 << 31) - 1, 5, -7], np.int64)
        c.eff = pool[x % len(pool)] + np.where(x % len(pool) >= 2, x % 11, 0)
    else:
        c.tag = (np.uint32(0xFFFFFFFE) - (c.tag * np.uint32(0x1000193))).astype(np.uint32)
        hi = np.where(x % 3 == 0, np.uint64(U64), np.uint64(1 << 63))
        with np.errstate(over="ignore"):
            c.add_tok = np.where(c.add_tok != 0, hi - c.add_tok * np.uint64(x.size % 7 + 1),
                                 np.uint64(0)).astype(np.uint64)
            c.rem_tok = (np.uint64(U64) - c.rem_tok * np.uint64(0x100000001)).astype(np.uint64)
    return c


def ingest_base_cases():
    A = _abi
    out = [case_slot_chain(), case_slot_chain(A.SET_AW, 70, True).with_max(),
           case_txid_top(), case_txid_top(A.REGISTER_MV, 8, True).with_max(),
           case_txid_reuse(), case_txid_reuse(A.SET_AW, 16, True).with_max(),
           case_order(), case_order(A.REGISTER_MV, 5, True)]
    out += cases_sizes() + cases_key_gaps()
    out += [case_rem_lists(A.SET_AW), case_rem_lists(A.REGISTER_MV),
            case_rem_lists(A.SET_AW, empty=True)]
    out += [case_dc_words(D, s) for D in DC_WIDTHS for s in (False, True)]
    return out


def ingest_cases():
    """name -> case, every ingest case plain and widened (the widening mode
    rotates over the cases)."""
    out = {}
    for i, c in enumerate(ingest_base_cases()):
        out[c.name] = c
        w = widen(c, WIDE_MODES[i % len(WIDE_MODES)])
        out[w.name] = w
    return out


# ====================================================================== GST
GST_THREADS = 256                     # gst.hip
GST_STEPS = 32                        # block steps per band at least
COL_WIDTHS = (2, 4, 8, 16, 32, 64, 128, 256, 512)
GEN_WIDTHS = (1, 3, 5, 255, 257, 300, 2047, 2048, 2049, 4096)
SPECIAL = (0, 1 << 32, (1 << 63) - 1, 1 << 63, TOP)


def gst_plan(D, P, E, unroll=4, blocks=None, aligned=True):
    """launch_gst_min's choice: dict(kernel="cols" / "general", RG, U, rows
    (per band), bands)."""
    if D <= 2 * GST_THREADS and (2 * GST_THREADS) % D == 0 and D % 2 == 0 and aligned:
        RG = 2 * GST_THREADS // D
        target = blocks if blocks else 1024
        bands = (target + E - 1) // E
        rows = max((P + bands - 1) // bands, GST_STEPS * RG)
        rows = (rows + RG - 1) // RG * RG
        return dict(kernel="cols", RG=RG, U=unroll, rows=rows, bands=(P + rows - 1) // rows)
    rows = max(2048 // D, 1)
    return dict(kernel="general", RG=None, U=None, rows=rows, bands=(P + rows - 1) // rows)


def col_p_values(D, U):
    RG = 2 * GST_THREADS // D
    ps = [1, RG - 1, RG, RG + 1, U * RG - 1, U * RG, U * RG + 1, 32 * RG - 1, 32 * RG, 32 * RG + 1,
          3 * 32 * RG + 1]
    return sorted({p for p in ps if p >= 1})


def gen_p_values(D):
    r = max(2048 // D, 1)
    return sorted({p for p in (1, r - 1, r, r + 1, 2 * r + 1) if p >= 1})


class GstCase:
    """clocks [E][P][D], defined [E][P] or None.  Column d of epoch e plays
    role (3 d + e) mod 8: roles 0..4 put the column's minimum, SPECIAL[(d + e)
    mod 5], in one named row (the band's first row, the last row, the last
    slot of the unrolled loop, a row of the tail loop, a middle row) and larger
    values or nothing elsewhere; 5 is absent from every partition; 6 is
    present only in undefined partitions, holding 0; 7 holds its minimum in
    every defined row.  An undefined partition's row holds 0 wherever the
    column's minimum is above 0.  `undef`: "some" (a pattern per epoch), "all"
    or "none"; `null_defined` passes NULL (every partition defined)."""

    ROLES = ("min_first_row", "min_last_row", "min_unrolled_last", "min_tail_loop", "min_middle",
             "absent_everywhere", "only_undefined", "min_everywhere")

    def __init__(self, D, P, E, unroll=4, nt=True, blocks=None, undef="some", null_defined=False,
                 offset8=False):
        self.D, self.P, self.E = D, P, E
        self.unroll, self.nt, self.blocks = unroll, nt, blocks
        self.null_defined, self.offset8, self.undef = null_defined, offset8, undef
        self.plan = gst_plan(D, P, E, unroll, blocks, aligned=not offset8)
        pl = self.plan
        self.name = (f"D{D}-P{P}-E{E}-U{unroll}-nt{int(nt)}-b{blocks or 'dflt'}-{undef}"
                     f"{'-null' if null_defined else ''}{'-off8' if offset8 else ''}")
        # named rows
        rows = {"min_first_row": 0, "min_last_row": P - 1, "min_middle": P // 2,
                "min_unrolled_last": None, "min_tail_loop": None}
        if pl["kernel"] == "cols":
            RG, U = pl["RG"], pl["U"]
            p1 = min(pl["rows"], P)
            n_it = 0
            while n_it * U * RG + (U - 1) * RG < p1:
                n_it += 1
            if n_it:
                rows["min_unrolled_last"] = (n_it * U - 1) * RG
            if n_it * U * RG < p1:
                rows["min_tail_loop"] = n_it * U * RG
        self.rows = rows
        named = {r for r in rows.values() if r is not None}
        defined = np.ones((E, P), np.uint8)
        p = np.arange(P)
        if undef == "all":
            defined[:] = 0
        elif undef == "some" and not null_defined:
            for e in range(E):
                if e % 3 == 0:
                    defined[e, p % 7 == 3] = 0
                elif e % 3 == 2:
                    defined[e, p % 5 == 1] = 0
                    defined[e, P - 1] = 0
            if undef == "some":
                for r in named:
                    defined[:, r] = 1
        self.defined = None if null_defined else defined
        dfn = np.ones((E, P), bool) if null_defined else defined.astype(bool)
        clocks = np.full((E, P, D), U64, np.uint64)
        self.role = np.zeros((E, D), np.int64)
        self.minval = np.zeros((E, D), np.uint64)
        self.minrow = np.full((E, D), -1, np.int64)
        pp = np.arange(P, dtype=np.uint64)
        for e in range(E):
            for d in range(D):
                role = (3 * d + e) % 8
                name = self.ROLES[role]
                if role < 5 and rows[name] is None:
                    role, name = 0, "min_first_row"
                self.role[e, d] = role
                mv = SPECIAL[(d + e) % 5]
                col = clocks[e, :, d]
                if role == 5:
                    continue
                if role == 6:
                    col[~dfn[e]] = 0
                    continue
                bump = (pp * np.uint64(7919) + np.uint64(d)) % np.uint64(1000) + np.uint64(1)
                hi = np.minimum(np.uint64(mv) + np.minimum(bump, np.uint64(TOP - mv)),
                                np.uint64(TOP))
                if role == 7:
                    col[:] = np.uint64(mv)
                else:
                    col[:] = hi
                    col[(pp + np.uint64(d)) % np.uint64(3) == 1] = U64   # absent here and there
                    r = rows[name]
                    col[r] = mv
                    self.minrow[e, d] = r
                if mv > 0:
                    col[~dfn[e]] = 0
                self.minval[e, d] = mv
        self.clocks = clocks
        self.edges = sorted({self.ROLES[r] for r in np.unique(self.role)} |
                            {f"value_{v:#x}" for v in np.unique(self.minval)})


def gst_col_cases(D, unroll, nt, null_defined, single_band):
    """The column kernel's shapes of one width under one knob setting: every
    P of col_p_values with E = 1 and 3; (cases, AGN_GST_BLOCKS or None)."""
    out = []
    for P in col_p_values(D, unroll):
        for E in (1, 3):
            blocks = 1 if single_band else 4 * E
            out.append(GstCase(D, P, E, unroll, nt, blocks, null_defined=null_defined))
    return out


def gst_general_cases(D, null_defined):
    return [GstCase(D, P, E, null_defined=null_defined) for P in gen_p_values(D) for E in (1, 3)]


def gst_misaligned_cases():
    return [GstCase(D, P, E, offset8=True) for D in (2, 8, 256) for P in gen_p_values(D)
            for E in (1, 3)]


def gst_undefined_cases():
    """Every partition undefined; P = 1 undefined."""
    out = []
    for D in (2, 8, 512, 5, 300):
        out += [GstCase(D, 1, 1, undef="all"), GstCase(D, 1, 3, undef="all"),
                GstCase(D, 70, 3, undef="all"), GstCase(D, 2 * (2048 // D) + 1, 1, undef="all")]
    return out


def classify_row(plan, P, p):
    """Where the column kernel reads row p: (band, loop, slot, last turn) with
    loop "unrolled" / "tail" and last turn = the unrolled loop's final
    iteration, by walking the owning thread's loops as k_gst_cols does."""
    RG, U, rows = plan["RG"], plan["U"], plan["rows"]
    band = p // rows
    p0 = band * rows
    p1 = min(p0 + rows, P)
    q = p0 + (p - p0) % RG
    while q + (U - 1) * RG < p1:
        for k in range(U):
            if q + k * RG == p:
                return band, "unrolled", k, not (q + U * RG + (U - 1) * RG < p1)
        q += U * RG
    while q < p1:
        if q == p:
            return band, "tail", 0, False
        q += RG
    raise AssertionError("row not read")


# ====================================================================== dep check
DEP_LDS = 48 << 10                    # gst.hip
DEP_WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)


def dep_group(D):
    for g in (1, 2, 4, 8, 16, 32):
        if D <= g:
            return g
    return 64


def dep_stage_bytes(D, P, sparse):
    return (P * D + (P * ((D + 63) // 64) if sparse else 0)) * 8


def dep_stage_pair(D, sparse):
    """(largest P that is staged, P + 1)."""
    per = dep_stage_bytes(D, 1, sparse)
    return DEP_LDS // per, DEP_LDS // per + 1


class DepCase:
    """deps at or below the partition clock; every second transaction has one
    DC ahead of it, cycling over the group's last lane, DC 0, D - 1 and
    others, with the origin cycling over 0, D - 1, the ahead DC, D and D + 5
    (an origin >= D exempts no column).  bad_part: every fifth transaction
    names a partition >= n_parts."""

    def __init__(self, D, n, P, sparse, bad_part=False, wide=None, edges=()):
        self.D, self.n, self.P, self.sparse = D, n, P, sparse
        self.name = f"D{D}-n{n}-P{P}-{'sparse' if sparse else 'dense'}" + \
            ("-badpart" if bad_part else "") + (f"-{wide}" if wide else "")
        self.edges = list(edges)
        W = (D + 63) // 64
        t = np.arange(n, dtype=np.int64)
        d = np.arange(D, dtype=np.int64)
        pp = np.arange(P, dtype=np.int64)
        pc = (1000 + (pp[:, None] * 131 + d[None, :] * 17) % 1000).astype(np.uint64)
        part = np.where(t % 3 == 0, P - 1 - (t // 3) % P, (t * 7 + 1) % P).astype(np.uint32)
        G = dep_group(D)
        last_lane = min(D, G) - 1 if D <= 64 else 63 + 64 * ((D - 64) // 64)
        cols = np.array([last_lane, 0, D - 1, 0, 0], np.int64)
        col = np.where(t % 5 == 3, (t * 5) % D, np.where(t % 5 == 4, (t * 3 + 1) % D,
                                                         cols[t % 5]))
        origs = np.stack([0 * t, D - 1 + 0 * t, col, D + 0 * t, D + 5 + 0 * t, (t * 11) % D])
        origin = origs[(t // 2) % 6, t].astype(np.uint32)
        deps = (pc[part] - ((t[:, None] * 3 + d[None, :]) % 40).astype(np.uint64)).astype(np.uint64)
        ahead = t % 2 == 1
        deps[ahead, col[ahead]] = pc[part[ahead], col[ahead]] + np.uint64(1)
        dm = pm = None
        if sparse:
            ppres = ((pp[:, None] * 3 + d[None, :]) % 5) != 0
            dpres = (((t[:, None] * 7 + d[None, :] * 3) % 10) >= 3) & ppres[part]
            extra = t % 10 == 6
            dpres[extra, (t[extra] * 3) % D] = True
            dpres[ahead, col[ahead]] |= (t[ahead] % 4 != 3)
            pm, dm = pack_mask(ppres), pack_mask(dpres)
            pc[~ppres] = _garbage(int((~ppres).sum()), 21)
            deps[~dpres] = _garbage(int((~dpres).sum()), 22)
        if wide:
            deps, pc = domain.remap_columns([deps, pc], [dm, pm], wide)
        self.bad = np.zeros(n, bool)
        if bad_part:
            self.bad = t % 5 == 2
            part = part.copy()
            part[self.bad] = np.where(t[self.bad] % 2 == 0, P, 0xFFFFFFFF).astype(np.uint32)
        self.deps, self.dm, self.origin, self.part = deps, dm, origin, part
        self.pc, self.pm = pc, pm
        self.col, self.ahead, self.last_lane = col, ahead, last_lane

    def arrays(self):
        return self.deps, self.dm, self.origin, self.part, self.pc, self.pm

    def good_rows(self):
        """The case restricted to the transactions with a known partition."""
        g = ~self.bad
        return (np.ascontiguousarray(self.deps[g]),
                None if self.dm is None else np.ascontiguousarray(self.dm[g]),
                np.ascontiguousarray(self.origin[g]), np.ascontiguousarray(self.part[g]),
                self.pc, self.pm)


def dep_cases():
    out = []
    for D in DEP_WIDTHS:
        tpw = 64 // dep_group(D)
        for n in sorted({1, tpw - 1, tpw, tpw + 1, 5 * tpw + 1} - {0}):
            out.append(DepCase(D, n, 7, sparse=bool(D % 2), edges=["group_width", "tile_tail",
                                                                    "origin", "last_lane"]))
    for D in (8, 64, 130):
        for sparse in (False, True):
            for P in dep_stage_pair(D, sparse):
                out.append(DepCase(D, 301, P, sparse, edges=["stage_limit"]))
    for D, sparse, mode in ((8, False, "carry32"), (5, True, "sign64"), (64, True, "carry32"),
                            (130, False, "sign64")):
        out.append(DepCase(D, 257, 11, sparse, wide=mode, edges=["wide"]))
    for D, sparse in ((3, True), (8, False), (64, True), (130, False)):
        out.append(DepCase(D, 203, 9, sparse, bad_part=True, edges=["bad_part"]))
    return out
