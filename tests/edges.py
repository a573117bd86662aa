"""Constructed logs that sit on the kernels' structural edges (helper, no tests).

The randomised parity tests draw their shapes; the builders here place one
named edge per key instead: a key length on a chunk / sub-iteration width,
the one excluded / included / invalid op on a chunk's last or first lane, a
live state exactly on a table limit, a removal token at a batch edge of the
chunk's token range, an op over a chunk edge, a keep pattern that cuts a
GC segment at a wave width.  Nothing is drawn: building a family twice gives
identical arrays.

Every materialize builder returns (log, req, cap, names); names[i] labels
request i's edge ("n=65 I64 X1 col=15") for assertion messages.  The GC
builders return (log, prune, thr, thr_mask, names), names per key.
"""
from __future__ import annotations

import numpy as np

from antidote_amd import _abi
from antidote_amd.encode import EncodedLog, EncodedRead, n_words, state_capacity

LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256,
           257)
POSITIONS = (0, 15, 16, 31, 32, 63, 64, 65, 127, 128)
LIVE_SIZES = (0, 1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 4095, 4096, 4097)
TOKEN_TOTALS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 300)
DROPS = (1, 31, 32, 33, 63, 64, 65)
READ_TXID = 77
GUARD_TAG, GUARD_TOK = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
FAST_CAP, SLOW_CAP, WAVE = 256, 4096, 64


def positions(n):
    """Family A's positions inside a key of n entries."""
    return sorted({p for p in POSITIONS + (n - 2, n - 1) if 0 <= p < n})


def rle(pat):
    """"IIIXI" -> "I3 X1 I1"."""
    out, i = [], 0
    while i < len(pat):
        j = i
        while j < len(pat) and pat[j] == pat[i]:
            j += 1
        out.append(f"{pat[i]}{j - i}")
        i = j
    return " ".join(out) if out else "-"


def one_at(n, p, one, rest):
    return rest * p + one + rest * (n - p - 1)


def pack_mask(present):
    """bool [n, D] -> presence words [n, W]."""
    n, D = present.shape
    m = np.zeros((n, n_words(D)), np.uint64)
    for d in range(D):
        m[:, d >> 6] |= present[:, d].astype(np.uint64) << np.uint64(d & 63)
    return m


def _garbage(shape, salt):
    n = int(np.prod(shape))
    return ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt))
            & np.uint64((1 << 50) - 1) | np.uint64(1 << 61)).reshape(shape)


def _entry_ops(pat):
    """Per entry: its op's index and class letter.  A lower-case letter is a
    further entry of the previous op (same id, clock, txid and DC set)."""
    letters = np.frombuffer(pat.encode(), np.uint8)
    cont = letters >= 97
    assert not len(letters) or not cont[0], pat
    opi = np.cumsum(~cont) - 1
    up = letters & np.uint8(0xDF)
    cls = up[np.flatnonzero(~cont)][opi] if len(letters) else up
    return opi, cls, up == ord("E")


def lww_fields(k, n):
    """register_lww entries of key k (tag = value id, add_tok = timestamp):
    even keys walk the edges of both domains (lww_model.TS_EDGE / TAG_EDGE: 0,
    2^32 +- 1, 2^63, 2^64 - 1 pass through whatever stages the 64-bit field),
    odd keys a small range in which ties at the top timestamp are common."""
    from lww_model import TAG_EDGE, TS_EDGE
    m = np.arange(n)
    if k % 2 == 0:
        ts = np.array(TS_EDGE, np.uint64)[(m * 3 + k // 2) % len(TS_EDGE)]
        tag = np.array(TAG_EDGE, np.uint32)[(m + k // 2) % len(TAG_EDGE)]
    else:
        ts = (1 + (m * 5 + k) % 4).astype(np.uint64)
        tag = ((m * 7 + k) % 3).astype(np.uint32)
    return tag, ts


def default_effects(crdt, k, n):
    """Entry m adds token (k+1, m+1) under elem / value 7m mod 5; every
    fourth entry removes the add five entries back (the same elem) and a
    token nobody added.  register_lww: lww_fields, no removals."""
    if crdt == _abi.REGISTER_LWW:
        return lww_fields(k, n) + ([[] for _ in range(n)],)
    m = np.arange(n)
    tag = ((m * 7) % 5).astype(np.uint32)
    add = (np.uint64(k + 1) << np.uint64(32)) | (m + 1).astype(np.uint64)
    rems = [[int(add[i - 5]), (9 << 56) | i] if i % 4 == 1 and i >= 5 else [] for i in range(n)]
    return tag, add, rems


def from_patterns(crdt, D, patterns, *, sparse=None, col=None, identity=True, effects=None,
                  base=None, room=None, names=None, mixed_keys=None):
    """One key per pattern string, oldest op first, one letter per entry:
    I included; X excluded (column col above R); P in the previous snapshot
    (every column <= SCT, the key is warm); T like P with the reading TxId;
    E included with EFFECT_INVALID / TAG_INVALID; lower case = a further
    entry of the previous op.

    sparse: None (dense), "uniform" (every entry of a key carries the key's
    DC set) or "mixed" (entries differ; mixed_keys limits that to some keys).
    Absent columns of op rows, R and SCT hold garbage.
    effects[k] = (tag, add_tok, removal lists) and base[k] = [(tag, tok)]
    override the default effects / empty base of set_aw and register_mv keys;
    room[i] overrides request i's output capacity."""
    K, W = len(patterns), n_words(D)
    lens = np.array([len(p) for p in patterns], np.int64)
    key_off = np.zeros(K + 1, np.uint64)
    key_off[1:] = np.cumsum(lens)
    E = int(key_off[-1])
    oc = np.zeros((E, D), np.uint64)
    pres = np.ones((E, D), bool)
    op_id = np.zeros(E, np.uint32)
    txid = np.zeros(E, np.uint64)
    invalid = np.zeros(E, bool)
    R = np.zeros((K, D), np.uint64)
    sct = np.zeros((K, D), np.uint64)
    Rp, Sp = np.ones((K, D), bool), np.ones((K, D), bool)
    sct_ign = np.ones(K, np.uint8)
    rtx = np.zeros(K, np.uint64)
    cols = []
    for k, pat in enumerate(patterns):
        n, a = len(pat), int(key_off[k])
        c = (k % D) if col is None else int(col if np.isscalar(col) else col[k]) % D
        cols.append(c)
        opi, cls, inv = _entry_ops(pat)
        S = 1000 + n + 5
        Rc = S + n + 10
        rows = np.repeat((1000 + opi)[:, None], D, axis=1)
        inc = (cls == ord("I")) | (cls == ord("E"))
        exc = cls == ord("X")
        assert (inc | exc | (cls == ord("P")) | (cls == ord("T"))).all(), pat
        rows[inc, c] = S + 1 + opi[inc]
        rows[exc, c] = Rc + 1 + opi[exc]
        oc[a:a + n] = rows
        op_id[a:a + n] = 5 + 3 * opi
        txid[a:a + n] = np.where(cls == ord("T"), READ_TXID, 1000 + opi)
        invalid[a:a + n] = inv
        R[k], sct[k] = S, S
        R[k, c] = Rc
        has_t = "T" in pat
        if "P" in pat or has_t or k % 3 == 2:
            sct_ign[k] = 0
        if has_t or k % 2 == 0:
            rtx[k] = READ_TXID
        if sparse and D >= 2:
            U = np.ones(D, bool)
            if D >= 3 and k % 2 == 1:
                U[(c + 1) % D] = False
            pres[a:a + n] = U
            if sparse == "mixed" and (mixed_keys is None or k in mixed_keys):
                drop = (c + 2) % D if D >= 3 else (c + 1) % D
                pres[a:a + n, drop] &= (opi % 3 != 1)
            Rp[k] = U if k % 4 == 3 else True
            Sp[k] = U if k % 2 == 0 else True
    log = EncodedLog(crdt_type=crdt, n_dcs=D, key_off=key_off, key_type=np.full(K, crdt, np.uint8),
                     oc=oc, oc_mask=None, op_id=op_id, txid=txid)
    if sparse:
        log.oc_mask = pack_mask(pres)
        oc[~pres] = _garbage(int((~pres).sum()), 1)
        R[~Rp] = _garbage(int((~Rp).sum()), 2)
        sct[~Sp] = _garbage(int((~Sp).sum()), 3)
    if crdt == _abi.COUNTER_PN:
        eff = np.zeros(E, np.int64)
        for k in range(K):
            a, n = int(key_off[k]), int(lens[k])
            m = np.arange(n, dtype=np.int64)
            eff[a:a + n] = (m * 37 + k) % 2001 - 1000
        eff[invalid] = _abi.EFFECT_INVALID
        log.eff = eff
    else:
        tag = np.zeros(E, np.uint32)
        add = np.zeros(E, np.uint64)
        rem_off = np.zeros(E + 1, np.uint32)
        rem = []
        for k in range(K):
            a, n = int(key_off[k]), int(lens[k])
            t, ad, rl = effects[k] if effects and effects.get(k) is not None \
                else default_effects(crdt, k, n)
            assert len(t) == len(ad) == len(rl) == n, (k, n)
            tag[a:a + n], add[a:a + n] = t, ad
            for m in range(n):
                rem.extend(rl[m])
                rem_off[a + m + 1] = len(rem)
        tag[invalid] = _abi.TAG_INVALID
        log.tag, log.add_tok, log.rem_off = tag, add, rem_off
        log.rem_tok = np.array(rem if rem else [0], np.uint64)
    boff = np.zeros(K + 1, np.uint64)
    btag, btok = [], []
    if crdt != _abi.COUNTER_PN:
        for k in range(K):
            for t, tk in (base or {}).get(k, []):
                btag.append(t)
                btok.append(tk)
            boff[k + 1] = len(btag)
    keys = np.arange(K, dtype=np.uint64)
    bval = (np.arange(K, dtype=np.int64) * 11) % 97 - 48
    Rm, Sm = pack_mask(Rp), pack_mask(Sp)
    if not sparse:
        Rm, Sm = np.zeros((K, W), np.uint64), np.zeros((K, W), np.uint64)
    labels = list(names) if names is not None else \
        [f"n={len(p)} {rle(p)} col={c}" for p, c in zip(patterns, cols)]
    if not identity:
        assert not base and room is None
        keys = keys[::-1].copy()
        ix = keys.astype(np.int64)
        R, Rm, sct, Sm, sct_ign, rtx, bval = R[ix], Rm[ix], sct[ix], Sm[ix], sct_ign[ix], \
            rtx[ix], bval[ix]
        labels = [labels[i] for i in ix]
    req = EncodedRead(n_dcs=D, req_type=crdt, keys=keys, R=np.ascontiguousarray(R),
                      R_mask=np.ascontiguousarray(Rm), sct=np.ascontiguousarray(sct),
                      sct_mask=np.ascontiguousarray(Sm), sct_ignore=np.ascontiguousarray(sct_ign),
                      txid=np.ascontiguousarray(rtx), base_value=np.ascontiguousarray(bval),
                      base_off=boff, base_tag=np.array(btag, np.uint32),
                      base_tok=np.array(btok, np.uint64))
    cap = None
    if crdt != _abi.COUNTER_PN:
        cap = state_capacity(log, req)
        if room is not None:
            sizes = np.diff(cap).astype(np.int64)
            for i, r in room.items():
                sizes[i] = r
            cap = np.zeros(K + 1, np.uint64)
            cap[1:] = np.cumsum(sizes)
    return log, req, cap, labels


# ------------------------------------------------------------------ family A: scan edges
def family_a_patterns(lengths=LENGTHS):
    pats = []
    for n in lengths:
        pats += ["I" * n, "X" * n]
        for p in positions(n):
            pats += [one_at(n, p, "X", "I"), one_at(n, p, "I", "P"), one_at(n, p, "T", "P"),
                     one_at(n, p, "E", "I")]
            if p + 1 < n:   # an E newer than the X
                pats.append("I" * p + "XE" + "I" * (n - p - 2))
            if p >= 1:      # an E older than the X
                pats.append("I" * (p - 1) + "EX" + "I" * (n - p - 1))
        if n >= 65:
            pats.append("I" * 63 + "EE" + "I" * (n - 65))
    return pats


def family_a(crdt, D, sparse=None, identity=True, lengths=LENGTHS):
    return from_patterns(crdt, D, family_a_patterns(lengths), sparse=sparse, identity=identity)


# ------------------------------------------------------------------ family B: table edges
def _tok(k, m):
    """Tokens that descend in add order."""
    return (np.uint64(k + 1) << np.uint64(32)) | np.uint64((1 << 20) - m)


def _adds(k, n, tag_of=lambda m: m % 3):
    tag = np.array([tag_of(m) for m in range(n)], np.uint32)
    add = np.array([_tok(k, m) for m in range(n)], np.uint64)
    return tag, add, [[] for _ in range(n)]


def _base_pairs(crdt, k, B):
    """B base pairs in the reference's state order."""
    pairs = [(x % 2, (1 << 60) | (k << 12) | (B - x)) for x in range(B)]
    pairs.sort(key=(lambda p: p[0]) if crdt == _abi.SET_AW else None)
    return pairs


def _churn(k, n, start=0, prev=None):
    """n entries, each adding a token and removing the previous entry's."""
    tag = np.full(n, 3, np.uint32)
    add = np.array([_tok(k, start + m) for m in range(n)], np.uint64)
    rems = [[int(add[m - 1])] if m else ([int(prev)] if prev is not None else [])
            for m in range(n)]
    return tag, add, rems


def _cat(*parts):
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
            [r for p in parts for r in p[2]])


def model_used(crdt, base_pairs, tag, add, rems, cap=FAST_CAP):
    """Host model of a candidate table's `used` for a key whose entries are
    all included: slots fill by 64-entry chunks, dead pairs leave only when a
    chunk's adds do not fit.  Returns (compactions, overflow)."""
    B = len(base_pairs)
    if cap == FAST_CAP and B > FAST_CAP - WAVE:
        return 0, True
    slots = [[tk, t, x, False] for x, (t, tk) in enumerate(base_pairs)]
    by_tok: dict = {}
    for s in slots:
        by_tok.setdefault(s[0], []).append(s)
    used, comp = B, 0
    for c0 in range(0, len(add), WAVE):
        c1 = min(c0 + WAVE, len(add))
        n_add = int((add[c0:c1] != 0).sum())
        if used + n_add > cap:
            comp += 1
            slots = [s for s in slots if not s[3]]
            used = len(slots)
            if used + n_add > cap:
                return comp, True
        for m in range(c0, c1):
            if add[m]:
                s = [int(add[m]), int(tag[m]), B + m, False]
                slots.append(s)
                by_tok.setdefault(s[0], []).append(s)
        used += n_add
        for m in range(c0, c1):
            for t in rems[m]:
                for s in by_tok.get(int(t), ()):
                    if (crdt != _abi.SET_AW or s[1] == int(tag[m])) and B + m > s[2]:
                        s[3] = True
    return comp, False


def family_b(crdt, D, sparse=None, sizes=LIVE_SIZES):
    """Live states on the limits of the fast (256) and slow (4096) tables.
    Returns (log, req, cap, names, meta): meta[i] = dict(L=intended live size,
    compacts=.., overflow=.., room=.., guard=..)."""
    pats, eff, base, names, meta, room = [], {}, {}, [], {}, {}

    def key(n, e, label, B=0, pat=None, **m):
        k = len(pats)
        pats.append(pat if pat is not None else "I" * n)
        eff[k] = e
        if B:
            base[k] = _base_pairs(crdt, k, B)
        names.append(label)
        meta[k] = m
        return k

    for L in sizes:
        for B in (0, 1, 4):
            if L < B:
                continue
            k = len(pats)
            key(L - B, _adds(k, L - B), f"L={L} base={B} adds={L - B} tokens descending", B=B, L=L)
    k = len(pats)
    key(600, _churn(k, 600), "churn 600 -> 1 live", L=1, compacts=True)
    k = len(pats)
    tail = _churn(k, 64, start=900, prev=_tok(k, 575))
    key(832, _cat(_churn(k, 576), _adds(k + 4096, 192), tail),
        "churn 576, 192 adds, churn 64 -> 193 live, slow pass", L=193, compacts=True,
        overflow=True)
    k = len(pats)
    n = 5000
    add = np.array([_tok(k, m) for m in range(n)], np.uint64)
    rems = [[int(add[m - 65])] if m >= 65 and (m - 65) % 2 == 0 else [] for m in range(n)]
    key(n, (np.zeros(n, np.uint32), add, rems), "5000 adds, every second removed 65 later",
        L=n - len(range(0, n - 65, 2)), overflow=True)
    # room one pair too small, guarded neighbours on both sides
    for L in (1, 65, 193, 257):
        k = len(pats)
        key(3, _adds(k, 3), f"neighbour before room L={L}", L=3, guard=True)
        k = len(pats)
        key(L, _adds(k, L), f"room={L - 1} for L={L}", L=L, room=L - 1)
        room[k] = L - 1
        k = len(pats)
        key(3, _adds(k, 3), f"neighbour after room L={L}", L=3, guard=True)
    # an invalid op after the table has overflowed: the error wins, no capacity flag
    k = len(pats)
    key(332, _adds(k, 332), "330 adds then E (overflow, then the error)", pat="I" * 330 + "EI",
        err=330)
    k = len(pats)
    key(2, _adds(k, 2), "base 193 then E", B=193, pat="IE", err=1)
    log, req, cap, _ = from_patterns(crdt, D, pats, effects=eff, base=base, room=room, col=D - 1,
                                     sparse=sparse)
    for k in range(len(pats)):   # cold keys: no SCT, no TxId games
        req.sct_ignore[k] = 1
    return log, req, cap, names, meta


def family_b300(crdt, D, sparse=None):
    """300 keys whose 193 base pairs overflow the fast table at once: more
    hand-ons than the slow pass's 256 blocks."""
    K = 300
    pats = ["I" * (k % 3) for k in range(K)]
    eff = {k: _adds(k, k % 3, tag_of=lambda m: 5) for k in range(K)}
    base = {k: _base_pairs(crdt, k, 193) for k in range(K)}
    names = [f"base=193 adds={k % 3}" for k in range(K)]
    log, req, cap, _ = from_patterns(crdt, D, pats, effects=eff, base=base, sparse=sparse)
    return log, req, cap, names


# ------------------------------------------------------------------ family C: removal tokens
def _chunk_lists(T, tokens):
    """T tokens over the 64 entries of a chunk, as even as possible."""
    q, r = divmod(T, WAVE)
    out, at = [], 0
    for m in range(WAVE):
        ln = q + (1 if m < r else 0)
        out.append(tokens[at:at + ln])
        at += ln
    return out


def family_c(crdt, D, sparse=None):
    """Keys of two chunks.  Chunk 1's removal lists total T tokens; one of
    them, at index idx of the chunk's token range, names an add.  meta[i] =
    dict(T=, idx=, target=, dies=bool, tok=the add's token)."""
    pats, eff, names, meta = [], {}, [], {}

    def key(T, idx, target, other_elem=False):
        k = len(pats)
        n = 2 * WAVE
        tag = np.ones(n, np.uint32)
        add = (np.uint64(k + 1) << np.uint64(32)) | np.arange(1, n + 1, dtype=np.uint64)
        toks = [(7 << 56) | (k << 12) | x for x in range(T)]
        lists = _chunk_lists(T, toks)
        owner = next(m for m in range(WAVE) if sum(len(x) for x in lists[:m + 1]) > idx)
        tgt = {"earlier chunk": 5, "earlier entry": WAVE + owner - 1, "same entry": WAVE + owner,
               "later entry": WAVE + owner + 1}[target]
        if target == "earlier entry" and owner == 0 or tgt >= n:
            return
        at = idx - sum(len(x) for x in lists[:owner])
        lists[owner] = list(lists[owner])
        lists[owner][at] = int(add[tgt])
        if other_elem:
            tag[tgt] = 2
        pats.append("I" * n)
        eff[k] = (tag, add, [[] for _ in range(WAVE)] + lists)
        dies = target in ("earlier chunk", "earlier entry") and not (other_elem and
                                                                    crdt == _abi.SET_AW)
        names.append(f"T={T} idx={idx} owner={WAVE + owner} target={target}"
                     + (" other elem" if other_elem else ""))
        meta[k] = dict(T=T, idx=idx, dies=dies, tok=int(add[tgt]), chunk=1)

    for T in TOKEN_TOTALS:
        for idx in sorted({i for i in (0, 63, 64, 127, 128, T - 1) if i < T}):
            for target in ("earlier chunk", "earlier entry", "same entry", "later entry"):
                key(T, idx, target)
            if crdt == _abi.SET_AW:
                key(T, idx, "earlier chunk", other_elem=True)
    # one list over a 64-token batch edge, empty lists on both sides
    for owner_cls in "IXP":
        k = len(pats)
        n = 2 * WAVE
        tag = np.ones(n, np.uint32)
        add = (np.uint64(k + 1) << np.uint64(32)) | np.arange(1, n + 1, dtype=np.uint64)
        toks = [(7 << 56) | (k << 12) | x for x in range(160)]
        lists = [[] for _ in range(n)]
        for m in range(6):
            lists[WAVE + m] = toks[5 * m:5 * m + 5]           # chunk tokens 0..29
        span = toks[30:130]                                   # chunk tokens 30..129
        hits = {63: 3, 64: 4, 129: 7}                         # chunk index -> target entry
        for ci, tgt in hits.items():
            span[ci - 30] = int(add[tgt])
        lists[WAVE + 10] = span
        lists[WAVE + 20] = toks[130:160]                      # chunk tokens 130..159
        pats.append(one_at(n, WAVE + 10, owner_cls, "I"))
        eff[k] = (tag, add, lists)
        names.append(f"list of 100 over chunk tokens 30..129, owner {owner_cls}")
        meta[k] = dict(T=160, span=True, dies=owner_cls == "I",
                       toks=[int(add[t]) for t in hits.values()], chunk=1)
    log, req, cap, _ = from_patterns(crdt, D, pats, effects=eff, sparse=sparse, col=D - 1)
    return log, req, cap, names, meta


# ------------------------------------------------------------------ family D: multi-entry ops
def family_d(D, sparse=None):
    """set_aw ops of five entries over the chunk edges at 64 and 128 (62..66
    and 126..130), ending on the edge (59..63, 123..127) and starting on it (64..68, 128..132)."""
    pats, names = [], []
    for first, cls in (("I", "included"), ("X", "excluded"), ("E", "first entry invalid")):
        rest = "i" if first != "X" else "x"
        op = first + rest * 4
        for starts in ((62, 126), (59,), (64,), (123, 128)):
            pat, at = "", 0
            for s in starts:
                pat += "I" * (s - at) + op
                at = s + 5
            pat += "I" * 5
            pats.append(pat)
            names.append(f"op over entries {', '.join(f'{s}..{s + 4}' for s in starts)} {cls}")
    log, req, cap, _ = from_patterns(_abi.SET_AW, D, pats, sparse=sparse)
    return log, req, cap, names


# ------------------------------------------------------------------ family F: hand-on lists
F_PATTERNS = ("III", "IXI", "XII", "PIT", "IIE", "PPI", "TPP", "XXX")


def family_f_counter(n_req, which, D=8):
    """Masked counter keys of three ops; which = "all" / "first" / "last":
    the keys whose entries carry differing DC sets."""
    pats = [F_PATTERNS[k % len(F_PATTERNS)] for k in range(n_req)]
    mixed = {"all": None, "first": {0}, "last": {n_req - 1}}[which]
    return from_patterns(_abi.COUNTER_PN, D, pats, sparse="mixed", mixed_keys=mixed)


def family_f_tags(crdt, n_req=8200, D=8):
    pats = [("II", "IX", "XI", "PI")[k % 4] for k in range(n_req)]
    return from_patterns(crdt, D, pats, sparse="mixed")


def is_mixed(log, k):
    a, b = int(log.key_off[k]), int(log.key_off[k + 1])
    return b > a and not (log.oc_mask[a:b] == log.oc_mask[a]).all()


# ------------------------------------------------------------------ family E: GC edges
def gc_patterns():
    """(keep pattern, selected, label): K kept, D dropped, oldest first."""
    out = []
    for n in LENGTHS:
        out.append(("K" * n, 1, f"n={n} all kept"))
        out.append(("D" * n, 1, f"n={n} none kept"))
        out.append(("".join("KD"[m % 2] for m in range(n)), 1, f"n={n} alternate"))
        for p in positions(n):
            out.append((one_at(n, p, "K", "D"), 1, f"n={n} one kept at {p}"))
    for n in (130, 257):
        for d in DROPS:
            out.append(("D" * d + "K" * (n - d), 1, f"n={n} prefix drop {d}"))
            out.append(("K" * (n - d) + "D" * d, 1, f"n={n} suffix drop {d}"))
    # keys not selected in between
    res = []
    for j, item in enumerate(out):
        res.append(item)
        if j % 7 == 3:
            res.append((item[0], 0, item[2] + " (not selected)"))
    return res


def gc_case(crdt, D, items, sparse=False, lists=None):
    """items: (keep pattern, selected, label[, key_off mod 32]) per key; a
    fourth field puts a filler key in front so that the key's segment starts
    at that offset mod 32.  lists[label] = removal lists of that key."""
    pats, sel, names = [], [], []
    at = 0
    for it in items:
        pat, s, label = it[:3]
        if len(it) > 3:
            fill = (it[3] - at) % 32
            if fill:
                pats.append("K" * fill)
                sel.append(1)
                names.append(f"filler {fill}")
                at += fill
            assert at % 32 == it[3]
        pats.append(pat)
        sel.append(s)
        names.append(label)
        at += len(pat)
    K, W = len(pats), n_words(D)
    lens = np.array([len(p) for p in pats], np.int64)
    key_off = np.zeros(K + 1, np.uint64)
    key_off[1:] = np.cumsum(lens)
    E = int(key_off[-1])
    oc = np.zeros((E, D), np.uint64)
    pres = np.ones((E, D), bool)
    op_id = np.zeros(E, np.uint32)
    thr = np.zeros((K, D), np.uint64)
    tp = np.ones((K, D), bool)
    for k, pat in enumerate(pats):
        n, a, c = len(pat), int(key_off[k]), k % D
        m = np.arange(n)
        S = 2000 + n
        rows = np.repeat((1000 + m)[:, None], D, axis=1)
        keep = np.frombuffer(pat.encode(), np.uint8) == ord("K")
        rows[keep, c] = S + 1 + m[keep]
        oc[a:a + n] = rows
        op_id[a:a + n] = 5 + 3 * m
        thr[k] = S
        if sparse and D >= 3:
            pres[a:a + n, (c + 1) % D] &= (m % 3 != 1)
            if k % 2:   # a DC missing from the threshold reads 0: drop one no op carries
                pres[a:a + n, (c + 2) % D] = False
                tp[k, (c + 2) % D] = False
    log = EncodedLog(crdt_type=crdt, n_dcs=D, key_off=key_off, key_type=np.full(K, crdt, np.uint8),
                     oc=oc, oc_mask=None, op_id=op_id,
                     txid=(np.arange(E, dtype=np.uint64) * np.uint64(3) + np.uint64(1)))
    tm = None
    if sparse:
        log.oc_mask = pack_mask(pres)
        oc[~pres] = _garbage(int((~pres).sum()), 4)
        tm = pack_mask(tp)
        thr[~tp] = _garbage(int((~tp).sum()), 5)
    if crdt == _abi.COUNTER_PN:
        log.eff = (np.arange(E, dtype=np.int64) * 37) % 2001 - 1000
    elif crdt == _abi.REGISTER_LWW:   # every removal range empty: rem_off all zero
        log.tag, log.add_tok = np.zeros(E, np.uint32), np.zeros(E, np.uint64)
        for k in range(K):
            a, n = int(key_off[k]), int(lens[k])
            log.tag[a:a + n], log.add_tok[a:a + n] = lww_fields(k, n)
        log.rem_off, log.rem_tok = np.zeros(E + 1, np.uint32), np.zeros(1, np.uint64)
    else:
        log.tag = (np.arange(E, dtype=np.uint32) * 7) % 5
        log.add_tok = np.arange(1, E + 1, dtype=np.uint64) | np.uint64(1 << 40)
        rem_off = np.zeros(E + 1, np.uint32)
        rem = []
        for k in range(K):
            a, n = int(key_off[k]), int(lens[k])
            rl = (lists or {}).get(names[k])
            for m in range(n):
                ln = len(rl[m]) if rl is not None else (m * 5 + k) % 4 if m % 29 else 6
                rem.extend((k << 24) | (m << 10) | x for x in range(ln))
                rem_off[a + m + 1] = len(rem)
        log.rem_off = rem_off
        log.rem_tok = np.array(rem if rem else [0], np.uint64)
    return log, np.array(sel, np.uint8), thr, tm, names


def family_e(crdt, D, sparse=False):
    items = list(gc_patterns())
    for off in (0, 1, 31):
        for pat, label in (("D" * 40 + "K" * 60, "prefix drop 40"), ("DK" * 50, "alternate"),
                           ("K" * 33 + "D" * 33, "suffix drop 33")):
            items.append((pat, 1, f"segment at {off} mod 32, n={len(pat)} {label}", off))
    return gc_case(crdt, D, items, sparse=sparse)


RING_LISTS = (0, 5, 64, 65, 200)


def family_e_ring(crdt, D):
    """700-entry keys, 1..4 removal tokens on every entry, the oldest entry
    dropped: more than 1024 tokens move through the 512-slot ring.  One list
    of 5 / 64 / 65 / 200 tokens in the middle flushes the ring."""
    items, lists = [], {}
    for long in RING_LISTS:
        label = f"ring n=700 oldest dropped, list of {long} at 350" if long else \
            "ring n=700 oldest dropped"
        rl = [[0] * (1 + (m * 7) % 4) for m in range(700)]
        if long:
            rl[350] = [0] * long
        items.append(("D" + "K" * 699, 1, label))
        lists[label] = rl
        items.append(("KD" * 10, 1, f"short key after {label}"))
    return gc_case(crdt, D, items, lists=lists)


def family_e_small(n_keys, D=8):
    """Counter logs of 1 / 2 / 3 / 5 / 7 keys: the 2- and 4-keys-per-wave
    forms end on a partial wave."""
    pool = [("D" * 3 + "K" * 70, 1), ("K" * 64, 1), ("D" * 65, 1), ("DK" * 20, 1), ("K" * 5, 0),
            ("D" * 31 + "K", 1), ("KD" * 64, 1)]
    items = [(p, s, f"n_keys={n_keys} key {j}: {rle(p)}") for j, (p, s) in
             enumerate(pool[:n_keys])]
    return gc_case(_abi.COUNTER_PN, D, items)
