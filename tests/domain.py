"""Remaps of an encoded case (synth.random_case and friends) that move its
values anywhere in the ABI's 64-bit domain (include/antidote_gpu.h, "Value
domain") without changing what the materializer computes.

The materializer reads clocks only through column-wise <=, max and copy, so a
strictly increasing map of the present clock entries of a key keeps every
inclusion decision; tokens, tags and txids are only compared for equality and
order, op ids only for equality (and copied into `hole`), so rank-preserving
maps keep the result up to the same map.  `unmap_result` applies those maps to
a result of the original case.

One exception, inherent to the reference's dict clocks: a DC missing from SCT
reads 0, so a present op-clock entry that the `zero` mode maps to 0 now
compares <= an absent SCT column where it did not before.  `zero_meets_absent`
names the requests this can touch (masked, warm requests only).

Helper module: no tests in it.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field

import numpy as np

from antidote_amd import _abi

U64 = np.uint64
TOP = (1 << 64) - 2                    # largest legal present clock entry
B32 = 395812 << 32                     # a 2^32 boundary at microsecond-epoch size (~1.7e15)
B63 = 1 << 63
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
CLOCK_MODES = ("carry32", "sign64", "hi32", "top", "zero")
MIXED = ("carry32", "sign64", "hi32", "top", "zero")   # `mixed`: by k % 5


def present_bits(mask, n, D):
    """(n, D) bool presence of a (n, W) mask array; None = every column."""
    if mask is None:
        return np.ones((n, D), bool)
    d = np.arange(D)
    return ((mask[:, d >> 6] >> (d & 63).astype(U64)) & U64(1)).astype(bool)


@dataclass
class ClockMap:
    """One strictly increasing map per key: v -> v + add[k] (mod 2^64), or for
    hi32 keys v -> ((v - lo[k]) << 32) | (0xffffffff - (v - lo[k]))."""
    mode: list            # per key: the mode name
    add: np.ndarray       # u64 per key
    lo: np.ndarray        # u64 per key (hi32: the key's minimum)
    pivot: np.ndarray     # u64 per key: values >= pivot lie on the upper side

    def apply(self, keys, vals):
        """vals (n, D) or (n,) u64 of the keys `keys` (n,) -> mapped copy."""
        keys = np.asarray(keys).astype(np.int64)
        vals = np.asarray(vals, U64)
        shape = (-1,) + (1,) * (vals.ndim - 1)
        add, lo = self.add[keys].reshape(shape), self.lo[keys].reshape(shape)
        hi = np.array([m == "hi32" for m in self.mode], bool)[keys].reshape(shape)
        with np.errstate(over="ignore"):
            lin = vals + add
            d = vals - lo
            h = (d << U64(32)) | (U64(0xFFFFFFFF) - (d & U64(0xFFFFFFFF)))
        return np.where(hi, h, lin)

    def boundary(self, k):
        """The mapped value at which key k's upper side starts."""
        return int(self.apply(np.array([k]), np.array([self.pivot[k]], U64))[0])


def _key_of_entry(log):
    return np.repeat(np.arange(log.n_keys), np.diff(log.key_off.astype(np.int64)))


def _req_presence(req, sparse):
    n, D = req.n_req, req.n_dcs
    rp = present_bits(req.R_mask if sparse else None, n, D)
    if req.sct is None:
        sp = np.zeros((n, D), bool)
    else:
        sp = present_bits(req.sct_mask if sparse else None, n, D)
        if req.sct_ignore is not None:
            sp &= (np.asarray(req.sct_ignore) == 0)[:, None]
    return rp, sp


def clock_map(log, req, mode, sparse=None):
    """The per-key ClockMap of `mode` for this case (see the module docstring
    and remap_clocks)."""
    if sparse is None:
        sparse = log.oc_mask is not None
    K, D, E = log.n_keys, log.n_dcs, log.n_entries
    op = present_bits(log.oc_mask, E, D)
    rp, sp = _req_presence(req, sparse)
    rkeys = req.keys.astype(np.int64)
    modes, add, lo, pivot = [], np.zeros(K, U64), np.zeros(K, U64), np.zeros(K, U64)
    by_key: dict = {}
    for i, k in enumerate(rkeys):
        by_key.setdefault(int(k), []).append(i)
    for k in range(K):
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        ocv = log.oc[a:b][op[a:b]]
        rows = by_key.get(k, [])
        rv = np.concatenate([req.R[i][rp[i]] for i in rows]) if rows else np.zeros(0, U64)
        sv = np.concatenate([req.sct[i][sp[i]] for i in rows]) if rows and req.sct is not None \
            else np.zeros(0, U64)
        allv = np.concatenate([ocv, rv, sv])
        m = MIXED[k % 5] if mode == "mixed" else mode
        modes.append(m)
        if allv.size == 0:
            continue                      # nothing present: identity
        mn, mx = int(allv.min()), int(allv.max())
        src = ocv if ocv.size else (rv if rv.size else allv)
        p = int(np.sort(src)[src.size // 2])          # (upper) median
        if m == "carry32":
            off = B32 - p
        elif m == "sign64":
            off = B63 - p
        elif m == "top":
            off = TOP - mx
        elif m == "zero":
            off, p = -mn, mn + (mx - mn + 1) // 2
        elif m == "hi32":
            assert mx - mn < (1 << 32), "hi32 needs a key's clocks within 2^32"
            off = 0
            if ocv.size:                 # the halves of the op clocks' own range
                p = int(ocv.min()) + (int(ocv.max()) - int(ocv.min()) + 1) // 2
            lo[k] = mn
        else:
            raise ValueError(mode)
        if m != "hi32":
            assert 0 <= mn + off and mx + off <= TOP, (m, k, mn, mx)
        add[k] = off % (1 << 64)
        pivot[k] = p
    return ClockMap(modes, add, lo, pivot)


def remap_clocks(log, req, mode, extra=(), sparse=None):
    """Copies of (log, req) with the present entries of oc, R and sct remapped
    per key (a request uses the map of the key it reads); masks untouched,
    absent columns (and the SCT rows of sct_ignore requests) keep what they
    held.  extra: (array (n, D), key index (n,), mask (n, W) or None) triples
    of further clock rows, remapped with their key's map.
    Returns (log, req, [extra arrays], ClockMap)."""
    if sparse is None:
        sparse = log.oc_mask is not None
    cm = clock_map(log, req, mode, sparse)
    log2, req2 = copy.copy(log), copy.copy(req)
    E, D = log.n_entries, log.n_dcs
    op = present_bits(log.oc_mask, E, D)
    log2.oc = np.where(op, cm.apply(_key_of_entry(log), log.oc), log.oc) if E else log.oc.copy()
    rp, sp = _req_presence(req, sparse)
    req2.R = np.ascontiguousarray(np.where(rp, cm.apply(req.keys, req.R), req.R))
    if req.sct is not None:
        req2.sct = np.ascontiguousarray(np.where(sp, cm.apply(req.keys, req.sct), req.sct))
    out = []
    for arr, keys, mask in extra:
        pres = present_bits(mask, arr.shape[0], arr.shape[1])
        out.append(np.ascontiguousarray(np.where(pres, cm.apply(keys, arr), arr)))
    return log2, req2, out, cm


def remap_columns(arrays, masks, mode):
    """For select_base / dep_check rows, which compare across partitions: one
    map per column over all the arrays, v -> B - p_d + v with p_d the median
    of column d's present entries (`carry32` / `sign64`).  Returns copies."""
    B = {"carry32": B32, "sign64": B63}[mode]
    D = arrays[0].shape[-1]
    pres = [present_bits(m, a.shape[0], D) for a, m in zip(arrays, masks)]
    off = np.zeros(D, U64)
    for d in range(D):
        col = np.concatenate([a[:, d][p[:, d]] for a, p in zip(arrays, pres)])
        if col.size:
            p_d = int(np.sort(col)[col.size // 2])
            assert B - p_d + int(col.min()) >= 0 and B - p_d + int(col.max()) <= TOP
            off[d] = (B - p_d) % (1 << 64)
    with np.errstate(over="ignore"):
        return [np.ascontiguousarray(np.where(p, a + off, a)) for a, p in zip(arrays, pres)]


def remap_rows(groups, K, mode):
    """Clock rows outside an encoded case (snapshot-cache clocks, R, LastOpCt):
    groups = [(array (n, D), key index (n,), presence (n, D) bool)], remapped
    with one map per key, v -> v + off_k, off_k chosen as in remap_clocks
    (`carry32` / `sign64`: the pivot is the median of the key's entries in the
    first group that has any; `top` / `zero`).  Entries 2^31 or more away from
    the pivot (a read far before or after everything else) keep their value
    where that keeps the order, else the whole key keeps its values.
    Returns copies."""
    vals: list = [[] for _ in range(K)]
    first: list = [None] * K
    for arr, keys, pres in groups:
        keys = np.asarray(keys).astype(np.int64)
        order = np.argsort(keys, kind="stable")
        bounds = np.searchsorted(keys[order], np.arange(K + 1))
        for k in range(K):
            rows = order[bounds[k]:bounds[k + 1]]
            if rows.size:
                v = arr[rows][pres[rows]]
                if v.size:
                    vals[k].append(v)
                    if first[k] is None:
                        first[k] = v
    off = np.zeros(K, U64)
    cmin, cmax = np.ones(K, U64), np.zeros(K, U64)      # empty core: nothing mapped
    for k in range(K):
        if not vals[k]:
            continue
        allv = [int(x) for x in np.concatenate(vals[k])]
        p = int(np.sort(first[k])[first[k].size // 2])
        core = [v for v in allv if abs(v - p) < 1 << 31]
        mn, mx = min(core), max(core)
        o = {"carry32": B32 - p, "sign64": B63 - p, "top": TOP - mx, "zero": -mn}[mode]
        if mn + o < 0 or mx + o > TOP:
            continue
        if any(v >= mn + o for v in allv if v < mn) or any(v <= mx + o for v in allv if v > mx):
            continue
        off[k], cmin[k], cmax[k] = o % (1 << 64), mn, mx
    out = []
    with np.errstate(over="ignore"):
        for arr, keys, pres in groups:
            sh = (-1,) + (1,) * (arr.ndim - 1)
            ki = np.asarray(keys).astype(np.int64)
            core = pres & (arr >= cmin[ki].reshape(sh)) & (arr <= cmax[ki].reshape(sh))
            out.append(np.ascontiguousarray(np.where(core, arr + off[ki].reshape(sh), arr)))
    return out


def side_shares(log, cm):
    """Of the present oc entries: (share below the key's pivot, share at or
    above it, keys with >= 8 ops that have entries on one side only)."""
    op = present_bits(log.oc_mask, log.n_entries, log.n_dcs)
    piv = cm.pivot[_key_of_entry(log)][:, None]
    up = (log.oc >= piv) & op
    dn = (log.oc < piv) & op
    one_sided = []
    for k in range(log.n_keys):
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        if b - a >= 8 and not (up[a:b].any() and dn[a:b].any()):
            one_sided.append(k)
    n = max(int(op.sum()), 1)
    return dn.sum() / n, up.sum() / n, one_sided


def zero_meets_absent(log, req, cm, sparse):
    """Requests whose result the `zero` map may legitimately change: a present
    op-clock entry mapped to 0 in a column that the request's SCT lacks."""
    if not sparse or req.sct is None:
        return set()
    op = present_bits(log.oc_mask, log.n_entries, log.n_dcs)
    _, sp = _req_presence(req, sparse)
    out = set()
    for i, k in enumerate(req.keys.astype(np.int64)):
        if cm.mode[k] != "zero" or req.sct_ignore[i]:
            continue
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        hit = (log.oc[a:b] == U64((-int(cm.add[k])) % (1 << 64))) & op[a:b] & ~sp[i][None, :]
        if hit.any():
            out.add(i)
    return out


# ---------------------------------------------------------------- payload
PAYLOAD_MODES = {
    # name: effects, tokens, tags, op ids, txids
    "lowsame": dict(eff=True, tok="lowsame", tag="hi", ids="sign", txid="hi"),
    "top": dict(eff=True, tok="top", tag="sign", ids="top", txid="lo"),
    # not monotone in the tokens: the oracle has to be re-run (set_aw's state
    # order is the tokens' list order, register_mv's is sorted by token)
    "mul": dict(eff=True, tok="mul", tag="hi", ids="top", txid="hi"),
}
MONOTONE_PAYLOAD = ("lowsame", "top")
MUL = 0xD6E8FEB86659FD93


@dataclass
class PayloadMap:
    tok: dict = field(default_factory=dict)      # old token -> new
    tag: dict = field(default_factory=dict)      # old tag -> new
    id_off: np.ndarray | None = None             # per key, added to its op ids


def widen_i64(rng, v, wide=1 / 3):
    """Effects / base values over the i64 domain: a share `wide` uniform over
    [-(2^63-1), 2^63-1], as many +-2^32 +- small and +-2^31 +- small, the rest
    left small; a few exact INT64_MAX and INT64_MIN + 1.  INT64_MIN (the
    reserved invalid effect) stays."""
    v = np.asarray(v, np.int64)
    out = v.copy()
    n = v.size
    u = rng.random(n)
    big = rng.integers(-INT64_MAX, INT64_MAX, n, dtype=np.int64, endpoint=True)
    sign = np.where(rng.random(n) < 0.5, -1, 1).astype(np.int64)
    word = np.where(rng.random(n) < 0.5, 1 << 32, 1 << 31).astype(np.int64)
    near = sign * word + rng.integers(-40, 41, n)
    out = np.where(u < wide, big, out)
    out = np.where((u >= wide) & (u < 2 * wide), near, out)
    e = rng.random(n)
    out = np.where(e < 0.01, INT64_MAX, out)
    out = np.where((e >= 0.01) & (e < 0.02), INT64_MIN + 1, out)
    return np.where(v == INT64_MIN, v, out).astype(np.int64)


def _rank_map(vals, fn):
    vals = sorted(set(int(x) for x in vals))
    return {v: fn(r, len(vals)) for r, v in enumerate(vals)}


def _lut(arr, m, dtype):
    return np.array([m.get(int(x), int(x)) for x in arr], dtype).reshape(np.shape(arr))


def remap_payload(log, req, mode, seed=0, wide=1 / 3):
    """Copies of (log, req) with the non-clock values widened (PAYLOAD_MODES,
    or a dict of the same fields).  INT64_MIN effects, 0xFFFFFFFF tags and
    zero tokens / txids stay what they are.  Returns (log, req, PayloadMap)."""
    spec = PAYLOAD_MODES[mode] if isinstance(mode, str) else mode
    rng = np.random.default_rng(seed)
    log2, req2 = copy.copy(log), copy.copy(req)
    pm = PayloadMap()
    K = log.n_keys
    if spec.get("eff"):
        if log.eff is not None:
            log2.eff = widen_i64(rng, log.eff, wide)
        if log.crdt_type == _abi.COUNTER_PN:
            req2.base_value = widen_i64(rng, req.base_value, wide)
    if spec.get("tok") and log.add_tok is not None:
        toks = [x for a in (log.add_tok, log.rem_tok, req.base_tok) for x in a if x != 0]
        kind = spec["tok"]
        if kind == "lowsame":
            pm.tok = _rank_map(toks, lambda r, n: ((r + 1) << 32) | 1)
        elif kind == "top":
            pm.tok = _rank_map(toks, lambda r, n: (1 << 64) - 1 - (n - 1 - r))
        elif kind == "mul":
            pm.tok = {int(t): (int(t) * MUL) % (1 << 64) for t in set(int(x) for x in toks)}
            assert 0 not in pm.tok.values()
        else:
            raise ValueError(kind)
        log2.add_tok = _lut(log.add_tok, pm.tok, U64)
        log2.rem_tok = _lut(log.rem_tok, pm.tok, U64)
        req2.base_tok = _lut(req.base_tok, pm.tok, U64)
    if spec.get("tag") and log.tag is not None:
        tags = [x for a in (log.tag, req.base_tag) for x in a if x != _abi.TAG_INVALID]
        if spec["tag"] == "hi":
            pm.tag = _rank_map(tags, lambda r, n: 0xFFFFFFFE - (n - 1 - r))
        else:
            pm.tag = _rank_map(tags, lambda r, n: (1 << 31) - n // 2 + r)
        log2.tag = _lut(log.tag, pm.tag, np.uint32)
        req2.base_tag = _lut(req.base_tag, pm.tag, np.uint32)
    if log.crdt_type == _abi.REGISTER_MV and req2.base_tok.size:
        # a register_mv state is sorted by {Value, Token}: a map that is not
        # monotone in the tokens (`mul`) has to put the base states back in order
        req2.base_tag, req2.base_tok = req2.base_tag.copy(), req2.base_tok.copy()
        for i in range(req.n_req):
            a, b = int(req.base_off[i]), int(req.base_off[i + 1])
            o = np.lexsort((req2.base_tok[a:b], req2.base_tag[a:b]))
            req2.base_tag[a:b], req2.base_tok[a:b] = req2.base_tag[a:b][o], req2.base_tok[a:b][o]
    if spec.get("ids"):
        off = np.zeros(K, np.int64)
        for k in range(K):
            a, b = int(log.key_off[k]), int(log.key_off[k + 1])
            if b == a:
                continue
            ids = log.op_id[a:b].astype(np.int64)
            if spec["ids"] == "sign":
                off[k] = (1 << 31) - int(np.sort(ids)[ids.size // 2])
            else:
                off[k] = 0xFFFFFFFE - int(ids.max())
            assert ids.min() + off[k] >= 1 and ids.max() + off[k] <= 0xFFFFFFFE
        pm.id_off = off
        log2.op_id = (log.op_id.astype(np.int64) + off[_key_of_entry(log)]).astype(np.uint32)
    if spec.get("txid"):
        f = (lambda t: (t << U64(32)) | U64(5)) if spec["txid"] == "hi" else \
            (lambda t: (U64(5) << U64(32)) | t)
        log2.txid = np.where(log.txid != 0, f(log.txid.astype(U64)), U64(0)).astype(U64)
        req2.txid = np.where(req.txid != 0, f(req.txid.astype(U64)), U64(0)).astype(U64)
    return log2, req2, pm


def unmap_result(res, log, req, cm=None, pm=None, sparse=None):
    """What the remapped case must give, from a result `res` of the original
    (log, req): lastct through the key's clock map where present, hole through
    the key's id offset, out_tag / out_tok through the rank maps, everything
    else equal."""
    if sparse is None:
        sparse = log.oc_mask is not None
    out = copy.deepcopy(res)
    n, D = req.n_req, log.n_dcs
    keys = req.keys.astype(np.int64)
    err = (res.flags & (_abi.F_ERR_CORRUPTED | _abi.F_ERR_UNEXPECTED)) != 0
    if cm is not None:
        pres = present_bits(res.lastct_mask if sparse else None, n, D)
        pres &= ((res.flags & _abi.F_CT_IGNORE) == 0)[:, None]
        pres &= ((res.flags & _abi.F_ERR_CORRUPTED) == 0)[:, None]
        out.lastct = np.where(pres, cm.apply(keys, res.lastct), res.lastct)
    if pm is not None and pm.id_off is not None:
        nonempty = np.diff(log.key_off.astype(np.int64))[keys] > 0
        corrupt = (res.flags & _abi.F_ERR_CORRUPTED) != 0
        out.hole = np.where(nonempty & ~corrupt, res.hole + pm.id_off[keys], res.hole)
    if pm is not None and res.out_tag is not None:
        for i in range(n):
            if err[i] or (res.flags[i] & _abi.F_ERR_CAPACITY):
                continue
            o, m = int(res.out_off[i]), int(res.out_n[i])
            if pm.tag:
                out.out_tag[o:o + m] = _lut(res.out_tag[o:o + m], pm.tag, np.uint32)
            if pm.tok:
                out.out_tok[o:o + m] = _lut(res.out_tok[o:o + m], pm.tok, U64)
    return out


def std_case(seed, crdt, D, sparse, K=130, nmax=150, **kw):
    """random_case at the value-domain tests' shape: odd K, keys past 64 and
    past 128 ops, the usual warm / txid / invalid / corrupt / base / multi
    rates."""
    from synth import random_case
    args = dict(sparse=sparse, warm=0.4, txid=0.3, invalid=0.02, corrupt=0.03, base=0.4,
                multi=0.15 if crdt == _abi.SET_AW else 0.0, identity=(D % 2 == 0))
    args.update(kw)
    log, req, cap = random_case(seed, crdt, K, D, nmax, **args)
    if sparse and D > 17:
        # with 3 % of R's columns absent hardly any op of a wide clock is
        # included: most reads name every DC (the steady state)
        rng = np.random.default_rng(seed + 1)
        full = np.zeros(req.R_mask.shape[1], U64)
        for d in range(D):
            full[d >> 6] |= U64(1 << (d & 63))
        req.R_mask[rng.random(req.n_req) < 0.8] = full
    return log, req, cap


def domain_case(idx, base, clock="mixed", payload=None, sparse=None):
    """A (log, req, ...) case moved into the wide domain: `clock` remap plus
    one payload mode, rotated by the case's index unless given."""
    log, req = base[0], base[1]
    if payload is None:
        payload = tuple(PAYLOAD_MODES)[idx % len(PAYLOAD_MODES)]
    log, req, _, _ = remap_clocks(log, req, clock, sparse=sparse)
    log, req, _ = remap_payload(log, req, payload, seed=idx)
    return log, req


def run_oracle(oracle_lib, log, req, cap=None, sparse=None, threads=4):
    """oracle_materialize on an encoded case -> ResultArrays."""
    import ctypes as C

    from antidote_amd.encode import alloc_result, log_struct, read_struct, result_struct
    if sparse is None:
        sparse = log.oc_mask is not None
    res = alloc_result(req.n_req, log.n_dcs, sparse=sparse, cap_off=cap)
    ls, rs, os_ = log_struct(log), read_struct(req, sparse=sparse), result_struct(res)
    if not sparse:
        ls.oc_mask = None
    assert oracle_lib.oracle_materialize(C.byref(ls), C.byref(rs), C.byref(os_), threads) == 0
    return res
