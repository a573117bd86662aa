"""Constructed cases for the fused counter_b cached read (k_bcounter_serve):
helper, no tests.  Nothing is drawn: building a case twice gives identical
arrays.

  family(D, full)     one agn_read_cached batch of constructed keys: the log,
                      a prebuilt cache whose snapshots' states are planted in
                      its arena, one request per key, and per key the edge it
                      was built for
  masked(fam)         the same batch over a log with presence masks
  chain(lib, fam)     the reference: oracle_ss_lookup -> bcounter_model.model
                      (bases read back from the planted states) ->
                      oracle_ss_store, as tests/test_bcounter.py's Mirror does
  bc_steps(script)    cache_edges' batcher scripts with counter_b effects
"""
from __future__ import annotations

import copy
import ctypes as C
import functools

import numpy as np

import bcounter_model as bm
import cache_edges as ce
from antidote_amd import _abi
from antidote_amd.encode import EncodedLog, EncodedRead, log_struct, result_struct
from lww_model import opi

BC = _abi.COUNTER_B
THRESHOLD, KEEP, MIN_OPS = _abi.SNAPSHOT_THRESHOLD, _abi.SNAPSHOT_MIN, _abi.MIN_OP_STORE_SS
SLOTS = THRESHOLD
R0 = 1_000_000        # every read clock column
SCT0 = 50             # the hit snapshot's clock: below every op (100 + p)
LOOKS = ("new", "hit0", "hit8", "log")
# D of the fused shapes; the families that run in full, and the masked ones
DENSE_DS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 32, 33, 64)
FULL = ((3, False), (8, False), (5, True), (33, True))
# masked: every fused shape but D = 1 (masked() takes a DC other than column 0
# out of an op, so it needs D >= 2; a one-DC log has no DC an op could lack)
MASKED_DS = (2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 32, 33, 64)
# (D, the full family?, masked log?) of every agn_read_cached family the GPU
# test runs and the CPU test proves the reach of
FAMILIES = [(D, (D, False) in FULL, False) for D in DENSE_DS] + \
           [(D, (D, True) in FULL, True) for D in MASKED_DS]
FAMILY_IDS = [f"D{d}-{'full' if f else 'lite'}-{'masked' if m else 'dense'}" for d, f, m in FAMILIES]


class Family:
    pass


def lengths(D):
    """0, 1, 63, 64, 65, 128, 129 in units of the shape's ops per iteration."""
    o = opi(D)
    return sorted({0, 1, o - 1, o, o + 1, 2 * o, 2 * o + 1})


ZIG = (40, 10, 30, 20, 50)    # a key's slots in an order that is not ascending


def zig_ops(n):
    """n ops over five slots named in ZIG's order, the middle one excluded."""
    return [(ZIG[p % 5], p + 1, not (n >= 3 and p == n // 2)) for p in range(n)]


def planted_bases():
    """Cached states of 0, 1, 64, 65 and 200 pairs, one with duplicate tags and
    one in descending tag order -- an arena written by hand need not be what a
    store would have written, and the fold takes it as it is."""
    return [("base 0 pairs", []),
            ("base 1 pair", [(30, 7)]),
            ("base 64 pairs, descending", [(3000 - x, x) for x in range(64)]),
            ("base 65 pairs", [(2000 + 3 * x, -x) for x in range(65)]),
            ("base 200 pairs", [(5000 + (x * 37) % 200, x - 100) for x in range(200)]),
            ("base with duplicate tags", [(10, 1), (90, 2), (10, 3), (5, 0), (90, -2)]),
            ("base descending, shared with the log", [(50, 5), (40, 4), (30, 3), (20, 2)])]


def specs_for(D, full):
    o = opi(D)
    out = []

    def add(name, ops, base=None, look="hit0", ncache=2, gap=MIN_OPS, gc=0, room=None,
            mistyped=False, kind="other"):
        if look == "new":
            ncache = 0
        if look == "hit8":
            ncache = 9
        out.append(dict(name=name, ops=list(ops), base=base, look=look, ncache=ncache, gap=gap,
                        gc=gc, room=room, mistyped=mistyped, kind=kind))

    x = 0
    for n in lengths(D):
        look = LOOKS[x % 4]
        add(f"length {n}", zig_ops(n), base=[(20, 9), (70, 1)] if look.startswith("hit") else None,
            look=look, gc=(x // 4) % 2, kind="length")
        x += 1
    slot = bm.slot_specs()
    if not full:      # 1, 2, 64, 65, and 255 / 256 / 257 from the log alone and with a base
        slot = [s for i, s in enumerate(slot) if i in (0, 2, 3, 4, 6, 7, 9, 10, 12, 13, 15)]
    for i, s in enumerate(slot):
        base = s.get("base")
        look = ("hit0", "hit8")[i % 2] if base else ("new", "hit0", "log")[i % 3]
        add(f"slots #{i}: {len(s['ops'])} ops, {len(base or [])} base pairs", s["ops"], base,
            look=look, gc=i % 2 if look != "hit8" else 0, kind="slots")
    # store outcomes
    six = zig_ops(7)            # count 6
    for cnt in (4, 5):
        ops = [(ZIG[p % 5], p + 1, True) for p in range(cnt)]
        add(f"count {cnt}", ops, [(30, 1)], kind="store")
        add(f"count {cnt}, GC read", ops, [(30, 1)], gc=1, kind="store")
        add(f"count {cnt} on an absent key", ops, look="new", kind="store")
    for gap in (4, 5):
        add(f"op-id gap {gap}", six, [(60, 2), (10, 1)], gap=gap, kind="store")
    add("hit at slot 0, stored", six, [(60, 2), (10, 1)], kind="store")
    add("list 8 -> 9", six, [(60, 2)], ncache=8, kind="store")
    add("list 9 -> 10: collected", six, [(60, 2)], ncache=9, kind="store")
    add("list 9, GC read", six, [(60, 2)], ncache=9, gc=1, kind="store")
    add("hit 8 of 9", six, [(60, 2), (10, 1)], look="hit8", kind="store")
    add("hit 8 of 9, GC read", six, [(60, 2), (10, 1)], look="hit8", gc=1, kind="store")
    add("LOG", six, look="log", ncache=3, kind="store")
    add("LOG, GC read", six, look="log", ncache=9, gc=1, kind="store")
    if full:
        for i, s in enumerate(bm.error_specs()):
            base = s.get("base")
            add(f"errors #{i}", s["ops"], base, look=("hit0", "new")[i % 2] if not base else "hit0",
                gc=(i // 2) % 2, room=s.get("room"), mistyped=bool(s.get("mistyped")), kind="error")
        for i, (name, base) in enumerate(planted_bases()):
            add(name, zig_ops(o + 2), base, look=("hit0", "hit8")[i % 2], gc=i % 2 if i % 2 == 0 else 0,
                kind="base")
    return out


@functools.lru_cache(maxsize=None)
def family(D, full=True):
    """One key per spec.  Entry p of a key has clock 100 + p in every column
    against R = 10^6; an excluded entry's column 0 is 2 * 10^6.  A hit
    snapshot's clock is 50 everywhere, so every op is outside it."""
    specs = specs_for(D, full)
    K = len(specs)
    assert K <= 64
    lens = np.array([len(s["ops"]) for s in specs], np.int64)
    key_off = np.zeros(K + 1, np.uint64)
    key_off[1:] = np.cumsum(lens)
    E = int(key_off[-1])
    oc, op_id = np.zeros((E, D), np.uint64), np.zeros(E, np.uint32)
    tag, amt = np.zeros(E, np.uint32), np.zeros(E, np.uint64)
    key_type = np.full(K + 3, BC, np.uint8)
    R = np.full((K, D), R0, np.uint64)
    gc = np.zeros(K, np.uint8)
    n_arr = np.zeros(K, np.uint32)
    clock = np.full((K, SLOTS, D), 0xDEAD0000, np.uint64)     # rows past n: nothing reads them
    last_op = np.full((K, SLOTS), -777, np.int64)
    value = np.full((K, SLOTS), _abi.ss_state(0, 0), np.int64)   # arena references (device)
    handle = np.zeros((K, SLOTS), np.int64)                      # indices into states (oracle)
    states = [[]]
    st_tag, st_tok = [0xDEAD], [0xDEAD]                          # the arena, a gap in front
    cap_off = np.zeros(K + 1, np.uint64)
    xc = 1 % D
    e = 0
    for k, s in enumerate(specs):
        n = len(s["ops"])
        first_excl = -1
        for p, (t, v, inc) in enumerate(s["ops"]):
            oc[e] = 100 + p
            if not inc:
                oc[e, 0] = 2 * R0
                if first_excl < 0:
                    first_excl = p
            op_id[e], tag[e], amt[e] = 2 * p + 1, t, int(v) & bm.M64
            e += 1
        hole = 2 * first_excl if first_excl >= 0 else (2 * n - 1 if n else 0)
        gc[k] = s["gc"]
        if s["mistyped"]:
            key_type[k] = _abi.SET_AW
        nb = len(s["base"] or [])
        cap_off[k + 1] = cap_off[k] + (n + nb if s["room"] is None else s["room"])
        nc, look = s["ncache"], s["look"]
        n_arr[k] = nc
        f = {"new": None, "hit0": 0, "hit8": 8, "log": -1}[look]
        for j in range(nc):
            if look == "hit0":
                row = np.full(D, SCT0 - j, np.uint64)
            elif look == "hit8":
                row = np.full(D, SCT0, np.uint64)
                if j < 8:
                    row[xc] = R0 + 8 - j
            else:
                row = np.full(D, SCT0, np.uint64)
                row[xc] = R0 + nc - j
            clock[k, j] = row
            last_op[k, j] = (hole - s["gap"]) - 6 * j
            if s["base"] is not None and j == f:
                pairs = [(int(t), int(v) & bm.M64) for t, v in s["base"]]
            elif j % 2:        # other slots hold states too: they are released when dropped
                pairs = [(7, j)]
            else:
                pairs = []
            value[k, j] = _abi.ss_state(len(st_tag), len(pairs))
            st_tag += [t for t, _ in pairs] + [0xBEEF]
            st_tok += [v for _, v in pairs] + [0xBEEF]
            if pairs:
                states.append(pairs)
                handle[k, j] = len(states) - 1
    fam = Family()
    fam.D, fam.K, fam.S, fam.opi, fam.full = D, K, SLOTS, opi(D), full
    fam.specs = specs
    fam.names = [f"k={k} {s['look']} n={s['ncache']} gc={s['gc']} {s['name']}"
                 for k, s in enumerate(specs)]
    fam.log = EncodedLog(crdt_type=BC, n_dcs=D, key_off=key_off, key_type=key_type, oc=oc,
                         oc_mask=None, op_id=op_id, txid=np.zeros(E, np.uint64), tag=tag,
                         add_tok=amt, rem_off=np.zeros(E + 1, np.uint32),
                         rem_tok=np.zeros(1, np.uint64))
    fam.keys = np.arange(K, dtype=np.uint64)
    fam.R, fam.gc, fam.cap_off = R, gc, cap_off
    fam.cache = {"n": n_arr, "clock": clock, "last_op": last_op, "value": value}
    fam.handle, fam.states = handle, states
    used = len(st_tag)
    fam.arena_cap = used + int(cap_off[-1]) + 64          # room for every store of the batch
    fam.state_tag = np.array(st_tag + [0] * (fam.arena_cap - used), np.uint32)
    fam.state_tok = np.array(st_tok + [0] * (fam.arena_cap - used), np.uint64)
    fam.ctl = np.array([used, 0, 0, 0], np.uint64)
    return fam


@functools.lru_cache(maxsize=None)
def masked_family(D, full=True):
    return masked(family(D, full))


def masked(fam):
    """fam with presence masks on its log (oc_mask; D >= 2): two ops in three
    lack one DC other than column 0, and hold garbage far above every read
    clock there -- taken for present, the column would exclude the op.  Cache,
    read clocks and results stay dense: the form a masked partition's log has
    over a dense-clock cache."""
    D = fam.D
    assert D >= 2
    out = copy.copy(fam)
    log = copy.copy(fam.log)
    E = log.n_entries
    W = (D + 63) // 64
    log.oc = fam.log.oc.copy()
    full = [(1 << min(64, D - 64 * w)) - 1 for w in range(W)]
    log.oc_mask = np.tile(np.array(full, np.uint64), (E, 1))
    for e in range(E):
        if e % 3 == 0:
            continue
        d = 1 + (e * 5) % (D - 1)
        log.oc_mask[e, d >> 6] &= np.uint64(~(1 << (d & 63)) & bm.M64)
        log.oc[e, d] = np.uint64((1 << 61) | (977 * e + d))
    out.log = log
    return out


def requests(fam):
    """(EncodedRead with the lookup's outputs still empty, cap_off, gc): one
    request per key, in key order."""
    n = fam.K
    req = EncodedRead(n_dcs=fam.D, req_type=BC, keys=fam.keys.copy(), R=fam.R.copy(), R_mask=None,
                      sct=np.zeros((n, fam.D), np.uint64), sct_mask=None,
                      sct_ignore=np.zeros(n + 8, np.uint8), txid=np.zeros(n, np.uint64),
                      base_value=np.zeros(n, np.int64), base_off=np.zeros(n + 1, np.uint64),
                      base_tag=np.zeros(0, np.uint32), base_tok=np.zeros(0, np.uint64))
    return req, fam.cap_off.copy(), fam.gc.copy()


def chain(lib, fam):
    """read/6 of fam's keys on the host: the C oracle's lookup over the cache
    (its value slots handles into `states`), the model from the hit states, the
    C oracle's store.  Returns the model's result and per-key info, status,
    first, prune (per key), thresholds, the cache arrays afterwards and the
    states their handles name."""
    D, K, S = fam.D, fam.K, fam.S
    arrs = {x: a.copy() for x, a in fam.cache.items()}
    arrs["value"] = fam.handle.copy()
    c = ce.cache_struct(D, S, K, arrs, ce.ptr)
    req, co, gc = requests(fam)
    n = req.n_req
    first, status = np.zeros(n + 8, np.uint8), np.zeros(n + 8, np.uint8)
    assert lib.oracle_ss_lookup(C.byref(c), n, ce.ptr(req.keys), ce.ptr(req.R), None,
                                ce.ptr(req.sct), None, ce.ptr(req.sct_ignore),
                                ce.ptr(req.base_value), ce.ptr(first), ce.ptr(status)) == 0
    states = [list(s) for s in fam.states]
    bases = [states[int(h)] for h in req.base_value]
    req.sct_ignore = req.sct_ignore[:n]
    res, _incl, info = bm.model(fam.log, req, False, co, bases=bases)
    handle = np.zeros(n, np.int64)
    for i in range(n):
        if res.out_n[i] and not int(res.flags[i]) & _abi.F_ERR_CAPACITY:
            o, m = int(co[i]), int(res.out_n[i])
            states.append(list(zip(res.out_tag[o:o + m].tolist(), res.out_tok[o:o + m].tolist())))
            handle[i] = len(states) - 1
    rs = result_struct(res)
    rs.lastct_mask = None       # dense clocks, as the device store reads them
    ls = log_struct(fam.log)
    prune, thr = np.zeros(K + 8, np.uint8), np.zeros((K, D), np.uint64)
    gc8 = np.concatenate([gc, np.zeros(8, np.uint8)])
    n_before = arrs["n"].copy()
    assert lib.oracle_ss_store(C.byref(c), C.byref(ls), n, ce.ptr(req.keys), ce.ptr(first),
                               ce.ptr(status), ce.ptr(gc8), C.byref(rs), ce.ptr(handle),
                               ce.ptr(prune), ce.ptr(thr), None) == 0
    return dict(res=res, info=info, status=status[:n], first=first[:n], prune=prune[:K], thr=thr,
                arrs=arrs, states=states, handle=handle, n_before=n_before, cap=co,
                bases=bases)


def fold_order(ops, base):
    """The slot table's order after the kernel's fold: base pairs first, then
    the included valid entries, each slot where it first appears."""
    seen = []
    for t, _v in base:
        if t not in seen:
            seen.append(t)
    for t, _v, inc in ops:
        if inc and t != _abi.TAG_INVALID and t not in seen:
            seen.append(t)
    return seen


def decode_states(value, n, state_tag, state_tok):
    """Every live slot's state through its AGN_SS_STATE reference:
    {(key, slot): [(tag, tok), ...]} in arena order."""
    out = {}
    for k in range(len(n)):
        for j in range(int(n[k])):
            start, pairs = _abi.ss_state_unpack(int(value[k, j]))
            out[(k, j)] = list(zip(state_tag[start:start + pairs].tolist(),
                                   state_tok[start:start + pairs].tolist()))
    return out


# ------------------------------------------------------------------ batcher scripts
SCRIPT_NAMES = ("grow", "deep", "below", "gc_twice", "invalid")
SCRIPT_SLOTS = (40, 10, 30, 20, 50, 15)


def script_entry(t, bad=False):
    """The (slot, amount) of a script's op number t: slots first appear in an
    order that is not ascending; amounts are small and signed, 0 included."""
    if bad:
        return _abi.TAG_INVALID, 0
    return SCRIPT_SLOTS[(t + t // 7) % len(SCRIPT_SLOTS)], ((t * 5) % 9 - 4) & bm.M64


def bc_steps(script):
    """cache_edges.Script steps with every scripted effect replaced by its
    entry: ("append", [(oc row, (slot, amount), DC set or None)]) | the read
    steps."""
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
