"""Cases for the packed op-log index (agn_log_index_pack) and the packed form
of k_counter_quad2 (helper, no tests): counter_pn at D = 8, dense clocks.

A key is packed when each of its columns spans at most 2^32 - 1; the kernel
serves a pair of adjacent requests from the packed rows when both keys are
packed and at most 64 entries long, and reads oc for every other pair.  The
keys below sit on those edges, and `served_packed` says, from the log alone,
which requests the packed rows serve.  Nothing is drawn at random but the
filler clocks, from fixed seeds."""
import dataclasses

import numpy as np

from antidote_amd import _abi
from antidote_amd.encode import EncodedLog, EncodedRead

D = 8
U64 = np.uint64
M32 = (1 << 32) - 1
TOPV = (1 << 64) - 1
T0 = 1_700_000_000_000_000          # a microsecond timestamp, 1.7e15
KNOBS = [(e, s) for e in "01" for s in "01"]   # AGN_Q2_EFF, AGN_Q2_STORE
FIELDS = ("value", "hole", "lastct", "count", "flags", "err_pos")


# ---------------------------------------------------------------- reference packer
def pack_reference(log):
    """(base [K][8] u64, ok [K] u8, rows [E][8] u32) of the issue's definition;
    rows of unpacked keys are 0 here (unspecified on the device)."""
    K, E = log.n_keys, log.n_entries
    oc = np.asarray(log.oc, U64).reshape(E, D)
    base = np.zeros((K, D), U64)
    ok = np.ones(K, np.uint8)
    rows = np.zeros((E, D), np.uint32)
    for k in range(K):
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        if a == b:
            continue
        seg = oc[a:b]
        base[k] = seg.min(axis=0)
        span = seg.max(axis=0) - base[k]
        ok[k] = 1 if (span <= U64(M32)).all() else 0
        if ok[k]:
            rows[a:b] = (seg - base[k]).astype(np.uint32)
    return base, ok, rows


def key_of_entry(log):
    return np.repeat(np.arange(log.n_keys), np.diff(log.key_off).astype(np.int64))


def served_packed(log, req):
    """Per request: the packed rows serve it -- its pair's keys (requests 2j
    and 2j + 1; the unpaired last request stands for both) are both packed and
    within one 64-entry chunk."""
    _, ok, _ = pack_reference(log)
    lens = np.diff(log.key_off).astype(np.int64)
    keys = req.keys.astype(np.int64)
    good = (ok[keys] == 1) & (lens[keys] <= 64)
    out = np.zeros(req.n_req, bool)
    for j in range(0, req.n_req, 2):
        pair = good[j:j + 2].all() and log.n_entries != 0
        out[j:j + 2] = pair
    return out


# ---------------------------------------------------------------- key builders
def filler(seed, n, spread=1000):
    """n rows of timestamps near T0, rising by op (a DC's clock never runs
    backwards), columns apart by less than 2^32."""
    rng = np.random.default_rng(seed)
    step = rng.integers(1, spread, size=(n, D)).cumsum(axis=0)
    return (T0 + rng.integers(0, 1 << 20, size=D)[None, :] + step).astype(U64)


def mid_R(rows, frac=0.5):
    """R that includes about `frac` of the ops: a row from inside the key."""
    if len(rows) == 0:
        return np.full(D, T0, U64)
    return rows[min(len(rows) - 1, int(len(rows) * frac))].copy()


@dataclasses.dataclass
class Key:
    name: str
    rows: np.ndarray             # [n][8] u64
    R: np.ndarray                # [8] u64
    invalid: tuple = ()          # entries whose effect is EFFECT_INVALID
    corrupt: bool = False        # key_type differs from the request's type


def plain(name, seed, n, frac=0.5):
    r = filler(seed, n)
    return Key(name, r, mid_R(r, frac))


def col_edit(name, seed, n, col, values, R=None, frac=0.5):
    """filler rows with column `col` replaced by `values` (cycled over the ops)."""
    r = filler(seed, n)
    r[:, col] = np.array([int(values[m % len(values)]) for m in range(n)], dtype=U64)
    Rr = mid_R(r, frac)
    if R is not None:
        Rr[col] = U64(R)
    return Key(name, r, Rr)


def edge_keys():
    """The keys the issue names, each with its place in the packer's domain."""
    ks = []
    # column range exactly 2^32 - 1: packed; exactly 2^32: not packed
    ks.append(col_edit("span=2^32-1", 1, 40, 3, [T0, T0 + M32, T0 + 5], R=T0 + M32 - 1))
    ks.append(col_edit("span=2^32", 2, 40, 3, [T0, T0 + M32 + 1, T0 + 5], R=T0 + 7))
    # base 0 with delta 0xFFFFFFFF (R includes it / is one below it)
    ks.append(col_edit("base0 delta=ffffffff R=", 3, 33, 0, [0, M32, 17], R=M32))
    ks.append(col_edit("base0 delta=ffffffff R-1", 4, 33, 0, [0, M32, 17], R=M32 - 1))
    # values at 2^64 - 1
    ks.append(col_edit("top column", 5, 20, 7, [TOPV, TOPV - 9, TOPV - M32], R=TOPV - 1))
    ks.append(col_edit("top column all in", 6, 20, 7, [TOPV, TOPV - 9], R=TOPV))
    # an all-zero column (a DC never seen) beside 1.7e15 columns
    ks.append(col_edit("zero column", 7, 64, 5, [0], R=0))
    ks.append(col_edit("zero column R>0", 8, 63, 5, [0], R=12))
    # R below the base in one column: every op excluded
    k = plain("R<base", 9, 30)
    k.R[2] = k.rows[:, 2].min() - U64(1)
    ks.append(k)
    # R - base >= 2^32 in one column, and in every column
    k = plain("R-base>=2^32 one", 10, 30)
    k.R[4] = k.rows[:, 4].min() + U64(1 << 32)
    ks.append(k)
    k = plain("R-base>=2^32 all", 11, 64)
    k.R[:] = k.rows.max(axis=0) + U64(1 << 40)
    ks.append(k)
    # R equal to an entry's value in a column, and one below it
    k = plain("R==entry", 12, 50)
    k.R[:] = k.rows[-1]
    k.R[6] = k.rows[25, 6]
    ks.append(k)
    k = plain("R==entry-1", 13, 50)
    k.R[:] = k.rows[-1]
    k.R[6] = k.rows[25, 6] - U64(1)
    ks.append(k)
    # an invalid effect among the included ops (the second one is excluded)
    k = plain("invalid included", 14, 40, 0.7)
    k.invalid = (5, 39)
    ks.append(k)
    return ks


def build(keys, order=None):
    """(log, req, names) of a list of Key; order: req.keys (None = identity)."""
    K = len(keys)
    lens = np.array([len(k.rows) for k in keys], np.int64)
    key_off = np.zeros(K + 1, U64)
    key_off[1:] = np.cumsum(lens)
    E = int(key_off[-1])
    oc = np.concatenate([k.rows.reshape(-1, D) for k in keys] + [np.zeros((0, D), U64)])
    op_id = np.concatenate([3 + 2 * np.arange(n, dtype=np.uint32) for n in lens] +
                           [np.zeros(0, np.uint32)])
    eff = np.concatenate([(np.arange(n, dtype=np.int64) * 37 + 11 * j) % 2001 - 1000
                          for j, n in enumerate(lens)] + [np.zeros(0, np.int64)])
    for j, k in enumerate(keys):
        for m in k.invalid:
            eff[int(key_off[j]) + m] = _abi.EFFECT_INVALID
    ktype = np.full(K, _abi.COUNTER_PN, np.uint8)
    for j, k in enumerate(keys):
        if k.corrupt:
            ktype[j] = _abi.SET_AW
    log = EncodedLog(crdt_type=_abi.COUNTER_PN, n_dcs=D, key_off=key_off, key_type=ktype,
                     oc=np.ascontiguousarray(oc, U64), oc_mask=None, op_id=op_id,
                     txid=np.zeros(E, U64), eff=eff)
    ids = np.arange(K, dtype=U64) if order is None else np.asarray(order, U64)
    ix = ids.astype(np.int64)
    R = np.stack([keys[i].R for i in ix]).astype(U64)
    n = len(ix)
    req = EncodedRead(n_dcs=D, req_type=_abi.COUNTER_PN, keys=ids, R=np.ascontiguousarray(R),
                      R_mask=np.zeros((n, 1), U64), sct=None, sct_mask=None, sct_ignore=None,
                      txid=np.zeros(n, U64), base_value=(np.arange(n, dtype=np.int64) * 13) % 89 - 40,
                      base_off=np.zeros(n + 1, U64), base_tag=np.zeros(0, np.uint32),
                      base_tok=np.zeros(0, U64))
    return log, req, [keys[i].name for i in ix]


def pair_keys():
    """Pairs by composition (requests 2j, 2j + 1 with the identity key map)."""
    unp = col_edit("unpacked 10", 21, 10, 1, [T0, T0 + (1 << 33)], R=T0 + 5)
    bad = plain("corrupt", 29, 20)
    bad.corrupt = True
    return [
        plain("packed 64", 20, 64), plain("packed 63", 22, 63),          # both packed
        plain("packed 1", 23, 1, 0.0), unp,                             # packed + unpacked
        plain("packed 5", 24, 5), plain("packed 65", 25, 65),            # packed + 65 ops
        plain("empty", 26, 0), plain("packed 64 b", 27, 64, 0.9),        # length 0 beside 64
        bad, plain("good partner", 30, 33),                             # corrupt + good
        plain("good partner b", 31, 7), dataclasses.replace(bad, name="corrupt b"),
    ]


OWN = ("edges", "pairs_odd", "pairs_even", "keys_reversed", "keys_shuffled")
EFFECT = ("a", "b", "b_keys", "corrupt", "end1", "end65")     # effect_cases.CASES, read cold
CASES = OWN + tuple("effect:" + c for c in EFFECT)


def case(name):
    """(log, req, names).  pairs_odd ends on an unpaired request whose key ends
    at the log's end; pairs_even's last pair does; the keys_* cases read
    through req.keys out of key order."""
    if name == "edges":
        return build(edge_keys())
    if name == "pairs_odd":
        return build(pair_keys() + edge_keys()[:4] + [plain("tail 9", 40, 9)])
    if name == "pairs_even":
        return build(pair_keys() + [plain("last-1", 41, 64), plain("last 3", 42, 3, 0.99)])
    if name == "keys_reversed":
        ks = pair_keys() + edge_keys()
        return build(ks, order=np.arange(len(ks))[::-1])
    if name == "keys_shuffled":
        ks = pair_keys() + edge_keys()
        order = (np.arange(len(ks)) * 7 + 3) % len(ks)     # 7 is coprime to 26: a permutation
        assert len(set(order)) == len(ks)
        return build(ks, order=order)
    if name.startswith("effect:"):   # tests/effect_cases.py, cold
        import effect_cases as ec
        log, req, names, _ = ec.build(name[7:])
        return log, ec.cold(req), names
    raise KeyError(name)


def poison_oc(log, req, value=TOPV):
    """A copy of log whose oc rows are all ones for every key that only
    requests served from the packed rows read."""
    served = served_packed(log, req)
    keys = req.keys.astype(np.int64)
    only = set(keys[served]) - set(keys[~served])
    oc = np.asarray(log.oc, U64).reshape(-1, D).copy()
    koe = key_of_entry(log)
    oc[np.isin(koe, sorted(only))] = U64(value)
    return dataclasses.replace(log, oc=oc), sorted(only)
