"""Cases for k_counter_pack4, the four-requests-per-wave packed read of a whole
partition (helper, no tests): counter_pn at D = 8, dense clocks, cold, the
identity key map (req.keys == NULL on the device; the host request keeps
keys = arange, which the oracle reads as the same batch).

Block b of the kernel serves requests 4b .. 4b+3 from the packed rows when all
four exist, are packed, at most 64 ops long and not corrupt; every other group
reads oc one request after the other.  The cases below are the smallest logs
on those edges, built with pack_cases.build / Key / col_edit; `served4` says,
from the log alone, which requests the straight path serves.  Nothing is drawn
at random but pack_cases' filler clocks, from fixed seeds."""
import ctypes as C
import dataclasses

import numpy as np

import pack_cases as pc
from antidote_amd.encode import EncodedLog, alloc_result, log_struct, ptr, read_struct, result_struct

D, U64, T0, M32 = pc.D, pc.U64, pc.T0, pc.M32
Key, plain, col_edit, filler = pc.Key, pc.plain, pc.col_edit, pc.filler
REASONS = ("long", "unpacked", "corrupt")


@dataclasses.dataclass
class Case:
    log: EncodedLog
    req: object
    names: list
    key_len: np.ndarray = None      # segments with slack (agn_log.key_len)
    index_ids: bool = False         # build agn_log.key_id0 on the device
    special: dict = dataclasses.field(default_factory=dict)   # kind -> request indices


def lens_of(c):
    return (c.key_len if c.key_len is not None else np.diff(c.log.key_off)).astype(np.int64)


def packed_of(c):
    """pack_ok per key (pack_cases.pack_reference's rule, over the key's own entries)."""
    oc = np.asarray(c.log.oc, U64).reshape(-1, D)
    ok = np.ones(c.log.n_keys, bool)
    for k, n in enumerate(lens_of(c)):
        if n:
            seg = oc[int(c.log.key_off[k]):int(c.log.key_off[k]) + int(n)]
            ok[k] = bool(((seg.max(axis=0) - seg.min(axis=0)) <= U64(M32)).all())
    return ok


def unservable(c):
    """Per key: the reason the straight path does not take its group, or ''."""
    lens, ok = lens_of(c), packed_of(c)
    out = []
    for k in range(c.log.n_keys):
        corrupt = lens[k] != 0 and c.log.key_type[k] != c.req.req_type
        out.append("long" if lens[k] > 64 else "unpacked" if not ok[k] else "corrupt" if corrupt else "")
    return out


def served4(c):
    """Per request: its group of four is complete and every key of it servable."""
    why = unservable(c)
    K = c.log.n_keys
    out = np.zeros(K, bool)
    for g in range(0, K - 3, 4):
        out[g:g + 4] = c.log.n_entries != 0 and not any(why[g:g + 4])
    return out


# ---------------------------------------------------------------- key builders
def long_key(name, seed):
    return plain(name, seed, 65)


def unpacked_key(name, seed):
    return col_edit(name, seed, 10, 1, [T0, T0 + (1 << 32)], R=T0 + 5)   # a column spanning 2^32


def corrupt_key(name, seed):
    k = plain(name, seed, 20)
    k.corrupt = True
    return k


def empty_key(name, seed):
    return plain(name, seed, 0)


SPECIAL = {"long": long_key, "unpacked": unpacked_key, "corrupt": corrupt_key, "empty": empty_key}


def limited(name, seed, n, col=3):
    """Every op inside R but for column `col`, which stops after op n // 2:
    the neighbour every isolated key below is a variation of."""
    r = filler(seed, n)
    R = r[-1].copy()
    R[col] = r[n // 2, col]
    return Key(name, r, R)


def iso_noR(name, seed, n):          # R below the base in one column: every op excluded
    k = limited(name, seed, n)
    k.R[6] = k.rows[:, 6].min() - U64(1)
    return k


def iso_saturate(name, seed, n):     # R - base >= 2^32 in the limiting column: every op included
    k = limited(name, seed, n)
    k.R[3] = k.rows[:, 3].min() + U64((1 << 32) + 5)
    return k


def iso_thr_eq(name, seed, n):       # R on another op's value: its delta equals the threshold
    k = limited(name, seed, n)
    k.R[3] = k.rows[n // 2 + 3, 3]
    return k


def crossed(name, seed, n, at_base):
    """Column 0 runs backwards, so no op holds every column's minimum.  With
    R = the column minima (R - base = 0 everywhere, not below it) every op is
    excluded: count 0 without noR.  Else R = the maxima: every op included."""
    r = filler(seed, n)
    r[:, 0] = r[::-1, 0].copy()
    return Key(name, r, r.min(axis=0) if at_base else r.max(axis=0))


ISO = {"noR": (limited, iso_noR), "saturate": (limited, iso_saturate),
       "thr_eq": (limited, iso_thr_eq),
       "count0": (lambda nm, s, n: crossed(nm, s, n, False), lambda nm, s, n: crossed(nm, s, n, True))}


def groups_with(make_plain, make_special, n=24):
    """Group 0 plain; groups 1..4 with the special key at positions 0..3."""
    keys, special = [make_plain(f"g0 k{j}", 300 + j, n) for j in range(4)], []
    for pos in range(4):
        for j in range(4):
            if j == pos:
                special.append(len(keys))
                keys.append(make_special(f"g{pos + 1} special@{j}", 310 + pos, n))
            else:
                keys.append(make_plain(f"g{pos + 1} k{j}", 310 + pos, n))   # the same rows
    return keys, special


def ctmax_keys():
    """Four keys whose bases differ in every column, key g's largest delta in column 2g + 1."""
    keys = []
    for g in range(4):
        r = filler(400 + g, 30) + U64((g + 1) * 1_000_003) * np.arange(1, D + 1, dtype=U64)[None, :]
        r[-1, 2 * g + 1] += U64(1 << 30)
        keys.append(Key(f"ctmax k{g}", r, r.max(axis=0)))
    return keys


def with_invalid(included):
    """A different entry of each key holds AGN_EFFECT_INVALID: inside R, or past it."""
    keys = []
    for j, m in enumerate((0, 5, 17, 30)):
        k = plain(f"invalid@{m} {'in' if included else 'out'}", 500 + j, 40, 0.5)   # ops 0..20 included
        k.invalid = (m if included else 40 - 1 - m // 2,)
        if included:
            k.R[:] = k.rows[max(m, 20)]
        keys.append(k)
    return keys


def segmented(log):
    """The same keys as segments with slack after each (agn_log.key_len); the slack holds garbage."""
    K = log.n_keys
    lens = np.diff(log.key_off).astype(np.int64)
    pad = 1 + (np.arange(K) % 3) * 2
    start = np.zeros(K + 1, np.int64)
    start[1:] = np.cumsum(lens + pad)
    E2 = int(start[-1])
    src = np.concatenate([np.arange(lens[k]) + int(log.key_off[k]) for k in range(K)]).astype(np.int64)
    dst = np.concatenate([np.arange(lens[k]) + start[k] for k in range(K)]).astype(np.int64)
    oc = np.full((E2, D), 0x5A5A5A5A5A5A5A5A, U64)
    op_id, eff = np.full(E2, 0xFFFFFFF0, np.uint32), np.full(E2, 99999, np.int64)
    oc[dst], op_id[dst], eff[dst] = np.asarray(log.oc, U64).reshape(-1, D)[src], log.op_id[src], log.eff[src]
    seg = EncodedLog(crdt_type=log.crdt_type, n_dcs=D, key_off=start.astype(U64), key_type=log.key_type,
                     oc=oc, oc_mask=None, op_id=op_id, txid=np.zeros(E2, U64), eff=eff)
    return seg, lens.astype(U64)


def mixed_lengths(K):
    return [plain(f"k{j} n={n}", 200 + j, n, 0.3 + 0.07 * j)
            for j, n in zip(range(K), (17, 64, 1, 40, 63, 9, 33, 2, 50))]


N_KEYS = (1, 2, 3, 4, 5, 7, 8, 9)
CASES = (tuple(f"n{K}" for K in N_KEYS) + REASONS + ("empty",) + tuple(ISO) +
         ("ctmax", "len_64_last", "len_short_last", "invalid", "nobase", "id0", "segmented"))


def case(name):
    special = {}
    if name[0] == "n" and name[1:].isdigit():
        keys = mixed_lengths(int(name[1:]))
    elif name in SPECIAL:
        keys, special[name] = groups_with(lambda nm, s, n: plain(nm, s, n), lambda nm, s, n: SPECIAL[name](nm, s))
    elif name in ISO:
        keys, special[name] = groups_with(*ISO[name])
    elif name == "ctmax":
        keys = ctmax_keys()
    elif name == "len_64_last":      # the last rows of the log are read whole
        keys = [plain("n=1", 600, 1, 0.0), plain("n=63", 601, 63), plain("n=64", 602, 64),
                plain("n=64 last", 603, 64, 0.9)]
    elif name == "len_short_last":   # the row loads past the log's end are clamped
        keys = [plain("n=64", 610, 64), plain("n=63", 611, 63), plain("n=1", 612, 1, 0.0),
                plain("n=5 last", 613, 5)]
    elif name == "invalid":
        keys = with_invalid(True) + with_invalid(False)
    else:
        keys = mixed_lengths(8)
    log, req, names = pc.build(keys)
    c = Case(log, req, names, special=special)
    if name == "nobase":
        c.req = dataclasses.replace(req, base_value=None)
    if name == "id0":                # consecutive op ids: agn_log_index_ids gives every key a base
        ids = np.concatenate([1000 * k + np.arange(n, dtype=np.uint32) for k, n in enumerate(lens_of(c))])
        c.log, c.index_ids = dataclasses.replace(log, op_id=ids.astype(np.uint32)), True
    if name == "segmented":
        c.log, c.key_len = segmented(log)
    return c


def run_oracle(oracle_lib, c, log=None):
    """oracle_materialize of the case (over `log` when given: the poisoned copy)."""
    log = c.log if log is None else log
    res = alloc_result(c.req.n_req, D, sparse=False)
    ls, rs, os_ = log_struct(log), read_struct(c.req, sparse=False), result_struct(res)
    ls.oc_mask = None
    if c.key_len is not None:
        ls.key_len = ptr(c.key_len)
    assert oracle_lib.oracle_materialize(C.byref(ls), C.byref(rs), C.byref(os_), 2) == 0
    return res


def poison_oc(c, value=pc.TOPV):
    """A copy of the log whose oc rows are all ones for the keys of fully served groups."""
    served = served4(c)
    oc = np.asarray(c.log.oc, U64).reshape(-1, D).copy()
    lens = lens_of(c)
    for k in np.flatnonzero(served):
        a = int(c.log.key_off[k])
        oc[a:a + int(lens[k])] = U64(value)
    return dataclasses.replace(c.log, oc=oc)
