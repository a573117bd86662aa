"""Cases for k_counter_pack8, the eight-requests-per-wave read of a whole
partition over the narrow tier of the packed index (agn_log_index_pack16;
helper, no tests): counter_pn at D = 8, dense clocks, cold, the identity key
map (req.keys == NULL on the device; the host request keeps keys = arange).

Block b of the kernel serves requests 8b .. 8b+7 from the u16 rows when all
eight exist, are narrow (packed, every column spanning at most 65 535), at most
64 ops long and not corrupt; every other group reads oc one request after the
other.  The cases are the smallest logs on those edges, built with
pack_cases.build / Key / col_edit and pack4_cases' key builders; `served8`
says, from the log alone, which requests the straight path serves.  Nothing is
drawn at random but pack_cases' filler clocks, from fixed seeds (their columns
rise by less than 1000 per op: a key of at most 64 of them is narrow)."""
import dataclasses

import numpy as np

import pack4_cases as p4
import pack_cases as pc

D, U64, T0, M32 = pc.D, pc.U64, pc.T0, pc.M32
M16 = (1 << 16) - 1
TOP = (1 << 64) - 2                  # the top of the value domain (include/antidote_gpu.h)
Key, plain, col_edit, filler = pc.Key, pc.plain, pc.col_edit, pc.filler
Case, lens_of, run_oracle, segmented = p4.Case, p4.lens_of, p4.run_oracle, p4.segmented
REASONS = ("wide", "unpacked", "long", "corrupt")
N_SPECIAL = 24                       # ops of the keys of the reason and threshold cases


# ---------------------------------------------------------------- the numpy restatement
def spans_of(c):
    """[K][8] column spans over each key's own entries (0 for an empty key)."""
    oc = np.asarray(c.log.oc, U64).reshape(-1, D)
    out = np.zeros((c.log.n_keys, D), U64)
    for k, n in enumerate(lens_of(c)):
        if n:
            seg = oc[int(c.log.key_off[k]):int(c.log.key_off[k]) + int(n)]
            out[k] = seg.max(axis=0) - seg.min(axis=0)
    return out


def narrow_of(c):
    """narrow[k] of agn_log_index_pack16: every column spans at most 65 535."""
    return (spans_of(c) <= U64(M16)).all(axis=1)


def rows16_reference(c):
    """(narrow [K] u8, rows16 [E][8] u16); rows of wide keys are 0 here
    (unspecified on the device)."""
    oc = np.asarray(c.log.oc, U64).reshape(-1, D)
    nar = narrow_of(c)
    rows = np.zeros((c.log.n_entries, D), np.uint16)
    for k, n in enumerate(lens_of(c)):
        if n and nar[k]:
            a = int(c.log.key_off[k])
            seg = oc[a:a + int(n)]
            rows[a:a + int(n)] = (seg - seg.min(axis=0)).astype(np.uint16)
    return nar.astype(np.uint8), rows


def unservable(c):
    """Per key: the reason the straight path does not take its group, or ''."""
    lens, span = lens_of(c), spans_of(c)
    out = []
    for k in range(c.log.n_keys):
        corrupt = lens[k] != 0 and c.log.key_type[k] != c.req.req_type
        top = int(span[k].max())
        out.append("long" if lens[k] > 64 else "unpacked" if top > M32 else "wide" if top > M16
                   else "corrupt" if corrupt else "")
    return out


def served8(c):
    """Per request: its group of eight is complete and every key of it servable."""
    why = unservable(c)
    K = c.log.n_keys
    out = np.zeros(K, bool)
    for g in range(0, K - 7, 8):
        out[g:g + 8] = c.log.n_entries != 0 and not any(why[g:g + 8])
    return out


def entries_of(c, served):
    """Entry mask of the keys of `served` requests."""
    m = np.zeros(c.log.n_entries, bool)
    lens = lens_of(c)
    for k in np.flatnonzero(served):
        a = int(c.log.key_off[k])
        m[a:a + int(lens[k])] = True
    return m


def poison_oc(c, value=pc.TOPV):
    """A copy of the log whose oc rows are all ones for the keys of fully served groups."""
    oc = np.asarray(c.log.oc, U64).reshape(-1, D).copy()
    oc[entries_of(c, served8(c))] = U64(value)
    return dataclasses.replace(c.log, oc=oc)


# ---------------------------------------------------------------- key builders
def wide_key(name, seed):            # one column spans exactly 65 536: packed, not narrow
    return col_edit(name, seed, N_SPECIAL, 1, [T0, T0 + M16 + 1], R=T0 + 5)


def unpacked_key(name, seed):        # one column spans 2^32: not packed
    return col_edit(name, seed, N_SPECIAL, 1, [T0, T0 + (1 << 32)], R=T0 + 5)


def long_key(name, seed):
    return plain(name, seed, 65)


def corrupt_key(name, seed):
    k = plain(name, seed, N_SPECIAL)
    k.corrupt = True
    return k


def empty_key(name, seed):
    return plain(name, seed, 0)


SPECIAL = {"wide": wide_key, "unpacked": unpacked_key, "long": long_key, "corrupt": corrupt_key,
           "empty": empty_key}


def edge_rows(seed, n):
    """filler rows whose column 3 spans exactly 65 535, reached by the last op alone."""
    r = filler(seed, n)
    r[:, 3] = U64(T0) + U64(60_000 // n) * np.arange(n, dtype=U64)
    r[-1, 3] = U64(T0 + M16)
    return r


def edge_limited(name, seed, n):     # the neighbour: column 3 stops after op n // 2
    r = edge_rows(seed, n)
    R = r[-1].copy()
    R[3] = r[n // 2, 3]
    return Key(name, r, R)


def edge_full(name, seed, n):        # R - base = 65 535, the largest true threshold: all included
    r = edge_rows(seed, n)
    return Key(name, r, r[-1].copy())


def edge_minus1(name, seed, n):      # R - base = 65 534: the op at delta 65 535 is excluded
    k = edge_full(name, seed, n)
    k.R[3] = U64(T0 + M16 - 1)
    return k


def iso_saturate2(name, seed, n):
    """R - base = 65 536 in the limiting column and >= 2^32 in another: both
    thresholds saturate, every op is included."""
    k = p4.limited(name, seed, n)
    k.R[3] = k.rows[:, 3].min() + U64(M16 + 1)
    k.R[5] = k.rows[:, 5].min() + U64((1 << 32) + 7)
    return k


ISO = {"noR": (p4.limited, p4.iso_noR),
       "count0": (lambda nm, s, n: p4.crossed(nm, s, n, False), lambda nm, s, n: p4.crossed(nm, s, n, True)),
       "thr_eq": (p4.limited, p4.iso_thr_eq),
       "span_full": (edge_limited, edge_full),
       "span_minus1": (edge_limited, edge_minus1),
       "saturate": (p4.limited, iso_saturate2)}


def groups_with(make_plain, make_special, n=N_SPECIAL):
    """Group 0 plain; groups 1..8 with the special key at positions 0..7."""
    keys, special = [make_plain(f"g0 k{j}", 300 + j, n) for j in range(8)], []
    for pos in range(8):
        for j in range(8):
            if j == pos:
                special.append(len(keys))
                keys.append(make_special(f"g{pos + 1} special@{j}", 310 + pos, n))
            else:
                keys.append(make_plain(f"g{pos + 1} k{j}", 310 + pos, n))   # the same rows
    return keys, special


HALF_PATTERN = ((0, 0), (M16, 0), (0, M16))      # (column 2j, column 2j + 1) deltas, cycled over the ops
HALF_N = 12


def half_keys(low_thr):
    """Eight keys, key 2j + h on dword j, half h: columns 2j, 2j + 1 hold 65 535
    beside 0 and 0 beside 65 535 (and 0, 0), every other column rises.  R
    includes everything but for the threshold of column 2j + h, `low_thr`
    (65 534 or 0): exactly the ops with 65 535 in that column are excluded."""
    keys = []
    for j in range(4):
        for h in range(2):
            r = filler(700 + 2 * j + h, HALF_N)
            for m in range(HALF_N):
                r[m, 2 * j] = U64(T0 + HALF_PATTERN[m % 3][0])
                r[m, 2 * j + 1] = U64(T0 + HALF_PATTERN[m % 3][1])
            R = r.max(axis=0)
            R[2 * j + h] = U64(T0 + low_thr)
            keys.append(Key(f"half dword{j} half{h} thr={low_thr}", r, R))
    return keys


FOLD_N = 64


def fold_op(g, d):
    return (7 * g + 3 * d) % FOLD_N


def fold_keys():
    """Eight 64-op keys, bases apart in every column, every op included; the
    largest delta of (key g, DC d) sits in op (7g + 3d) mod 64 alone."""
    keys = []
    for g in range(8):
        base = U64(T0) + U64((g + 1) * 1_000_003) * np.arange(1, D + 1, dtype=U64)
        r = base[None, :] + np.arange(FOLD_N, dtype=U64)[:, None] * U64(3)
        for d in range(D):
            r[fold_op(g, d), d] = base[d] + U64(40_000 + 1000 * g + 100 * d)
        keys.append(Key(f"fold k{g}", r, r.max(axis=0)))
    return keys


def high_keys():
    """Keys whose bases lie within 65 535 of 2^64 - 2; two of them reach it."""
    keys = []
    for j in range(8):
        r = filler(800 + j, 24)
        r = r - r.min(axis=0)[None, :] + U64(TOP - 60_000)       # every column starts at the base
        if j in (2, 5):
            r[-1, j] = U64(TOP)
        frac = 0.3 + 0.08 * j
        keys.append(Key(f"high k{j}", r, pc.mid_R(r, frac) if j != 5 else r.max(axis=0)))
    return keys


def lengths(ns, seed):
    return [plain(f"k{j} n={n}", seed + j, n, 0.0 if n == 1 else 0.25 + 0.08 * (j % 8))
            for j, n in enumerate(ns)]


SIDE_LENS = (17, 64, 1, 40, 63, 9, 33, 2, 50, 24, 64, 5, 31, 1, 63, 12)

N_KEYS = (1, 7, 8, 9, 15, 16, 17, 24)
CASES = (tuple(f"n{K}" for K in N_KEYS) + REASONS + ("empty",) + tuple(ISO) +
         ("half_65534", "half_0", "fold", "high", "len_64_last", "len_short_last", "invalid",
          "nobase", "id0", "segmented"))


def case(name):
    special = {}
    if name[0] == "n" and name[1:].isdigit():
        keys = [plain(f"k{j}", 200 + j, N_SPECIAL, 0.2 + 0.03 * j) for j in range(int(name[1:]))]
    elif name in SPECIAL:
        keys, special[name] = groups_with(lambda nm, s, n: plain(nm, s, n),
                                          lambda nm, s, n: SPECIAL[name](nm, s))
    elif name in ISO:
        keys, special[name] = groups_with(*ISO[name])
    elif name.startswith("half_"):
        keys = half_keys(int(name[5:]))
    elif name == "fold":
        keys = fold_keys()
    elif name == "high":
        keys = high_keys()
    elif name == "len_64_last":      # a first key of one op; the last rows of the log are read whole
        keys = lengths((1, 63, 64, 24, 64, 1, 63, 64), 600)
    elif name == "len_short_last":   # the row loads past the log's end are clamped
        keys = lengths((64, 63, 1, 64, 24, 63, 1, 5), 610)
    elif name == "invalid":          # one group: included invalid effects in keys 0-3, excluded ones in 4-7
        keys = p4.with_invalid(True) + p4.with_invalid(False)
    else:
        keys = lengths(SIDE_LENS, 900)
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


def mixed_index_case():
    """The index builder's log: narrow, wide (65 536 and 2^20), unpacked, empty
    and 65-entry keys side by side."""
    keys = [plain("narrow 24", 950, 24), wide_key("wide 65536", 951), empty_key("empty", 952),
            unpacked_key("unpacked", 953), long_key("long narrow 65", 954),
            col_edit("wide 2^20", 955, 30, 6, [T0 + (1 << 20), T0, T0 + 9]), plain("narrow 64", 956, 64),
            edge_full("span 65535", 957, 40), plain("narrow 1", 958, 1),
            col_edit("long wide 65", 959, 65, 0, [T0, T0 + 70_000]), plain("narrow 63 last", 960, 63)]
    log, req, names = pc.build(keys)
    return Case(log, req, names)


def bound_case(n_keys):
    """n_keys 8-op keys, key 0 alone wide: n_wide * 1024 <= n_keys holds from 1024 keys on."""
    keys = [col_edit("wide", 970, 8, 2, [T0, T0 + 70_000], R=T0 + 5)]
    keys += [plain(f"k{j}", 971 + (j % 5), 8, 0.6) for j in range(1, n_keys)]
    log, req, names = pc.build(keys)
    return Case(log, req, names)
