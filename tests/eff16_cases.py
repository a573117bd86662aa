"""Cases for k_counter_pack8<true>, the eight-requests-per-wave read over the
effect tier of the packed index (agn_log_index_eff16; helper, no tests): the
logs of tests/pack8_cases.py with all three tiers registered, and logs of 8, 16
and 17 keys -- one group, two groups, two groups and a tail -- whose effects
sit on the tier's edges.  Built on pack8_cases / pack_cases; nothing new is
drawn at random.

eff16[e] = eff[e] where -32767 <= eff[e] <= 32767, else the escape 0x8000
(-32768): AGN_EFFECT_INVALID and an effect of exactly -32768 escape.  A served
group (pack8_cases.served8) loads eff16 for every lane and reads `eff` only for
the included lanes that hold the escape."""
import dataclasses

import numpy as np

import pack8_cases as p8
import pack_cases as pc
from antidote_amd import _abi

D, U64 = pc.D, pc.U64
I64MAX, I64MIN = (1 << 63) - 1, -(1 << 63)
INVALID = _abi.EFFECT_INVALID
ESC = -32768
FITS = 32767
Case, Key, plain, lens_of, served8, run_oracle = p8.Case, p8.Key, p8.plain, p8.lens_of, p8.served8, p8.run_oracle


# ---------------------------------------------------------------- the numpy restatement
def eff16_reference(eff):
    """(eff16 [E] i16, n_escaped) of the definition above."""
    eff = np.asarray(eff, np.int64)
    fits = (eff >= -FITS) & (eff <= FITS)
    return np.where(fits, eff, ESC).astype(np.int16), int((~fits).sum())


def escaped_of(c):
    return eff16_reference(c.log.eff)[0] == ESC


def included_of(c):
    """Per entry: the op lies in its key's segment and inside the request's R
    (cold, dense clocks: every column at most R's)."""
    oc = np.asarray(c.log.oc, U64).reshape(-1, D)
    out = np.zeros(c.log.n_entries, bool)
    for k, n in enumerate(lens_of(c)):
        a = int(c.log.key_off[k])
        out[a:a + int(n)] = (oc[a:a + int(n)] <= c.req.R[k][None, :]).all(axis=1)
    return out


def expected_value(c):
    """Per request: base_value plus the included ops' effects other than
    AGN_EFFECT_INVALID, mod 2^64 as i64 -- what every kernel stores as `value`,
    under an error flag too (the invalid op is skipped, the rest are summed)."""
    inc = included_of(c)
    out = np.zeros(c.log.n_keys, np.int64)
    for k, n in enumerate(lens_of(c)):
        a = int(c.log.key_off[k])
        s = 0 if c.req.base_value is None else int(c.req.base_value[k])
        s += sum(int(v) for v in c.log.eff[a:a + int(n)][inc[a:a + int(n)]] if int(v) != INVALID)
        s &= (1 << 64) - 1
        out[k] = s - (1 << 64) if s >> 63 else s
    return out


def entry(c, k, op):
    return int(c.log.key_off[k]) + op


def poison_eff(c):
    """A copy of the log whose eff is AGN_EFFECT_INVALID at every non-escaped
    entry of the served groups' keys: the tier's fast path never reads those."""
    eff = np.asarray(c.log.eff, np.int64).copy()
    eff[p8.entries_of(c, served8(c)) & ~escaped_of(c)] = INVALID
    return dataclasses.replace(c.log, eff=eff)


# ---------------------------------------------------------------- key builders
def all_in(name, seed, n):
    """n filler ops, every one inside R."""
    k = plain(name, seed, n)
    k.R = k.rows.max(axis=0) if n else k.R
    return k


@dataclasses.dataclass
class Spec:
    key: Key
    eff: dict = dataclasses.field(default_factory=dict)   # op -> effect (the others keep pack_cases')
    fill: int = None                                       # every op's effect
    base: int = None                                       # the request's base_value


def group_a():
    """One group: the i32 sums' extremes, fitting and escaping values side by
    side, escapes at lanes 0 and 63 with a wrapping base, invalid effects on
    included and excluded ops, a short key before a key that opens on escapes,
    and a last op that escapes."""
    half = plain("a5 invalid excluded only", 1105, 40)     # R = op 20's row: ops 21.. are excluded
    return [
        Spec(all_in("a0 64 x 32767", 1100, 64), fill=FITS),
        Spec(all_in("a1 64 x -32767", 1101, 64), fill=-FITS),
        Spec(all_in("a2 fits beside escapes", 1102, 24),
             eff={0: FITS, 1: -FITS, 2: FITS + 1, 3: ESC, 4: FITS, 23: -FITS}),
        Spec(all_in("a3 escapes at lanes 0 and 63, wrapping", 1103, 64),
             eff={0: I64MAX, 63: I64MIN + 1, 31: 70_000}, base=I64MAX - 5),
        Spec(all_in("a4 invalid twice, included", 1104, 40), eff={3: 1 << 40, 5: INVALID, 17: INVALID, 30: ESC}),
        Spec(half, eff={39: INVALID, 38: 1 << 33, 2: -(1 << 33)}),
        Spec(all_in("a6 short, 9 ops", 1106, 9), eff={8: FITS}),
        Spec(all_in("a7 opens on escapes, last op escapes", 1107, 24),
             eff={0: INVALID, 1: 1 << 35, 2: ESC, 23: -(1 << 34)}),
    ]


def group_b():
    """A second group: an empty key, an invalid effect at lane 63 alone, keys of
    1, 63 and 64 ops, and a short last key whose last op escapes."""
    return [
        Spec(all_in("b0 empty", 1110, 0)),
        Spec(all_in("b1 invalid at lane 63", 1111, 64), eff={63: INVALID, 0: ESC + 1}),
        Spec(all_in("b2 one op, an escape", 1112, 1), eff={0: 99_999}),
        Spec(plain("b3 63 ops", 1113, 63, 0.4), eff={10: FITS + 1, 62: INVALID}),
        Spec(all_in("b4 64 ops", 1114, 64), eff={63: 1 << 50}, base=I64MIN + 3),
        Spec(plain("b5 33 ops", 1115, 33, 0.7)),
        Spec(all_in("b6 2 ops", 1116, 2), eff={0: -FITS, 1: FITS}),
        Spec(all_in("b7 short last, last op escapes", 1117, 5), eff={4: I64MAX, 0: I64MAX}, base=7),
    ]


def tail():
    return [Spec(all_in("t0 tail: escapes through oc", 1120, 12), eff={1: INVALID, 2: 1 << 36, 11: ESC})]


def two_keys():
    """Two groups of plain keys; included escapes in keys 1 and 6 of group 0 only."""
    sp = [Spec(plain(f"w{j}", 1130 + j, 24, 0.6)) for j in range(16)]
    sp[1].eff = {0: 1 << 20, 7: -40_000}
    sp[6].eff = {3: ESC}
    return sp


GAP_KEYS = (3, 10)                   # 40 and 64 ops, one in each group


def id0_gap():
    """pack8_cases' id0 log (an id index, built on the device) with a gap in
    the ids of two served, non-empty keys: agn_log_index_ids gives them
    AGN_ID0_NONE, and their NewLastOp comes from op_id."""
    c = p8.case("id0")
    ids = np.asarray(c.log.op_id, np.uint32).copy()
    for k in GAP_KEYS:
        a = int(c.log.key_off[k])
        ids[a + 2:a + int(lens_of(c)[k])] += 500     # consecutive up to op 1, then 500 further on
    return Case(dataclasses.replace(c.log, op_id=ids), c.req, c.names, index_ids=True)


def build(specs):
    log, req, names = pc.build([s.key for s in specs])
    eff = np.asarray(log.eff, np.int64).copy()
    base = np.asarray(req.base_value, np.int64).copy()
    for k, s in enumerate(specs):
        a, n = int(log.key_off[k]), len(s.key.rows)
        if s.fill is not None:
            eff[a:a + n] = s.fill
        for op, v in s.eff.items():
            assert 0 <= op < n, (s.key.name, op)
            eff[a + op] = v
        if s.base is not None:
            base[k] = s.base
    return Case(dataclasses.replace(log, eff=eff), dataclasses.replace(req, base_value=base), names)


EDGES = {"edges8": lambda: group_a(), "edges16": lambda: group_a() + group_b(),
         "edges17": lambda: group_a() + group_b() + tail(), "two_keys": two_keys}
EDGE_CASES = tuple(EDGES)
ID_CASES = ("id0_gap",)
POISON_CASES = EDGE_CASES + ID_CASES + ("n17", "wide", "invalid", "segmented", "id0")
_CASES = {}


def case(name):
    """An edge case of this file, or the pack8_cases case of that name."""
    if name not in _CASES:
        _CASES[name] = (build(EDGES[name]()) if name in EDGES else id0_gap() if name == "id0_gap"
                        else p8.case(name))
    return _CASES[name]


def bound_case(short):
    """16 keys of 64 ops, every op included, one escape: 1024 entries, the bound
    n_esc * 1024 <= n_entries holds; with one key of 63 ops it does not."""
    sp = [Spec(all_in(f"k{j}", 1150 + j, 63 if (short and j == 9) else 64)) for j in range(16)]
    sp[4].eff = {20: 1 << 30}
    return build(sp)
