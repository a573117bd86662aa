"""Cases for the deferred effect fetch and the paired result stores of
k_counter_quad2 (helper, no tests): counter_pn at D = 8, built with
edges.from_patterns.

The kernel fetches an op's effect only when the op is included, and two
adjacent requests share one wave and, when both are served, one set of stores.
So the cases put the included / excluded / covered ops on the chunk, 16-op
line and key edges, poison the effects nobody may read, and place every
pattern once in either slot of a pair.  Nothing is drawn."""
import dataclasses

import numpy as np

import edges
from antidote_amd import _abi
from synth import cold  # noqa: F401  (the same requests without SCT; callers use effect_cases.cold)

D = 8
LENGTHS = (1, 63, 64, 65, 128, 129, 257)
POISONS = ("invalid", "big")
KNOBS = [(e, s) for e in "01" for s in "01"]   # AGN_Q2_EFF, AGN_Q2_STORE


def spots(n):
    return sorted({p for p in (0, 15, 16, 63, 64, n - 1) if p < n})


def blocks(n, first, second):
    return "".join((first, second)[(m // 16) % 2] for m in range(n))


def put(pat, at):
    """pat with the letters of `at` (position -> letter) set; positions
    outside the key are dropped."""
    s = list(pat)
    for p, c in at.items():
        if 0 <= p < len(s):
            s[p] = c
    return "".join(s)


def base_patterns():
    pats = []
    for n in LENGTHS:
        pats += ["I" * n, "X" * n, "P" * n]
        for p in spots(n):
            pats += [edges.one_at(n, p, "I", "X"), edges.one_at(n, p, "I", "P"),
                     edges.one_at(n, p, "X", "I"), edges.one_at(n, p, "T", "P")]
        pats += ["".join("IX"[m % 2] for m in range(n)), "".join("XI"[m % 2] for m in range(n)),
                 blocks(n, "I", "X"), blocks(n, "X", "I")]
        if n >= 3:   # an invalid effect beside poisoned excluded ops
            pats += ["XEI" + "I" * (n - 3), "IXE" + "I" * (n - 3)]
        for p in (63, 64):
            if p < n:
                pats.append(put("X" * n, {p: "E", p - 2: "I"}))
                pats.append(put("".join("XI"[m % 2] for m in range(n)), {p: "E", p - 1: "X", p + 1: "X"}))
        if n >= 129:   # one E per chunk: the lower position is the error
            pats.append(put("".join("IX"[m % 2] for m in range(n)), {70: "E", 6: "E", 128: "E"}))
            pats.append(put("X" * n, {63: "E", 64: "E", 128: "E"}))
            pats.append(put("".join("XI"[m % 2] for m in range(n)), {127: "E", 65: "E"}))
    return pats


# key indices of CORRUPT whose key_type is flipped: (corrupt, ok), (ok, corrupt),
# (corrupt, corrupt), (ok, ok), and a corrupt last request without a partner
CORRUPT_PATTERNS = ["I" * 65, "IX" * 20, "XI" * 40, "I" * 64 + "XE", "P" * 10 + "TI", "X" * 129,
                    "IIXI", "PPPI", "IXE"]
CORRUPT = (0, 3, 4, 5, 8)

CASES = ("a", "b", "b_keys", "corrupt", "end1", "end65")


def patterns_of(case):
    if case == "a":
        return base_patterns()
    if case in ("b", "b_keys"):       # every pattern in the other slot of its pair
        return ["I"] + base_patterns()
    if case == "corrupt":
        return list(CORRUPT_PATTERNS)
    # the log's last entry is the only included op of the last key
    return ["IX" * 10, "XP" * 3, {"end1": "I", "end65": "X" * 64 + "I"}[case]]


def letters_of(pats):
    return np.frombuffer("".join(pats).encode(), np.uint8)


def poison(log, pats, kind, which="XP"):
    """A copy of log with the effect of every entry whose letter is in `which`
    overwritten: EFFECT_INVALID, or 2^62 + the entry's position in its key."""
    let = letters_of(pats)
    hit = np.isin(let, np.frombuffer(which.encode(), np.uint8))
    eff = log.eff.copy()
    if kind == "invalid":
        eff[hit] = _abi.EFFECT_INVALID
    else:
        pos = np.concatenate([np.arange(len(p), dtype=np.int64) for p in pats])
        eff[hit] = (1 << 62) + pos[hit]
    return dataclasses.replace(log, eff=eff)


def build(case, style=None):
    """(clean log, req, names, patterns) of a case; style None (dense) or
    "uniform" (presence masks, every entry of a key with the key's DC set)."""
    pats = patterns_of(case)
    log, req, _, names = edges.from_patterns(_abi.COUNTER_PN, D, pats, sparse=style,
                                            identity=(case != "b_keys"))
    if case == "corrupt":
        log.key_type = log.key_type.copy()
        log.key_type[list(CORRUPT)] = _abi.SET_AW
    return log, req, names, pats
