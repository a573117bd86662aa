"""Random logs for the packed index tiers (agn_log_index_pack / pack16 / eff16)
and the kernels that read them -- k_counter_pack4, k_counter_pack8<false|true>
and the packed form of k_counter_quad2 (helper, no tests): counter_pn at
D = 8, dense clocks, cold.

The hand-built cases of pack_cases / pack4_cases / pack8_cases / eff16_cases
put one edge at a time into otherwise plain groups.  Here synth.random_case
draws the log, with lengths on and around the 64-op chunk, and a few keys are
then made wide (a column spanning 2^20), unpacked (2^40), corrupt or long, and
a few effects escape the i16 tier, wherever the draw puts them: in any slot of
a group of 4 or 8, next to each other, in the last group.  The served* /
unservable / *_reference restatements of those files apply to a Case built
here as they are.  tests/test_counter_tiers_random_cpu.py holds the conditions
on these inputs, for every seed of SEEDS."""
import dataclasses
import functools

import numpy as np

import pack4_cases as p4
import pack8_cases as p8
import pack_cases as pc
from antidote_amd import _abi
from synth import cold, random_case, rekey

D, U64 = pc.D, pc.U64
I64MAX, I64MIN = (1 << 63) - 1, -(1 << 63)
EDGE_LENS = np.array([0, 1, 2, 31, 32, 33, 62, 63, 64])
ESCAPES = np.array([-32768, 32768, -32769, 70_000, -70_000, 1 << 40, -(1 << 40), I64MAX, I64MIN + 1],
                   np.int64)
# K = 0, 5 and 7 mod 8: whole groups only, a tail of 5 (one group of 4 and one
# request), a tail of 7
SEEDS = {296: 0, 301: 0, 303: 0}
VARIANTS = ("plain", "long", "seg")
TIERS = ("none", "u32", "narrow", "eff")
KEYMAPS = ("identity", "arange", "perm", "repeat")
CASES = [(K, v) for K in SEEDS for v in VARIANTS]


def lengths(rng, K, long):
    lens = np.where(rng.random(K) < 0.5, rng.choice(EDGE_LENS, K), rng.integers(0, 65, K))
    if long:
        hit = rng.random(K) < 0.02
        lens[hit] = rng.integers(65, 201, int(hit.sum()))
    return lens


@functools.lru_cache(maxsize=None)
def case(K, variant):
    """A pack8_cases.Case.  "plain": lengths 0..64; "long": 2 % of the keys
    65..200 ops long; "seg": the plain log as key_len segments with garbage
    slack, every other key's op ids consecutive, and an id index
    (agn_log_index_ids) built on the device."""
    seed = 611_953 + 1000 * SEEDS[K] + K
    rng = np.random.default_rng(seed + 1)
    lens = lengths(rng, K, variant == "long")
    log, req, _ = random_case(seed, _abi.COUNTER_PN, K, D, 64, invalid=0.005, corrupt=0.02,
                              lens=lens)
    req = cold(req)
    off = log.key_off.astype(np.int64)
    oc, eff = log.oc.copy(), log.eff.copy()
    # wide and unpacked keys: 2^20 or 2^40 on one column of one op
    for k in np.flatnonzero((lens > 0) & (rng.random(K) < 0.03)):
        e = off[k] + int(rng.integers(0, lens[k]))
        oc[e, int(rng.integers(0, D))] += U64(1 << (20 if rng.random() < 0.5 else 40))
    # effects outside +-32767, the escape value -32768 itself among them
    esc = np.flatnonzero(rng.random(len(eff)) < 0.01)
    eff[esc] = ESCAPES[np.arange(len(esc)) % len(ESCAPES)]
    base = req.base_value.copy()
    ext = np.flatnonzero(rng.random(K) < 0.04)
    base[ext] = np.where(np.arange(len(ext)) % 2 == 0, I64MIN, I64MAX)
    op_id = log.op_id.copy()
    if variant == "seg":
        for k in range(0, K, 2):
            op_id[off[k]:off[k + 1]] = 1000 * k + np.arange(lens[k], dtype=np.uint32)
    log = dataclasses.replace(log, oc=oc, eff=eff, op_id=op_id, txid=np.zeros(len(eff), U64))
    req = dataclasses.replace(req, base_value=base, R_mask=np.zeros((K, 1), U64),
                              txid=np.zeros(K, U64))
    c = p8.Case(log, req, [f"k{k} n={n}" for k, n in enumerate(lens)])
    if variant == "seg":
        c.log, c.key_len = p4.segmented(log)
        c.index_ids = True
    return c


def keyed(c, keymap):
    """The case read through a key map: "identity" (req.keys == NULL on the
    device), "arange", a permutation, or synth.rekey's "repeat"."""
    K, req = c.log.n_keys, c.req
    if keymap in ("identity", "arange"):
        return c
    if keymap == "perm":
        p = np.random.default_rng(K).permutation(K)
        req2 = dataclasses.replace(req, keys=p.astype(U64), R=np.ascontiguousarray(req.R[p]),
                                   R_mask=req.R_mask[p], txid=req.txid[p],
                                   base_value=np.ascontiguousarray(req.base_value[p]))
        names = [c.names[k] for k in p]
    else:
        req2, _ = rekey(c.log, req, "repeat", K)
        req2 = dataclasses.replace(req2, txid=np.zeros(req2.n_req, U64))
        names = [c.names[int(k)] for k in req2.keys]
    return dataclasses.replace(c, req=req2, names=names)


def noR_keys(c):
    """Keys with an op whose R lies below the key's minimum in some column:
    the packed thresholds R - base would wrap, every op is excluded."""
    oc = np.asarray(c.log.oc, U64).reshape(-1, D)
    out = np.zeros(c.log.n_keys, bool)
    for k, n in enumerate(p8.lens_of(c)):
        if n:
            a = int(c.log.key_off[k])
            out[k] = bool((c.req.R[k] < oc[a:a + int(n)].min(axis=0)).any())
    return out
