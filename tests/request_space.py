"""Inputs of the randomised tests over the regions of the request space that
tests/synth.py's plain batches never enter (helper, no tests): cold batches
(sct == NULL) and key maps that are no permutation (synth.rekey).  The GPU
tests (test_gpu_parity.py, test_batcher.py) and the CPU tests that hold the
conditions on these inputs (test_oracle_crosscheck.py) build them here, so
both see the same arrays."""
import ctypes as C
import dataclasses
import functools

import numpy as np

from antidote_amd import _abi
from antidote_amd.encode import alloc_result, log_struct, read_struct, result_struct
from synth import cold, random_case, rekey

ALL_TYPES = (_abi.COUNTER_PN, _abi.SET_AW, _abi.REGISTER_MV, _abi.REGISTER_LWW)
ERR = _abi.F_ERR_CORRUPTED | _abi.F_ERR_UNEXPECTED


def run_oracle(oracle_lib, log, req, cap, sparse, threads=4):
    res = alloc_result(req.n_req, log.n_dcs, sparse=sparse, cap_off=cap)
    ls, rs, os_ = log_struct(log), read_struct(req, sparse=sparse), result_struct(res)
    if not sparse:
        ls.oc_mask = None
    assert oracle_lib.oracle_materialize(C.byref(ls), C.byref(rs), C.byref(os_), threads) == 0
    return res


def ignore_all(req):
    """The same requests with the SCT arrays present and every sct_ignore set."""
    return dataclasses.replace(req, sct_ignore=np.ones(req.n_req, np.uint8))


def multi_of(crdt):
    return 0.15 if crdt == _abi.SET_AW else 0.0


def lifted(req, seed, p=0.8):
    """Wide clocks (D >= 33) only.  random_case's R is the maximum of a prefix
    of the key's ops plus a jitter in [-4, 16) per column, and under presence
    masks each DC is absent from R with probability 0.03: over 33 and more
    columns nearly every request then loses a column and includes nothing.
    A share p of the requests therefore gets R + 4 in every column (the jitter
    becomes [0, 20): the prefix is inside) and every DC present in R_mask; the
    others stay as drawn."""
    D = req.n_dcs
    if D < 33:
        return req
    lift = np.random.default_rng(seed).random(req.n_req) < p
    R, Rm = req.R.copy(), req.R_mask.copy()
    R[lift] += np.uint64(4)
    if Rm.any():                      # presence masks in use: all D bits
        full = np.zeros(Rm.shape[1], np.uint64)
        for d in range(D):
            full[d >> 6] |= np.uint64(1 << (d & 63))
        Rm[lift] = full
    return dataclasses.replace(req, R=R, R_mask=Rm)


# ------------------------------------------------------------------ cold batches
# txid = 0.3: a cold read has no SCT for a TxId match to override, so the
# request's TxId must change nothing.  invalid is low because compare skips the
# values under an error flag.
COLD_D = (1, 2, 3, 5, 8, 12, 16, 17, 33, 64, 100, 256)
COLD_SHAPES = [(crdt, D, sparse) for crdt in ALL_TYPES for D in COLD_D for sparse in (False, True)]


@functools.lru_cache(maxsize=2)
def cold_case(crdt, D, sparse):
    """(log, warm-capable req, cap): the SCT arrays are filled (warm = 0.4), so
    that cold(req) drops real rows and ignore_all(req) has real rows to ignore."""
    K = 240 if D <= 64 else 96
    nmax = 130 if D <= 16 else 70
    seed = 15_485_863 + 104_729 * crdt + 37 * D + sparse
    log, req, cap = random_case(seed, crdt, K, D, nmax, sparse=sparse, warm=0.4, txid=0.3,
                                base=0.4, invalid=0.005, corrupt=0.02, multi=multi_of(crdt),
                                identity=(D % 2 == 0))
    return log, lifted(req, seed), cap


def check_conditions(res, n):
    """At least half of the requests include an op, at most a quarter end in an
    error flag."""
    with_op = float((res.count[:n] > 0).mean())
    err = float(((res.flags[:n] & ERR) != 0).mean())
    assert with_op >= 0.5 and err <= 0.25, (with_op, err)
    return with_op, err


# ------------------------------------------------------------------ rekeyed batches
REKEY_D = (3, 8, 16, 64)
REKEY_MODES = ("subset", "repeat")
REKEY_SHAPES = [(crdt, D, sparse) for crdt in ALL_TYPES for D in REKEY_D for sparse in (False, True)]


@functools.lru_cache(maxsize=2)
def rekey_base(crdt, D, sparse, K, nmax):
    seed = 32_452_843 + 1_299_709 * crdt + 41 * D + sparse + 7 * K
    log, req, cap = random_case(seed, crdt, K, D, nmax, sparse=sparse, warm=0.4, txid=0.3,
                                base=0.4, invalid=0.005, corrupt=0.02, multi=multi_of(crdt),
                                identity=(D % 2 == 0))
    return log, lifted(req, seed), cap


def rekey_case(crdt, D, sparse, warm, mode, K=200, nmax=100):
    """(log, req2, cap2) of the base batch under synth.rekey; cold: without SCT."""
    log, req, _ = rekey_base(crdt, D, sparse, K, nmax)
    req2, cap2 = rekey(log, req if warm else cold(req), mode,
                       977 * crdt + 13 * D + 2 * sparse + warm + 5 * REKEY_MODES.index(mode))
    return log, req2, cap2


def check_rekey_properties(log, req, req2, mode):
    """What synth.rekey states about its key maps."""
    K, n = log.n_keys, req2.n_req
    keys = req2.keys.astype(np.int64)
    assert keys.min() >= 0 and keys.max() < K
    if mode == "subset":
        assert n == max(1, K // 3) and len(set(keys.tolist())) == n
        assert n < 3 or (np.diff(keys) < 0).any()            # not in key order
        return
    assert n == 2 * K + 1 > K
    assert K - len(set(keys.tolist())) >= K / 4              # keys never requested
    run = np.r_[0, np.flatnonzero(np.diff(keys) != 0) + 1]   # starts of runs of one key
    best = 0
    for s, e in zip(run, list(run[1:]) + [n]):
        # the run covers a whole aligned group of 8 and one request more
        if e - s >= 9 and (-(-s // 8) * 8 + 8 <= e):
            best = max(best, e - s)
    assert best >= 9
    # every request of a repeated key has its own R (and the rows are near the key's)
    row_of = np.zeros(K, np.int64)
    row_of[req.keys.astype(np.int64)] = np.arange(K)
    d = req2.R.astype(np.int64) - req.R[row_of[keys]].astype(np.int64)
    assert d.min() >= -3 and d.max() <= 3 and (d != 0).any()
    hot = np.bincount(keys, minlength=K).argmax()
    rows = req2.R[keys == hot]
    assert len(rows) >= 9 and len({r.tobytes() for r in rows}) > 1
    assert (req2.R >= 1).all()
    assert len(req2.txid) == n and len(req2.base_value) == n and len(req2.base_off) == n + 1
    if req2.sct is not None:
        assert req2.sct.shape == req2.R.shape and len(req2.sct_ignore) == n
        assert 0 < int(req2.sct_ignore.sum()) < n
