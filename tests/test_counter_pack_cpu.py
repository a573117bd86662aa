"""Conditions on the inputs of tests/test_counter_pack.py (no GPU): the numpy
reference of the packer (tests/pack_cases.py, pack_reference) round-trips
every u64, the case list reaches every pair composition and key length the
packed form of k_counter_quad2 distinguishes, and the oc poison of the GPU
test proves what it is meant to prove.

The poison overwrites oc with all ones for the keys that only requests served
from the packed rows read.  The oracle reads oc, so the GPU test compares
against the oracle's result on the CLEAN log; here we check that this result
is independent of the poison where it must be -- the requests not served
packed see no poisoned key, and give the same result on either log -- and that
the poison is visible everywhere else: a served request that includes an op
changes on the poisoned log, so a kernel that read oc for it would fail."""
import numpy as np
import pytest

import pack_cases as pc
from antidote_amd import _abi
from domain import run_oracle


def same(a, b, idx):
    return all(np.array_equal(getattr(a, f)[idx], getattr(b, f)[idx]) for f in pc.FIELDS)


@pytest.mark.parametrize("name", pc.CASES)
def test_reference_round_trips(name):
    log, req, _ = pc.case(name)
    base, ok, rows = pc.pack_reference(log)
    oc = np.asarray(log.oc, np.uint64).reshape(-1, pc.D)
    koe = pc.key_of_entry(log)
    packed = ok[koe] == 1
    back = base[koe] + rows.astype(np.uint64)      # never overflows: it is the value
    assert np.array_equal(back[packed], oc[packed])
    lens = np.diff(log.key_off).astype(np.int64)
    assert (ok[lens == 0] == 1).all() and not base[lens == 0].any()
    for k in np.flatnonzero(lens):
        seg = oc[int(log.key_off[k]):int(log.key_off[k + 1])]
        assert np.array_equal(base[k], seg.min(axis=0))
        assert bool(ok[k]) == bool(((seg.max(axis=0) - seg.min(axis=0)) <= pc.M32).all())


def test_packer_edges_reached():
    log, req, names = pc.case("edges")
    base, ok, rows = pc.pack_reference(log)
    oc = np.asarray(log.oc, np.uint64).reshape(-1, pc.D)
    k = {n: i for i, n in enumerate(names)}
    seg = lambda n: slice(int(log.key_off[k[n]]), int(log.key_off[k[n] + 1]))  # noqa: E731
    span = lambda n: (oc[seg(n)].max(axis=0) - oc[seg(n)].min(axis=0)).max()   # noqa: E731
    assert span("span=2^32-1") == pc.M32 and ok[k["span=2^32-1"]] == 1
    assert span("span=2^32") == pc.M32 + 1 and ok[k["span=2^32"]] == 0
    for n in ("base0 delta=ffffffff R=", "base0 delta=ffffffff R-1"):
        assert base[k[n], 0] == 0 and rows[seg(n), 0].max() == pc.M32 and ok[k[n]] == 1
    assert oc[seg("top column")].max() == pc.TOPV and ok[k["top column"]] == 1
    z = oc[seg("zero column")]
    assert not z[:, 5].any() and (np.delete(z, 5, axis=1) >= pc.T0).all()
    # the reads: R below the base, R - base past 2^32, R on an entry and one below it
    R = req.R
    assert (R[k["R<base"]] < base[k["R<base"]]).sum() == 1
    assert ((R[k["R-base>=2^32 one"]] - base[k["R-base>=2^32 one"]]) >> np.uint64(32) > 0).sum() == 1
    assert ((R[k["R-base>=2^32 all"]] - base[k["R-base>=2^32 all"]]) >> np.uint64(32) > 0).all()
    e = oc[seg("R==entry")][25, 6]
    assert R[k["R==entry"], 6] == e
    assert R[k["R==entry-1"], 6] == oc[seg("R==entry-1")][25, 6] - 1


def test_pair_compositions_reached(oracle_lib):
    seen, lens_seen = set(), set()
    for name in pc.OWN:
        log, req, names = pc.case(name)
        _, ok, _ = pc.pack_reference(log)
        lens = np.diff(log.key_off).astype(np.int64)
        keys = req.keys.astype(np.int64)
        served = pc.served_packed(log, req)
        ident = np.array_equal(keys, np.arange(req.n_req))
        if not ident:
            seen.add("out of key order")
            assert sorted(keys) == list(range(log.n_keys))
        for j in range(0, req.n_req - 1, 2):
            a, b = keys[j], keys[j + 1]
            okp = (bool(ok[a]), bool(ok[b]))
            short = (lens[a] <= 64, lens[b] <= 64)
            if all(okp) and all(short):
                seen.add("both packed")
                assert served[j] and served[j + 1]
                lens_seen |= {int(lens[a]), int(lens[b])}
            else:
                assert not served[j] and not served[j + 1]
            if all(short) and sorted(okp) == [False, True]:
                seen.add("packed + unpacked")
            if all(okp) and sorted((int(lens[a]), int(lens[b]))) [1] == 65 and min(lens[a], lens[b]) <= 64:
                seen.add("packed + 65 ops")
            if b == log.n_keys - 1 and lens[b] > 0 and served[j + 1]:
                seen.add("second key ends the log")
        if req.n_req % 2:
            last = keys[-1]
            if ok[last] and lens[last] <= 64:
                seen.add("unpaired last request")
                assert served[-1]
                if last == log.n_keys - 1:
                    seen.add("unpaired last request ends the log")
        want = run_oracle(oracle_lib, log, req, sparse=False)
        if (want.flags[served] & _abi.F_ERR_UNEXPECTED).any():
            seen.add("invalid effect included, served packed")
        cor = (want.flags & _abi.F_ERR_CORRUPTED) != 0
        for j in np.flatnonzero(cor):
            if served[j] and not cor[j ^ 1 if (j ^ 1) < req.n_req else j]:
                seen.add("corrupt beside a good partner, served packed")
    assert seen == {"both packed", "packed + unpacked", "packed + 65 ops", "unpaired last request",
                    "unpaired last request ends the log", "second key ends the log",
                    "out of key order", "invalid effect included, served packed",
                    "corrupt beside a good partner, served packed"}, seen
    assert {0, 1, 63, 64} <= lens_seen, lens_seen


@pytest.mark.parametrize("name", pc.CASES)
def test_oc_poison_proves_the_path(oracle_lib, name):
    log, req, names = pc.case(name)
    served = pc.served_packed(log, req)
    plog, only = pc.poison_oc(log, req)
    clean = run_oracle(oracle_lib, log, req, sparse=False)
    dirty = run_oracle(oracle_lib, plog, req, sparse=False)
    # not served packed: no poisoned key, the same result
    assert not np.isin(req.keys[~served].astype(np.int64), only).any()
    assert same(clean, dirty, ~served)
    # served packed with an included op: the poison shows
    live = served & (clean.count > 0)
    for i in np.flatnonzero(live):
        assert not same(clean, dirty, [i]), names[i]
    if name in pc.OWN:
        assert live.sum() >= 5 and (~served).any()
    # neither excluded nor included everywhere: the cases exercise the compare
    assert (clean.count > 0).any() and (clean.hole != dirty.hole).any()
