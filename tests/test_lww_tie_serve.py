"""The fused register_lww cached read (k_lww_serve) held to the label rule at
every serve_dispatch shape, dense and masked, on the constructed ties of
tests/lww_tie_serve_cases.py (reach: tests/test_lww_tie_serve_cpu.py).

Twin partitions with one label table, one on the fused kernel and one on the
kernel sequence (AGN_LWW_FUSED=0), run the family's script: the planted
snapshot, the constructed read, a read at a later clock with no new op, one
more op at TOP and a read.  After every read the two are equal in every result
field and in key_meta, equal to the model chain (flags, hole, count, LastOpCt
and its mask, out_n, the pair, the status), and -- for every labelled key --
serve the reference transcription's vnode's state with no AGN_F_TS_TIE.  The
unlabelled keys are flagged on both arms and equal the model, which records
today's behaviour.  No key is skipped on any read.  A shape's family runs as
PARTS cases (the keys k = part mod PARTS), each on fresh partitions, so that
no case outlasts the slowest of tests/test_lww_serve.py; path_stats counts a
planted snapshot's store as a batch that is not one fused launch, on both arms.

Beyond the fused widths (D = 65 dense, D = 129 masked) the same family runs
through one cached partition on the sequence (launch_tags with the table), and
through the uncached batcher (materialize_ordered with the caller's own base
pair and SCT) at D = 8 dense and D = 5 masked."""
import functools

import numpy as np
import pytest

import lww_tie_serve_cases as tc
from antidote_amd import _abi
from antidote_amd.engine import Batcher, OpLog
from lww_model import LWW
from test_lww_serve import ERRS, Part, same_result, twins

pytestmark = pytest.mark.gpu

DS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 32, 33, 64]
TIE = _abi.F_TS_TIE
RELABEL = {(8, False, "first"), (5, True, "reversed"), (33, True, "first")}


PARTS = 6       # a shape's family runs as PARTS cases: the keys k with k % PARTS == part


@functools.lru_cache(maxsize=4)
def families(D, masked):
    return tc.family(D, masked)


@functools.lru_cache(maxsize=2)
def expected(D, masked, table, part=None):
    """The family and the host's run of its keys of `part` (None: all)."""
    fam = families(D, masked)
    ks = tuple(range(fam.K)) if part is None else tuple(range(part, fam.K, PARTS))
    out, quirk = tc.script(fam, table, ks)
    assert quirk == set()
    return fam, out, ks


def labels_to(parts, labels):
    for p in parts:
        p.ol.tag_order(0, labels)


def plant(p, fam, k):
    s = fam.keys[k]
    if s["look"] != "hit":
        return 0
    b = s["base"]
    p.bt.store(k, fam.sct[k], clock_mask=fam.full if fam.masked else None, last_op=s["prev"],
               count=s["prev"], tags=None if b is None else [b[0]],
               toks=None if b is None else [b[1]], gc=True)
    return 1


def append(p, k, oc, mask, ts, tag, tx0=1):
    n = len(ts)
    ids, _due = p.ol.append(np.full(n, k, np.uint64), oc, oc_mask=mask, tag=tag, add_tok=ts,
                            txid=np.arange(tx0, tx0 + n, dtype=np.uint64))
    return ids


def read(p, fam, k, R, gc):
    return p.bt.read(k, R=R, R_mask=fam.full if fam.masked else None, gc=bool(gc), out_cap=4)


def check(g, w, fam, table, labelled, ctx):
    """One read's result against the host's: every field."""
    assert g["status"] == w["status"], (ctx, "status", g["status"], w["status"])
    assert g["flags"] == w["flags"], (ctx, "flags", g["flags"], w["flags"])
    assert g["count"] == w["count"] and g["hole"] == w["hole"], (ctx, g["count"], g["hole"], w)
    if not w["flags"] & _abi.F_CT_IGNORE:
        assert np.array_equal(g["lastct"], w["lastct"]), (ctx, g["lastct"], w["lastct"])
        if fam.masked:
            assert np.array_equal(g["lastct_mask"], w["lastct_mask"]), (ctx, "LastOpCt mask")
    assert g["out_n"] == w["out_n"] == 1 and g["err_pos"] == 0xFFFFFFFF, (ctx, g["out_n"])
    got = (int(g["out_tag"][0]), int(g["out_tok"][0]))
    assert got == w["pair"], (ctx, got, w["pair"])
    if labelled:
        assert not g["flags"] & (TIE | ERRS), (ctx, g["flags"])
        assert (got[1], tc.value(table, got[0])) == w["vnode"], (ctx, got, w["vnode"])


def load(parts, fam, ks):
    """Every key's planted snapshot, then its ops.  -> stores per partition."""
    stores = 0
    for k in ks:
        for p in parts:
            n = plant(p, fam, k)
        stores += n
        for p in parts:
            ids = append(p, k, fam.oc[k], fam.mask[k], fam.ts[k], fam.tag[k])
            assert np.array_equal(ids, np.arange(1, fam.keys[k]["n"] + 1)), "ids 1.. per key"
    return stores


def run_reads(parts, fam, out, table, which):
    """Read number `which` of every key of `out` on every partition."""
    for k in out:
        s = fam.keys[k]
        w = out[k]["reads"][which]
        ctx = (fam.D, fam.masked, table, s["name"], tc.READS[which])
        gs = [read(p, fam, k, w["R"], w["gc"]) for p in parts]
        if len(gs) == 2:
            same_result(gs[0], gs[1], ctx)
            ka = np.array([k], np.uint64)
            ma, mb = parts[0].ol.key_meta(ka), parts[1].ol.key_meta(ka)
            assert all(np.array_equal(x, y) for x, y in zip(ma, mb)), (ctx, "key_meta", ma, mb)
        for g in gs:
            check(g, w, fam, table, not s["unl"], ctx)
            assert bool(g["flags"] & TIE) == bool(w["flags"] & TIE), ctx
        if which == 0:
            assert bool(gs[0]["flags"] & TIE) == s["unl"], ctx


def one_more_op(parts, fam, out):
    for k in out:
        oc, m, ts, tag = out[k]["extra"]
        for p in parts:
            append(p, k, oc.reshape(1, fam.D), None if m is None else m.reshape(1, fam.W),
                   np.array([ts], np.uint64), np.array([tag], np.uint32), tx0=5000)


SHAPES = [(D, m, t, part) for D in DS for m in (False, True) if D >= 2 or not m
          for t in tc.TABLES for part in range(PARTS)]


@pytest.mark.parametrize("D,masked,table,part", SHAPES,
                         ids=[f"D{d}-{'masked' if m else 'dense'}-{t}-{p}"
                              for d, m, t, p in SHAPES])
def test_fused_and_sequence_settle_ties_by_label(eng, monkeypatch, D, masked, table, part):
    fam, out, ks = expected(D, masked, table, part)
    labels = tc.TABLES[table]
    pa, pb = twins(eng, monkeypatch, D, masked, fam.K, max_batch=8)
    parts = (pa, pb)
    try:
        labels_to(parts, labels)
        stores = load(parts, fam, ks)
        # a store is a batch of its own, counted with the batches that are not one fused launch
        before = [p.bt.path_stats() for p in parts]
        assert all(b == {"fused": 0, "sequence": stores} for b in before), before
        run_reads(parts, fam, out, table, 0)
        if (D, masked, table) in RELABEL:      # every label rewritten, the order kept
            labels_to(parts, labels // np.uint64(3))
        run_reads(parts, fam, out, table, 1)
        one_more_op(parts, fam, out)
        run_reads(parts, fam, out, table, 2)
        sa, sb = pa.bt.path_stats(), pb.bt.path_stats()
        assert sa == {"fused": 3 * len(ks), "sequence": stores}, sa      # no read on the sequence
        assert sb == {"fused": 0, "sequence": stores + 3 * len(ks)}, sb  # and none fused
        assert pa.bt.stats()["reads"] == pb.bt.stats()["reads"] == 3 * len(ks)
    finally:
        pa.close()
        pb.close()


WIDE = [(65, False, "first"), (65, False, "reversed"), (129, True, "first"),
        (129, True, "reversed")]


@pytest.mark.parametrize("D,masked,table", WIDE,
                         ids=[f"D{d}-{'masked' if m else 'dense'}-{t}" for d, m, t in WIDE])
def test_cached_sequence_beyond_the_fused_widths(eng, monkeypatch, D, masked, table):
    """run_batch_cached_tags -> launch_tags(..., ord): no fused kernel at these
    widths, so the default partition serves from the kernel sequence."""
    monkeypatch.delenv("AGN_LWW_FUSED", raising=False)
    fam, out, ks = expected(D, masked, table)
    p = Part(eng, D, masked, fam.K, max_batch=8)
    try:
        labels_to((p,), tc.TABLES[table])
        stores = load((p,), fam, ks)
        run_reads((p,), fam, out, table, 0)
        run_reads((p,), fam, out, table, 1)
        one_more_op((p,), fam, out)
        run_reads((p,), fam, out, table, 2)
        assert p.bt.path_stats() == {"fused": 0, "sequence": stores + 3 * fam.K}
    finally:
        p.close()


@functools.lru_cache(maxsize=None)
def direct(D, masked, table):
    """The constructed read of every key as one materialize/4 with the caller's
    own SCT and base pair: the model's result under `table` (None: no table)."""
    fam = tc.family(D, masked, repeats=False)
    labels = None if table is None else tc.TABLES[table]
    want = []
    for k, s in enumerate(fam.keys):
        ch = tc.KeyChain(D, masked, labels)
        if s["look"] == "hit":
            ch.plant(s["base"], fam.sct[k], s["prev"])
        for q in range(s["n"]):
            ch.append(fam.oc[k][q], fam.mask[k][q] if masked else None, fam.ts[k][q],
                      fam.tag[k][q])
        want.append(ch.read(fam.R[k], 0))
    return fam, want


def read_direct(bt, fam, k):
    s = fam.keys[k]
    hit, b = s["look"] == "hit", s["base"]
    return bt.read(k, R=fam.R[k], R_mask=fam.full if fam.masked else None,
                   sct=fam.sct[k] if hit else None,
                   sct_mask=fam.full if hit and fam.masked else None,
                   base_tag=None if b is None else [b[0]], base_tok=None if b is None else [b[1]],
                   out_cap=4)


UNCACHED = [(D, m, t) for D, m in ((8, False), (5, True)) for t in ("first", "reversed", None)]


@pytest.mark.parametrize("D,masked,table", UNCACHED,
                         ids=[f"D{d}-{'masked' if m else 'dense'}-{t or 'no-table'}"
                              for d, m, t in UNCACHED])
def test_uncached_batcher_with_labels(eng, D, masked, table):
    """run_batch -> materialize_ordered(..., oplog_lww_order): the caller's base
    pair and SCT meet the table; a fresh log without one gives the id order,
    flagged."""
    fam, want = direct(D, masked, table)
    with OpLog(eng, LWW, D, fam.K, sparse=masked) as ol, Batcher(ol, max_batch=8) as bt:
        if table is not None:
            ol.tag_order(0, tc.TABLES[table])
        for k in range(fam.K):
            ol.append(np.full(fam.keys[k]["n"], k, np.uint64), fam.oc[k], oc_mask=fam.mask[k],
                      tag=fam.tag[k], add_tok=fam.ts[k],
                      txid=np.arange(1, fam.keys[k]["n"] + 1, dtype=np.uint64))
        flagged = changed = 0
        for k, s in enumerate(fam.keys):
            g, w = read_direct(bt, fam, k), want[k]
            ctx = (D, masked, table, s["name"])
            assert g["flags"] == w["flags"], (ctx, g["flags"], w["flags"])
            assert g["count"] == w["count"] and g["hole"] == w["hole"], (ctx, g, w)
            assert g["err_pos"] == 0xFFFFFFFF, ctx
            if not w["flags"] & _abi.F_CT_IGNORE:
                assert np.array_equal(g["lastct"], w["lastct"]), ctx
                if masked:
                    assert np.array_equal(g["lastct_mask"], w["lastct_mask"]), ctx
            assert g["out_n"] == 1, ctx
            got = (int(g["out_tag"][0]), int(g["out_tok"][0]))
            assert got == w["pair"], (ctx, got, w["pair"])
            # the id order over the tags at TOP, from the builder's own positions
            T = [t for q, t in s["tied"].items() if w["incl"][q]]
            T += [s["base"][0]] if s["base"] and s["base"][1] == tc.TOP else []
            assert w["info"]["nT"] == len(set(T)), ctx
            if table is None:       # no table: the id order, every tie flagged
                assert bool(g["flags"] & TIE) == (len(set(T)) > 1), ctx
                assert got[0] == max(T), ctx
            else:
                assert bool(g["flags"] & TIE) == s["unl"], ctx
            flagged += bool(g["flags"] & TIE)
            changed += got[0] != max(T)
        # the table changes the id-order answer of many keys; without one, of none
        assert flagged > (10 if table is None else 5), flagged
        assert (changed > 10) if table is not None else (changed == 0), changed
