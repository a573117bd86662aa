"""The constructed edge cases of tests/edges.py through the HIP kernels, every
key against the C oracle bit for bit (tests/test_edges_cpu.py checks the
oracle against the dict transcription on the same cases and that each named
edge is reached).

Family A (scan edges) runs through every counter kernel and masked form and
every tags shape; B (table limits and the capacity contract), C (removal
token batches) and D (ops over a chunk edge) through every tags shape; E (GC)
through agn_prune_ops in both forms and agn_oplog_prune with its knobs; F
(hand-on lists) through the masked list passes."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import edges
import test_oplog as tol
from antidote_amd import _abi
from antidote_amd.encode import (EncodedRead, alloc_result, log_struct, n_words, read_struct,
                                 result_struct)
from antidote_amd.engine import OpLog
import synth
from synth import compare
from test_gpu_parity import COUNTER_IMPLS, _set_impl
from test_prune import oracle_prune

pytestmark = pytest.mark.gpu

TAGS = (_abi.SET_AW, _abi.REGISTER_MV)
CAPF = _abi.F_ERR_CAPACITY
_LAST: dict = {}


@contextlib.contextmanager
def scratch(eng):
    """Frees the device buffers allocated inside the block."""
    before = set(eng._bufs)
    try:
        yield
    finally:
        for b in list(eng._bufs - before):
            b.free()


def built(oracle_lib, key, build, sparse):
    """(case, oracle result) of the builder, kept for the next test of the
    same case (the parameters are ordered so that those follow each other)."""
    if _LAST.get("key") != key:
        _LAST.clear()
        case = build()
        log, req, cap = case[:3]
        res = alloc_result(req.n_req, log.n_dcs, sparse=bool(sparse), cap_off=cap)
        ls, rs, os_ = log_struct(log), read_struct(req, sparse=bool(sparse)), result_struct(res)
        if not sparse:
            ls.oc_mask = None
        assert oracle_lib.oracle_materialize(C.byref(ls), C.byref(rs), C.byref(os_), 4) == 0
        _LAST.update(key=key, case=case, res=res)
    return _LAST["case"], _LAST["res"]


def explain(bad, names):
    return [(names[b[0]],) + tuple(b[1:]) for b in bad[:8]]


def check(crdt, D, got, want, sparse, names, skip=()):
    bad = [b for b in compare(crdt, D, got, want, bool(sparse), len(names)) if b[0] not in skip]
    assert not bad, explain(bad, names)
    if crdt != _abi.COUNTER_PN:
        ok = (want.flags & (_abi.F_ERR_UNEXPECTED | _abi.F_ERR_CORRUPTED)) == 0
        for i in skip:
            ok[i] = False
        assert np.array_equal(got.out_n[ok], want.out_n[ok])
    err = (want.flags & _abi.F_ERR_UNEXPECTED) != 0
    assert np.array_equal(got.err_pos[err], want.err_pos[err])


# ------------------------------------------------------------------ family A, counters
A_DENSE = [(D, impl) for D in (1, 3, 4, 8, 12, 17, 64, 100, 256) for impl in COUNTER_IMPLS]


def cold(case):
    """The same requests without SCT (the cold kernels)."""
    return (case[0], synth.cold(case[1])) + tuple(case[2:])


def with_cold(params, ids=None, group=lambda p: p[0]):
    """The parameter sets as they are (ids unchanged) and once more with a
    trailing True: the cold form of the case, id + "-cold".  The cold sets of
    a run of sets with one `group` value (one built case) follow the run."""
    out, run = [], []
    for j, p in enumerate(params):
        p = p if isinstance(p, tuple) else (p,)
        name = ids[j] if ids is not None else "-".join(str(x) for x in p)
        if run and group(p) != group(params[j - 1] if isinstance(params[j - 1], tuple)
                                     else (params[j - 1],)):
            out += run
            run = []
        out.append(pytest.param(*p, False, id=name))
        run.append(pytest.param(*p, True, id=name + "-cold"))
    return out + run


def maybe_cold(build, is_cold):
    return (lambda: cold(build())) if is_cold else build


@pytest.mark.parametrize("D,impl,is_cold", with_cold(A_DENSE))
def test_scan_edges_counter(eng, oracle_lib, monkeypatch, D, impl, is_cold):
    _set_impl(monkeypatch, impl)
    crdt = _abi.COUNTER_PN
    (log, req, _, names), want = built(oracle_lib, ("a", crdt, D, None, is_cold), maybe_cold(
        lambda: edges.family_a(crdt, D, identity=(D % 2 == 0)), is_cold), None)
    got = eng.materialize_host(log, req, sparse=False)
    check(crdt, D, got, want, None, names)


# test_presence.py's knob combinations (see test_presence_vs_oracle)
MASKED_IMPLS = {"vgpr": "0", "quad": "2", "quad2": "3", "general": "0", "split": "2",
                "split_km1": "2", "split_ctflag": "2", "split_mixed": "2", "split_two": "2",
                "split_cold": "2", "split_one_cold": "2"}
A_MASKED = [(D, style, impl, path) for D in (3, 8) for style in ("uniform", "mixed")
            for cold in (False, True) for impl in MASKED_IMPLS if impl.endswith("cold") == cold
            for path in ("host", "device_indexed", "device_no_index")
            if not (impl.startswith("split") and path == "host")]


def presence_knobs(monkeypatch, impl):
    monkeypatch.delenv("AGN_COUNTER_GLDS", raising=False)
    monkeypatch.setenv("AGN_COUNTER_VARIANT", MASKED_IMPLS[impl])
    monkeypatch.setenv("AGN_COUNTER_EARLY", "1" if impl.startswith("split") else "0")
    monkeypatch.setenv("AGN_Q8E_KM", "1" if impl == "split_km1" else "0")
    if impl == "split_cold":
        monkeypatch.delenv("AGN_Q8E_TWO", raising=False)
    else:
        monkeypatch.setenv("AGN_Q8E_TWO", "1" if impl == "split_two" else "0")
    if impl == "general":
        monkeypatch.setenv("AGN_COUNTER_IMPL", "general")
    else:
        monkeypatch.delenv("AGN_COUNTER_IMPL", raising=False)


def masked_device(eng, log, req, index, hints=0):
    with scratch(eng):
        dl, dr = eng.upload_log(log), eng.upload_read(req, sparse=True)
        dr.struct.hints = hints
        if index:
            eng.index_masks(dl)
        dres = eng.alloc_result(req.n_req, log.n_dcs, sparse=True)
        eng.materialize(dl, dr, dres)
        return eng.fetch_result(dres)


@pytest.mark.parametrize("D,style,impl,path", A_MASKED)
def test_scan_edges_counter_masked(eng, oracle_lib, monkeypatch, D, style, impl, path):
    presence_knobs(monkeypatch, impl)
    crdt = _abi.COUNTER_PN
    is_cold = impl.endswith("cold")

    def build():
        case = edges.family_a(crdt, D, style, identity=(D % 2 == 0))
        return cold(case) if is_cold else case
    (log, req, _, names), want = built(oracle_lib, ("a", crdt, D, style, is_cold), build, style)
    if path == "host":
        got = eng.materialize_host(log, req, sparse=True)
    else:
        got = masked_device(eng, log, req, path == "device_indexed",
                            {"split_ctflag": _abi.HINT_CT_FLAG,
                             "split_mixed": _abi.HINT_MIXED}.get(impl, 0))
    check(crdt, D, got, want, style, names)


# ------------------------------------------------------------------ families A-D, tags
# (D, presence style, knobs): one lane per op (D <= 8), contiguous rows (CT)
# with 4 and 8 DCs per lane and the strided loads of AGN_TAGS_CT=0, the
# general shape, the per-entry-mask pass (AGN_TAGS_MSK=0 / mixed keys) and
# the masked dense passes.
TAG_MODES = [(D, None, {}) for D in (2, 5, 8)]
for _D in (16, 64, 128):
    TAG_MODES += [(_D, None, {}), (_D, None, {"AGN_TAGS_DPL8": "1"}), (_D, None, {"AGN_TAGS_CT": "0"})]
TAG_MODES.append((100, None, {}))
for _D in (3, 8, 16):
    for _style in ("uniform", "mixed"):
        TAG_MODES += [(_D, _style, {"AGN_TAGS_MSK": "1"}), (_D, _style, {"AGN_TAGS_MSK": "0"})]
TAG_IDS = ["D%d-%s-%s" % (D, s or "dense", "".join(f"{k[9:]}{v}" for k, v in kn.items()) or "auto")
           for D, s, kn in TAG_MODES]


def tag_knobs(monkeypatch, knobs):
    for k in ("AGN_TAGS_DPL8", "AGN_TAGS_CT", "AGN_TAGS_MSK"):
        if k in knobs:
            monkeypatch.setenv(k, knobs[k])
        else:
            monkeypatch.delenv(k, raising=False)


def tags_case(family, crdt, D, style):
    if family == "a":
        return edges.family_a(crdt, D, style, identity=(D % 2 == 0))
    if family == "c":
        return edges.family_c(crdt, D, style)[:4]
    return edges.family_d(D, style)


# multi-entry ops (family D) are set_aw's
TAG_CASES = [(f, c, m) for f in "acd" for c in TAGS for m in TAG_MODES
             if f != "d" or c == _abi.SET_AW]


@pytest.mark.parametrize("family,crdt,mode,is_cold", with_cold(
    TAG_CASES, [f"{f}-{c}-{TAG_IDS[TAG_MODES.index(m)]}" for f, c, m in TAG_CASES],
    group=lambda p: (p[0], p[1], p[2][0], p[2][1])))
def test_tags_edges(eng, oracle_lib, monkeypatch, family, crdt, mode, is_cold):
    """Families A (scan edges), C (removal-token batches) and D (ops over a
    chunk edge) through every tags shape, with SCT arrays and without."""
    D, style, knobs = mode
    tag_knobs(monkeypatch, knobs)
    (log, req, cap, names), want = built(oracle_lib, (family, crdt, D, style, is_cold), maybe_cold(
        lambda: tags_case(family, crdt, D, style), is_cold), style)
    got = eng.materialize_host(log, req, sparse=bool(style), cap_off=cap)
    check(crdt, D, got, want, style, names)


def guarded_run(eng, log, req, cap, style):
    """agn_materialize over device arrays whose out_tag / out_tok ranges were
    filled with a guard value."""
    total = max(int(cap[-1]), 1)
    with scratch(eng):
        dl, dr = eng.upload_log(log), eng.upload_read(req, sparse=bool(style))
        if style:
            eng.index_masks(dl)
        else:
            dl.struct.oc_mask = None
        dres = eng.alloc_result(req.n_req, log.n_dcs, sparse=bool(style), cap_off=cap)
        for name, dt, v in (("out_tag", np.uint32, edges.GUARD_TAG),
                            ("out_tok", np.uint64, edges.GUARD_TOK)):
            b = eng.upload(np.full(total, v, dt))
            dres.bufs[name].free()
            dres.bufs[name] = b
            setattr(dres.struct, name, b.ptr)
        eng.materialize(dl, dr, dres)
        eng.sync()
        return eng.fetch_result(dres)


def check_guarded(crdt, D, got, want, style, names, cap, over=()):
    """Every field against the oracle, out_n included; a request in `over`
    (more than 4096 live pairs, room given) carries the oracle's result plus
    AGN_F_ERR_CAPACITY and out_n = 0.  Outside the written states the output
    arrays still hold the guard: a request without room, one in `over` and
    the slack of the others wrote nothing."""
    n = len(names)
    check(crdt, D, got, want, style, names, skip=over)
    wtag = np.full(len(got.out_tag), edges.GUARD_TAG, np.uint32)
    wtok = np.full(len(got.out_tok), edges.GUARD_TOK, np.uint64)
    for i in range(n):
        wf = int(want.flags[i])
        if i in over:
            assert not wf & (CAPF | _abi.F_ERR_UNEXPECTED), names[i]
            assert int(got.flags[i]) == wf | CAPF, names[i]
            assert int(got.out_n[i]) == 0, names[i]
            for f in ("hole", "count", "err_pos"):
                assert int(getattr(got, f)[i]) == int(getattr(want, f)[i]), (names[i], f)
            assert np.array_equal(got.lastct[i], want.lastct[i]), names[i]
            if style:
                assert np.array_equal(got.lastct_mask[i], want.lastct_mask[i]), names[i]
            continue
        if wf & CAPF:   # room too small: as the oracle, the state's size reported
            assert int(got.out_n[i]) == int(want.out_n[i]) > int(cap[i + 1] - cap[i]), names[i]
        elif not wf & (_abi.F_ERR_UNEXPECTED | _abi.F_ERR_CORRUPTED):
            o, k = int(cap[i]), int(want.out_n[i])
            wtag[o:o + k], wtok[o:o + k] = want.out_tag[o:o + k], want.out_tok[o:o + k]
    for i in np.flatnonzero((got.out_tag != wtag) | (got.out_tok != wtok))[:1]:
        r = int(np.searchsorted(cap, i, side="right")) - 1
        raise AssertionError(f"output slot {i} (request {r}: {names[r]}) differs")


@pytest.mark.parametrize("mode,crdt,is_cold", with_cold(
    [(m, c) for c in TAGS for m in TAG_MODES], [f"{i}-{c}" for c in TAGS for i in TAG_IDS],
    group=lambda p: (p[1], p[0][0], p[0][1])))
def test_table_edges(eng, oracle_lib, monkeypatch, mode, crdt, is_cold):
    """Family B: live states on the limits of the 256- and 4096-slot tables,
    compacting churn, room one pair too small between guarded neighbours and
    more than 4096 live pairs (the engine's own limit)."""
    D, style, knobs = mode
    tag_knobs(monkeypatch, knobs)
    (log, req, cap, names, meta), want = built(oracle_lib, ("b", crdt, D, style, is_cold), maybe_cold(
        lambda: edges.family_b(crdt, D, style), is_cold), style)
    over = tuple(k for k, m in meta.items() if m.get("L", 0) > edges.SLOW_CAP)
    assert len(over) == 3 and sum("room" in m for m in meta.values()) == 4
    got = guarded_run(eng, log, req, cap, style)
    check_guarded(crdt, D, got, want, style, names, cap, over)


@pytest.mark.parametrize("D,style,crdt,is_cold", with_cold(
    [(D, st, c) for c in TAGS for D, st in [(5, None), (16, None), (8, "uniform")]],
    group=lambda p: p))
def test_table_overflow_batch(eng, oracle_lib, crdt, D, style, is_cold):
    """300 keys handed to the 4096-slot pass at once (its grid is 256 blocks)."""
    (log, req, cap, names), want = built(oracle_lib, ("b300", crdt, D, style, is_cold), maybe_cold(
        lambda: edges.family_b300(crdt, D, style), is_cold), style)
    got = guarded_run(eng, log, req, cap, style)
    check_guarded(crdt, D, got, want, style, names, cap)


# ------------------------------------------------------------------ family F
F_COUNTER = [(1, "all"), (1023, "all"), (1023, "first"), (1023, "last"), (1025, "all"),
             (1025, "first"), (1025, "last"), (2049, "all"), (2049, "first"), (2049, "last")]


@pytest.mark.parametrize("impl", ["default", "split", "split_two", "split_cold"])
@pytest.mark.parametrize("n_req,which", F_COUNTER)
def test_hand_on_lists_counter(eng, oracle_lib, monkeypatch, n_req, which, impl):
    """Masked D = 8 counters: the mixed keys k_counter_q8e hands on to the
    list pass k_counter_q8m, one, 1023, 1025 and 2049 of them and a lone one
    at either end of the batch."""
    if impl != "default":
        presence_knobs(monkeypatch, impl)
    crdt = _abi.COUNTER_PN
    is_cold = impl.endswith("cold")

    def build():
        case = edges.family_f_counter(n_req, which)
        return cold(case) if is_cold else case
    (log, req, _, names), want = built(oracle_lib, ("f", n_req, which, is_cold), build, "mixed")
    got = masked_device(eng, log, req, True)
    check(crdt, 8, got, want, "mixed", names)


@pytest.mark.parametrize("msk,crdt,is_cold", with_cold(
    [(m, c) for c in TAGS for m in ("1", "0")], group=lambda p: p[1]))
def test_hand_on_lists_tags(eng, oracle_lib, monkeypatch, msk, crdt, is_cold):
    """8200 masked keys, all mixed: more hand-ons than the list pass's 8192 blocks."""
    monkeypatch.setenv("AGN_TAGS_MSK", msk)
    (log, req, cap, names), want = built(oracle_lib, ("f", crdt, is_cold), maybe_cold(
        lambda: edges.family_f_tags(crdt), is_cold), "mixed")
    got = eng.materialize_host(log, req, sparse=True, cap_off=cap)
    check(crdt, 8, got, want, "mixed", names)


# ------------------------------------------------------------------ family E
def gc_built(oracle_lib, key, build):
    if _LAST.get("key") != key:
        _LAST.clear()
        case = build()
        log, prune, thr, tm, names = case
        _LAST.update(key=key, case=case, res=oracle_prune(oracle_lib, log, prune, thr, tm))
    return _LAST["case"], _LAST["res"]


GC_LOGS = {
    "counter8": lambda: edges.family_e(_abi.COUNTER_PN, 8),
    "counter3s": lambda: edges.family_e(_abi.COUNTER_PN, 3, True),
    "counter70s": lambda: edges.family_e(_abi.COUNTER_PN, 70, True),
    "set5": lambda: edges.family_e(_abi.SET_AW, 5),
    "set16s": lambda: edges.family_e(_abi.SET_AW, 16, True),
    "register8s": lambda: edges.family_e(_abi.REGISTER_MV, 8, True),
    "lww8": lambda: edges.family_e(_abi.REGISTER_LWW, 8),
    "ring_set5": lambda: edges.family_e_ring(_abi.SET_AW, 5),
    "ring_register16": lambda: edges.family_e_ring(_abi.REGISTER_MV, 16),
}
for _n in (1, 2, 3, 5, 7):
    GC_LOGS[f"small{_n}"] = (lambda n: lambda: edges.family_e_small(n))(_n)


def run_prune_ops(eng, log, prune, thr, tm, segmented):
    dlog = eng.upload_log(log)
    if log.oc_mask is None:
        dlog.struct.oc_mask = None
    dout = eng.alloc_log_like(log)
    K = log.n_keys
    kl = kid = None
    if segmented:
        kl, kid = eng.empty(8 * K), eng.empty(4 * K)
        dout.struct.key_len, dout.struct.key_id0 = kl.ptr, kid.ptr
    bp, bt = eng.upload(prune), eng.upload(thr)
    btm = eng.upload(tm) if tm is not None else None
    fl, tot = eng.empty(4 * K), eng.empty(16)
    eng.prune_ops(dlog, bp.ptr, bt.ptr, btm.ptr if btm else None, dout, fl.ptr, tot.ptr)
    eng.sync()
    got = {n: eng.download(dout.bufs[n], *dout.shapes[n]) for n in dout.shapes}
    return (got, eng.download(fl, np.uint32, (K,)), eng.download(tot, np.uint64, (2,)),
            eng.download(kl, np.uint64, (K,)) if kl else None,
            eng.download(kid, np.uint32, (K,)) if kid else None)


@pytest.mark.parametrize("name", list(GC_LOGS))
def test_gc_edges_csr(eng, oracle_lib, name):
    """agn_prune_ops, CSR form: every output array as the oracle's."""
    (log, prune, thr, tm, names), (want, wflags, n_out) = gc_built(oracle_lib, name, GC_LOGS[name])
    with scratch(eng):
        got, flags, totals, _, _ = run_prune_ops(eng, log, prune, thr, tm, False)
    assert int(totals[0]) == n_out
    bad = np.flatnonzero(flags != wflags)
    assert not len(bad), [names[k] for k in bad[:8]]
    assert np.array_equal(got["key_off"], want["key_off"])
    nr = int(want["rem_off"][n_out]) if log.rem_off is not None else 0
    if log.rem_off is not None:
        assert int(totals[1]) == nr
    for name_, g in got.items():
        w = want[name_]
        m = {"key_off": len(w), "rem_off": n_out + 1, "rem_tok": nr}.get(name_, n_out)
        if not np.array_equal(g[:m], w[:m]):
            e = int(np.flatnonzero((g[:m] != w[:m]).reshape(m, -1).any(axis=1))[0])
            k = int(np.searchsorted(want["key_off"], e, side="right")) - 1
            raise AssertionError(f"{name_}[{e}] differs" +
                                 (f" (key {names[k]})" if name_ != "rem_tok" else ""))


SEG_KNOBS = ["0", "1", "pf0", "pf1", "pf2", "pf3", "mw8"]


def check_segments(log, got, starts, lens, want, names):
    tags = log.rem_off is not None
    for k in range(log.n_keys):
        a, b = int(starts[k]), int(starts[k]) + int(lens[k])
        wa, wb = int(want["key_off"][k]), int(want["key_off"][k + 1])
        assert b - a == wb - wa, names[k]
        for f in ("oc", "oc_mask", "op_id", "txid", "eff", "tag", "add_tok"):
            if f in got:
                assert np.array_equal(got[f][a:b], want[f][wa:wb]), (names[k], f)
        if tags:
            ro, wro = got["rem_off"], want["rem_off"]
            for e, we in zip(range(a, b), range(wa, wb)):
                assert np.array_equal(got["rem_tok"][int(ro[e]):int(ro[e + 1])],
                                      want["rem_tok"][int(wro[we]):int(wro[we + 1])]), \
                    (names[k], e - a)


@pytest.mark.parametrize("ct", SEG_KNOBS)
@pytest.mark.parametrize("name", list(GC_LOGS))
def test_gc_edges_segmented(eng, oracle_lib, monkeypatch, name, ct):
    """agn_prune_ops with out.key_len, under the knobs of
    test_prune_segmented_gpu_vs_oracle."""
    from test_id_index import expected_index
    monkeypatch.setenv("AGN_PRUNE_CT", ct if ct in ("0", "1") else "0")
    if ct.startswith("pf"):
        monkeypatch.setenv("AGN_PRUNE_PF", ct[2:])
    else:
        monkeypatch.delenv("AGN_PRUNE_PF", raising=False)
    monkeypatch.setenv("AGN_PRUNE_MINW", ct[2:] if ct.startswith("mw") else "1")
    (log, prune, thr, tm, names), (want, wflags, n_out) = gc_built(oracle_lib, name, GC_LOGS[name])
    K = log.n_keys
    with scratch(eng):
        got, flags, totals, lens, kid = run_prune_ops(eng, log, prune, thr, tm, True)
    assert int(totals[0]) == n_out
    if log.rem_off is not None:
        assert int(totals[1]) == int(want["rem_off"][n_out])
    bad = np.flatnonzero(flags != wflags)
    assert not len(bad), [names[k] for k in bad[:8]]
    starts = got["key_off"][:K]
    assert np.array_equal(starts, log.key_off[:K])
    check_segments(log, got, starts, lens, want, names)
    assert np.array_equal(kid, expected_index(starts, lens, got["op_id"]))


def read_all(log):
    """One cold request per key that includes every op."""
    K, D, W = log.n_keys, log.n_dcs, n_words(log.n_dcs)
    full = edges.pack_mask(np.ones((K, D), bool))
    return EncodedRead(n_dcs=D, req_type=log.crdt_type, keys=np.arange(K, dtype=np.uint64),
                       R=np.full((K, D), 1 << 40, np.uint64), R_mask=full,
                       sct=np.zeros((K, D), np.uint64), sct_mask=np.zeros((K, W), np.uint64),
                       sct_ignore=np.ones(K, np.uint8), txid=np.zeros(K, np.uint64),
                       base_value=np.zeros(K, np.int64), base_off=np.zeros(K + 1, np.uint64),
                       base_tag=np.zeros(0, np.uint32), base_tok=np.zeros(0, np.uint64))


ANCHORS = {"tail": {}, "tail4": {"AGN_PRUNE_WPB": "4"}, "tailq2": {"AGN_PRUNE_TAIL_KPW": "2"},
           "tailq4": {"AGN_PRUNE_TAIL_KPW": "4"}, "front": {"AGN_PRUNE_TAIL": "0"},
           "front4": {"AGN_PRUNE_TAIL": "0", "AGN_PRUNE_WPB": "4"}}


@pytest.mark.parametrize("anchor", list(ANCHORS))
@pytest.mark.parametrize("name", list(GC_LOGS))
def test_gc_edges_oplog(eng, oracle_lib, monkeypatch, name, anchor):
    """agn_oplog_prune in place (tail form, start-anchored form, 2 / 4 counter
    keys per wave, 4 waves per block): every key's segment as the oracle's
    output, then the pruned view materialized against the oracle."""
    env = {"AGN_PRUNE_TAIL": "1", "AGN_PRUNE_WPB": "1", "AGN_PRUNE_TAIL_MINW": "8",
           "AGN_PRUNE_TAIL_KPW": "1", **ANCHORS[anchor]}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    (log0, prune, thr, tm, names), _ = gc_built(oracle_lib, name, GC_LOGS[name])
    crdt, D, K = log0.crdt_type, log0.n_dcs, log0.n_keys
    sparse, tags = log0.oc_mask is not None, log0.crdt_type != _abi.COUNTER_PN
    rng = np.random.default_rng(5)
    with scratch(eng), OpLog(eng, crdt, D, K, sparse=sparse, init_slots=2) as ol:
        ids = tol.append_ops(ol, log0, tol.interleave(rng, tol.ops_of(log0)), rng, max_batch=400)
        log = tol.renumbered(log0, ids)
        want, wflags, n_out = oracle_prune(oracle_lib, log, prune, thr, tm)
        bp, bt = eng.upload(prune), eng.upload(thr)
        btm = eng.upload(tm) if tm is not None else None
        fl = eng.empty(4 * K)
        ol.prune(bp.ptr, bt.ptr, btm.ptr if btm else None, fl.ptr)
        flags = eng.download(fl, np.uint32, (K,))
        bad = np.flatnonzero(flags != wflags)
        assert not len(bad), [names[k] for k in bad[:8]]
        assert ol.stats()["entries"] == n_out
        view = ol.flush()
        tol.check_id_index(eng, view, K)
        segs = tol.segments(eng, view, K, D, n_words(D), tags, sparse)
        for k in range(K):
            for f, v in tol.csr_key(want, k, tags).items():
                g = segs[k][f]
                same = g == v if f == "rems" else np.array_equal(np.asarray(g), np.asarray(v))
                assert same, (names[k], f)
        pruned = tol.pruned_log(want, n_out, crdt, D, K, sparse)
        bad = tol.materialize_view(eng, oracle_lib, view, pruned, read_all(pruned), sparse)
        assert not bad, explain(bad, names)
        # and without SCT arrays (every type's cold form, register_lww's included)
        bad = tol.materialize_view(eng, oracle_lib, view, pruned, synth.cold(read_all(pruned)),
                                   sparse)
        assert not bad, ("cold", explain(bad, names))
