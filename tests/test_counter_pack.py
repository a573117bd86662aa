"""The packed op-log index (agn_log_index_pack) and the packed form of
k_counter_quad2 on the GPU, on the cases of tests/pack_cases.py
(tests/test_counter_pack_cpu.py holds the conditions on those inputs):

  1. the builder against the numpy reference, exact;
  2. cold dense reads with the index registered against the C oracle, bit for
     bit, under all four AGN_Q2_EFF / AGN_Q2_STORE combinations;
  3. the path, by poison: with oc overwritten for the keys only packed pairs
     read the results still match, and with pack_rows overwritten they match
     under AGN_Q2_PACK=0;
  4. warm and masked reads of the registered log ignore the index;
  5. dropping the registration returns the log to oc."""
import dataclasses

import numpy as np
import pytest

import pack_cases as pc
from antidote_amd import _abi
from domain import CLOCK_MODES, domain_case, run_oracle, std_case
from synth import compare
from test_edges import scratch

pytestmark = pytest.mark.gpu

_WANT = {}


def want_of(oracle_lib, name):
    """(log, req, names, oracle result) of a case, computed once."""
    if name not in _WANT:
        log, req, names = pc.case(name)
        _WANT[name] = (log, req, names, run_oracle(oracle_lib, log, req, sparse=False))
    return _WANT[name]


def quad2(monkeypatch):
    monkeypatch.delenv("AGN_COUNTER_GLDS", raising=False)
    monkeypatch.delenv("AGN_COUNTER_IMPL", raising=False)
    monkeypatch.delenv("AGN_Q2_PACK", raising=False)
    monkeypatch.setenv("AGN_COUNTER_VARIANT", "3")   # k_counter_quad2


def put(eng, buf, arr):
    arr = np.ascontiguousarray(arr)
    eng.lib.agn_memcpy_h2d(eng.ctx, buf.ptr, arr.ctypes.data, arr.nbytes, None)
    eng.sync()


def read(eng, dl, req, sparse=False):
    dr = eng.upload_read(req, sparse=sparse)
    dres = eng.alloc_result(req.n_req, pc.D, sparse=sparse)
    eng.materialize(dl, dr, dres)
    return eng.fetch_result(dres)


def check(got, want, req, names, what, sparse=False):
    bad = compare(_abi.COUNTER_PN, pc.D, got, want, sparse, req.n_req)
    assert not bad, (what, [(names[b[0]],) + tuple(b[1:]) for b in bad[:8]])


def builder_logs():
    logs = {n: (lambda n=n: pc.case(n)[0]) for n in pc.CASES}
    for i, mode in enumerate(CLOCK_MODES + ("mixed",)):
        logs["domain:" + mode] = lambda i=i, mode=mode: domain_case(
            i, std_case(4100 + i, _abi.COUNTER_PN, pc.D, False), clock=mode, sparse=False)[0]
    return logs


BUILDER = builder_logs()


@pytest.mark.parametrize("name", sorted(BUILDER))
def test_builder_vs_numpy(eng, name):
    log = BUILDER[name]()
    base, ok, rows = pc.pack_reference(log)
    K, E = log.n_keys, log.n_entries
    with scratch(eng):
        dl = eng.upload_log(log)
        b_rows, b_base, b_ok, n_un = eng.index_pack(dl)
        g_ok = eng.download(b_ok, np.uint8, (K,))
        g_base = eng.download(b_base, np.uint64, (K, pc.D))
        g_rows = eng.download(b_rows, np.uint32, (E, pc.D))
        eng.drop_pack(dl)
    assert np.array_equal(g_ok, ok)
    assert n_un == int((ok == 0).sum())
    assert np.array_equal(g_base[ok == 1], base[ok == 1])
    packed = ok[pc.key_of_entry(log)] == 1
    assert np.array_equal(g_rows[packed], rows[packed])


@pytest.mark.parametrize("name", pc.CASES)
def test_packed_read_vs_oracle(eng, oracle_lib, monkeypatch, name):
    log, req, names, want = want_of(oracle_lib, name)
    quad2(monkeypatch)
    with scratch(eng):
        dl = eng.upload_log(log)
        eng.index_pack(dl)
        for e, s in pc.KNOBS:
            monkeypatch.setenv("AGN_Q2_EFF", e)
            monkeypatch.setenv("AGN_Q2_STORE", s)
            check(read(eng, dl, req), want, req, names, f"AGN_Q2_EFF={e} AGN_Q2_STORE={s}")
        eng.drop_pack(dl)


@pytest.mark.parametrize("name", pc.CASES)
def test_path_by_poison(eng, oracle_lib, monkeypatch, name):
    log, req, names, want = want_of(oracle_lib, name)
    plog, only = pc.poison_oc(log, req)
    quad2(monkeypatch)
    with scratch(eng):
        dl = eng.upload_log(log)
        rows, _, _, _ = eng.index_pack(dl)
        put(eng, dl.bufs["oc"], plog.oc)                 # the packed pairs' keys: all ones
        check(read(eng, dl, req), want, req, names, "oc poisoned")
        if (pc.served_packed(log, req) & (want.count > 0)).any():
            # and the poison has teeth: without the index the results differ
            monkeypatch.setenv("AGN_Q2_PACK", "0")
            got = read(eng, dl, req)
            assert compare(_abi.COUNTER_PN, pc.D, got, want, False, req.n_req)
            monkeypatch.delenv("AGN_Q2_PACK")
        put(eng, dl.bufs["oc"], log.oc)
        eng.lib.agn_memset_d(eng.ctx, rows.ptr, 0xFF, rows.nbytes, None)
        monkeypatch.setenv("AGN_Q2_PACK", "0")
        check(read(eng, dl, req), want, req, names, "rows poisoned, AGN_Q2_PACK=0")
        eng.drop_pack(dl)


def warm_of(log, req):
    """The same reads against a base snapshot: SCT = the key's row a quarter in."""
    oc = np.asarray(log.oc, np.uint64).reshape(-1, pc.D)
    sct = np.zeros((req.n_req, pc.D), np.uint64)
    for i, k in enumerate(req.keys.astype(np.int64)):
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        if b > a:
            sct[i] = oc[a + (b - a) // 4]
    return dataclasses.replace(req, sct=sct, sct_mask=np.zeros((req.n_req, 1), np.uint64),
                               sct_ignore=(np.arange(req.n_req) % 5 == 4).astype(np.uint8))


@pytest.mark.parametrize("name", pc.OWN)
def test_index_ignored_warm_and_masked(eng, oracle_lib, monkeypatch, name):
    log, req, names = pc.case(name)
    quad2(monkeypatch)
    wreq = warm_of(log, req)
    mreq = dataclasses.replace(req, R_mask=np.full((req.n_req, 1), 0xFF, np.uint64))
    with scratch(eng):
        dl = eng.upload_log(log)
        rows, _, _, _ = eng.index_pack(dl)
        eng.lib.agn_memset_d(eng.ctx, rows.ptr, 0xFF, rows.nbytes, None)
        check(read(eng, dl, wreq), run_oracle(oracle_lib, log, wreq, sparse=False), wreq, names,
              "warm")
        check(read(eng, dl, mreq, sparse=True), run_oracle(oracle_lib, log, mreq, sparse=True),
              mreq, names, "masked", sparse=True)
        eng.drop_pack(dl)


@pytest.mark.parametrize("name", pc.OWN[:2])
def test_drop_returns_to_oc(eng, oracle_lib, monkeypatch, name):
    log, req, names, want = want_of(oracle_lib, name)
    quad2(monkeypatch)
    with scratch(eng):
        dl = eng.upload_log(log)
        rows, _, _, _ = eng.index_pack(dl)
        eng.lib.agn_memset_d(eng.ctx, rows.ptr, 0xFF, rows.nbytes, None)
        eng.drop_pack(dl)
        check(read(eng, dl, req), want, req, names, "registration dropped")


def test_index_pack_arguments(eng):
    log, _, _ = pc.case("edges")
    with scratch(eng):
        dl = eng.upload_log(log)
        bufs = [eng.empty(log.n_entries * 32), eng.empty(log.n_keys * 64), eng.empty(64)]
        call = lambda ls, r, b, o: eng.lib.agn_log_index_pack(  # noqa: E731
            eng.ctx, ls, r and r.ptr, b and b.ptr, o and o.ptr, None, None)
        import ctypes as C
        for field, value in (("n_dcs", 7), ("crdt_type", _abi.SET_AW), ("oc_mask", bufs[1].ptr)):
            ls = _abi.AgnLog.from_buffer_copy(dl.struct)
            setattr(ls, field, value)
            assert call(C.byref(ls), *bufs) == _abi.ENOTSUP, field
        assert call(C.byref(dl.struct), bufs[0], None, bufs[2]) == _abi.EINVAL
        assert call(C.byref(dl.struct), bufs[0], bufs[1], None) == _abi.EINVAL
        ls = _abi.AgnLog.from_buffer_copy(dl.struct)
        ls.oc = None
        assert call(C.byref(ls), *bufs) == _abi.EINVAL
        assert call(None, *bufs) == _abi.EINVAL
        assert call(C.byref(dl.struct), None, None, None) == _abi.OK   # nothing registered: a no-op
