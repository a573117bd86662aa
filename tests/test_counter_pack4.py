"""k_counter_pack4 on the GPU: the packed cold read of a whole partition
(req.keys == NULL), four requests per wave, on the cases of
tests/pack4_cases.py (tests/test_counter_pack4_cpu.py holds the conditions on
those inputs):

  1. every request bit-identical to the C oracle with AGN_Q2_FOUR unset, =1
     and =0;
  2. the path, by poison: with oc overwritten for the keys of fully served
     groups the results still match, and differ under AGN_Q2_FOUR=0
     AGN_Q2_PACK=0; with pack_rows overwritten the groups the fallback serves
     still match;
  3. a keyed batch over the same log (keys = arange) equals the identity batch."""
import numpy as np
import pytest

import pack4_cases as p4
import pack_cases as pc
from antidote_amd import _abi
from synth import compare
from test_edges import scratch

pytestmark = pytest.mark.gpu

_WANT = {}


def want_of(oracle_lib, name):
    if name not in _WANT:
        c = p4.case(name)
        _WANT[name] = (c, p4.run_oracle(oracle_lib, c))
    return _WANT[name]


def knobs(monkeypatch, **kv):
    for k in ("AGN_COUNTER_GLDS", "AGN_COUNTER_IMPL", "AGN_COUNTER_VARIANT", "AGN_Q2_EFF",
              "AGN_Q2_STORE", "AGN_Q2_PACK", "AGN_Q2_FOUR", "AGN_XCD_REMAP", "AGN_XCD_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def put(eng, buf, arr):
    arr = np.ascontiguousarray(arr)
    eng.lib.agn_memcpy_h2d(eng.ctx, buf.ptr, arr.ctypes.data, arr.nbytes, None)
    eng.sync()


def device_log(eng, c):
    """The case's log on the device with its packed index registered."""
    dl = eng.upload_log(c.log)
    if c.key_len is not None:
        dl.bufs["key_len"] = eng.upload(c.key_len)
        dl.struct.key_len = dl.bufs["key_len"].ptr
    if c.index_ids:
        eng.index_ids(dl)
    rows, _, _, _ = eng.index_pack(dl)
    return dl, rows


def read(eng, dl, c, identity=True):
    dr = eng.upload_read(c.req, sparse=False)
    if identity:
        dr.struct.keys = None          # the identity key map: request i reads key i
    dres = eng.alloc_result(c.req.n_req, pc.D, sparse=False)
    eng.materialize(dl, dr, dres)
    return eng.fetch_result(dres)


def bad_requests(got, want, n):
    return sorted({b[0] for b in compare(_abi.COUNTER_PN, pc.D, got, want, False, n)})


def check(got, want, c, what, only=None):
    bad = compare(_abi.COUNTER_PN, pc.D, got, want, False, c.req.n_req)
    if only is not None:
        bad = [b for b in bad if only[b[0]]]
    assert not bad, (what, [(c.names[b[0]],) + tuple(b[1:]) for b in bad[:8]])


@pytest.mark.parametrize("name", p4.CASES)
def test_identity_read_vs_oracle(eng, oracle_lib, monkeypatch, name):
    c, want = want_of(oracle_lib, name)
    with scratch(eng):
        dl, _ = device_log(eng, c)
        for four in (None, "1", "0"):
            knobs(monkeypatch, **({} if four is None else {"AGN_Q2_FOUR": four}))
            check(read(eng, dl, c), want, c, f"AGN_Q2_FOUR={four}")
        eng.drop_pack(dl)


@pytest.mark.parametrize("name", p4.CASES)
def test_path_by_poison(eng, oracle_lib, monkeypatch, name):
    c, want = want_of(oracle_lib, name)
    served = p4.served4(c)
    with scratch(eng):
        dl, rows = device_log(eng, c)
        knobs(monkeypatch, AGN_Q2_FOUR="1")
        put(eng, dl.bufs["oc"], p4.poison_oc(c).oc)      # the served groups' keys: all ones
        check(read(eng, dl, c), want, c, "oc poisoned")
        live = served & (want.count > 0)
        if live.any():
            # the poison has teeth: read from oc, exactly the served requests with an op differ
            knobs(monkeypatch, AGN_Q2_FOUR="0", AGN_Q2_PACK="0")
            got = read(eng, dl, c)
            assert set(np.flatnonzero(live)) <= set(bad_requests(got, want, c.req.n_req))
            check(got, want, c, "oc poisoned, no index: the fallback's groups", only=~served)
        put(eng, dl.bufs["oc"], c.log.oc)
        eng.lib.agn_memset_d(eng.ctx, rows.ptr, 0xFF, rows.nbytes, None)
        knobs(monkeypatch, AGN_Q2_FOUR="1")
        check(read(eng, dl, c), want, c, "rows poisoned: the fallback's groups", only=~served)
        eng.drop_pack(dl)


@pytest.mark.parametrize("name", ("n9", "long", "corrupt", "thr_eq", "segmented"))
def test_keyed_batch_equals_identity(eng, oracle_lib, monkeypatch, name):
    c, want = want_of(oracle_lib, name)
    with scratch(eng):
        dl, _ = device_log(eng, c)
        knobs(monkeypatch)
        ident, keyed = read(eng, dl, c), read(eng, dl, c, identity=False)
        eng.drop_pack(dl)
    check(keyed, want, c, "keys = arange")
    check(ident, want, c, "identity")
    assert np.array_equal(ident.flags, keyed.flags) and np.array_equal(ident.err_pos, keyed.err_pos)
    live = ident.flags != _abi.F_ERR_CORRUPTED       # a corrupt request writes flags and err_pos only
    for f in pc.FIELDS:
        assert np.array_equal(getattr(ident, f)[live], getattr(keyed, f)[live]), f
