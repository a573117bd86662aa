"""k_counter_pack8 and the narrow tier of the packed index on the GPU
(agn_log_index_pack16): the cold read of a whole partition (req.keys == NULL),
eight requests per wave over u16 rows, on the cases of tests/pack8_cases.py
(tests/test_counter_pack8_cpu.py holds the conditions on those inputs):

  1. every request bit-identical to the C oracle with AGN_Q2_NARROW unset, =1
     and =0;
  2. the path, by poison: with oc and the u32 rows overwritten the served
     groups still match; with rows16 overwritten they differ, match again under
     AGN_Q2_NARROW=0, and the groups the fallback serves never notice;
  3. the index: narrow, n_wide and rows16 against numpy, the refusals, the
     drops (rows16 = NULL, agn_dev_free of rows16) and the launcher's bound on
     the log's wide keys.

AGN_Q2_NARROW=1 takes the kernel whatever the log's count of wide keys (unset,
a log of fewer than 1024 keys with one wide key keeps k_counter_pack4), which
is how the small logs here reach its fallback."""
import ctypes as C

import numpy as np
import pytest

import pack8_cases as p8
import pack_cases as pc
from antidote_amd import _abi
from synth import compare
from test_edges import scratch

pytestmark = pytest.mark.gpu

_WANT = {}


def want_of(oracle_lib, name):
    if name not in _WANT:
        c = p8.case(name)
        _WANT[name] = (c, p8.run_oracle(oracle_lib, c))
    return _WANT[name]


def knobs(monkeypatch, **kv):
    for k in ("AGN_COUNTER_GLDS", "AGN_COUNTER_IMPL", "AGN_COUNTER_VARIANT", "AGN_Q2_EFF",
              "AGN_Q2_STORE", "AGN_Q2_PACK", "AGN_Q2_FOUR", "AGN_Q2_NARROW", "AGN_XCD_REMAP",
              "AGN_XCD_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def put(eng, buf, arr):
    arr = np.ascontiguousarray(arr)
    eng.lib.agn_memcpy_h2d(eng.ctx, buf.ptr, arr.ctypes.data, arr.nbytes, None)
    eng.sync()


def fill(eng, buf, byte=0xFF):
    eng.lib.agn_memset_d(eng.ctx, buf.ptr, byte, buf.nbytes, None)
    eng.sync()


def device_log(eng, c):
    """The case's log on the device with both tiers registered: (dl, rows, rows16)."""
    dl = eng.upload_log(c.log)
    if c.key_len is not None:
        dl.bufs["key_len"] = eng.upload(c.key_len)
        dl.struct.key_len = dl.bufs["key_len"].ptr
    if c.index_ids:
        eng.index_ids(dl)
    rows, _, _, _ = eng.index_pack(dl)
    rows16, _, _ = eng.index_pack16(dl)
    return dl, rows, rows16


def read(eng, dl, c):
    dr = eng.upload_read(c.req, sparse=False)
    dr.struct.keys = None              # the identity key map: request i reads key i
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


@pytest.mark.parametrize("name", p8.CASES)
def test_identity_read_vs_oracle(eng, oracle_lib, monkeypatch, name):
    c, want = want_of(oracle_lib, name)
    with scratch(eng):
        dl, _, _ = device_log(eng, c)
        for nar in (None, "1", "0"):
            knobs(monkeypatch, **({} if nar is None else {"AGN_Q2_NARROW": nar}))
            check(read(eng, dl, c), want, c, f"AGN_Q2_NARROW={nar}")
        eng.drop_pack(dl)


@pytest.mark.parametrize("name", p8.CASES)
def test_path_by_poison(eng, oracle_lib, monkeypatch, name):
    c, want = want_of(oracle_lib, name)
    served = p8.served8(c)
    live = served & (want.count > 0)
    with scratch(eng):
        dl, rows, rows16 = device_log(eng, c)
        # oc (the served groups' keys) and every u32 row overwritten: rows16 serves
        put(eng, dl.bufs["oc"], p8.poison_oc(c).oc)
        fill(eng, rows)
        knobs(monkeypatch, AGN_Q2_NARROW="1")
        check(read(eng, dl, c), want, c, "oc and rows poisoned")
        put(eng, dl.bufs["oc"], c.log.oc)
        eng.index_pack(dl)                 # the u32 rows again (drops the narrow tier) ...
        rows16, _, _ = eng.index_pack16(dl)
        fill(eng, rows16)                  # ... and rows16 overwritten
        for nar in (None, "1"):
            wide_log = not p8.narrow_of(c).all()
            if nar is None and wide_log:
                continue                   # a small log with a wide key: unset, k_counter_pack4 (the bound)
            knobs(monkeypatch, **({} if nar is None else {"AGN_Q2_NARROW": nar}))
            got = read(eng, dl, c)
            check(got, want, c, "rows16 poisoned: the fallback's groups", only=~served)
            # the poison has teeth: every served request with an op differs
            assert set(np.flatnonzero(live)) <= set(bad_requests(got, want, c.req.n_req)), nar
        knobs(monkeypatch, AGN_Q2_NARROW="0")
        check(read(eng, dl, c), want, c, "rows16 poisoned, AGN_Q2_NARROW=0")
        eng.drop_pack(dl)


def test_index_vs_numpy(eng):
    c = p8.mixed_index_case()
    nar, rows = p8.rows16_reference(c)
    K, E = c.log.n_keys, c.log.n_entries
    assert set(p8.unservable(c)) == {"", "wide", "unpacked", "long"} and 0 in p8.lens_of(c)
    with scratch(eng):
        dl = eng.upload_log(c.log)
        eng.index_pack(dl)
        b_rows16, b_nar, n_wide = eng.index_pack16(dl)
        g_nar = eng.download(b_nar, np.uint8, (K,))
        g_rows = eng.download(b_rows16, np.uint16, (E, pc.D))
        eng.drop_pack(dl)
    assert np.array_equal(g_nar, nar)
    assert n_wide == int((nar == 0).sum()) and 0 < n_wide < K
    keep = nar[pc.key_of_entry(c.log)] == 1
    assert keep.any() and np.array_equal(g_rows[keep], rows[keep])


def test_index_pack16_arguments(eng):
    c = p8.case("n9")
    with scratch(eng):
        dl = eng.upload_log(c.log)
        r16, nar = eng.empty(c.log.n_entries * 16 + 16), eng.empty(16 + 8)
        call = lambda ls, r, n: eng.lib.agn_log_index_pack16(eng.ctx, ls, r, n, None, None)  # noqa: E731
        ls = C.byref(dl.struct)
        assert call(ls, r16.ptr, nar.ptr) == _abi.EINVAL          # no u32 index registered
        assert call(ls, None, None) == _abi.OK                    # nothing registered: a no-op
        eng.index_pack(dl)
        assert call(ls, r16.ptr, None) == _abi.EINVAL
        assert call(ls, r16.ptr + 8, nar.ptr) == _abi.EINVAL      # rows16: 16-byte units
        assert call(ls, r16.ptr, nar.ptr + 2) == _abi.EINVAL      # narrow: aligned dwords
        assert call(None, r16.ptr, nar.ptr) == _abi.EINVAL
        for field, value in (("n_dcs", 7), ("crdt_type", _abi.SET_AW), ("oc_mask", r16.ptr)):
            bad = _abi.AgnLog.from_buffer_copy(dl.struct)
            setattr(bad, field, value)
            assert call(C.byref(bad), r16.ptr, nar.ptr) == _abi.ENOTSUP, field
        n = C.c_uint64(99)
        assert eng.lib.agn_log_index_pack16(eng.ctx, ls, r16.ptr, nar.ptr, C.byref(n), None) == _abi.OK
        assert n.value == 0
        eng.drop_pack(dl)
        assert call(ls, r16.ptr, nar.ptr) == _abi.EINVAL          # dropped with the u32 index


@pytest.mark.parametrize("how", ("null", "dev_free"))
def test_drop_returns_to_the_u32_rows(eng, oracle_lib, monkeypatch, how):
    c, want = want_of(oracle_lib, "n17")
    served = p8.served8(c)
    knobs(monkeypatch)
    with scratch(eng):
        dl, rows, rows16 = device_log(eng, c)
        fill(eng, rows16)
        got = read(eng, dl, c)             # the narrow tier is in use
        assert set(np.flatnonzero(served & (want.count > 0))) <= set(bad_requests(got, want, c.req.n_req))
        if how == "null":
            eng.drop_pack16(dl)
        else:
            rows16.free()
        put(eng, dl.bufs["oc"], p8.poison_oc(c).oc)       # neither oc nor rows16: the u32 rows
        check(read(eng, dl, c), want, c, f"narrow tier dropped ({how})")
        eng.drop_pack(dl)


def test_wide_bound_keeps_the_u32_launch(eng, oracle_lib, monkeypatch):
    """One wide key: at 1024 keys the bound n_wide * 1024 <= n_keys holds and the
    read scans rows16; at 1016 keys it does not, and rows16 is never read."""
    knobs(monkeypatch)
    for n_keys, narrow_launch in ((1024, True), (1016, False)):
        c = p8.bound_case(n_keys)
        want = p8.run_oracle(oracle_lib, c)
        served = p8.served8(c)
        assert not served[:8].any() and served[8:n_keys // 8 * 8].all()
        with scratch(eng):
            dl, _, rows16 = device_log(eng, c)
            check(read(eng, dl, c), want, c, f"{n_keys} keys")
            fill(eng, rows16)
            got = read(eng, dl, c)
            eng.drop_pack(dl)
        if narrow_launch:
            check(got, want, c, "rows16 poisoned: the wide key's group", only=~served)
            assert set(np.flatnonzero(served & (want.count > 0))) <= set(bad_requests(got, want, n_keys))
        else:
            check(got, want, c, "rows16 poisoned, more than one key in 1024 wide")
