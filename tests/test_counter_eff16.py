"""k_counter_pack8<true> and the effect tier of the packed index on the GPU
(agn_log_index_eff16): the cold read of a whole partition, eight requests per
wave over u16 rows with the i16 effects loaded beside them, on the cases of
tests/eff16_cases.py (tests/test_counter_eff16_cpu.py holds the conditions on
those inputs):

  1. every request of every pack8_cases case, of the effect-edge logs (8, 16
     and 17 keys) and of a log whose id index lacks a base for two served keys
     bit-identical to the C oracle with AGN_Q2_EFF16 unset, =1 and =0 -- and,
     since the oracle's value is not compared under an error flag, `value`
     equal to numpy's sum of the included valid effects, and every field a
     request defines under =1 equal to round 11's kernel's under =0;
  2. the path, by poison: with `eff` overwritten at every non-escaped entry of
     the served groups they still match (the fast path does not read it); with
     eff16 overwritten they differ, match again under AGN_Q2_EFF16=0, and the
     groups the fallback serves never notice;
  3. the index: eff16 and n_escaped against numpy, the refusals, the drops
     (eff16 = NULL, agn_dev_free of eff16 or of the recorded eff array,
     agn_log_index_pack16 again), a log struct whose eff is another array, and
     the launcher's bound on the log's escaped entries.

AGN_Q2_EFF16=1 takes the tier whatever the log's count of escapes, and
AGN_Q2_NARROW=1 the narrow kernel whatever its count of wide keys: the small
logs here reach the kernel this way."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import eff16_cases as e16
import pack8_cases as p8
import pack_cases as pc
from antidote_amd import _abi
from test_counter_pack8 import bad_requests, check, fill, put, read
from test_edges import scratch

pytestmark = pytest.mark.gpu

_WANT = {}
FORCE = {"AGN_Q2_NARROW": "1", "AGN_Q2_EFF16": "1"}


def want_of(oracle_lib, name):
    if name not in _WANT:
        c = e16.case(name)
        _WANT[name] = (c, e16.run_oracle(oracle_lib, c))
    return _WANT[name]


def knobs(monkeypatch, **kv):
    for k in ("AGN_COUNTER_GLDS", "AGN_COUNTER_IMPL", "AGN_COUNTER_VARIANT", "AGN_Q2_EFF",
              "AGN_Q2_STORE", "AGN_Q2_PACK", "AGN_Q2_FOUR", "AGN_Q2_NARROW", "AGN_Q2_EFF16",
              "AGN_XCD_REMAP", "AGN_XCD_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def device_log(eng, c):
    """The case's log on the device with all three tiers registered: (dl, eff16)."""
    dl = eng.upload_log(c.log)
    if c.key_len is not None:
        dl.bufs["key_len"] = eng.upload(c.key_len)
        dl.struct.key_len = dl.bufs["key_len"].ptr
    if c.index_ids:
        eng.index_ids(dl)
    eng.index_pack(dl)
    eng.index_pack16(dl)
    eff16, n_esc = eng.index_eff16(dl)
    assert n_esc == e16.eff16_reference(c.log.eff)[1]
    return dl, eff16


def live_of(c, want):
    return e16.served8(c) & (want.count > 0)


ALL_CASES = p8.CASES + e16.EDGE_CASES + e16.ID_CASES


@pytest.mark.parametrize("name", ALL_CASES)
def test_identity_read_vs_oracle(eng, oracle_lib, monkeypatch, name):
    c, want = want_of(oracle_lib, name)
    outs = {}
    with scratch(eng):
        dl, _ = device_log(eng, c)
        for x in (None, "1", "0"):
            knobs(monkeypatch, **({} if x is None else {"AGN_Q2_EFF16": x}))
            outs[x] = read(eng, dl, c)
            check(outs[x], want, c, f"AGN_Q2_EFF16={x}")
        for x in ("1", "0"):               # and in the narrow kernel whatever the log's wide keys
            knobs(monkeypatch, AGN_Q2_NARROW="1", AGN_Q2_EFF16=x)
            outs["n" + x] = read(eng, dl, c)
            check(outs["n" + x], want, c, f"AGN_Q2_NARROW=1 AGN_Q2_EFF16={x}")
        eng.drop_pack(dl)
    # Under AGN_F_ERR_UNEXPECTED the oracle's value is not compared: the
    # invalid op is skipped and the rest are summed, from numpy.  A corrupt
    # key's request defines flags and err_pos only (checked above); its other
    # fields are whatever the result buffers held.
    defined = (want.flags & _abi.F_ERR_CORRUPTED) == 0
    value = e16.expected_value(c)
    for x, got in outs.items():
        assert np.array_equal(got.value[defined], value[defined]), f"value, {x}"
    for f in pc.FIELDS:                    # and every defined field as round 11's kernel stores it
        assert np.array_equal(getattr(outs["n1"], f)[defined], getattr(outs["n0"], f)[defined]), f
        assert np.array_equal(getattr(outs["1"], f)[defined], getattr(outs["0"], f)[defined]), f


@pytest.mark.parametrize("name", e16.POISON_CASES)
def test_path_by_poison(eng, oracle_lib, monkeypatch, name):
    c, want = want_of(oracle_lib, name)
    served, live = e16.served8(c), live_of(c, want)
    with scratch(eng):
        dl, eff16 = device_log(eng, c)
        # (a) eff invalid wherever the tier does not escape: eff16 serves
        put(eng, dl.bufs["eff"], e16.poison_eff(c).eff)
        knobs(monkeypatch, **FORCE)
        check(read(eng, dl, c), want, c, "eff poisoned")
        # (b) eff again, eff16 overwritten with 0x7F7F: no escape, every effect 32 639
        put(eng, dl.bufs["eff"], c.log.eff)
        fill(eng, eff16, 0x7F)
        got = read(eng, dl, c)
        check(got, want, c, "eff16 poisoned: the fallback's groups", only=~served)
        assert live.any() and set(np.flatnonzero(live)) <= set(bad_requests(got, want, c.req.n_req))
        knobs(monkeypatch, AGN_Q2_NARROW="1", AGN_Q2_EFF16="0")
        check(read(eng, dl, c), want, c, "eff16 poisoned, AGN_Q2_EFF16=0")
        eng.drop_pack(dl)


@pytest.mark.parametrize("which", ("edges17", "bound_short"))
def test_index_vs_numpy(eng, which):
    c = e16.case("edges17") if which == "edges17" else e16.bound_case(True)
    ref, n_ref = e16.eff16_reference(c.log.eff)
    E = c.log.n_entries
    assert E % 8 != 0                      # the builder's last entries, short of a 16-byte unit
    with scratch(eng):
        dl = eng.upload_log(c.log)
        eng.index_pack(dl)
        eng.index_pack16(dl)
        buf, n_esc = eng.index_eff16(dl)
        got = eng.download(buf, np.int16, (E,))
        eng.drop_pack(dl)
    assert np.array_equal(got, ref) and n_esc == n_ref


def test_index_eff16_arguments(eng):
    c = e16.case("edges8")
    with scratch(eng):
        dl = eng.upload_log(c.log)
        buf = eng.empty(c.log.n_entries * 2 + 32)
        call = lambda ls, p: eng.lib.agn_log_index_eff16(eng.ctx, ls, p, None, None)  # noqa: E731
        ls = C.byref(dl.struct)
        assert call(ls, None) == _abi.OK                          # nothing registered: a no-op
        assert call(ls, buf.ptr) == _abi.EINVAL                   # no index at all
        eng.index_pack(dl)
        assert call(ls, buf.ptr) == _abi.EINVAL                   # the u32 index, no narrow tier
        eng.index_pack16(dl)
        assert call(ls, buf.ptr + 8) == _abi.EINVAL               # eff16: 16-byte units
        assert call(ls, buf.ptr + 2) == _abi.EINVAL
        assert call(None, buf.ptr) == _abi.EINVAL
        bad = _abi.AgnLog.from_buffer_copy(dl.struct)
        bad.eff = None
        assert call(C.byref(bad), buf.ptr) == _abi.EINVAL         # eff == NULL
        for field, value in (("n_dcs", 7), ("crdt_type", _abi.SET_AW), ("oc_mask", buf.ptr)):
            bad = _abi.AgnLog.from_buffer_copy(dl.struct)
            setattr(bad, field, value)
            assert call(C.byref(bad), buf.ptr) == _abi.ENOTSUP, field
        n = C.c_uint64(0)
        assert eng.lib.agn_log_index_eff16(eng.ctx, ls, buf.ptr, C.byref(n), None) == _abi.OK
        assert n.value == e16.eff16_reference(c.log.eff)[1] > 0
        assert call(ls, None) == _abi.OK and call(ls, None) == _abi.OK   # dropped, and again: a no-op
        eng.drop_pack16(dl)
        assert call(ls, buf.ptr) == _abi.EINVAL                   # the narrow tier went
        eng.drop_pack(dl)


@pytest.mark.parametrize("how", ("null", "dev_free", "pack16_again", "eff_free"))
def test_drop_returns_to_eff(eng, oracle_lib, monkeypatch, how):
    c, want = want_of(oracle_lib, "edges16")
    live = live_of(c, want)
    knobs(monkeypatch, **FORCE)
    with scratch(eng):
        dl, eff16 = device_log(eng, c)
        fill(eng, eff16, 0x7F)
        got = read(eng, dl, c)             # the effect tier is in use
        assert set(np.flatnonzero(live)) <= set(bad_requests(got, want, c.req.n_req))
        if how == "null":
            eng.drop_eff16(dl)
        elif how == "dev_free":
            eff16.free()
        elif how == "pack16_again":
            eng.index_pack16(dl)           # the narrow tier rebuilt: the effect tier goes with the old one
        else:                              # the array the tier was built from is freed: a new one,
            dl.bufs["eff"].free()          # at the same address or not, is not the tier's
            dl.bufs["eff"] = eng.upload(c.log.eff)
            dl.struct.eff = dl.bufs["eff"].ptr
        check(read(eng, dl, c), want, c, f"effect tier dropped ({how})")
        eng.drop_pack(dl)


def test_eff_pointer_mismatch_reads_that_eff(eng, oracle_lib, monkeypatch):
    """The registry's key has no eff: a log struct with the same oc and key_off
    whose eff is another array is served from that array, not from the tier."""
    c, _ = want_of(oracle_lib, "edges16")
    eff2 = np.where(c.log.eff == _abi.EFFECT_INVALID, 77, 3 - np.asarray(c.log.eff, np.int64) // 2)
    c2 = dataclasses.replace(c, log=dataclasses.replace(c.log, eff=eff2.astype(np.int64)))
    want2 = e16.run_oracle(oracle_lib, c2)
    knobs(monkeypatch, **FORCE)
    with scratch(eng):
        dl, _ = device_log(eng, c)
        other = eng.upload(c2.log.eff)
        ls2 = _abi.AgnLog.from_buffer_copy(dl.struct)
        ls2.eff = other.ptr
        check(read(eng, ls2, c2), want2, c2, "eff of another array")
        eng.drop_pack(dl)


def test_escape_bound_keeps_the_gathered_effects(eng, oracle_lib, monkeypatch):
    """One escaped entry: at 1024 entries the bound n_esc * 1024 <= n_entries
    holds and the read loads eff16; at 1023 it does not, and eff16 is never read."""
    knobs(monkeypatch)
    for short, tier in ((False, True), (True, False)):
        c = e16.bound_case(short)
        want = e16.run_oracle(oracle_lib, c)
        assert c.log.n_entries == (1023 if short else 1024) and e16.served8(c).all()
        with scratch(eng):
            dl, eff16 = device_log(eng, c)
            check(read(eng, dl, c), want, c, f"{c.log.n_entries} entries")
            fill(eng, eff16, 0x7F)
            got = read(eng, dl, c)
            eng.drop_pack(dl)
        if tier:
            assert set(range(16)) == set(bad_requests(got, want, 16))
        else:
            check(got, want, c, "eff16 poisoned, more than one entry in 1024 escaped")
