"""Random logs through the tiers of the packed index on the GPU: k_counter_pack4,
k_counter_pack8<false|true> and the packed form of k_counter_quad2 on the logs
of tests/tier_cases.py (tests/test_counter_tiers_random_cpu.py holds the
conditions on those inputs).

A log is read with no index registered, with the u32 index, with the narrow
tier added and with the effect tier added; under the default knobs and under
AGN_Q2_NARROW=1, AGN_Q2_EFF16=1, AGN_Q2_FOUR=0 and AGN_Q2_PACK=0 alone (and,
since a log of 300 keys with a wide key or an escaped effect stays under the
launcher's bounds, AGN_Q2_NARROW=1 with AGN_Q2_EFF16=1: the only way to the
effect tier's kernel here); as a whole partition (req.keys == NULL) and through
the key maps arange, a permutation and synth.rekey's repeated keys.  Every run
equals the oracle bit for bit: no result depends on the index.

The path, by poison (pack4_cases / pack8_cases.poison_oc, eff16_cases.poison_eff
on the random log): a served group reads neither oc nor a non-escaped effect.
The index builders are held to the numpy restatements on the same logs."""
import numpy as np
import pytest

import eff16_cases as e16
import pack4_cases as p4
import pack8_cases as p8
import pack_cases as pc
import tier_cases as tc
from antidote_amd import _abi
from synth import compare
from test_counter_pack8 import fill, put
from test_edges import scratch

pytestmark = pytest.mark.gpu

KNOBS = ({}, {"AGN_Q2_NARROW": "1"}, {"AGN_Q2_EFF16": "1"}, {"AGN_Q2_FOUR": "0"}, {"AGN_Q2_PACK": "0"},
         {"AGN_Q2_NARROW": "1", "AGN_Q2_EFF16": "1"})
ALL_KNOBS = ("AGN_COUNTER_GLDS", "AGN_COUNTER_IMPL", "AGN_COUNTER_VARIANT", "AGN_Q2_EFF", "AGN_Q2_STORE",
             "AGN_Q2_PACK", "AGN_Q2_FOUR", "AGN_Q2_NARROW", "AGN_Q2_EFF16", "AGN_XCD_REMAP",
             "AGN_XCD_CHUNK")
_WANT = {}


def want_of(oracle_lib, K, variant, keymap):
    """(case under the key map, oracle result), computed once."""
    key = (K, variant, "identity" if keymap == "arange" else keymap)
    if key not in _WANT:
        c = tc.keyed(tc.case(K, variant), keymap)
        _WANT[key] = (c, p8.run_oracle(oracle_lib, c))
    return _WANT[key]


def knobs(monkeypatch, kv):
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def device_log(eng, c, tier):
    """The case's log on the device with the tiers up to `tier` registered."""
    dl = eng.upload_log(c.log)
    if c.key_len is not None:
        dl.bufs["key_len"] = eng.upload(c.key_len)
        dl.struct.key_len = dl.bufs["key_len"].ptr
    if c.index_ids:
        eng.index_ids(dl)
    t = tc.TIERS.index(tier)
    bufs = {}
    if t >= 1:
        bufs["rows"], _, bufs["ok"], _ = eng.index_pack(dl)
    if t >= 2:
        bufs["rows16"], bufs["narrow"], bufs["n_wide"] = eng.index_pack16(dl)
    if t >= 3:
        bufs["eff16"], bufs["n_esc"] = eng.index_eff16(dl)
    return dl, bufs


def read(eng, dl, c, identity):
    dr = eng.upload_read(c.req, sparse=False)
    if identity:
        dr.struct.keys = None          # the whole partition: request i reads key i
    dres = eng.alloc_result(c.req.n_req, pc.D, sparse=False)
    eng.materialize(dl, dr, dres)
    return eng.fetch_result(dres)


def check(got, want, c, what):
    bad = compare(_abi.COUNTER_PN, pc.D, got, want, False, c.req.n_req)
    assert not bad, (what, [(c.names[b[0]],) + tuple(b[1:]) for b in bad[:8]])


@pytest.mark.parametrize("tier", tc.TIERS)
@pytest.mark.parametrize("K,variant", tc.CASES)
def test_random_log_vs_oracle(eng, oracle_lib, monkeypatch, K, variant, tier):
    with scratch(eng):
        dl, _ = device_log(eng, tc.case(K, variant), tier)
        for kv in KNOBS:
            knobs(monkeypatch, kv)
            for keymap in tc.KEYMAPS:
                c, want = want_of(oracle_lib, K, variant, keymap)
                check(read(eng, dl, c, keymap == "identity"), want, c, (tier, kv, keymap))
        if tier != "none":
            eng.drop_pack(dl)


@pytest.mark.parametrize("K,variant", tc.CASES)
def test_path_by_poison(eng, oracle_lib, monkeypatch, K, variant):
    c, want = want_of(oracle_lib, K, variant, "identity")
    with scratch(eng):
        # the u32 index: groups of four never read oc
        dl, b = device_log(eng, c, "u32")
        knobs(monkeypatch, {})
        put(eng, dl.bufs["oc"], p4.poison_oc(c).oc)
        check(read(eng, dl, c, True), want, c, "oc poisoned, groups of four")
        knobs(monkeypatch, {"AGN_Q2_PACK": "0"})        # the poison has teeth
        got = read(eng, dl, c, True)
        live = p4.served4(c) & (want.count > 0)
        bad = {x[0] for x in compare(_abi.COUNTER_PN, pc.D, got, want, False, K)}
        assert set(np.flatnonzero(live)) <= bad
        eng.drop_pack(dl)
    with scratch(eng):
        # all tiers: groups of eight read neither oc, nor the u32 rows, nor a
        # non-escaped effect
        dl, b = device_log(eng, c, "eff")
        put(eng, dl.bufs["oc"], p8.poison_oc(c).oc)
        fill(eng, b["rows"])
        knobs(monkeypatch, {"AGN_Q2_NARROW": "1"})
        check(read(eng, dl, c, True), want, c, "oc and u32 rows poisoned, groups of eight")
        put(eng, dl.bufs["eff"], e16.poison_eff(c).eff)
        knobs(monkeypatch, {"AGN_Q2_NARROW": "1", "AGN_Q2_EFF16": "1"})
        check(read(eng, dl, c, True), want, c, "and eff poisoned where the tier does not escape")
        eng.drop_pack(dl)


@pytest.mark.parametrize("K,variant", tc.CASES)
def test_index_builders_vs_numpy(eng, K, variant):
    c = tc.case(K, variant)
    E = c.log.n_entries
    live = p8.entries_of(c, np.ones(K, bool))          # entries inside a key's segment
    _, ok, rows = pc.pack_reference(c.log) if c.key_len is None else (None, None, None)
    nar, rows16 = p8.rows16_reference(c)
    eff16, n_esc = e16.eff16_reference(c.log.eff)
    with scratch(eng):
        dl, b = device_log(eng, c, "eff")
        g_nar = eng.download(b["narrow"], np.uint8, (K,))
        g_rows16 = eng.download(b["rows16"], np.uint16, (E, pc.D))
        g_eff16 = eng.download(b["eff16"], np.int16, (E,))
        if ok is not None:
            g_ok = eng.download(b["ok"], np.uint8, (K,))
            g_rows = eng.download(b["rows"], np.uint32, (E, pc.D))
        eng.drop_pack(dl)
    assert np.array_equal(g_nar, nar) and b["n_wide"] == int((nar == 0).sum())
    keep = live & (nar[np.repeat(np.arange(K), np.diff(c.log.key_off).astype(np.int64))] == 1)
    assert keep.any() and np.array_equal(g_rows16[keep], rows16[keep])
    assert np.array_equal(g_eff16[live], eff16[live]) and b["n_esc"] == n_esc
    if c.key_len is None:
        assert np.array_equal(g_ok, ok)
        packed = ok[pc.key_of_entry(c.log)] == 1
        assert np.array_equal(g_rows[packed], rows[packed])
