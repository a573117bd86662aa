"""Conditions on the inputs of tests/test_counter_tiers_random.py (no GPU): the
random logs of tests/tier_cases.py reach what they are for.  For every seed
used, from the log alone (pack4_cases.served4, pack8_cases.served8 /
unservable) and from the oracle:

  - the straight paths serve most but not all groups: served4 in [0.5, 0.97],
    served8 in [0.3, 0.9];
  - wide, unpacked, corrupt and empty keys occur, long ones in the "long" logs;
  - at least 3 served keys have R below a column's minimum (the noR override
    of the packed verdicts), in groups of 4 and in groups of 8;
  - at least 3 included escaped effects sit in served groups of 8;
  - error flags are on at most a quarter of the requests, and most requests
    include an op;
  - the poisons of the path tests change the oracle's results of served
    requests and of no other."""
import numpy as np
import pytest

import eff16_cases as e16
import pack4_cases as p4
import pack8_cases as p8
import pack_cases as pc
import tier_cases as tc
from antidote_amd import _abi

ERR = _abi.F_ERR_CORRUPTED | _abi.F_ERR_UNEXPECTED


def figures(oracle_lib, c):
    want = p8.run_oracle(oracle_lib, c)
    s4, s8 = p4.served4(c), p8.served8(c)
    noR = tc.noR_keys(c)
    esc_in = e16.included_of(c) & e16.escaped_of(c) & p8.entries_of(c, s8)
    return dict(served4=float(s4.mean()), served8=float(s8.mean()), why=set(p8.unservable(c)),
                empty=int((p8.lens_of(c) == 0).sum()), noR4=int((noR & s4).sum()),
                noR8=int((noR & s8).sum()), esc=int(esc_in.sum()),
                err=float(((want.flags & ERR) != 0).mean()),
                with_op=float((want.count > 0).mean()), want=want)


def check_figures(f, variant):
    assert 0.5 <= f["served4"] <= 0.97, f["served4"]
    assert 0.3 <= f["served8"] <= 0.9, f["served8"]
    need = {"wide", "unpacked", "corrupt", ""} | ({"long"} if variant == "long" else set())
    assert need <= f["why"], f["why"]
    assert (variant == "long") == ("long" in f["why"])
    assert f["empty"] > 0
    assert f["noR4"] >= 3 and f["noR8"] >= 3, (f["noR4"], f["noR8"])
    assert f["esc"] >= 3, f["esc"]
    assert f["err"] <= 0.25 and f["with_op"] >= 0.5, (f["err"], f["with_op"])


@pytest.mark.parametrize("K,variant", tc.CASES)
def test_random_logs_meet_their_conditions(oracle_lib, K, variant):
    c = tc.case(K, variant)
    assert c.log.n_keys == K == c.req.n_req and c.req.sct is None
    assert (c.key_len is not None) == c.index_ids == (variant == "seg")
    assert (p8.lens_of(c).max() > 64) == (variant == "long") and p8.lens_of(c).max() >= 64
    f = figures(oracle_lib, c)
    print(K, variant, {k: v for k, v in f.items() if k != "want"})
    check_figures(f, variant)
    # base_value reaches both ends of its domain, effects both sides of the tier's range
    assert c.req.base_value.min() == tc.I64MIN and c.req.base_value.max() == tc.I64MAX
    eff = c.log.eff[p8.entries_of(c, np.ones(K, bool))]
    assert (eff == -32768).any() and (eff > 32767).any() and (eff == _abi.EFFECT_INVALID).any()
    # the index restatements hold on a random log: narrow <=> no wide / unpacked reason
    nar, rows16 = p8.rows16_reference(c)
    why = np.array(p8.unservable(c))
    lens = p8.lens_of(c)
    spans = p8.spans_of(c).max(axis=1)
    assert np.array_equal(nar == 1, spans <= p8.M16) and 0 < int((nar == 0).sum()) < K // 8
    assert set(why[(nar == 0) & (lens <= 64)]) <= {"wide", "unpacked"}
    _, n_esc = e16.eff16_reference(c.log.eff)
    assert n_esc >= 3


@pytest.mark.parametrize("K,variant", tc.CASES)
def test_key_maps(oracle_lib, K, variant):
    c = tc.case(K, variant)
    perm, rep = tc.keyed(c, "perm"), tc.keyed(c, "repeat")
    assert sorted(perm.req.keys.tolist()) == list(range(K)) and (np.diff(perm.req.keys.astype(int)) < 0).any()
    assert rep.req.n_req == 2 * K + 1 and rep.req.sct is None and not rep.req.txid.any()
    assert tc.keyed(c, "identity") is c and tc.keyed(c, "arange") is c
    # the repeated batch still mostly includes ops (the oracle reads row i for request i)
    want = p8.run_oracle(oracle_lib, rep)
    assert (want.count > 0).mean() >= 0.5 and ((want.flags & ERR) != 0).mean() <= 0.25
    # a permuted request reads what the identity request of its key reads
    wp, wi = p8.run_oracle(oracle_lib, perm), p8.run_oracle(oracle_lib, c)
    p = perm.req.keys.astype(np.int64)
    for f in ("count", "flags", "hole"):
        assert np.array_equal(getattr(wp, f), getattr(wi, f)[p]), f
    if variant != "seg":        # pack_cases.served_packed reads key_off alone
        sp = pc.served_packed(c.log, perm.req)
        assert sp.mean() >= 0.5 and not sp.all()     # packed pairs and pairs that read oc


@pytest.mark.parametrize("K,variant", tc.CASES)
def test_poisons_prove_the_paths(oracle_lib, K, variant):
    c = tc.case(K, variant)
    clean = p8.run_oracle(oracle_lib, c)
    same = lambda a, b, idx: all(np.array_equal(getattr(a, f)[idx], getattr(b, f)[idx])  # noqa: E731
                                 for f in pc.FIELDS)
    for served, poisoned in ((p4.served4(c), p4.poison_oc(c)), (p8.served8(c), p8.poison_oc(c))):
        dirty = p8.run_oracle(oracle_lib, c, poisoned)
        assert same(clean, dirty, ~served)
        live = served & (clean.count > 0)
        assert live.sum() >= K // 8
        assert not any(same(clean, dirty, [i]) for i in np.flatnonzero(live))
    s8 = p8.served8(c)
    dirty = p8.run_oracle(oracle_lib, c, e16.poison_eff(c))
    assert same(clean, dirty, ~s8) and not same(clean, dirty, s8)
