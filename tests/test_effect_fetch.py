"""k_counter_quad2's deferred effect fetch (AGN_Q2_EFF) and paired result
stores (AGN_Q2_STORE) against the C oracle, bit for bit, on the cases of
tests/effect_cases.py (tests/test_effect_fetch_cpu.py holds the conditions on
those inputs).

The effects nobody may read are poisoned: a kernel that loads a wrong lane, or
folds a lane it did not load, shows up in value, flags or err_pos.  Every case
runs cold and warm, dense and with presence masks (the key DC sets indexed:
the dense scan; not indexed: the per-entry-mask scan), under all four
combinations of the two knobs."""
import pytest

import effect_cases as ec
from antidote_amd import _abi
from synth import compare
from test_edges import masked_device
from test_effect_fetch_cpu import run_oracle

pytestmark = pytest.mark.gpu

FORMS = ("dense", "masked_indexed", "masked_no_index")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("is_cold", [True, False], ids=["cold", "warm"])
@pytest.mark.parametrize("kind", ec.POISONS)
@pytest.mark.parametrize("case", ec.CASES)
def test_effect_fetch_vs_oracle(eng, oracle_lib, monkeypatch, case, kind, is_cold, form):
    style = None if form == "dense" else "uniform"
    log, req, names, pats = ec.build(case, style)
    log = ec.poison(log, pats, kind)
    if is_cold:
        req = ec.cold(req)
    want = run_oracle(oracle_lib, log, req, style)
    monkeypatch.delenv("AGN_COUNTER_GLDS", raising=False)
    monkeypatch.delenv("AGN_COUNTER_IMPL", raising=False)
    monkeypatch.setenv("AGN_COUNTER_VARIANT", "3")   # k_counter_quad2
    monkeypatch.setenv("AGN_COUNTER_EARLY", "0")
    for e, s in ec.KNOBS:
        monkeypatch.setenv("AGN_Q2_EFF", e)
        monkeypatch.setenv("AGN_Q2_STORE", s)
        if style is None:
            got = eng.materialize_host(log, req, sparse=False)
        else:
            got = masked_device(eng, log, req, form == "masked_indexed")
        bad = compare(_abi.COUNTER_PN, ec.D, got, want, bool(style), req.n_req)
        assert not bad, (f"AGN_Q2_EFF={e} AGN_Q2_STORE={s}",
                         [(names[b[0]],) + tuple(b[1:]) for b in bad[:8]])
        if case == "corrupt":   # the partner of a corrupt request is complete
            ok = (want.flags & _abi.F_ERR_CORRUPTED) == 0
            assert (got.flags[~ok] == _abi.F_ERR_CORRUPTED).all()
            assert (got.err_pos[~ok] == 0xFFFFFFFF).all()
            done = (want.flags & (_abi.F_ERR_CORRUPTED | _abi.F_ERR_UNEXPECTED)) == 0
            for f in ("value", "hole", "count", "flags"):   # (an error leaves count open)
                assert (getattr(got, f)[done] == getattr(want, f)[done]).all(), f
