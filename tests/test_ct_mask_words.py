"""LastOpCt mask words of the general kernels at 129 <= D <= 192: the wave
covers the DCs in four column groups (KeyFilter::write_ct, T = 4) but a mask
row has three words; the fourth group's (empty) ballot must not be stored into
the next request's first word."""
import ctypes as C

import numpy as np
import pytest

from antidote_amd import _abi
from antidote_amd.encode import alloc_result, log_struct, read_struct, result_struct
from synth import compare, random_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D", [129, 150, 192])
def test_counter_general_mask_words(eng, oracle_lib, monkeypatch, D):
    monkeypatch.setenv("AGN_COUNTER_IMPL", "general")
    log, req, _ = random_case(D, _abi.COUNTER_PN, 96, D, 12, sparse=True, warm=0.5, empty=0.05)
    got = eng.materialize_host(log, req, sparse=True)
    want = alloc_result(req.n_req, D, sparse=True)
    assert oracle_lib.oracle_materialize(C.byref(log_struct(log)), C.byref(read_struct(req)),
                                         C.byref(result_struct(want)), 2) == 0
    # a stray store zeroes a neighbour's first word: enough of them must be non-zero
    assert (want.lastct_mask[:, 0] != 0).sum() >= 10
    bad = compare(_abi.COUNTER_PN, D, got, want, True, req.n_req)
    assert not bad, bad[:8]
    live = (want.flags & _abi.F_CT_IGNORE) == 0
    assert np.array_equal(got.lastct_mask[live], want.lastct_mask[live])
