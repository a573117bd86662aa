"""agn_oplog_load without a GPU: the header and the ctypes table agree on the
call and on ABI version 7, and the twin builder of tests/test_oplog_load.py
derives same_op / agn_oplog_set_counter correctly from a key's op ids."""
import ctypes as C
import os
import re

import numpy as np

from antidote_amd import _abi
from oplog_load_util import LENGTHS, take, twin_steps, with_lengths
from synth import random_case

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_header_and_abi_table_agree():
    h = open(os.path.join(ROOT, "include", "antidote_gpu.h")).read()
    assert re.search(r"^#define AGN_ABI_VERSION 7$", h, re.M)
    assert _abi.ABI_VERSION == 7
    m = re.search(r"^int agn_oplog_load\(([^)]*)\);", h, re.M)
    assert m, "agn_oplog_load is not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["agn_oplog *log", "const agn_log *src", "void *stream"]
    res, argtypes = _abi.PROTOTYPES["agn_oplog_load"]
    assert res is C.c_int
    assert argtypes == [C.c_void_p, C.POINTER(_abi.AgnLog), C.c_void_p]


def replay(steps):
    """What agn_oplog_append assigns when fed `steps` (its id rule, :630)."""
    counter, ids = 0, []
    for i, (set_to, same) in enumerate(steps):
        if set_to is not None:
            assert not same, "a counter is never set inside an op"
            counter = set_to
        if same:
            assert i > 0, "same_op needs a preceding entry"
        else:
            counter += 1
        ids.append(counter)
    return ids


def test_twin_steps_on_hand_written_ids():
    assert twin_steps([]) == []
    assert twin_steps([1, 2, 3]) == [(None, 0)] * 3
    assert twin_steps([2]) == [(1, 0)]
    assert twin_steps([1, 1, 1]) == [(None, 0), (None, 1), (None, 1)]
    assert twin_steps([5, 5, 6, 9]) == [(4, 0), (None, 1), (None, 0), (8, 0)]
    assert twin_steps([1, 3, 3, 4]) == [(None, 0), (2, 0), (None, 1), (None, 0)]
    assert twin_steps(np.array([7, 8, 8, 0xFFFFFFFE], np.uint32)) == \
        [(6, 0), (None, 0), (None, 1), (0xFFFFFFFD, 0)]
    for ids in ([1, 2, 3], [5, 5, 6, 9], [1, 3, 3, 4], [4, 4, 4, 5, 7, 7], [1]):
        assert replay(twin_steps(ids)) == ids


def test_constructed_lengths():
    log, req, _ = random_case(3, _abi.SET_AW, 20, 3, 220, multi=0.25, empty=0.0)
    out, r = with_lengths(log, req, LENGTHS)
    assert (out.key_off[1:] - out.key_off[:-1]).astype(int).tolist() == LENGTHS
    assert LENGTHS[0] == 0 and LENGTHS[-1] == 0 and 0 in LENGTHS[5:-5]
    assert r.n_req == len(LENGTHS) and out.rem_off[-1] <= len(out.rem_tok)
    one, _ = take(log, req, [(2, 1)])
    e = int(log.key_off[2])
    assert one.op_id[0] == log.op_id[e] and np.array_equal(one.oc[0], log.oc[e])
    assert one.rem_tok[:int(one.rem_off[1])].tolist() == \
        log.rem_tok[int(log.rem_off[e]):int(log.rem_off[e + 1])].tolist()
