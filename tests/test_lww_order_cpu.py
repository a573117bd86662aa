"""tests/lww_order_model.py: without labels it is tests/lww_model.py, and the
constructed cases of tests/test_lww_order.py reach every branch of the rule."""
import numpy as np
import pytest

import lww_model as lm
import lww_order_model as om
from antidote_amd import _abi


@pytest.mark.parametrize("idx", range(len(lm.gpu_cases())), ids=[c[0] for c in lm.gpu_cases()])
def test_no_labels_equals_lww_model(idx):
    """lww_model's own random logs: same winner, same AGN_F_TS_TIE, with no
    table and with a table of zeros."""
    _id, seed, D, sparse, kw = lm.gpu_cases()[idx]
    log, req, cap = lm.lww_case(seed, D, reps=2, **kw)
    want, _incl, info = lm.model(log, req, sparse, cap)
    ties = 0
    for order in (None, np.zeros(2, np.uint64)):
        got, _incl, _ = om.model(log, req, sparse, cap, order=order)
        for f in ("flags", "out_n", "out_tag", "out_tok", "count", "hole", "err_pos"):
            assert np.array_equal(getattr(got, f), getattr(want, f)), f
        ties += int(((want.flags & _abi.F_TS_TIE) != 0).sum())
    assert ties > 0 or D > 64 or not any(c["tie"] for c in info)


def test_settle_by_hand():
    o = np.array([0, 30, 20, 10], np.uint64)
    assert om.settle([(5, 1)], o) == (5, 1, False, 1)
    assert om.settle([(5, 1), (5, 2), (5, 3), (4, 0)], o) == (5, 1, False, 3)
    assert om.settle([(5, 2), (5, 3)], o) == (5, 2, False, 2)
    assert om.settle([(5, 0), (5, 3)], o) == (5, 3, True, 2)       # tag 0 unlabelled
    assert om.settle([(5, 1), (5, 4)], o) == (5, 1, True, 2)       # tag 4 past the table
    assert om.settle([(5, 4), (5, 9)], o) == (5, 9, True, 2)       # both: the larger id
    assert om.settle([(5, 1), (5, 2)], None) == (5, 2, True, 2)    # no table: today's rule
    assert om.settle([(5, 0), (6, 3)], o) == (6, 3, False, 1)      # an unlabelled loser below wts
    assert om.settle([((1 << 64) - 1, 2), ((1 << 64) - 1, 1)], o)[:2] == ((1 << 64) - 1, 1)


@pytest.mark.parametrize("D", om.DS)
def test_constructed_cases_reach_every_branch(D):
    sparse = D % 2 == 1
    log, req, cap = om.tie_case(D, sparse)
    names = [k[0] for k in om.tie_keys()]
    assert sorted(set(np.diff(log.key_off.astype(np.int64)).tolist())) >= sorted(om.LENS)
    res, incl, info = om.model(log, req, sparse, cap, order=om.ORDERS["against"])
    assert all(x.all() for x in incl), "every entry is included"
    assert not (res.flags & (_abi.F_TS_TIE | _abi.F_ERR_UNEXPECTED | _abi.F_ERR_CAPACITY)).any()
    assert all(i["labelled"] for i in info)
    by = dict(zip(names, info))
    assert all(by[f"len{n}"]["nT"] == 1 for n in om.LENS) and by["same-tag-twice"]["nT"] == 1
    if D <= 8:      # one lane per op, 64 ops per iteration: ops 0 and 64 share lane 0
        assert by["lane-0-64"]["in_lane"] and not by["lane-0-64"]["across_lanes"]
        assert by["three-way"]["in_lane"] and by["three-way"]["across_lanes"]
    assert by["lanes-3-40"]["across_lanes"] and not by["lanes-3-40"]["in_lane"] or D > 32
    assert by["lanes-3-40"]["nT"] == 2 and by["lanes-3-40-odd"]["nT"] == 2
    assert by["base-op"]["base_tie"] and by["base-op-long"]["base_tie"]
    assert by["three-way"]["nT"] == 3 and by["three-way-base"]["nT"] == 3
    assert by["three-way-base"]["base_tie"] and not by["base-below"]["base_tie"]
    # the labels run against the id order: where tags tie, the id-order
    # winner (lww_model) is the wrong answer
    idw, _i, _ = lm.model(log, req, sparse, cap)
    tied = np.array([i["nT"] > 1 for i in info])
    o = cap[:-1].astype(np.int64)
    assert tied.sum() == 10 and (res.out_tag[o][tied] != idw.out_tag[o][tied]).all()
    assert (res.out_tag[o][~tied] == idw.out_tag[o][~tied]).all()
    assert (res.out_tok[o] == om.TS_TOP).all()
    # rewritten with order-preserving values: the same; reversed: the other winner
    same, _i, _ = om.model(log, req, sparse, cap, order=om.ORDERS["against-rewritten"])
    assert np.array_equal(same.out_tag, res.out_tag) and np.array_equal(same.flags, res.flags)
    rev, _i, _ = om.model(log, req, sparse, cap, order=om.ORDERS["reversed"])
    assert (rev.out_tag[o][tied] != res.out_tag[o][tied]).all()
    assert not (rev.flags & _abi.F_TS_TIE).any()
    # one tag unlabelled / past the table: flagged exactly where it is in T
    for name, tag in (("tag2-unlabelled", 2), ("tag3-past", 3)):
        r, _i, inf = om.model(log, req, sparse, cap, order=om.ORDERS[name])
        flagged = (r.flags & _abi.F_TS_TIE) != 0
        in_T = np.array([tag in set(k[2].values()) | ({k[3][0]} if k[3] and k[3][1] == om.TS_TOP
                                                     else set()) for k in om.tie_keys()])
        assert np.array_equal(flagged, tied & in_T) and flagged.any() and (tied & ~flagged).any()
        assert any(i["past_table"] for i in inf) == (name == "tag3-past")
        assert any(not i["labelled"] for i in inf)
