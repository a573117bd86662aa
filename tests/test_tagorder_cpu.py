"""agn_tagorder (host-only, no GPU): the value-order labels of a register_lww
log.  The policy is the header's: labels in [1, 2^64 - 2]; an insert between
neighbours lo and hi (missing: 0 and 2^64 - 1) takes lo + (hi - lo) / 2; if
that equals lo, every label becomes (i + 1) * floor((2^64 - 1) / (n + 1)).
Every expectation below is derived from that, none is measured."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from antidote_amd import _abi
from antidote_amd._lib import EngineError
from antidote_amd.encode import term_key
from antidote_amd.engine import TagOrder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1


def check_order(o, want):
    assert len(o) == len(want)
    assert [o.at(i) for i in range(len(want))] == want
    labs = [int(o.labels(t, 1)[0]) for t in want]
    assert all(1 <= x <= U64 - 1 for x in labs)
    assert all(a < b for a, b in zip(labs, labs[1:]))


def even(n):
    return [(i + 1) * (U64 // (n + 1)) for i in range(n)]


def labels_in_order(o):
    return [int(o.labels(o.at(i), 1)[0]) for i in range(len(o))]


class Model:
    """The header's policy in Python: the sorted tags and their labels."""

    def __init__(self):
        self.tags, self.labels = [], []

    def insert(self, pos, tag):
        lo = self.labels[pos - 1] if pos else 0
        hi = self.labels[pos] if pos < len(self.tags) else U64
        mid = lo + (hi - lo) // 2
        self.tags.insert(pos, tag)
        self.labels.insert(pos, mid)
        if mid != lo:
            return False
        self.labels = even(len(self.tags))
        return True


def check_full(o, m):
    """Order and labels against the model, and the properties themselves."""
    check_order(o, m.tags)
    assert labels_in_order(o) == m.labels


def test_random_inserts_against_sorted_list():
    """2 000 random inserts.  After each: the order around the insert and the
    labels there equal the model's, lie strictly between the neighbours' and
    within [1, 2^64 - 2], and `relabelled` is the model's; the whole order and
    every label are checked after each relabel and every 50 inserts (and after
    each of the last 50).  The C driver (below) checks the whole order after
    every single insert."""
    rng = np.random.default_rng(17)
    m, relabels = Model(), 0
    with TagOrder() as o:
        for i in range(2000):
            pos = int(rng.integers(0, len(m.tags) + 1))
            if i % 7 == 0:      # front, back and one fixed gap close gaps: relabels happen
                pos = (0, len(m.tags), min(5, len(m.tags)))[(i // 7) % 3]
            tag = 0xFFFFFFFE - i if i % 3 == 0 else i
            want_rel = m.insert(pos, tag)
            rel = o.insert(pos, tag)
            assert rel is want_rel, (i, pos)
            relabels += rel
            n = len(m.tags)
            assert len(o) == n
            lo_p, hi_p = max(pos - 1, 0), min(pos + 1, n - 1)
            labs = []
            for q in range(lo_p, hi_p + 1):
                assert o.at(q) == m.tags[q], (i, q)
                labs.append(int(o.labels(m.tags[q], 1)[0]))
            assert labs == m.labels[lo_p:hi_p + 1], (i, pos)
            assert all(1 <= x <= U64 - 1 for x in labs)
            assert all(a < b for a, b in zip(labs, labs[1:])), (i, pos, labs)
            if rel or i % 50 == 0 or i >= 1950:
                check_full(o, m)
        check_full(o, m)
    # 96 of the inserts are scripted to the front; each halves the first label
    # (rounding down) from at most 2^63 - 1, so without a relabel the 64th
    # would find the midpoint 0 = lo: at least one relabel must have happened
    assert relabels >= 1, relabels


def test_front_inserts_relabel_at_the_64th():
    with TagOrder() as o:
        for i in range(63):
            assert o.insert(0, i) is False
            assert int(o.labels(i, 1)[0]) == (1 << (63 - i)) - 1
        assert labels_in_order(o) == [(1 << k) - 1 for k in range(1, 64)]
        assert o.insert(0, 63) is True
        assert [o.at(i) for i in range(64)] == list(range(63, -1, -1))
        assert labels_in_order(o) == even(64)
        # the next one fits again
        assert o.insert(0, 64) is False
        assert int(o.labels(64, 1)[0]) == even(64)[0] // 2


def test_back_and_middle_inserts_reach_a_relabel():
    with TagOrder() as o:
        n = 0
        while not o.insert(n, n):
            n += 1
            assert n < 100
        n += 1
        # the gap below 2^64 - 1 is 2^63 after the first insert and halves
        # (rounded up) with each: 1 after the 64th, so the 65th relabels
        assert n == 65 and labels_in_order(o) == even(65)
        lo, hi = even(65)[10], even(65)[11]
        k = 0
        while True:
            rel = o.insert(11, n)
            n += 1
            if rel:
                break
            hi = lo + (hi - lo) // 2
            assert int(o.labels(n - 1, 1)[0]) == hi
            k += 1
            assert k < 100
        assert hi == lo + 1 and labels_in_order(o) == even(n)
        assert [o.at(i) for i in range(11)] == list(range(11))


def test_labels_over_a_range_with_holes():
    with TagOrder() as o:
        for pos, tag in enumerate((3, 5, 6, 40)):
            o.insert(pos, tag)
        got = o.labels(0, 42)
        assert [int(t) for t in np.nonzero(got)[0]] == [3, 5, 6, 40]
        assert got[3] < got[5] < got[6] < got[40]
        assert not o.labels(0xFFFFFFF0, 16).any() and len(o.labels(7, 0)) == 0


def test_errors_are_einval_and_change_nothing():
    with TagOrder() as o:
        for pos, tag in enumerate((10, 20, 30)):
            o.insert(pos, tag)
        before = labels_in_order(o)
        for pos, tag in ((4, 40), (0, 20), (3, 10), (0, _abi.TAG_INVALID)):
            with pytest.raises(EngineError) as e:
                o.insert(pos, tag)
            assert e.value.code == _abi.EINVAL
        with pytest.raises(EngineError) as e:
            o.at(3)
        assert e.value.code == _abi.EINVAL
        assert labels_in_order(o) == before and [o.at(i) for i in range(3)] == [10, 20, 30]
        assert o.lib.agn_tagorder_insert(None, 0, 1, None) == _abi.EINVAL
        assert o.lib.agn_tagorder_size(o.h, None) == _abi.EINVAL


def test_insert_term_keeps_erlang_term_order():
    """insert_term's binary search with encode.term_key: values interned in an
    arbitrary order end up sorted number < atom < tuple < list < binary."""
    vals = [b"b", 3, "atom", (1, 2), b"a", [1], 2.5, b"", (0,), "b", -7, b"ab", [0, 9], True]
    with TagOrder() as o:
        for tag, v in enumerate(vals):
            o.insert_term(tag, v)
        got = [vals[o.at(i)] for i in range(len(vals))]
        assert got == sorted(vals, key=term_key)
        labs = o.labels(0, len(vals))
        by_label = [vals[int(t)] for t in np.argsort(labs)]
        assert by_label == got and labs.all()


def test_driver_under_sanitizers(tmp_path):
    """The helper's source and tests/tagorder_driver.cpp (its own main, the
    same sequences) built with -fsanitize=address,undefined and run as a
    program: nothing is preloaded, nothing is loaded into Python."""
    # clang links the sanitizer runtimes statically: the program needs nothing
    # in front of it in the library list
    rocm = "/opt/rocm/llvm/bin/clang++"
    cxx = rocm if os.path.exists(rocm) else shutil.which("clang++") or shutil.which("g++")
    exe = str(tmp_path / "tagorder_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-x", "c++", os.path.join(ROOT, "antidote_amd", "csrc", "tagorder.hip"),
                           os.path.join(ROOT, "tests", "tagorder_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tagorder_driver: ok" in r.stdout and "runtime error" not in r.stderr
