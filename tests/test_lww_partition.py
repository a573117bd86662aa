"""The register_lww partition twin (tests/lww_partition.py: the NIF's C-ABI
calls) against the reference transcription's vnode, read for read and ListLen
for ListLen.  Values are interned in descending term order, so the id order is
the reverse of the term order and every timestamp tie would go the wrong way
by ids; 70 of them pass the label allocator through one relabel."""
import numpy as np
import pytest

from antidote_amd import _abi
from lww_partition import TYPE, LwwPartition
from oracle import py_oracle as po
from test_ss_states import LWW_NEW, placeholder, vc

pytestmark = pytest.mark.gpu

K, D, STEPS, N_VALS = 64, 3, 3000, 70
BAD_KEY, ZERO_KEY = 62, 63      # one invalid effect, one Ts = 0 effect
BAD_EFFECT, ZERO_EFFECT = "assign", (0, b"zero")


def value(j):
    """Value number j in arrival order: descending in term order."""
    return b"val-%03d" % (N_VALS - 1 - j)


class Workload:
    """One causal clock for every key.  A quarter of the keys (key % 4 == 0)
    draw their timestamps from three values, so two DCs assign at equal Ts all
    the time; the others from the microsecond range.  Keys 0..7 take half of
    the ops (they reach op_insert_gc's GC reads)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.clk = np.full(D, 1000, np.int64)
        self.seen = 0

    def key(self):
        return int(self.rng.integers(0, 8)) if self.rng.random() < 0.5 else \
            int(self.rng.integers(8, BAD_KEY))

    def op(self, key, fresh=True):
        c = int(self.rng.integers(0, D))
        ss = np.maximum(self.clk - self.rng.integers(0, 40, D), 0)
        self.clk[c] += int(self.rng.integers(1, 30))
        oc = ss.copy()
        oc[c] = self.clk[c]
        if fresh and self.seen < N_VALS and (self.seen < 4 or self.rng.random() < 0.15):
            j = self.seen               # the next new value: a front insert
            self.seen += 1
        else:
            j = int(self.rng.integers(0, self.seen))
        ts = 500 + int(self.rng.integers(0, 3)) if key % 4 == 0 else \
            int(self.rng.integers(1, 1 << 50))
        return c, ss, int(self.clk[c]), oc, (ts, value(j))

    def read_clock(self, lag=400):
        return np.maximum(self.clk - self.rng.integers(0, lag, D), 0)


def test_partition_vs_reference(eng):
    w = Workload(77)
    vn = po.MaterializerVnode(disk_log=True)
    part = LwwPartition(eng, D, K)
    quirk, served, tied_reads, errors = set(), 0, 0, 0
    special = {400: (BAD_KEY, BAD_EFFECT), 401: (ZERO_KEY, ZERO_EFFECT)}
    try:
        for s in range(STEPS):
            if s in special or w.rng.random() < 0.7:
                key = special[s][0] if s in special else \
                    int(w.rng.choice([BAD_KEY, ZERO_KEY])) if w.rng.random() < 0.03 else w.key()
                c, ss, ct, oc, eff = w.op(key, fresh=s not in special)
                if s in special:
                    eff = special[s][1]
                pay = po.Payload(key, TYPE, eff, vc(ss), (c, ct), s + 1)
                try:
                    vn.update(key, pay)
                except po.BadMatch:
                    quirk.add(key)
                part.update(key, pay, oc, s + 1)
                if placeholder(vn, key):
                    quirk.add(key)
                continue
            key = int(w.rng.choice([BAD_KEY, ZERO_KEY])) if w.rng.random() < 0.06 else w.key()
            R = w.read_clock(lag=400 if w.rng.random() < 0.85 else 20000)
            got, g = part.read(key, R)
            assert not g["flags"] & _abi.F_TS_TIE and got != ("error", "ts_tie"), (s, key, g)
            if key in quirk:
                continue
            try:
                want = vn.read(key, TYPE, vc(R), po.IGNORE)
            except po.BadMatch:
                quirk.add(key)
                continue
            if key == ZERO_KEY and got[0] == "error":
                # the encoder's one stated deviation (DESIGN.md
                # §4.2c): update/2 folds Ts = 0, the encoder stores an invalid entry
                assert got == ("error", ("unexpected_operation", ZERO_EFFECT, TYPE)), (s, got)
                errors += 1
                continue
            assert want == got, (s, key, g["status"], want, got)
            served += 1
            errors += got[0] == "error"
            if got[0] == "ok" and got[1] != LWW_NEW and key % 4 == 0:
                # how many reads had a choice to make: the winner's Ts under another value
                tied_reads += sum(1 for p in part.disk if p.key == key and p.op_param[0] == got[1][0]
                                  and p.op_param[1] != got[1][1] and po.vc_le(p.snapshot_time, vc(R))) > 0
            if placeholder(vn, key):
                quirk.add(key)
        ln, ll, _ct = part.ol.key_meta()
        print(f"served={served} tied_reads={tied_reads} errors={errors} gc_reads={part.gc_reads} "
              f"log_reads={part.log_reads} log_gc={part.log_gc} relabels={part.relabels} "
              f"values={len(part.terms)} quirk={sorted(quirk)}")
        assert len(part.terms) == N_VALS and part.relabels == 1, (len(part.terms), part.relabels)
        assert [part.order.at(i) for i in range(N_VALS)] == list(range(N_VALS - 1, -1, -1))
        assert served > 600 and tied_reads > 50 and errors >= 2 and part.gc_reads > 5
        assert not part.flags_seen & _abi.F_TS_TIE
        assert quirk == set(), sorted(quirk)
        for k in range(K):
            if k in vn.ops_cache:
                length, list_len = vn.ops_cache[k][1]
                assert (int(ln[k]), int(ll[k])) == (length, list_len), k
    finally:
        part.close()
