"""The launch bound of k_counter_pack8 (launch_quad2: n_wide * 1024 <= n_keys),
measured where it bites: a cfg2-shaped log in which exactly one key in EVERY,
evenly spread, is wide (one clock moved 70 000 us), read cold with the narrow
kernel on (AGN_Q2_NARROW=1, whatever the bound says) against off (=0),
interleaved in one process, outputs bit-identical.

  python scripts/ab_narrow_bound.py [--keys 1048576] [--every 1024] [--rounds 12]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from antidote_amd._lib import set_knob  # noqa: E402
from antidote_amd import _abi  # noqa: E402
from antidote_amd.engine import Engine  # noqa: E402
from bench import CONFIGS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=1 << 20)
ap.add_argument("--every", type=int, action="append", default=[])
ap.add_argument("--rounds", type=int, default=12)
a = ap.parse_args()
FIELDS = ("value", "hole", "lastct", "count", "flags", "err_pos")
eng = Engine(0)
sp = torch.cuda.current_stream().cuda_stream
cfg = CONFIGS[2]
K, N = a.keys, cfg["ops_per_key"]
for every in a.every or [1024]:
    g = _abi.AgnGenCfg(crdt_type=cfg["crdt_type"], n_dcs=cfg["n_dcs"], n_keys=K, ops_per_key=N,
                       n_elems=cfg["n_elems"], seed=cfg["seed"], key_base=0, key_stride=1, warm=0)
    dl, dr = eng.gen_dev(g)
    # the last op of every `every`-th key, column 0: + 70 000 (its column then spans > 65 535)
    wide = np.arange(every // 2, K, every, dtype=np.int64)
    v = np.zeros(1, np.uint64)
    for k in wide:
        p = dl.oc + (int(k) * N + N - 1) * 8 * 8
        eng.lib.agn_memcpy_d2h(eng.ctx, v.ctypes.data, p, 8, None)
        eng.sync()
        v += np.uint64(70_000)
        eng.lib.agn_memcpy_h2d(eng.ctx, p, v.ctypes.data, 8, None)
        eng.sync()
    rows, base, ok, n_un = eng.index_pack(dl)          # replaces the index agn_gen_dev built
    rows16, narrow, n_wide = eng.index_pack16(dl)
    assert n_un == 0 and n_wide == len(wide), (n_un, n_wide, len(wide))
    res = eng.alloc_result(K, cfg["n_dcs"], sparse=False)
    names = ("off", "on")
    times = {x: [] for x in names}
    for rnd in range(a.rounds):
        for x in (names if rnd % 2 == 0 else names[::-1]):
            set_knob("AGN_Q2_NARROW", "1" if x == "on" else "0")
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            eng.materialize(dl, dr, res, stream=sp)
            e.record()
            torch.cuda.synchronize()
            if rnd >= 2:
                times[x].append(b.elapsed_time(e))
    outs = {}
    for x in names:
        set_knob("AGN_Q2_NARROW", "1" if x == "on" else "0")
        eng.materialize(dl, dr, res, stream=sp)
        torch.cuda.synchronize()
        outs[x] = eng.fetch_result(res)
    set_knob("AGN_Q2_NARROW", None)
    same = all(np.array_equal(getattr(outs["on"], f), getattr(outs["off"], f)) for f in FIELDS)
    ms = {x: float(np.median(t)) for x, t in times.items()}
    print(f"{K} keys x {N} ops, 1 key in {every} wide ({n_wide} keys, {n_wide * 8 / K:.4f} of the "
          f"groups fall back): off {ms['off']:.3f} ms  on {ms['on']:.3f} ms  "
          f"off/on {ms['off'] / ms['on']:.3f}  same={same}", flush=True)
    eng.drop_pack(dl)
    for b in (rows, base, ok, rows16, narrow, *res.bufs.values()):
        b.free()
    eng.free_gen(dl, dr)
