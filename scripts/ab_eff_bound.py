"""The launch bound of k_counter_pack8<true> (launch_quad2: n_esc * 1024 <=
n_entries), measured where it bites: a cfg2-shaped log in which exactly one
entry in EVERY, evenly spread, holds an effect that escapes the i16 tier
(2^40), read cold with the effect tier on (AGN_Q2_EFF16=1, whatever the bound
says) against off (=0), interleaved in one process, outputs bit-identical.

  python scripts/ab_eff_bound.py [--keys 1048576] [--every 1024] [--rounds 12]
"""
import argparse
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
E = K * N
for every in a.every or [1024]:
    g = _abi.AgnGenCfg(crdt_type=cfg["crdt_type"], n_dcs=cfg["n_dcs"], n_keys=K, ops_per_key=N,
                       n_elems=cfg["n_elems"], seed=cfg["seed"], key_base=0, key_stride=1, warm=0)
    dl, dr = eng.gen_dev(g)
    # entry every // 2 of each run of `every` entries: 2^40, which the tier cannot hold
    eff = np.empty(E, np.int64)
    eng.lib.agn_memcpy_d2h(eng.ctx, eff.ctypes.data, dl.eff, eff.nbytes, None)
    eng.sync()
    eff[every // 2::every] = 1 << 40
    eng.lib.agn_memcpy_h2d(eng.ctx, dl.eff, eff.ctypes.data, eff.nbytes, None)
    eng.sync()
    eff16, n_esc = eng.index_eff16(dl)                 # replaces the tier agn_gen_dev built
    assert n_esc == len(eff[every // 2::every]), (n_esc, E // every)
    res = eng.alloc_result(K, cfg["n_dcs"], sparse=False)
    names = ("off", "on")
    times = {x: [] for x in names}
    for rnd in range(a.rounds):
        for x in (names if rnd % 2 == 0 else names[::-1]):
            set_knob("AGN_Q2_EFF16", "1" if x == "on" else "0")
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            eng.materialize(dl, dr, res, stream=sp)
            e.record()
            torch.cuda.synchronize()
            if rnd >= 2:
                times[x].append(b.elapsed_time(e))
    outs = {}
    for x in names:
        set_knob("AGN_Q2_EFF16", "1" if x == "on" else "0")
        eng.materialize(dl, dr, res, stream=sp)
        torch.cuda.synchronize()
        outs[x] = eng.fetch_result(res)
    set_knob("AGN_Q2_EFF16", None)
    same = all(np.array_equal(getattr(outs["on"], f), getattr(outs["off"], f)) for f in FIELDS)
    ms = {x: float(np.median(t)) for x, t in times.items()}
    print(f"{K} keys x {N} ops, 1 entry in {every} escaped ({n_esc} entries, at most "
          f"{min(1.0, n_esc * 8 / K):.3f} of the groups branch): off {ms['off']:.3f} ms  "
          f"on {ms['on']:.3f} ms  off/on {ms['off'] / ms['on']:.3f}  same={same}", flush=True)
    eng.drop_eff16(dl)
    for b in (eff16, *res.bufs.values()):
        b.free()
    eng.free_gen(dl, dr)
