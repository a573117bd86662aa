"""A/B of agn_read_cached for counter_b: the one fused launch
(k_bcounter_serve, mat_bcounter.hip, AGN_BCOUNTER_FUSED=1) against the kernel
sequence (agn_ss_lookup -> k_bcounter -> agn_ss_store, the knob unset), one
process, the two forms interleaved.

D = 8, generator keys of 64 ops over 4 slots per key, dense clocks.  A first pass over every key
stores its snapshot; the timed reads repeat the same clocks, so each is a warm
hit on slot 0 that includes no further op and stores nothing (the steady state
of a served partition).  Sizes: 2^10 ... 2^20 requests (the first n keys).
Every result array, the status, the prune flags and the cache after the read
are asserted equal between the two forms.

  python scripts/ab_bcounter_serve.py [rounds] [n1,n2,...]

AGN_READ_CACHED_SPLIT=0 is set for the run, so "fused" is the fused launch at
every size (agn_read_cached_path is asked and its answer printed).
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from antidote_amd._lib import set_knob  # noqa: E402

SIZES = tuple(1 << x for x in (10, 12, 13, 14, 15, 16, 18, 20))
KNOB = "AGN_BCOUNTER_FUSED"
FORMS = {"fused": "1", "sequence": None}
E = 4      # slots per key


def main():
    import torch
    from antidote_amd import _abi
    from antidote_amd.engine import Engine, read_cached_path
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    sizes = tuple(int(x) for x in sys.argv[2].split(",")) if len(sys.argv) > 2 else SIZES
    K, N, D, S = max(sizes), 64, 8, _abi.SNAPSHOT_THRESHOLD
    torch.cuda.set_device(0)
    eng = Engine(0)
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    set_knob("AGN_READ_CACHED_SPLIT", "0")
    g = _abi.AgnGenCfg(crdt_type=_abi.COUNTER_B, n_dcs=D, n_keys=K, ops_per_key=N, n_elems=E,
                       seed=20250114, key_base=0, key_stride=1, warm=0)
    dl, dr = eng.gen_dev(g)
    dev = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    cap = 2 * E * K
    bufs = dict(n=dev(K, torch.int32), clock=dev(K * S * D, torch.int64),
                last_op=dev(K * S, torch.int64), value=dev(K * S, torch.int64),
                ctl=dev(4, torch.int64), tag=dev(cap, torch.int32), tok=dev(cap, torch.int64),
                status=dev(K, torch.uint8), prune=dev(K, torch.uint8), thr=dev(K * D, torch.int64),
                keys=torch.arange(K, dtype=torch.int64, device="cuda"))
    c = _abi.AgnSsCache()
    c.n_dcs, c.slots, c.n_keys = D, S, K
    c.n, c.clock, c.last_op, c.value = (bufs[x].data_ptr() for x in
                                        ("n", "clock", "last_op", "value"))
    c.state_tag, c.state_tok, c.state_cap = bufs["tag"].data_ptr(), bufs["tok"].data_ptr(), cap
    c.state_ctl = bufs["ctl"].data_ptr()
    res = eng.alloc_result(K, D, sparse=False, cap_off=np.arange(K + 1, dtype=np.uint64) * np.uint64(E))

    def run(n):
        eng.read_cached(c, dl, n, dr.keys or bufs["keys"].data_ptr(), dr.R, None, None, res,
                        bufs["status"].data_ptr(), bufs["prune"].data_ptr(),
                        bufs["thr"].data_ptr(), stream=sp)

    def snap():
        r = eng.fetch_result(res)
        return {**{f: getattr(r, f).copy() for f in ("hole", "lastct", "count", "flags", "err_pos",
                                                     "out_n", "out_tag", "out_tok")},
                "status": bufs["status"].cpu().numpy(), "prune": bufs["prune"].cpu().numpy(),
                **{"cache_" + x: bufs[x].cpu().numpy() for x in ("n", "clock", "last_op", "value",
                                                                 "ctl")}}

    set_knob(KNOB, "1")
    run(K)          # NEW: every key's first snapshot is stored
    torch.cuda.synchronize()
    first = snap()
    run(K)          # the hit on it
    torch.cuda.synchronize()
    out = {"D": D, "ops_per_key": N, "rounds": rounds,
           "first_pass": {"new": int((first["status"] == _abi.SS_NEW).sum()),
                          "count_sum": int(first["count"].sum())}, "sizes": {}}
    for n in sizes:
        ms = {f: [] for f in FORMS}
        got, path = {}, {}
        names = list(FORMS)
        for r in range(rounds + 1):     # round 0 warms both forms up and keeps their results
            for f in (names if r % 2 == 0 else names[::-1]):
                set_knob(KNOB, FORMS[f])
                path[f] = read_cached_path(c, dl, n)
                b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.record(st)
                run(n)
                e.record(st)
                torch.cuda.synchronize()
                if r:
                    ms[f].append(b.elapsed_time(e))
                else:
                    got[f] = snap()
        a, s = got["fused"], got["sequence"]
        hit = a["status"][:n] == _abi.SS_HIT
        out["sizes"][str(n)] = {
            "path_fused": path, "ms_median": {f: float(np.median(x)) for f, x in ms.items()},
            "ms_min": {f: float(min(x)) for f, x in ms.items()},
            "ms_max": {f: float(max(x)) for f, x in ms.items()},
            "warm_hits": int(hit.sum()), "stored": int(a["prune"][:n].sum()),
            "count_sum": int(a["count"][:n].sum()),
            "results_equal": True}
        for x in a:     # every result array, and the cache, between the arms
            m = len(a[x]) if x.startswith("cache_") or x in ("out_tag", "out_tok", "lastct") else n
            assert np.array_equal(a[x][:m], s[x][:m]), (n, x)
    set_knob(KNOB, None)
    set_knob("AGN_READ_CACHED_SPLIT", None)
    print(json.dumps(out), flush=True)
    eng.free_gen(dl, dr)
    eng.close()


if __name__ == "__main__":
    main()
