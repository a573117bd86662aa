"""A/B of the register_lww kernel (k_lww, mat_lww.hip) against the general
counter kernel (k_counter, AGN_COUNTER_IMPL=general) in one process, variants
interleaved, at cfg2's shape: 10M keys x 64 ops, D = 8, cold, generator data.
Both scan the same clocks with the same filter (filter.hpp); the counter reads
8 bytes of effect per op, k_lww up to 12 (timestamp + tag):

  counter_general  8*D + 8 bytes per op
  lww_early        ts / tag loaded with the chunk's rows: 8*D + 12 per op
  lww_late         ts / tag loaded after the verdict (AGN_LWW_LOAD=late):
                   8*D per op + 12 per included op

The log is agn_gen_dev's register_lww log; the counter variant reads the same
oc / op_id / key_off with an effect array beside them.  The filter outputs of
the three variants (hole, count, LastOpCt, NEWSS / CT_IGNORE) must agree, and
the two k_lww variants in every field.

  python scripts/ab_lww.py [rounds] [keys]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from antidote_amd._lib import env_changed  # noqa: E402

PEAK = 8.0e12  # HBM3E bytes/s (MI355X)
VARIANTS = {"counter_general": {"AGN_COUNTER_IMPL": "general"},
            "lww_early": {"AGN_LWW_LOAD": "early"},
            "lww_late": {"AGN_LWW_LOAD": "late"}}
KNOBS = ("AGN_COUNTER_IMPL", "AGN_LWW_LOAD")


def main():
    import torch
    from antidote_amd import _abi
    from antidote_amd.engine import Engine
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    N, D = 64, 8
    torch.cuda.set_device(0)
    eng = Engine(0)
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    g = _abi.AgnGenCfg(crdt_type=_abi.REGISTER_LWW, n_dcs=D, n_keys=K, ops_per_key=N, n_elems=16,
                       seed=20250113, key_base=0, key_stride=1, warm=0)
    dl, dr = eng.gen_dev(g)
    eff = torch.randint(-1000, 1001, (K * N,), dtype=torch.int64, device="cuda")
    cl, cr = _abi.AgnLog(), _abi.AgnRead()
    C.memmove(C.addressof(cl), C.addressof(dl), C.sizeof(cl))
    C.memmove(C.addressof(cr), C.addressof(dr), C.sizeof(cr))
    cl.crdt_type = cr.req_type = _abi.COUNTER_PN
    cl.eff, cl.tag, cl.add_tok, cl.rem_off, cl.rem_tok = eff.data_ptr(), None, None, None, None
    res_c = eng.alloc_result(K, D, sparse=False)
    res_l = eng.alloc_result(K, D, sparse=False, cap_off=np.arange(K + 1, dtype=np.uint64))
    args = {"counter_general": (cl, cr, res_c), "lww_early": (dl, dr, res_l),
            "lww_late": (dl, dr, res_l)}

    def setenv(env):
        for k in KNOBS:
            if k in env:
                os.environ[k] = env[k]
            else:
                os.environ.pop(k, None)
        env_changed()
    names = list(VARIANTS)
    ms = {n: [] for n in names}
    got = {}
    for r in range(rounds + 1):  # round 0 warms every variant up and keeps its results
        for n in (names if r % 2 == 0 else names[::-1]):
            ls, rs, res = args[n]
            setenv(VARIANTS[n])
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record(st)
            eng.materialize(ls, rs, res, stream=sp)
            e.record(st)
            torch.cuda.synchronize()
            if r:
                ms[n].append(b.elapsed_time(e))
            else:
                got[n] = eng.fetch_result(res)
    setenv({})
    filt = ("hole", "lastct", "count")
    keep = np.uint32(_abi.F_NEWSS | _abi.F_CT_IGNORE)  # the filter's flags (not AGN_F_TS_TIE)
    ref = got["lww_early"]
    same = {n: all(np.array_equal(getattr(got[n], f), getattr(ref, f)) for f in filt) and
            np.array_equal(got[n].flags & keep, ref.flags & keep) for n in names}
    same["lww_late"] = same["lww_late"] and all(
        np.array_equal(getattr(got["lww_late"], f), getattr(ref, f))
        for f in ("flags", "out_n", "out_tag", "out_tok", "err_pos"))
    incl = float(got["lww_early"].count.sum()) / (K * N)
    per_key = 16 + 8 * D + 8 * D + 20
    per_op = {"counter_general": 8 * D + 8, "lww_early": 8 * D + 12, "lww_late": 8 * D + 12 * incl}
    extra = {"counter_general": 12, "lww_early": 32, "lww_late": 32}  # value | out_off pair, out_n, pair
    med = {n: float(np.median(x)) for n, x in ms.items()}
    byts = {n: K * N * per_op[n] + K * (per_key + extra[n]) for n in names}
    base = med["counter_general"]
    print(json.dumps({
        "keys": K, "ops_per_key": N, "D": D, "rounds": rounds, "included_fraction": incl,
        "ms_median": med, "ms_min": {n: float(min(x)) for n, x in ms.items()},
        "ms_max": {n: float(max(x)) for n, x in ms.items()},
        "bytes_per_op": per_op,
        "hbm_fraction_of_8TBs": {n: byts[n] / (med[n] * 1e-3) / PEAK for n in names},
        "vs_counter_general": {n: med[n] / base for n in names},
        "expected_ratio_early": (8 * D + 12) / (8 * D + 8) + 0.1,
        "results_equal": same}), flush=True)
    eng.free_gen(dl, dr)
    eng.close()


if __name__ == "__main__":
    main()
