"""A/B of the counter_b kernel (k_bcounter, mat_bcounter.hip) against the
register_lww kernel (k_lww, mat_lww.hip) in one process, the two interleaved,
at cfg2's shape: 10M keys x 64 ops, D = 8, cold, generator data.  Both scan the
same clocks with the same filter (filter.hpp) and stream the same 8*D + 12
bytes per op (the rows, add_tok and tag, loaded with the rows); k_lww folds a
maximum in registers, k_bcounter a group-by-sum through its LDS slot table, so
the ratio is the fold's cost.  The log is agn_gen_dev's counter_b log with 1,
4, 16 and 64 distinct slots per key; k_lww reads the very same arrays as a
register_lww log (tag = value id, add_tok = timestamp).  A fifth run is warm
(the generator's base snapshot times) with base states of 4 pairs at 4 slots.
The filter outputs of the two kernels (hole, count, LastOpCt, NEWSS /
CT_IGNORE) must agree.

  python scripts/ab_bcounter.py [rounds] [keys]
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PEAK = 8.0e12  # HBM3E bytes/s (MI355X)
N, D = 64, 8
RUNS = [(1, False), (4, False), (16, False), (64, False), (4, True)]  # (slots, warm)


def result(torch, abi, K, cap):
    """An agn_result over torch buffers with `cap` pairs of room per request."""
    t = {"hole": torch.empty(K, dtype=torch.int64, device="cuda"),
         "lastct": torch.empty(K * D, dtype=torch.int64, device="cuda"),
         "count": torch.empty(K, dtype=torch.int32, device="cuda"),
         "flags": torch.empty(K, dtype=torch.int32, device="cuda"),
         "err_pos": torch.empty(K, dtype=torch.int32, device="cuda"),
         "out_off": torch.arange(K + 1, dtype=torch.int64, device="cuda") * cap,
         "out_n": torch.empty(K, dtype=torch.int32, device="cuda"),
         "out_tag": torch.empty(K * cap, dtype=torch.int32, device="cuda"),
         "out_tok": torch.empty(K * cap, dtype=torch.int64, device="cuda")}
    s = abi.AgnResult()
    for name, x in t.items():
        setattr(s, name, x.data_ptr())
    return s, t


def one_run(torch, abi, eng, K, slots, warm, rounds):
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    g = abi.AgnGenCfg(crdt_type=abi.COUNTER_B, n_dcs=D, n_keys=K, ops_per_key=N, n_elems=slots,
                      seed=20250113, key_base=0, key_stride=1, warm=1 if warm else 0)
    bl, br = eng.gen_dev(g)
    keep = []
    n_base = 0
    if warm:  # base states of 4 pairs (slots 0..3); k_lww takes the first as its pair
        n_base = 4
        boff = torch.arange(K + 1, dtype=torch.int64, device="cuda") * n_base
        btag = torch.arange(n_base, dtype=torch.int32, device="cuda").repeat(K)
        btok = torch.randint(-1000, 1001, (K * n_base,), dtype=torch.int64, device="cuda")
        keep = [boff, btag, btok]
        br.base_off, br.base_tag, br.base_tok = boff.data_ptr(), btag.data_ptr(), btok.data_ptr()
    ll, lr = abi.AgnLog(), abi.AgnRead()
    C.memmove(C.addressof(ll), C.addressof(bl), C.sizeof(ll))
    C.memmove(C.addressof(lr), C.addressof(br), C.sizeof(lr))
    ll.crdt_type = lr.req_type = abi.REGISTER_LWW
    res_b, tb = result(torch, abi, K, max(slots, n_base))
    res_l, tl = result(torch, abi, K, 1)
    args = {"bcounter": (bl, br, res_b), "lww": (ll, lr, res_l)}
    names = list(args)
    ms = {n: [] for n in names}
    for r in range(rounds + 1):  # round 0 warms both up
        for n in (names if r % 2 == 0 else names[::-1]):
            ls, rs, res = args[n]
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record(st)
            eng.materialize(ls, rs, res, stream=sp)
            e.record(st)
            torch.cuda.synchronize()
            if r:
                ms[n].append(b.elapsed_time(e))
    mask = abi.F_NEWSS | abi.F_CT_IGNORE
    same = all(bool(torch.equal(tb[f], tl[f])) for f in ("hole", "count", "lastct")) and \
        bool(torch.equal(tb["flags"] & mask, tl["flags"] & mask))
    bad = int((tb["flags"] & (abi.F_ERR_UNEXPECTED | abi.F_ERR_CAPACITY |
                              abi.F_ERR_CORRUPTED)).ne(0).sum())
    incl = float(tb["count"].sum()) / (K * N)
    pairs = float(tb["out_n"].sum()) / K
    med = {n: sorted(x)[len(x) // 2] for n, x in ms.items()}
    per_key = 16 + 8 * D + 8 * D + 20 + 16 + 4 + (8 * D if warm else 0)
    byts = {"bcounter": K * (N * (8 * D + 12) + per_key + 12 * pairs + 12 * n_base),
            "lww": K * (N * (8 * D + 12) + per_key + 12 + (12 if warm else 0))}
    out = {"slots": slots, "warm": warm, "included_fraction": incl, "pairs_per_key": pairs,
           "ms_median": med, "ms_min": {n: min(x) for n, x in ms.items()},
           "ms_max": {n: max(x) for n, x in ms.items()},
           "tb_per_s": {n: byts[n] / (med[n] * 1e-3) / 1e12 for n in names},
           "hbm_fraction_of_8TBs": {n: byts[n] / (med[n] * 1e-3) / PEAK for n in names},
           "bcounter_vs_lww": med["bcounter"] / med["lww"],
           "filter_outputs_equal": same, "failed_requests": bad}
    br.base_off = br.base_tag = br.base_tok = None  # torch's, not the generator's to free
    del tb, tl, keep
    eng.free_gen(bl, br)
    torch.cuda.empty_cache()
    return out


def main():
    import torch
    from antidote_amd import _abi
    from antidote_amd.engine import Engine
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    torch.cuda.set_device(0)
    eng = Engine(0)
    runs = [one_run(torch, _abi, eng, K, slots, warm, rounds) for slots, warm in RUNS]
    print(json.dumps({"keys": K, "ops_per_key": N, "D": D, "rounds": rounds,
                      "bytes_per_op": 8 * D + 12, "runs": runs}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
