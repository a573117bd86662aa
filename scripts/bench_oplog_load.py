"""Times agn_oplog_load (recovery: a device log into a pristine engine-owned op
log, device to device) on an agn_gen_dev counter log: K keys x N ops, D = 8
dense clocks, each rep into a fresh log.  Beside it, in the same process:

  (a) the only path before agn_oplog_load: the log copied to the host and
      pushed through agn_oplog_append + agn_oplog_flush, at a K small enough
      to finish (Ka = min(K, 20000)), per entry;
  (b) the box's copy rate: tools/libagn_probe.so agn_probe_copy, 1:1
      read:write (one-shot 4 KiB waves, non-temporal 16-byte accesses).

Bytes moved by the load = 2 x entries x (8 D + 20) + the per-key words.

  python scripts/bench_oplog_load.py [K] [N] [reps]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from antidote_amd import _abi  # noqa: E402
from antidote_amd.engine import Engine, OpLog  # noqa: E402

D = 8
PER_ENTRY = 8 * D + 8 + 8 + 4          # OpSSCommit row, txid, effect, op id
# per key: the index pass reads key_off[k], [k + 1] and writes five record
# words; the host's two segment-start words come back; the copy and key passes
# read seven words and key_off[k], and write key_off, key_len, key_id0, key_lcap
PER_KEY = 16 + 20 + 8 + 28 + 8 + 24


def gen(eng, K, N, seed=11):
    cfg = _abi.AgnGenCfg(crdt_type=_abi.COUNTER_PN, n_dcs=D, n_keys=K, ops_per_key=N, n_elems=1,
                         seed=seed, key_base=0, key_stride=1, warm=0)
    log, req = eng.gen_dev(cfg)
    eng.sync()
    return log, req


def probe_copy_gbs(eng, torch, nbytes=1 << 30):
    path = os.path.join(ROOT, "tools", "libagn_probe.so")
    if not os.path.exists(path):
        return None
    lib = C.CDLL(path)
    lib.agn_probe_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    src, dst = eng.empty(nbytes), eng.empty(nbytes)
    eng.lib.agn_memset_d(eng.ctx, src.ptr, 1, nbytes, None)
    rates = []
    for rep in range(2 + 5):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        if lib.agn_probe_copy(src.ptr, dst.ptr, nbytes, 4, None) != 0:
            return None
        e.record()
        torch.cuda.synchronize()
        if rep >= 2:
            rates.append(2 * (nbytes // 8192 * 8192) / (b.elapsed_time(e) * 1e-3) / 1e9)
    src.free()
    dst.free()
    return {"median": float(np.median(rates)), "min": min(rates), "max": max(rates)}


def host_path(eng, K, N):
    """(a): D2H of the log, agn_oplog_append of every entry, flush."""
    log, req = gen(eng, K, N, seed=12)
    E = K * N
    t0 = time.perf_counter()
    get = lambda p, dt, n: np.empty(n, dt) if not p else _d2h(eng, p, dt, n)  # noqa: E731
    oc = get(log.oc, np.uint64, E * D).reshape(E, D)
    eff = get(log.eff, np.int64, E)
    txid = get(log.txid, np.uint64, E) if log.txid else np.zeros(E, np.uint64)
    off = get(log.key_off, np.uint64, K + 1)
    t1 = time.perf_counter()
    keys = np.repeat(np.arange(K, dtype=np.uint64), np.diff(off).astype(np.int64))
    with OpLog(eng, _abi.COUNTER_PN, D, K, init_slots=N) as ol:
        t2 = time.perf_counter()
        ol.append(keys, oc, txid=txid, eff=eff)
        t3 = time.perf_counter()
        ol.flush()
        eng.sync()
        t4 = time.perf_counter()
    eng.free_gen(log, req)
    return {"keys": K, "entries": E, "d2h_ms": (t1 - t0) * 1e3, "append_ms": (t3 - t2) * 1e3,
            "flush_ms": (t4 - t3) * 1e3,
            "ns_per_entry": ((t1 - t0) + (t4 - t2)) * 1e9 / E}


def _d2h(eng, ptr, dt, n):
    out = np.empty(n, dt)
    eng.lib.agn_memcpy_d2h(eng.ctx, out.ctypes.data, ptr, out.nbytes, None)
    eng.sync()
    return out


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    import torch
    torch.cuda.init()
    eng = Engine(0)
    log, req = gen(eng, K, N)
    E = K * N
    wall, gpu = [], []
    for r in range(reps + 1):                      # the first rep warms the pool
        with OpLog(eng, _abi.COUNTER_PN, D, K, init_slots=N) as ol:
            eng.sync()
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            t0 = time.perf_counter()
            ol.load(log)                           # blocks until the load is done
            t1 = time.perf_counter()
            e.record()
            torch.cuda.synchronize()
            if r:
                wall.append((t1 - t0) * 1e3)
                gpu.append(b.elapsed_time(e))
            st = ol.stats()
            assert st["entries"] == E and st["slots"] == K * (N + 1), st
    eng.free_gen(log, req)
    moved = 2 * E * PER_ENTRY + K * PER_KEY
    ms, gms = float(np.median(wall)), float(np.median(gpu))
    probe = probe_copy_gbs(eng, torch)
    host = host_path(eng, min(K, 20000), N)
    load_gbs = moved / (ms * 1e-3) / 1e9
    out = {"keys": K, "ops_per_key": N, "n_dcs": D, "entries": E, "bytes_moved": moved,
           "load_wall_ms_median": ms, "load_wall_ms_all": wall,
           "load_gpu_ms_median": gms, "load_gpu_ms_all": gpu,
           "load_GBps_wall": load_gbs, "load_ns_per_entry": ms * 1e6 / E,
           "probe_copy_GBps": probe,
           "load_over_probe": load_gbs / probe["median"] if probe else None,
           "host_path": host,
           "host_path_over_load_per_entry": host["ns_per_entry"] / (ms * 1e6 / E),
           "note": "load_gpu_ms = events around the call on its stream; the call blocks and its "
                   "host phase (per-key records -> segment starts) lies between its two device "
                   "passes, so the events span it too"}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
