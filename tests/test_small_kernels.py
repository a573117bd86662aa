"""The constructed cases of tests/small_kernels.py through the HIP kernels,
every output array against the C oracle bit for bit
(tests/test_small_kernels_cpu.py checks the oracle against the dict
transcriptions on the same cases and that each named edge is reached).

agn_log_ingest: every case with op_id_base 0 and out_totals, then with base 1
and without; the output buffers are pre-filled, so a key offset the kernels
did not write shows.  agn_gst_min: the vector BEFORE finalize (what crosses
RCCL), then agn_gst_finalize, then agn_gst_scalar on top of both, under the
unroll / non-temporal / band knobs, with `defined` given and NULL.
agn_dep_check: both staging forms on either side of the 48 KiB limit, every
group width, partly live last tiles, and rows that name an unknown partition."""
import ctypes as C

import numpy as np
import pytest

import small_kernels as sk
from antidote_amd import _abi
from test_edges import scratch
from test_ingest import log_struct_of, oracle_ingest
from test_next_rows import dep_oracle, ptr

pytestmark = pytest.mark.gpu

U64 = sk.U64
INGEST = sk.ingest_cases()
REC_FIELDS = ("kind", "txid", "key", "commit_dc", "commit_time", "ss", "ss_mask", "eff", "tag",
              "add_tok", "rem_off", "rem_tok")
FILL = 0xA5


# ====================================================================== ingest
def run_ingest(eng, rc, base, with_totals):
    """agn_log_ingest over device arrays pre-filled with 0xA5 bytes ->
    (arrays, totals or None)."""
    dev = {f: eng.upload(getattr(rc, f)) for f in REC_FIELDS if getattr(rc, f) is not None}
    rs = rc.struct({f: b.ptr for f, b in dev.items()})
    outs = {}
    for f, a in rc.out_arrays().items():
        if a is not None:
            a = np.ascontiguousarray(a)
            fill = np.full(max(a.nbytes, 8), FILL, np.uint8)
            outs[f] = (eng.upload(fill), a.dtype, a.shape)
    os_ = log_struct_of({f: b.ptr for f, (b, _, _) in outs.items()})
    mt = eng.upload(rc.max_t) if rc.max_t is not None else None
    mm = eng.upload(rc.max_m) if rc.max_m is not None else None
    tot = eng.upload(np.full(16, FILL, np.uint8)) if with_totals else None
    rcode = eng.lib.agn_log_ingest(eng.ctx, C.byref(rs), rc.crdt, rc.D, rc.K,
                                   mt.ptr if mt else None, mm.ptr if mm else None, base,
                                   C.byref(os_), tot.ptr if tot else None, None)
    assert rcode == 0, eng.lib.agn_last_error()
    eng.sync()
    got = {f: eng.download(b, dt, shape) for f, (b, dt, shape) in outs.items()}
    return got, (eng.download(tot, np.uint64, (2,)) if tot else None)


@pytest.mark.parametrize("name", list(INGEST))
def test_ingest_edges(eng, oracle_lib, name):
    rc = INGEST[name]
    for base, with_totals in ((0, True), (1, False)):
        want, n_out = oracle_ingest(oracle_lib, rc, base)
        with scratch(eng):
            got, totals = run_ingest(eng, rc, base, with_totals)
        # the key offsets are complete: every word written, the last one n_out
        assert np.array_equal(got["key_off"], want["key_off"]), (name, base)
        assert int(got["key_off"][rc.K]) == n_out
        nr = int(want["rem_off"][n_out]) if "rem_off" in want else 0
        if with_totals:
            assert [int(x) for x in totals] == [n_out, nr]
        for f, g in got.items():
            w = want[f]
            m = {"key_off": len(w), "rem_off": n_out + 1, "rem_tok": nr}.get(f, n_out)
            assert np.array_equal(g[:m], w[:m]), (name, base, f)


# ====================================================================== GST
def gst_knobs(monkeypatch, unroll, nt, blocks):
    monkeypatch.setenv("AGN_GST_UNROLL", str(unroll))
    if nt:
        monkeypatch.delenv("AGN_GST_NT", raising=False)
    else:
        monkeypatch.setenv("AGN_GST_NT", "0")
    if blocks:
        monkeypatch.setenv("AGN_GST_BLOCKS", str(blocks))
    else:
        monkeypatch.delenv("AGN_GST_BLOCKS", raising=False)


def oracle_vec(lib, c, finalize):
    out = np.zeros((c.E, c.D + 1), np.uint64)
    assert lib.oracle_gst_min(c.D, c.P, c.E, c.clocks.ctypes.data, ptr(c.defined),
                              out.ctypes.data, finalize) == 0
    return out


def oracle_scalar(lib, c, vec):
    v, g = vec.copy(), np.zeros(c.E, np.uint64)
    assert lib.oracle_gst_scalar(c.D, c.E, ptr(v), ptr(g)) == 0
    return v, g


def run_gst(eng, oracle_lib, c):
    """agn_gst_min before finalize, agn_gst_finalize, and agn_gst_scalar on a
    copy of each, all against the oracle."""
    D, P, E = c.D, c.P, c.E
    shape = (E, D + 1)
    with scratch(eng):
        if c.offset8:   # the clocks start 8 bytes into their (16-byte aligned) buffer
            buf = eng.upload(np.concatenate([np.full(1, 0x5A5A, np.uint64), c.clocks.ravel()]))
            assert buf.ptr % 16 == 0
            cptr = buf.ptr + 8
        else:
            cptr = eng.upload(c.clocks).ptr
            assert cptr % 16 == 0
        dd = eng.upload(c.defined) if c.defined is not None else None
        out = eng.upload(np.full(E * (D + 1), 0xA5A5A5A5A5A5A5A5, np.uint64))
        eng.gst_min(D, P, E, cptr, dd.ptr if dd else None, out.ptr)
        pre = eng.download(out, np.uint64, shape)
        want_pre = oracle_vec(oracle_lib, c, 0)
        assert np.array_equal(pre, want_pre), (c.name, "before finalize",
                                               np.argwhere(pre != want_pre)[:4].tolist())
        sc, sg = eng.upload(pre), eng.empty(E * 8)
        eng.gst_scalar(D, E, sc.ptr, sg.ptr)
        wv, wg = oracle_scalar(oracle_lib, c, want_pre)
        assert np.array_equal(eng.download(sc, np.uint64, shape), wv), (c.name, "scalar")
        assert np.array_equal(eng.download(sg, np.uint64, (E,)), wg), (c.name, "scalar gst")
        eng.gst_finalize(D, E, out.ptr)
        fin = eng.download(out, np.uint64, shape)
        want_fin = oracle_vec(oracle_lib, c, 1)
        assert np.array_equal(fin, want_fin), (c.name, "after finalize")
        eng.gst_scalar(D, E, out.ptr, sg.ptr)
        wv, wg = oracle_scalar(oracle_lib, c, want_fin)
        assert np.array_equal(eng.download(out, np.uint64, shape), wv), (c.name, "scalar, final")
        assert np.array_equal(eng.download(sg, np.uint64, (E,)), wg), (c.name, "scalar gst, final")


@pytest.mark.parametrize("null_defined", [False, True], ids=["defined", "null"])
@pytest.mark.parametrize("single_band", [False, True], ids=["bands", "oneband"])
@pytest.mark.parametrize("unroll,nt", [(4, True), (8, True), (4, False), (8, False)])
@pytest.mark.parametrize("D", sk.COL_WIDTHS)
def test_gst_column_kernel(eng, oracle_lib, monkeypatch, D, unroll, nt, single_band, null_defined):
    """k_gst_cols<DEF, U, NT> at every width: P on the block-step, unroll and
    band boundaries, E = 1 and 3."""
    for c in sk.gst_col_cases(D, unroll, nt, null_defined, single_band):
        gst_knobs(monkeypatch, unroll, nt, c.blocks)
        run_gst(eng, oracle_lib, c)


@pytest.mark.parametrize("null_defined", [False, True], ids=["defined", "null"])
@pytest.mark.parametrize("D", sk.GEN_WIDTHS)
def test_gst_general_kernel(eng, oracle_lib, monkeypatch, D, null_defined):
    gst_knobs(monkeypatch, 4, True, None)
    for c in sk.gst_general_cases(D, null_defined):
        run_gst(eng, oracle_lib, c)


def test_gst_misaligned_clocks(eng, oracle_lib, monkeypatch):
    """An even D dividing 512 whose clocks are only 8-byte aligned."""
    gst_knobs(monkeypatch, 4, True, None)
    for c in sk.gst_misaligned_cases():
        run_gst(eng, oracle_lib, c)


@pytest.mark.parametrize("unroll", [4, 8])
def test_gst_all_undefined(eng, oracle_lib, monkeypatch, unroll):
    gst_knobs(monkeypatch, unroll, True, None)
    for c in sk.gst_undefined_cases():
        run_gst(eng, oracle_lib, c)


@pytest.mark.parametrize("D", [0, 4097])
def test_gst_unsupported_width(eng, D):
    """AGN_ENOTSUP before anything is launched: the output is untouched."""
    with scratch(eng):
        guard = np.full(8, 0xA5A5A5A5A5A5A5A5, np.uint64)
        out, clocks = eng.upload(guard), eng.upload(np.zeros(2 * 4097, np.uint64))
        rc = eng.lib.agn_gst_min(eng.ctx, D, 2, 1, clocks.ptr, None, out.ptr, None)
        assert rc == _abi.ENOTSUP
        eng.sync()
        assert np.array_equal(eng.download(out, np.uint64, (8,)), guard)


# ====================================================================== dep check
DEP = sk.dep_cases()


def run_dep(eng, c, arrays, n):
    bufs = [eng.upload(x) if x is not None else None for x in arrays]
    out = eng.upload(np.full(max(n, 8), FILL, np.uint8))
    eng.dep_check(c.D, n, *[b.ptr if b is not None else None for b in bufs[:4]], c.P,
                  bufs[4].ptr, bufs[5].ptr if bufs[5] is not None else None, out.ptr)
    return eng.download(out, np.uint8, (n,))


@pytest.mark.parametrize("c", DEP, ids=[c.name for c in DEP])
def test_dep_check_edges(eng, oracle_lib, c):
    with scratch(eng):
        got = run_dep(eng, c, c.arrays(), c.n)
    if c.bad.any():
        # an unknown partition (part[t] >= n_parts): out_ok = 0; the other
        # rows as the oracle on them alone
        assert not got[c.bad].any()
        want = dep_oracle(oracle_lib, c.D, *c.good_rows())
        assert np.array_equal(got[~c.bad], want)
        with scratch(eng):
            assert np.array_equal(run_dep(eng, c, c.good_rows(), int((~c.bad).sum())), want)
    else:
        assert np.array_equal(got, dep_oracle(oracle_lib, c.D, *c.arrays()))
