"""The constructed cases of tests/small_kernels.py without a GPU:

* the C oracle against the literal dict transcriptions (test_ingest's
  py_filter_terms, py_oracle's get_min_time / scalar_stable_time /
  dependencies_satisfied) on every case where that is affordable;
* attainment: each edge a case names is really reached -- a probe chain of 40
  and a wrap in the commit table, the txid 2^64 - 1 sharing its slot, an
  update committed by its txid's second commit record, the row a GST minimum
  sits in for the block step, unroll and bands in force, the staging limit of
  the dependency check ... -- so a builder change that loses an edge fails
  here instead of passing vacuously on the GPU;
* determinism: building twice gives identical arrays.

The slot function and launch plans used for attainment mirror
antidote_amd/csrc/ingest.hip and gst.hip (see small_kernels.py)."""
import numpy as np
import pytest

import small_kernels as sk
from antidote_amd import _abi
from oracle import py_oracle as po
from test_ingest import oracle_ingest, py_filter_terms, vc
from test_next_rows import as_dict, dep_oracle, ptr

U64 = sk.U64
INGEST = sk.ingest_cases()


# ====================================================================== ingest
def check_against_dict(rc, out, n_out, want):
    """test_ingest's comparison of the oracle's arrays with the dict walk."""
    D, sparse = rc.D, rc.sparse
    assert n_out == sum(len(v) for v in want.values())
    assert int(out["key_off"][0]) == 0 and int(out["key_off"][rc.K]) == n_out
    for k in range(rc.K):
        a, b = int(out["key_off"][k]), int(out["key_off"][k + 1])
        lst = want.get(k, [])
        assert b - a == len(lst), k
        for j, (u, oc) in enumerate(lst):
            e = a + j
            assert int(out["op_id"][e]) == j
            assert int(out["txid"][e]) == int(rc.txid[u])
            got = vc(out["oc"][e], None if out["oc_mask"] is None else out["oc_mask"][e], D)
            assert got == (oc if sparse else {d: oc.get(d, 0) for d in range(D)})
            if rc.crdt == _abi.COUNTER_PN:
                assert int(out["eff"][e]) == int(rc.eff[u])
            else:
                assert int(out["tag"][e]) == int(rc.tag[u])
                assert int(out["add_tok"][e]) == int(rc.add_tok[u])
                r0, r1 = int(out["rem_off"][e]), int(out["rem_off"][e + 1])
                assert list(out["rem_tok"][r0:r1]) == \
                    list(rc.rem_tok[int(rc.rem_off[u]):int(rc.rem_off[u + 1])])


def emitted_updates(want):
    return sorted(u for lst in want.values() for u, _ in lst)


def first_later_commit(rc, u):
    t = rc.txid[u]
    for x in range(u + 1, rc.n):
        if rc.kind[x] == _abi.REC_COMMIT and rc.txid[x] == t:
            return x
    return None


def ingest_reached(oracle_lib, rc, out, n_out, want):
    """One assertion block per edge name of small_kernels' ingest cases."""
    E = set(rc.edges)
    em = emitted_updates(want)
    ups = np.flatnonzero(rc.kind == _abi.REC_UPDATE)
    lens = np.diff(out["key_off"].astype(np.int64))
    if "wide" in E:
        mode = rc.edges[1]
        cm = rc.kind == _abi.REC_COMMIT
        pres = sk.domain.present_bits(rc.ss_mask, rc.n, rc.D) & cm[:, None]
        v = rc.ss[pres]
        if v.size:
            lo, hi = int(v.min()), int(v.max())
            if mode == "carry32":
                assert lo < sk.domain.B32 <= hi or lo == hi == sk.domain.B32
            elif mode == "sign64":
                assert lo < sk.domain.B63 <= hi or lo == hi == sk.domain.B63
            elif mode == "top":
                mx = [int(rc.max_t[sk.domain.present_bits(rc.max_m, rc.K, rc.D)].max())] \
                    if rc.max_t is not None else []
                assert max([hi, int(rc.commit_time[cm].max())] + mx) == sk.TOP
            elif mode == "zero":
                assert lo == 0
            else:
                # the order lives in the high words, the low words run against it
                assert mode == "hi32" and hi >= 1 << 32
                assert lo == hi or (hi >> 32 > lo >> 32 and hi & 0xFFFFFFFF < lo & 0xFFFFFFFF)
        if rc.eff is not None and rc.n >= 8:
            assert int(rc.eff.max()) == sk.domain.INT64_MAX
            assert int(rc.eff.min()) == sk.domain.INT64_MIN + 1
        if rc.eff is None and rc.n >= 8:
            assert int(rc.tag.max()) == 0xFFFFFFFE
            assert int(rc.add_tok.max()) >= 1 << 63
            if int(rc.rem_off[-1]):
                assert int(rc.rem_tok.max()) >= 1 << 63
        base = INGEST[rc.name.split("/")[0]]
        # an increasing map keeps every check_max_time decision, but for a present
        # 0 against a DC that Max lacks (dc_words' transaction 801)
        if mode != "zero" and "absent_dc" not in base.meta:
            assert n_out == oracle_ingest(oracle_lib, base, 0)[1]
        return
    if "slot_chain" in E:
        T, slots = rc.table()
        assert T == 256
        count = {s: slots.count(s) for s in set(slots)}
        assert max(count.values()) >= 40                     # a chain of at least 40
        assert count.get(T - 1, 0) >= 40                     # ... and one that wraps to slot 0
        assert count.get(100, 0) and count.get(101, 0)       # two chains that merge
        loose = {int(rc.txid[u]) for u in ups} - {int(rc.txid[c]) for c in rc.commits()}
        assert {sk.slot_of(t, T) for t in loose} >= {5, T - 1, 100}
        if rc.max_t is None:
            assert n_out == sum(1 for u in ups if first_later_commit(rc, u) is not None)
        assert n_out > 100
    if "txid_top" in E:
        T, slots = rc.table()
        assert T == rc.meta["T"] and slots.count(rc.meta["alias_slot"]) >= 7
        assert sk.slot_of(U64, T) == rc.meta["alias_slot"]
        got = [int(rc.txid[u]) for u in em]
        for t in sk.TOP_TXIDS:
            assert int((rc.txid == np.uint64(t)).sum()) == 4
            if rc.max_t is None:
                assert got.count(t) == 3, hex(t)
        assert got.count(U64) >= 1
    if "txid_reuse" in E:
        commits_of = {}
        for c in rc.commits():
            commits_of.setdefault(int(rc.txid[c]), []).append(int(c))
        assert sum(len(v) >= 2 for v in commits_of.values()) >= 4
        second = [u for u in ups if any(c < u for c in commits_of.get(int(rc.txid[u]), []))]
        assert len(second) >= 8
        if rc.max_t is None:
            # u c u c: the later updates wait for the later commit record
            assert sum(u in em for u in second) >= 6
            assert set(em) == {int(u) for u in ups if first_later_commit(rc, u) is not None
                               and rc.key[u] < rc.K}
        # an update after its txid's last commit is never emitted
        assert any(first_later_commit(rc, u) is None and int(rc.txid[u]) in commits_of
                   for u in ups)
        # a commit record before any update of its txid
        assert any(not any(u < c and rc.txid[u] == rc.txid[c] for u in ups)
                   for v in commits_of.values() if len(v) >= 2 for c in v[:1])
        # two commit records with no update between them
        assert any(not any(a < u < b and rc.txid[u] == np.uint64(t) for u in ups)
                   for t, v in commits_of.items() for a, b in zip(v, v[1:]))
        assert max(len({int(rc.key[u]) for u in ups if rc.txid[u] == np.uint64(t)})
                   for t in commits_of) >= 4
    if "order" in E:
        tx = [int(t) for t in out["txid"][:n_out]]
        ko = out["key_off"].astype(np.int64)
        assert tx[ko[0]:ko[1]] == [13, 12, 12, 11, 14]      # commit order, not first-update order
        assert tx[ko[1]:ko[2]] == [11]
        assert tx[ko[2]:ko[3]] == [21] * 3 + [20] * 9       # many updates of one key, stable
        assert tx[ko[3]:ko[4]] == [30, 31]                  # back-to-back commits of one key
        k2 = [u for u, _ in want[2]]
        assert k2 == sorted(k2[:3]) + sorted(k2[3:]) and k2[0] > k2[3]
    if "sizes" in E:
        tags = {e for e in E if e != "sizes"}
        for e in tags:
            if e.startswith("n="):
                assert rc.n == int(e[2:])
            elif e.startswith("n_keys="):
                assert rc.K == int(e[7:]) and (rc.K == 1 or (lens > 0).sum() > 1)
            elif e == "no_commit":
                assert not len(rc.commits()) and len(ups) and n_out == 0
            elif e == "only_commits":
                assert len(rc.commits()) == rc.n > 0 and n_out == 0
            elif e == "all_foreign":
                assert len(ups) and (rc.key[ups] >= rc.K).all() and len(rc.commits()) and \
                    n_out == 0
            else:
                assert e == "all_refused" and n_out == 0
                mt, rc.max_t = rc.max_t, None
                try:
                    assert oracle_ingest(oracle_lib, rc, 0)[1] > 50
                finally:
                    rc.max_t = mt
        assert tags
    if "key_gaps" in E:
        nz = np.flatnonzero(lens)
        if "only_key_0" in E:
            assert list(nz) == [0]
        elif "only_last_key" in E:
            assert list(nz) == [rc.K - 1]
        elif "every_97th" in E:
            assert len(nz) > 10 and (nz % 97 == 0).all()
        else:
            assert "run_of_1000" in E and not lens[500:1500].any() and lens[:500].any() and \
                lens[1500:].any()
    if "rem_lists" in E:
        ll = rc.rem_off.astype(np.int64)
        in_len = np.diff(ll)
        out_len = np.diff(out["rem_off"][:n_out + 1].astype(np.int64))
        assert n_out > 0
        if "all_empty" in E:
            assert int(rc.rem_off[-1]) == 0 and int(out["rem_off"][n_out]) == 0
        else:
            assert set(sk.REM_LENS) <= set(out_len.tolist())
            assert in_len[rc.commits()].min() >= 70            # lists on commit records
            dropped = [u for u in ups if u not in set(em)]
            assert dropped and all(in_len[u] == 100 for u in dropped)
            assert int(out["rem_off"][n_out]) == int(in_len[em].sum()) < int(in_len.sum())
    if "dc_words" in E:
        D = rc.D
        assert f"D={D}" in E
        cds = {c for c in sk.COMMIT_DCS + (D - 1,) if c < D}
        used = {int(rc.commit_dc[first_later_commit(rc, u)]) for u in em}
        assert used == cds, (used, cds)
        assert n_out >= 4
        if rc.sparse:
            gained = 0
            for u in em:
                c = first_later_commit(rc, u)
                cd = int(rc.commit_dc[c])
                gained += not (int(rc.ss_mask[c, cd >> 6]) >> (cd & 63)) & 1
            assert gained or D == 1     # OpSSCommit gains the commit DC's bit
            a, cx = rc.meta["absent_dc"], rc.meta["commits"]
            assert not (int(rc.max_m[1, a >> 6]) >> (a & 63)) & 1
            k1 = {int(rc.txid[u]) for u, _ in want.get(1, [])}
            k2 = {int(rc.txid[u]) for u, _ in want.get(2, [])}
            assert {801, 802, 803} <= k2
            if D > 1:
                assert {801, 803} <= k1 and 802 not in k1
            assert int(rc.ss[cx[0], a]) == 0 and int(rc.ss[cx[1], a]) != 0
            # garbage in absent columns
            pres = sk.domain.present_bits(rc.ss_mask, rc.n, D)
            assert D == 1 or (rc.ss[~pres] >= np.uint64(1 << 61)).all()


@pytest.mark.parametrize("name", list(INGEST))
def test_ingest_oracle_vs_dict_and_edges(oracle_lib, name):
    rc = INGEST[name]
    for base in (0, 1):
        out, n_out = oracle_ingest(oracle_lib, rc, base)
        want = py_filter_terms(rc)
        if base:
            assert (out["op_id"][:n_out] >= 1).all()
            out["op_id"][:n_out] -= 1
        check_against_dict(rc, out, n_out, want)
    assert rc.edges
    ingest_reached(oracle_lib, rc, out, n_out, want)


def test_ingest_edge_names_all_built():
    names = {e for c in INGEST.values() for e in c.edges}
    assert names >= {"slot_chain", "txid_top", "txid_reuse", "order", "sizes", "key_gaps",
                     "rem_lists", "dc_words", "wide", "no_commit", "only_commits", "all_foreign",
                     "all_refused", "only_key_0", "only_last_key", "every_97th", "run_of_1000",
                     "long_lists", "all_empty"} | set(sk.WIDE_MODES) | \
        {f"n={n}" for n in sk.SIZES_N} | {f"n_keys={k}" for k in sk.SIZES_K} | \
        {f"D={d}" for d in sk.DC_WIDTHS}
    assert any(c.crdt == t and "rem_lists" in c.edges for c in INGEST.values()
               for t in (_abi.SET_AW,)) and \
        any(c.crdt == _abi.REGISTER_MV and "rem_lists" in c.edges for c in INGEST.values())


def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return a is not None and b is not None and a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def test_ingest_builders_deterministic():
    again = sk.ingest_cases()
    assert list(again) == list(INGEST)
    for name, c in INGEST.items():
        d = again[name]
        for f, v in c.__dict__.items():
            assert same(v, d.__dict__[f]), (name, f)


# ====================================================================== GST
def gst_oracle(lib, c, finalize):
    out = np.zeros((c.E, c.D + 1), np.uint64)
    assert lib.oracle_gst_min(c.D, c.P, c.E, c.clocks.ctypes.data, ptr(c.defined),
                              out.ctypes.data, finalize) == 0
    return out


def gst_transcription(c):
    """get_min_time over {partition -> dict | undefined}, per epoch."""
    rows = []
    for e in range(c.E):
        parts = {}
        for p in range(c.P):
            if c.defined is not None and not c.defined[e, p]:
                parts[p] = po.UNDEFINED
            else:
                r = c.clocks[e, p]
                parts[p] = {int(d): int(r[d]) for d in np.flatnonzero(r != np.uint64(U64))}
        rows.append(po.get_min_time(parts))
    return rows


def gst_check(lib, c, reached, budget=60_000):
    pre, fin = gst_oracle(lib, c, 0), gst_oracle(lib, c, 1)
    pl = c.plan
    dfn = np.ones((c.E, c.P), bool) if c.defined is None else c.defined.astype(bool)
    for e in range(c.E):
        anyd, alld = dfn[e].any(), dfn[e].all()
        assert int(pre[e, c.D]) == int(alld)
        for d in range(c.D):
            role, name = int(c.role[e, d]), c.ROLES[int(c.role[e, d])]
            got = int(pre[e, d])
            if role == 5 or not anyd:
                assert got == U64, (c.name, e, d)
                reached.add("absent_everywhere" if role == 5 else "all_undefined")
                if not anyd and c.P == 1:
                    reached.add("p1_undefined")
                continue
            if role == 6:
                assert got == U64 and (alld or (c.clocks[e, ~dfn[e], d] == 0).all())
                if not alld:
                    reached.add(name)
                continue
            mv = int(c.minval[e, d])
            assert got == mv, (c.name, e, d)
            assert int(fin[e, d]) == (mv if alld else 0)
            if mv > 0 and not alld:   # an undefined partition's clock is below the minimum
                assert (c.clocks[e, ~dfn[e], d] == 0).all()
                reached.add("undefined_below_min")
            reached.add(f"value_{mv:#x}")
            if role == 7:
                reached.add(name)
                continue
            r = int(c.minrow[e, d])
            assert dfn[e, r] and int(c.clocks[e, r, d]) == mv
            others = np.delete(c.clocks[e, :, d][dfn[e]], int(dfn[e, :r].sum()))
            assert not others.size or int(others.min()) > mv or mv == sk.TOP
            if name == "min_first_row":
                assert r == 0
            elif name == "min_last_row":
                assert r == c.P - 1
                if pl["bands"] > 1 and c.P - (pl["bands"] - 1) * pl["rows"] == 1:
                    reached.add("single_row_last_band")
            elif name == "min_middle":
                assert r == c.P // 2
            if pl["kernel"] == "cols":
                band, loop, k, last = sk.classify_row(pl, c.P, r)
                assert band == r // pl["rows"] < pl["bands"]
                if name == "min_unrolled_last":
                    assert (loop, k, last) == ("unrolled", pl["U"] - 1, True)
                elif name == "min_tail_loop":
                    assert loop == "tail"
                reached.add(f"{loop}_loop")
            reached.add(name)
    if c.P * c.D * c.E <= budget:
        for e, want in enumerate(gst_transcription(c)):
            assert {d: int(fin[e, d]) for d in range(c.D) if int(fin[e, d]) != U64} == want
    # the scalar GST of both vectors against its restatement
    for vec in (pre, fin):
        v, g = vec.copy(), np.zeros(c.E, np.uint64)
        assert lib.oracle_gst_scalar(c.D, c.E, ptr(v), ptr(g)) == 0
        for e in range(c.E):
            want = po.scalar_stable_time({d: int(vec[e, d]) for d in range(c.D)
                                          if int(vec[e, d]) != U64})
            assert {d: int(v[e, d]) for d in range(c.D) if int(v[e, d]) != U64} == want
            assert int(g[e]) == (min(want.values()) if want else U64)


ROLE_EDGES = {"min_first_row", "min_last_row", "min_unrolled_last", "min_tail_loop", "min_middle",
              "absent_everywhere", "min_everywhere"}
VALUE_EDGES = {f"value_{v:#x}" for v in sk.SPECIAL}


@pytest.mark.parametrize("null_defined", [False, True], ids=["defined", "null"])
@pytest.mark.parametrize("single_band", [False, True], ids=["bands", "oneband"])
@pytest.mark.parametrize("unroll", [4, 8])
@pytest.mark.parametrize("D", sk.COL_WIDTHS)
def test_gst_column_cases(oracle_lib, D, unroll, single_band, null_defined):
    cases = sk.gst_col_cases(D, unroll, True, null_defined, single_band)
    RG = 512 // D
    want_p = {1, RG - 1, RG, RG + 1, unroll * RG - 1, unroll * RG, unroll * RG + 1, 32 * RG - 1,
              32 * RG, 32 * RG + 1, 3 * 32 * RG + 1} - {0}
    assert {c.P for c in cases} == want_p and {c.E for c in cases} == {1, 3}
    reached = set()
    for c in cases:
        pl = c.plan
        assert pl["kernel"] == "cols" and pl["RG"] == RG and pl["U"] == unroll
        if single_band:
            assert pl["bands"] == 1
        elif c.P == 3 * 32 * RG + 1:     # several bands, the last one a single row
            assert pl["bands"] == 4 and pl["rows"] == 32 * RG and c.P - 3 * pl["rows"] == 1
            reached.add("multi_band")
        assert (c.defined is None) == null_defined
        if not null_defined and c.E == 3 and c.P > 8:
            assert len({c.defined[e].tobytes() for e in range(3)}) == 3   # a pattern per epoch
        gst_check(oracle_lib, c, reached)
    want = set(ROLE_EDGES) | {"unrolled_loop", "tail_loop"}
    if D >= 8:
        want |= VALUE_EDGES
    if not single_band:
        want |= {"multi_band", "single_row_last_band"}
    if not null_defined:
        want |= {"undefined_below_min"} | ({"only_undefined"} if D >= 8 else set())
    if D < 8:   # columns (3 d + e) mod 8 of two or four DCs over three epochs
        want -= {"min_everywhere"} if D == 2 else set()
    assert want <= reached, sorted(want - reached)


@pytest.mark.parametrize("null_defined", [False, True], ids=["defined", "null"])
@pytest.mark.parametrize("D", sk.GEN_WIDTHS)
def test_gst_general_cases(oracle_lib, D, null_defined):
    cases = sk.gst_general_cases(D, null_defined)
    r = max(2048 // D, 1)
    assert {c.P for c in cases} == {p for p in (1, r - 1, r, r + 1, 2 * r + 1) if p >= 1}
    reached = set()
    for c in cases:
        assert c.plan["kernel"] == "general" and c.plan["rows"] == r
        if c.P == 2 * r + 1:
            assert c.plan["bands"] == 3
            reached.add("multi_band")
        gst_check(oracle_lib, c, reached, budget=30_000)
    want = {"multi_band", "single_row_last_band", "min_first_row", "min_last_row"}
    if D >= 8:
        want |= VALUE_EDGES | {"min_middle", "absent_everywhere", "min_everywhere"}
    assert want <= reached, sorted(want - reached)


def test_gst_misaligned_and_undefined_cases(oracle_lib):
    reached = set()
    mis = sk.gst_misaligned_cases()
    assert {c.D for c in mis} == {2, 8, 256}
    for c in mis:   # an even D dividing 512 whose pointer is 8 bytes off: the general kernel
        assert 512 % c.D == 0 and c.D % 2 == 0 and c.offset8 and c.plan["kernel"] == "general"
        assert sk.gst_plan(c.D, c.P, c.E)["kernel"] == "cols"
        gst_check(oracle_lib, c, reached)
    und = sk.gst_undefined_cases()
    for c in und:
        assert not c.defined.any()
        pre = gst_oracle(oracle_lib, c, 0)
        assert (pre[:, :c.D] == np.uint64(U64)).all() and not pre[:, c.D].any()
        assert (c.clocks != np.uint64(U64)).any()
        gst_check(oracle_lib, c, reached)
    assert {"all_undefined", "p1_undefined", "single_row_last_band"} <= reached
    assert {c.plan["kernel"] for c in und} == {"cols", "general"}


def test_gst_builders_deterministic():
    for a, b in zip(sk.gst_col_cases(8, 4, True, False, False) + sk.gst_general_cases(5, False),
                    sk.gst_col_cases(8, 4, True, False, False) + sk.gst_general_cases(5, False)):
        assert a.name == b.name and same(a.clocks, b.clocks) and same(a.defined, b.defined)


# ====================================================================== dep check
DEP = sk.dep_cases()


@pytest.mark.parametrize("c", DEP, ids=[c.name for c in DEP])
def test_dep_oracle_vs_dict_and_edges(oracle_lib, c):
    D, E = c.D, set(c.edges)
    deps, dm, origin, part, pc, pm = c.arrays()
    if c.bad.any():   # the oracle refuses the batch; the known rows alone
        ok = np.zeros(c.n, np.uint8)
        assert oracle_lib.oracle_dep_check(D, c.n, ptr(deps), ptr(dm), ptr(origin), ptr(part),
                                           c.P, ptr(pc), ptr(pm), ptr(ok)) == _abi.EINVAL
        assert (part[c.bad] >= c.P).all() and (part[~c.bad] < c.P).all()
        assert 0 < c.bad.sum() < c.n and {int(x) for x in part[c.bad]} == {c.P, 0xFFFFFFFF}
        deps, dm, origin, part, pc, pm = c.good_rows()
    got = dep_oracle(oracle_lib, D, deps, dm, origin, part, pc, pm)
    for t in range(len(origin)):
        want = po.dependencies_satisfied(
            int(origin[t]), as_dict(deps[t], None if dm is None else dm[t], D),
            as_dict(pc[part[t]], None if pm is None else pm[part[t]], D))
        assert bool(got[t]) == want, t
    G = sk.dep_group(D)
    tpw = 64 // G
    assert G >= min(D, 64) and (G == 1 or G // 2 < D)
    ok = np.ones(c.n, np.uint8)
    ok[~c.bad] = got
    pres = sk.domain.present_bits(c.dm, c.n, D)
    live = c.ahead & pres[np.arange(c.n), c.col] & ~c.bad
    exempt = c.origin.astype(np.int64) == c.col
    assert not ok[live & ~exempt].any() and ok[live & exempt].all() or D == 1
    if "tile_tail" in E:
        assert c.n in {1, tpw - 1, tpw, tpw + 1, 5 * tpw + 1}
    if c.n >= 60:
        assert 0 < got.mean() < 1
        assert {0, D - 1} <= {int(o) for o in c.origin} and (c.origin >= D).sum() > 10
        assert (live & exempt).sum() > 3                       # the origin column is exempt
        assert (live & (c.origin >= D)).sum() > 3              # an origin >= D exempts nothing
        assert (live & ~exempt & (c.col == c.last_lane)).sum() > 3   # the group's last lane
        assert c.last_lane == (D - 1 if D <= 64 else 127 if D >= 128 else 63)
    if "stage_limit" in E:
        lo, hi = sk.dep_stage_pair(D, c.sparse)
        assert c.P in (lo, hi)
        assert sk.dep_stage_bytes(D, lo, c.sparse) <= sk.DEP_LDS < sk.dep_stage_bytes(D, hi,
                                                                                     c.sparse)
        assert int(c.part.max()) == c.P - 1      # the last staged words are read
    if "wide" in E:
        v = c.deps[pres]
        B = sk.domain.B32 if "carry32" in c.name else sk.domain.B63
        assert int(v.min()) < B <= int(v.max())


def test_dep_edge_names_all_built():
    assert {e for c in DEP for e in c.edges} == {"group_width", "tile_tail", "origin", "last_lane",
                                                 "stage_limit", "wide", "bad_part"}
    assert {c.D for c in DEP if "group_width" in c.edges} == set(sk.DEP_WIDTHS)
    assert {(c.D, c.sparse, c.P) for c in DEP if "stage_limit" in c.edges} == {
        (8, False, 768), (8, False, 769), (8, True, 682), (8, True, 683),
        (64, False, 96), (64, False, 97), (64, True, 94), (64, True, 95),
        (130, False, 47), (130, False, 48), (130, True, 46), (130, True, 47)}
    again = sk.dep_cases()
    for a, b in zip(DEP, again):
        assert a.name == b.name and all(same(x, y) for x, y in zip(a.arrays(), b.arrays()))
