"""Host mirror of clocksi_materializer (src/clocksi_materializer.erl) over the
C ABI.  Same names, argument meaning and error behaviour:

  new(Type)                                   :41-43
  materialize(Type, TxId, MinSnapshotTime, #snapshot_get_response{}) :82-101
      -> ("ok", Snapshot, NewLastOp, LastOpCt | "ignore", IsNewSS, Count)
       | ("error", {unexpected_operation, Op, Type})
       raises CorruptedOpsCache on a type mismatch (:190-191)
  materialize_eager(Type, Snapshot, Ops)      :272-274

plus materialize_batch(...) — many materialize/4 calls in one launch, the
form the NIF's micro-batching queue uses.  Every filter decision and every
effect application runs in the HIP kernels (agn_materialize); this module
only encodes terms and decodes results.
"""
from __future__ import annotations

from . import _abi
from .encode import (IGNORE, ClocksiPayload, DcTable, LogEncoder, ReadEncoder, decode_clock,
                     term_key)
from .records import (COUNTER_B, COUNTER_PN, REGISTER_LWW, REGISTER_MV, SET_AW, CorruptedOpsCache,
                      MaterializedSnapshot, SnapshotGetResponse, ops_oldest_first)

_TYPE_IDS = {COUNTER_PN: _abi.COUNTER_PN, SET_AW: _abi.SET_AW, REGISTER_MV: _abi.REGISTER_MV,
             REGISTER_LWW: _abi.REGISTER_LWW, COUNTER_B: _abi.COUNTER_B}
LWW_NEW = (0, b"")  # antidote_crdt_register_lww:new() = {0, <<>>}
_engines: dict = {}


def engine(device: int = 0):
    from .engine import Engine
    e = _engines.get(device)
    if e is None:
        e = _engines[device] = Engine(device)
    return e


def type_id(typ: str) -> int:
    try:
        return _TYPE_IDS[typ]
    except KeyError:
        raise ValueError(("undef", typ)) from None  # Type:new() of an unknown module


def new(typ: str):
    """materializer:create_snapshot/1 = Type:new()."""
    type_id(typ)
    if typ == REGISTER_LWW:
        return LWW_NEW
    if typ == COUNTER_B:      # antidote_crdt_counter_b:new() = {[], []}
        return ([], [])
    return 0 if typ == COUNTER_PN else []


def value(typ: str, state):
    """Type:value/1."""
    if typ in (COUNTER_PN, COUNTER_B):
        return state
    if typ == SET_AW:
        return [e for e, _ in state]
    if typ == REGISTER_LWW:
        return state[1]
    return [v for v, _ in state]


def _n_dcs(clocks) -> int:
    dcs = set()
    for c in clocks:
        if isinstance(c, dict):
            dcs |= set(c)
    return max(1, len(dcs))


def _base_pairs(typ, snapshot):
    if typ == COUNTER_PN:
        return snapshot
    if typ == SET_AW:
        return [(e, list(toks)) for e, toks in snapshot]
    if typ == REGISTER_LWW:   # {Ts, Value}: no pair for new(), else (value, ts)
        ts, v = snapshot
        return [] if (ts, v) == LWW_NEW else [(v, ts)]
    if typ == COUNTER_B:      # {P, D}: one pair per orddict key, the slot terms of the encoder
        P, D = snapshot
        return [(("P", k), v) for k, v in P] + [(("D", k), v) for k, v in D]
    return [(v, t) for v, t in snapshot]


def _lww_values(reads):
    """Every value a register_lww batch can name (base states and well-formed
    effects), in Erlang term order: interned in this order, the device's tie
    break by tag id is update/2's max over the value terms, and the mirror
    never has to redo an AGN_F_TS_TIE read."""
    vals = {}
    for _tx, _r, resp in reads:
        snap = resp.materialized_snapshot.value
        if isinstance(snap, tuple) and len(snap) == 2:
            vals.setdefault(repr(term_key(snap[1])), snap[1])
        for _i, p in ops_oldest_first(resp.ops_list):
            e = p.op_param
            if isinstance(e, tuple) and len(e) == 2:
                vals.setdefault(repr(term_key(e[1])), e[1])
    return sorted(vals.values(), key=term_key)


def _decode_state(typ, enc, res, i):
    o, n = int(res.out_off[i]), int(res.out_n[i])
    if typ == REGISTER_LWW:   # out_n == 0: Type:new()
        return (int(res.out_tok[o]), enc.tags.term(int(res.out_tag[o]))) if n else LWW_NEW
    if typ == COUNTER_B:      # pairs -> {P, D}, each an orddict in term order
        P, D = [], []
        for t, k in zip(res.out_tag[o:o + n], res.out_tok[o:o + n]):
            kind, key = enc.tags.term(int(t))
            v = int(k) - (1 << 64) if int(k) >> 63 else int(k)
            (P if kind == "P" else D).append((key, v))
        return (sorted(P, key=lambda kv: term_key(kv[0])),
                sorted(D, key=lambda kv: term_key(kv[0])))
    pairs = [(enc.tags.term(int(t)), enc.tokens.term(int(k)))
             for t, k in zip(res.out_tag[o:o + n], res.out_tok[o:o + n])]
    if typ == SET_AW:
        st: dict = {}
        for e, tk in pairs:           # device order: elem id, then add order
            st.setdefault(e, []).append(tk)
        return sorted(st.items(), key=lambda kv: kv[0])   # orddict by elem term
    return sorted(pairs)              # insert_sorted({Value, Token})


def permissions(state) -> int:
    """antidote_crdt_counter_b:permissions/1: the {I, I} entries of P less D."""
    P, D = state
    return sum(v for (a, b), v in P if a == b) - sum(v for _, v in D)


def local_permissions(ident, state) -> int:
    """antidote_crdt_counter_b:localPermissions/2: received (own increments
    included) less granted less the id's decrements."""
    P, D = state
    received = sum(v for (_, to), v in P if to == ident)
    granted = sum(v for (frm, to), v in P if frm == ident and to != ident)
    return received - granted - sum(v for i, v in D if i == ident)


def materialize_batch(typ: str, reads, device: int = 0):
    """reads: [(TxId, MinSnapshotTime, SnapshotGetResponse)] -> list of
    materialize/4 results (CorruptedOpsCache instances are returned, not
    raised, so one bad key does not hide the others)."""
    tid = type_id(typ)
    resp_clocks = []
    for _tx, r, resp in reads:
        resp_clocks.append(r)
        if isinstance(resp.snapshot_time, dict):
            resp_clocks.append(resp.snapshot_time)
        for _i, p in ops_oldest_first(resp.ops_list):
            resp_clocks.append(p.snapshot_time)
            resp_clocks.append({p.commit_time[0]: p.commit_time[1]})
    D = _n_dcs(resp_clocks)
    enc = LogEncoder(tid, D, dcs=DcTable())
    rd = ReadEncoder(enc, tid)
    if tid == _abi.REGISTER_LWW:
        for v in _lww_values(reads):
            enc.tags.id(v)
    for txid, R, resp in reads:
        k = enc.add_key([(i, ClocksiPayload(p.key, p.type, p.op_param, p.snapshot_time,
                                            p.commit_time, p.txid))
                         for i, p in ops_oldest_first(resp.ops_list)])
        rd.add(k, R, resp.snapshot_time, txid,
               _base_pairs(typ, resp.materialized_snapshot.value))
    log = enc.build()
    req = rd.build()
    cap = None
    if tid != _abi.COUNTER_PN:
        from .encode import state_capacity
        cap = state_capacity(log, req)
    res = engine(device).materialize_host(log, req, sparse=True, cap_off=cap)
    out = []
    for i in range(req.n_req):
        f = int(res.flags[i])
        if f & _abi.F_ERR_CORRUPTED:
            out.append(CorruptedOpsCache())
            continue
        if f & _abi.F_ERR_UNEXPECTED:
            e = int(res.err_pos[i])
            out.append(("error", ("unexpected_operation", log.invalid_terms.get(e), typ)))
            continue
        if f & _abi.F_ERR_CAPACITY:
            raise RuntimeError("materialize: live state exceeds the device table capacity")
        ct = IGNORE if f & _abi.F_CT_IGNORE else decode_clock(res.lastct[i], res.lastct_mask[i],
                                                               enc.dcs)
        val = int(res.value[i]) if tid == _abi.COUNTER_PN else _decode_state(typ, enc, res, i)
        out.append(("ok", val, int(res.hole[i]), ct, bool(f & _abi.F_NEWSS), int(res.count[i])))
    return out


def materialize(typ: str, txid, min_snapshot_time: dict, resp: SnapshotGetResponse,
                device: int = 0):
    r = materialize_batch(typ, [(txid, min_snapshot_time, resp)], device)[0]
    if isinstance(r, CorruptedOpsCache):
        raise r
    return r


def materialize_eager(typ: str, snapshot, effects, device: int = 0):
    """Apply effects in order without checks (materializer:materialize_eager/3):
    one key whose ops are all inside the read snapshot."""
    ops = [(i + 1, ClocksiPayload("eager", typ, e, {"eager": 2 * i}, ("eager", 2 * i + 1), None))
           for i, e in enumerate(effects)]
    resp = SnapshotGetResponse(ops[::-1], len(ops), MaterializedSnapshot(0, snapshot), IGNORE,
                               True)
    r = materialize(typ, IGNORE, {"eager": 2 * len(effects) + 1}, resp, device)
    return r if r[0] == "error" else r[1]
