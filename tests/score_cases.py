"""What the tests of bb_examples_score share (not collected): the float64 statement of a scored row as a function of the float32
logits [n, A] and values [n] a network gave and of the records themselves (numpy structured array, _lib.example_dtype), and
hand-built records for the corners.

The definitions (include/blackbird_hip.h, bb_examples_score): row k is record index[k]; value = the network's, unchanged;
se = (value - z)^2 in float32, one subtraction and one multiplication; ce = -sum_a pi[a] ((logit[a] - mx) - lse) with
mx = max logit, lse = log sum exp(logit - mx) over all A logits and pi the row's label, 0 for a row without one.  The label is
float32(visits / total) -- divided in float64, rounded once --, a compact (DragonChess) child list spread to a dense A-wide row
by assignment, as Blackbird.py spreads it for the reference's blobs; first maxima are np.argmax's.  A malformed row -- index
outside [0, n_records), n_children > S, a compact action >= A -- is zeros with flags 0 and in no total."""
import numpy as np

from blackbird_amd import _lib
from tests import merge_cases as MC

C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS


def malformed(game, rec, r):
    """is row `r` (a record number, possibly out of range) of `rec` a malformed row"""
    gi = _lib.game_info(game)
    if r < 0 or r >= len(rec):
        return True
    nch = int(rec["n_children"][r])
    if nch > gi.S:
        return True
    return bool(not gi.dense and (rec["action"][r][:nch] >= gi.A).any())


def label(game, row):
    """the dense float32 label [A] of one well-formed record"""
    gi = _lib.game_info(game)
    pi = np.zeros(gi.A, dtype=np.float32)
    total = int(row["total"])
    if total == 0:
        return pi
    if gi.dense:
        return (row["visits"][:gi.A].astype(np.float64) / float(total)).astype(np.float32)
    nch = int(row["n_children"])
    pi[row["action"][:nch]] = (row["visits"][:nch].astype(np.float64) / float(total)).astype(np.float32)
    return pi


def statement(game, logits, values, rec, index=None):
    """rows [n, 3] float64 (value, se -- the float32 figure, exactly --, ce), mx, lse [n] float64, flags [n] uint8, ok [n] bool and
    the totals as eval_summary's arguments (dict), from float32 logits [n, A] and values [n] of the rows' states."""
    gi = _lib.game_info(game)
    idx = np.arange(len(rec), dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64).reshape(-1)
    n = len(idx)
    logits = np.asarray(logits, dtype=np.float32).reshape(n, gi.A)
    values = np.asarray(values, dtype=np.float32).reshape(n)
    rows, flags = np.zeros((n, 3)), np.zeros(n, dtype=np.uint8)
    mx, lse, ok = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
    for k, r in enumerate(idx):
        if malformed(game, rec, int(r)):
            continue
        ok[k] = True
        row = rec[int(r)]
        v, z = values[k], np.float32(row["z"])
        d = np.float32(v - z)
        f = _lib.ROW_COUNTED
        if z != 0:
            f |= _lib.ROW_DECIDED
        if (v > 0 and z > 0) or (v < 0 and z < 0):
            f |= _lib.ROW_SIGN_OK
        lg = logits[k].astype(np.float64)
        mx[k] = lg.max()
        lse[k] = np.log(np.exp(lg - mx[k]).sum())
        pi = label(game, row)
        ce = 0.0
        if (pi != 0).any():
            f |= _lib.ROW_HAS_POLICY
            ce = -float((pi.astype(np.float64) * ((lg - mx[k]) - lse[k])).sum())
            if int(np.argmax(logits[k])) == int(np.argmax(pi)):
                f |= _lib.ROW_TOP1
        rows[k] = (float(v), float(np.float32(d * d)), ce)
        flags[k] = f
    return {"rows": rows, "mx": mx, "lse": lse, "flags": flags, "ok": ok, "totals": totals(rows, flags)}


def totals(rows, flags):
    """eval_summary's arguments from per-row figures and flags: counts, and the float64 sums of se over the counted rows and of
    ce over the rows with a label"""
    rows, f = np.asarray(rows, dtype=np.float64), np.asarray(flags).astype(np.int64)
    counted, has = (f & _lib.ROW_COUNTED) != 0, (f & _lib.ROW_HAS_POLICY) != 0
    decided = (f & _lib.ROW_DECIDED) != 0
    return {"rows": int(counted.sum()), "policy_rows": int(has.sum()), "top1": int((has & ((f & _lib.ROW_TOP1) != 0)).sum()),
            "decided": int(decided.sum()), "sign_ok": int((decided & ((f & _lib.ROW_SIGN_OK) != 0)).sum()),
            "se_sum": float(rows[counted, 1].sum()), "ce_sum": float(rows[has, 2].sum())}


# ---- hand-built records --------------------------------------------------------------------------------------------------------
def _dc_record(actions, visits, z, *, total=None, n_children=None, game_id=900, ply=0):
    gi = _lib.game_info(DC)
    r = np.zeros(1, dtype=_lib.example_dtype(DC))
    r["state"] = _lib.game_initial(DC).view(np.uint8).reshape(1, -1)      # (host-computable: no kernel)
    k = len(actions)
    r["action"][0, :k] = np.asarray(actions, dtype=np.uint16)
    r["visits"][0, :k] = np.asarray(visits, dtype=np.uint32)
    r["total"] = int(np.sum(visits)) if total is None else total
    r["n_children"] = k if n_children is None else n_children
    r["game_id"], r["ply"], r["player"], r["z"] = game_id, ply, 1, z
    assert k <= gi.S
    return r[0]


def corners(game):
    """(records, names): hand-built records and {name: record number}.  Well-formed: 'terminal' (total 0), 'tie' (two top
    shares; DragonChess: the smaller action comes later in the list), z in {-1, 0, 1} among them; DragonChess also 'full' (144
    children, all three lane passes, actions up to 4031) and 'c65' (65 children).  Malformed: 'too_many' (n_children = S + 1) and,
    DragonChess, 'bad_action' (an action 4032)."""
    gi = _lib.game_info(game)
    rng = np.random.RandomState(41)
    if gi.dense:
        H, W = MC.SHAPE[game][:2]
        empty = np.zeros((H, W), dtype=np.int8)
        one = MC.play(game, empty, 3 if game == C4 else 4, 1)
        tie = np.zeros(gi.A, dtype=np.uint32)
        tie[[1, 2, 5]] = (7, 9, 9)
        some = rng.randint(1, 50, gi.A).astype(np.uint32)
        rows = [MC.record(game, one, 2, prev=1, z=0, visits=None, game_id=900, ply=1),                 # terminal: total 0
                MC.record(game, empty, 1, z=1, visits=tie, game_id=900),
                MC.record(game, one, 2, prev=1, z=-1, visits=some, game_id=901, ply=1),
                MC.record(game, empty, 1, z=0, visits=some[::-1].copy(), game_id=901),
                MC.record(game, empty, 1, z=1, visits=some, n_children=gi.S + 1, game_id=902)]
        return MC.stack(rows, game), {"terminal": 0, "tie": 1, "minus": 2, "draw": 3, "too_many": 4}
    full_a = np.concatenate([rng.choice(gi.A - 192, gi.S - 20, replace=False), gi.A - 1 - rng.choice(192, 20, replace=False)])
    full_a = full_a[rng.permutation(gi.S)]
    full_a[gi.S - 1] = gi.A - 1 if gi.A - 1 not in full_a[:gi.S - 1] else full_a[gi.S - 1]
    full_v = rng.randint(0, 30, gi.S)
    full_v[[5, 70, 143]] = (40, 41, 39)                                   # the top share sits in the second lane pass
    a65 = rng.choice(gi.A, 65, replace=False)
    v65 = rng.randint(1, 9, 65)
    v65[64] = 50                                                          # ... and here on the one child of the second pass
    rows = [_dc_record([], [], 0),                                        # terminal: total 0
            _dc_record([500, 100, 7, 3000], [9, 9, 3, 0], 1),             # tie: action 100 is the label's first maximum
            _dc_record(full_a, full_v, -1, game_id=901),
            _dc_record(a65, v65, 0, game_id=901, ply=1),
            _dc_record([5, 6], [1, 2], 1, n_children=gi.S + 1, game_id=902),
            _dc_record([5, gi.A, 6], [1, 2, 3], -1, game_id=902, ply=1)]
    assert len(np.unique(full_a)) == gi.S and full_a.max() == gi.A - 1
    return np.array(rows, dtype=_lib.example_dtype(DC)), {"terminal": 0, "tie": 1, "full": 2, "c65": 3, "too_many": 4, "bad_action": 5}
