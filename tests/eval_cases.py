"""What the tests of the held-out evaluation share (not collected): the float64 statement of the network's forward pass and of the
per-row figures bb_trainer_eval reports, for any dense game and network shape, written in numpy on its own (it shares no code
with tests/trainer_cases.py's `statement`, which is torch autograd over einsum), and a small generator of records along random
legal games (tests/merge_cases.py's playout_records, the helper tests/test_gpu_trainer_epoch.py uses).

The definitions (include/blackbird_hip.h, bb_trainer_eval): per row value = the network's tanh value, se = (value - z)^2,
ce = -sum_a pi[a] (logit[a] - max - log sum exp(logit - max)) with pi the row's policy label, 0 for a row without one; flags
bit 0 the row has a label, bit 1 first maximum of the logits == first maximum of the label, bit 2 z != 0, bit 3 value and z have
the same sign, bit 4 the row is well-formed.  No noise, no batch coupling, no L2 term."""
import numpy as np

from blackbird_amd import _lib
from blackbird_amd import weights as W
from tests import merge_cases as MC

LOGIT_ROOM = 1e-4     # bit 1 is compared where the top two logits of the statement differ by more than this
VALUE_ROOM = 1e-4     # bit 3 is compared where the statement's |value| exceeds this
COUNTS = ("rows", "policy_rows", "top1", "decided", "sign_ok")


def _conv(x, k, b):
    """tf.layers.conv2d, SAME, stride 1: x [n,H,W,Cin], k [kh,kw,Cin,F]"""
    n, H, Wd, _c = x.shape
    kh, kw = k.shape[:2]
    ph, pw = kh // 2, kw // 2
    xp = np.zeros((n, H + 2 * ph, Wd + 2 * pw, x.shape[3]), dtype=x.dtype)
    xp[:, ph:ph + H, pw:pw + Wd] = x
    out = np.zeros((n, H, Wd, k.shape[3]), dtype=x.dtype)
    for dy in range(kh):
        for dx in range(kw):
            out += xp[:, dy:dy + H, dx:dx + Wd] @ k[dy, dx]
    return out + b


def forward(w0, boards, dtype=np.float64):
    """(value [n], logits [n, A]) of the network `w0` (TF-named dict) on boards [n,H,W,C], in float64; batch norm in inference
    mode, epsilon 1e-3.  dtype=np.float32: the same expressions in float32, the yardstick of float32 arithmetic alone."""
    w = {k: np.asarray(v, dtype=dtype) for k, v in w0.items()}
    R = W.infer_shape(w0)[2]

    def layer(x, conv, norm):
        y = _conv(x, w[conv + "/kernel"], w[conv + "/bias"])
        g, be, mu, var = (w[f"{norm}/{f}"] for f in W.BN_FIELDS)
        return g * (y - mu) / np.sqrt(var + dtype(1e-3)) + be

    x = np.maximum(layer(np.asarray(boards, dtype=dtype), "resTower/conv_block/conv", "resTower/conv_block/batch_norm"), 0)
    for i in range(R):
        h = np.maximum(layer(x, f"resTower/block_{i}/conv_1", f"resTower/block_{i}/batch_norm_1"), 0)
        x = np.maximum(layer(h, f"resTower/block_{i}/conv_2", f"resTower/block_{i}/batch_norm_2") + x, 0)
    v = np.maximum(layer(x, "value/convolution", "value/batch_norm"), 0)                     # [n,H,W,1]
    v = np.maximum((v @ w["value/dense_1/kernel"] + w["value/dense_1/bias"]).sum(axis=(1, 2)), 0)
    value = np.tanh((v @ w["value/dense_2/kernel"] + w["value/dense_2/bias"]).sum(axis=1))
    p = np.maximum(layer(x, "policy/convolution", "policy/batch_norm"), 0)                   # [n,H,W,2]
    logits = (p @ w["policy/policy/kernel"] + w["policy/policy/bias"]).sum(axis=(1, 2))
    return value, logits


def statement(w0, boards, z, pi, dtype=np.float64):
    """The per-row figures and the totals of well-formed rows, in float64.  Returns a dict: rows [n,3] (value, se, ce), the bits
    has, top1, decided, sign_ok [n] (bool), top1_room / sign_room [n] (bool: the statement decides the bit with room), and the
    totals (COUNTS, se_sum, ce_sum)."""
    z = np.asarray(z, dtype=dtype).reshape(-1)
    pi = np.asarray(pi, dtype=dtype)
    n = len(z)
    if n == 0:
        value, logits = np.zeros(0), np.zeros((0, pi.shape[1]))
    else:
        value, logits = forward(w0, boards, dtype)
    has = (pi != 0).any(axis=1)
    shifted = logits - logits.max(axis=1, keepdims=True)
    logp = shifted - np.log(np.exp(shifted).sum(axis=1, keepdims=True))
    ce = np.where(has, -(pi * logp).sum(axis=1), 0.0)
    se = (value - z) ** 2
    top = np.sort(logits, axis=1)
    top1 = has & (np.argmax(logits, axis=1) == np.argmax(pi, axis=1))          # (np.argmax: the first maximum)
    decided = z != 0
    sign_ok = decided & (value * z > 0)
    return {"rows": np.stack([value, se, ce], axis=1), "has": has, "top1": top1, "decided": decided, "sign_ok": sign_ok,
            "top1_room": (top[:, -1] - top[:, -2]) > LOGIT_ROOM, "sign_room": np.abs(value) > VALUE_ROOM,
            "totals": {"rows": n, "policy_rows": int(has.sum()), "top1": int(top1.sum()), "decided": int(decided.sum()),
                       "sign_ok": int(sign_ok.sum()), "se_sum": float(se.sum()), "ce_sum": float(ce.sum())}}


def bits(flags):
    """the flags byte of bb_trainer_eval -> (has, top1, decided, sign_ok, counted) as bool arrays"""
    f = np.asarray(flags).astype(np.int64)
    return tuple((f & b) != 0 for b in (_lib.ROW_HAS_POLICY, _lib.ROW_TOP1, _lib.ROW_DECIDED, _lib.ROW_SIGN_OK, _lib.ROW_COUNTED))


# ---- records ---------------------------------------------------------------------------------------------------------------------
_records = {}


def records(game, n=130, seed=23):
    """n records along random legal games (several games, each ending in its terminal example: no visits, total 0), built once and
    left unchanged; record 1 has tied top visits (its first two visited actions share the largest count)."""
    key = (game, n, seed)
    if key not in _records:
        rec = MC.playout_records(game, n, seed)
        assert (rec["total"] == 0).any() and rec["total"][1] > 0 and len(np.unique(rec["game_id"])) >= 2
        A = MC.SHAPE[game][3]
        v = rec["visits"][1, :A].copy()
        live = np.flatnonzero(v > 0)
        assert len(live) >= 2
        v[live[0]] = v[live[1]] = int(v.max()) + 1
        rec["visits"][1, :A] = v
        rec["total"][1] = int(v.sum())
        _records[key] = rec
    return _records[key]


def index(game, n):
    """n record numbers of records(game): the tied-visits record, a terminal example, then the others in order; None (all of
    them in order) for 130"""
    rec = records(game)
    if n == len(rec):
        return None
    terminal = int(np.flatnonzero(rec["total"] == 0)[0])
    rest = [i for i in range(len(rec)) if i not in (1, terminal)]
    return np.array(([1, terminal] + rest)[:n], dtype=np.int64)


def host_rows(game, rec):
    """(planes, value, policy) of records as the host forms them, no GPU: the CPU oracle's encoding of the unpacked state,
    z, and pi = visits / total in float64 (zeros for a terminal example)"""
    from oracle import orc
    A = MC.SHAPE[game][3]
    og = {MC.C4: orc.C4, MC.TTT: orc.TTT}[game]
    st = np.ascontiguousarray(rec["state"]).view(_lib.STATE_DTYPE[game]).reshape(len(rec), -1)
    boards, players, prevs = _lib.unpack_grid(game, st)
    planes = np.concatenate([orc.encode(og, orc.state_from_arrays(og, b, p, int(v) or None)) for b, p, v in zip(boards, players, prevs)])
    tot = rec["total"].astype(np.float64)
    pi = np.where(tot[:, None] > 0, rec["visits"][:, :A].astype(np.float64) / np.maximum(tot, 1.0)[:, None], 0.0)
    return planes, rec["z"].astype(np.float64), pi


# ---- live inputs (tests/trainer_cases.py: live_weights, assert_live) ----------------------------------------------------------------
# (game name, R, D, n, weight seed): the rows are index(game, n) of records(game), the weights live_weights on those rows' planes.
# With init_weights alone the Connect4 value column is +-1 and se one of {0, 1, 4}.  R in {0, 2, 9}, D in {1, 64}, n in {1, 2, 130};
# the 1e-4 margin around every ReLU puts the 130 rows on the small board without blocks, as in LIVE_CASES.
LIVE_CASES = [("connect4", 0, 1, 1, 10), ("connect4", 9, 64, 1, 10), ("connect4", 2, 1, 2, 1808), ("tictactoe", 2, 64, 2, 63),
              ("tictactoe", 9, 1, 2, 3894), ("tictactoe", 0, 64, 130, 9113)]
COLUMNS = ("value", "se", "ce")
_live = {}


def live_case(case):
    """A live scorer case, computed once and left unchanged: the record numbers `index`, the host's rows `rows`, the weights `w`,
    the float64 statement `want`, and per column of (value, se, ce) the float32 statement's error relative to the column's largest
    |entry| (`figure`) and the tolerance min(8 figure, 1e-5) (`tol`)."""
    if case not in _live:
        from tests import trainer_cases as T
        name, R, D, n, w_seed = case
        game = {"connect4": MC.C4, "tictactoe": MC.TTT}[name]
        idx = index(game, n)
        rows = host_rows(game, records(game) if idx is None else records(game)[idx])
        w = T.live_weights(name, R, D, w_seed, rows[0])
        want = statement(w, *rows)
        low = statement(w, *rows, dtype=np.float32)
        figure = [float(np.abs(low["rows"][:, c] - want["rows"][:, c]).max() / np.abs(want["rows"][:, c]).max()) for c in range(3)]
        _live[case] = {"game": game, "index": idx, "rows": rows, "w": w, "want": want, "figure": figure,
                       "tol": [T.live_tol(f) for f in figure]}
    return _live[case]


# (game name, R, D, batch, weight seed, first record): two batches, records first .. first + 2 batch of the 40 playout records the
# epoch tests use (merge_cases.playout_records(game, 40, 21)); the weights are live_weights on the first batch's planes
EPOCH_LIVE_CASE = ("tictactoe", 2, 16, 6, 12, 2)


def epoch_live_case():
    """The live epoch case, computed once: the 40 records `rec`, the record numbers `order` (two batches), the given noise
    [2, A], the weights `w`, the host's rows of the first batch, the training statement there with its parts (`want`), the
    float32 figure of its data gradients and the tolerance."""
    if "epoch" not in _live:
        from tests import trainer_cases as T
        name, R, D, batch, w_seed, first = EPOCH_LIVE_CASE
        game = {"connect4": MC.C4, "tictactoe": MC.TTT}[name]
        rec = MC.playout_records(game, 40, 21)
        order = np.arange(first, first + 2 * batch, dtype=np.int64)
        rows = host_rows(game, rec[order[:batch]])
        noise = np.random.RandomState(16).beta(T.ALPHA, 1 - T.ALPHA, size=(2, MC.SHAPE[game][3])).astype(np.float32)
        w = T.live_weights(name, R, D, w_seed, rows[0])
        want = T.statement(w, *rows, noise[0], T.EPS, parts=True)
        figure = T.float32_figure(w, rows + (noise[0],), T.EPS, want)
        _live["epoch"] = {"game": game, "rec": rec, "order": order, "noise": noise, "w": w, "rows": rows, "want": want,
                          "figure": figure, "tol": T.live_tol(figure)}
    return _live["epoch"]


def any_game_records(game, n_games, per_game, seed):
    """headers only matter: n_games * per_game records of `game` (DragonChess too) whose game_id runs 7, 9, 11, ... in blocks of
    per_game, every other byte random -- what DeviceExamples.split_games reads is the game id alone"""
    rng = np.random.RandomState(seed)
    rec = np.zeros(n_games * per_game, dtype=_lib.example_dtype(game))
    raw = rec.view(np.uint8).reshape(len(rec), -1)
    raw[:] = rng.randint(0, 256, raw.shape)
    rec["game_id"] = np.repeat(7 + 2 * np.arange(n_games), per_game)
    rec["ply"] = np.tile(np.arange(per_game), n_games)
    return rec
