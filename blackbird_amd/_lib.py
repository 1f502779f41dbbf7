"""ctypes binding of libblackbird_hip.so (C ABI: include/blackbird_hip.h).

There is no CPU fallback: if the shared library is missing or no MI355X is visible, the first
operation raises.  The library is built in-tree (blackbird_amd/libblackbird_hip.so) by
`__graft_entry__.build()` / `make -C blackbird_amd/csrc`.
"""
import ctypes as C
import os

import numpy as np

from .weights import FIELDS as _weight_fields

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libblackbird_hip.so")

GAME_CONNECT4, GAME_TICTACTOE, GAME_DRAGONCHESS = 0, 1, 2
MCTS_DYNAMIC, MCTS_FIXED = 0, 1
EVAL_HASH, EVAL_NET, EVAL_ROLLOUT = 0, 1, 2
NET_FORM_AUTO, NET_FORM_F32, NET_FORM_SPLIT = 0, 1, 2   # bb_config.net_form
NET_EVAL_FUSED, NET_EVAL_SMALL, NET_EVAL_BATCH = 0, 1, 2   # bb_net_eval_structure
LAUNCH_AUTO, LAUNCH_LOCKSTEP, LAUNCH_ROUNDS, LAUNCH_WAVE = 0, 1, 2, 3    # bb_config.launch (LAUNCH_WAVE: the search API in one launch)
PLAY_LOCKSTEP, PLAY_ROUNDS, PLAY_QUEUE, PLAY_DC_FUSED, PLAY_WAVE_ROLLOUT = 0, 1, 3, 5, 6   # bb_selfplay_mode
NODE_EXPANDED, NODE_TERMINAL = 1, 2                      # bits of the flags word of bb_node_view / bb_node_edges
CHILD_NONE, CHILD_TERM_BIT = -1, 0x40000000              # their child words: no node yet; pool index | CHILD_TERM_BIT for a terminal child
OPT_ADAM, OPT_MOMENTUM, OPT_SGD = 0, 1, 2                # bb_train_config.optimizer
LOSS_REFERENCE, LOSS_PER_EXAMPLE = 0, 1                  # bb_trainer_set_loss
WEIGHTS_IMAGES = ("w0", "wt", "epi", "head", "x3")        # bb_weights_read's selector, BB_WEIGHTS_*: Engine.weights_image
TRAIN_PARAMS, TRAIN_GRADS, TRAIN_SLOT_M, TRAIN_SLOT_V, TRAIN_NOISE = 0, 1, 2, 3, 4   # bb_trainer_read
ROW_HAS_POLICY, ROW_TOP1, ROW_DECIDED, ROW_SIGN_OK, ROW_COUNTED = 1, 2, 4, 8, 16     # flags byte of bb_trainer_eval
EVAL_TOTALS_DTYPE = [(n, "<i8") for n in ("rows", "policy_rows", "top1", "decided", "sign_ok")] + [("se_sum", "<f8"), ("ce_sum", "<f8")]  # bb_eval_totals
OK, ERR_ARG, ERR_HIP, ERR_STATE, ERR_NAN, ERR_CAPACITY, ERR_WEIGHTS = 0, -1, -2, -3, -4, -5, -6

EXPORTS = (
    "bb_game_info_get", "bb_last_error", "bb_device_count", "bb_game_legal", "bb_game_apply", "bb_game_winner",
    "bb_game_encode", "bb_game_initial", "bb_create", "bb_destroy", "bb_load_weights", "bb_get_counters",
    "bb_reset_counters", "bb_synchronize", "bb_set_sims_per_move", "bb_timing_enable", "bb_timing_read", "bb_timing_net", "bb_selfplay_mode", "bb_net_form", "bb_net_eval_structure", "bb_net_eval", "bb_hash_eval", "bb_set_roots", "bb_run_sims", "bb_run_sims_masked", "bb_run_sims_structure", "bb_search_rollouts", "bb_selfplay_rollouts",
    "bb_sample_moves", "bb_move_roots", "bb_get_root_states", "bb_selfplay_begin", "bb_selfplay_set_starts", "bb_selfplay_set_temp_schedule", "bb_selfplay_step",
    "bb_selfplay_done", "bb_examples_fetch", "bb_examples_device", "bb_selfplay_headers", "bb_examples_fetch_games", "bb_reset_roots", "bb_node_view", "bb_node_edges", "bb_net_eval_keyed", "bb_set_rng_stream", "bb_fit_slots",
    "bb_examples_to_batch", "bb_examples_to_batch_sym", "bb_game_symmetries",
    "bb_examples_merge_workspace", "bb_examples_merge", "bb_examples_merged_to_batch",
    "bb_arena_create", "bb_arena_begin", "bb_arena_set_temp_schedule", "bb_arena_step", "bb_arena_status", "bb_arena_fetch", "bb_arena_destroy",
    "bb_trainer_create", "bb_trainer_destroy", "bb_trainer_step", "bb_trainer_epoch", "bb_trainer_param_count",
    "bb_trainer_read", "bb_trainer_eval", "bb_trainer_eval_tensors", "bb_trainer_set_loss",
    "bb_load_weights_device", "bb_trainer_load_engine", "bb_weights_read",
    "bb_examples_score_workspace", "bb_examples_score",
)


class GameInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("H", "W", "C", "A", "S", "state_bytes", "dense", "example_bytes")]


_FP = C.POINTER(C.c_float)


class NetWeights(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("H", "W", "C", "F", "R", "D", "A")] + [
        (n, _FP) for n in _weight_fields]


class Config(C.Structure):
    _fields_ = [("game", C.c_int32), ("n_slots", C.c_int32), ("mcts_kind", C.c_int32), ("max_depth", C.c_int32),
                ("evaluator", C.c_int32), ("sims_per_move", C.c_int32), ("max_plies", C.c_int32),
                ("max_games", C.c_int32), ("c_puct", C.c_double), ("seed", C.c_uint64), ("hash_salt", C.c_uint64),
                ("first_game_id", C.c_uint32), ("noise_on", C.c_int32), ("alpha", C.c_float), ("epsilon", C.c_float),
                ("device", C.c_int32), ("salt_per_game", C.c_int32), ("node_capacity", C.c_int32),
                ("net_form", C.c_int32), ("launch", C.c_int32), ("general_net", C.c_int32), ("track_ancestors", C.c_int32),
                ("search_cache", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("sims", "sum_depth", "nodes", "terminal_leaves", "games_finished",
                                           "plies", "overflow", "examples", "evals",
                                           "eval_cache_hits", "eval_cache_probes")]


class TrainConfig(C.Structure):
    _fields_ = [("game", C.c_int32), ("optimizer", C.c_int32), ("max_batch", C.c_int32), ("device", C.c_int32),
                ("momentum", C.c_float), ("alpha", C.c_float), ("epsilon", C.c_float), ("seed", C.c_uint64)]


class BlackbirdHipError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libblackbird_hip.so; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BlackbirdHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C blackbird_amd/csrc`).  blackbird_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, ip = C.c_void_p, C.c_int
    L.bb_last_error.restype = C.c_char_p
    L.bb_game_info_get.argtypes = [ip, C.POINTER(GameInfo)]
    L.bb_game_legal.argtypes = [ip, ip, vp, vp]
    L.bb_game_apply.argtypes = [ip, ip, vp, vp, vp]
    L.bb_game_winner.argtypes = [ip, ip, vp, vp, vp]
    L.bb_game_encode.argtypes = [ip, ip, vp, vp]
    L.bb_game_initial.argtypes = [ip, vp]
    L.bb_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.bb_destroy.argtypes = [vp]
    L.bb_load_weights.argtypes = [vp, C.POINTER(NetWeights)]
    L.bb_load_weights_device.argtypes = [vp, C.POINTER(NetWeights), vp]
    L.bb_trainer_load_engine.argtypes = [vp, vp, vp]
    L.bb_weights_read.argtypes = [vp, ip, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.bb_get_counters.argtypes = [vp, C.POINTER(Counters)]
    L.bb_reset_counters.argtypes = [vp]
    L.bb_synchronize.argtypes = [vp]
    L.bb_set_sims_per_move.argtypes = [vp, ip]
    L.bb_timing_enable.argtypes = [vp, ip]
    L.bb_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(ip)]
    L.bb_timing_net.argtypes = [vp, ip, ip, ip, C.POINTER(C.c_double)]
    L.bb_selfplay_mode.argtypes = [vp]
    L.bb_net_form.argtypes = [vp]
    L.bb_net_eval_structure.argtypes = [vp, ip, C.POINTER(C.c_int32)]
    L.bb_net_eval.argtypes = [vp, ip, vp, vp, vp, vp, vp, ip]
    L.bb_net_eval_keyed.argtypes = [vp, ip, vp, vp, vp, vp, vp, vp, vp]
    L.bb_set_rng_stream.argtypes = [vp, C.c_uint64, C.c_uint32]
    L.bb_fit_slots.argtypes = [C.POINTER(Config), C.POINTER(ip), C.POINTER(C.c_uint64)]
    L.bb_hash_eval.argtypes = [vp, ip, vp, vp, vp]
    L.bb_set_roots.argtypes = [vp, ip, vp, vp, vp]
    L.bb_run_sims.argtypes = [vp, ip]
    L.bb_run_sims_masked.argtypes = [vp, ip, vp]
    L.bb_run_sims_structure.argtypes = [vp, C.POINTER(C.c_int32)]
    L.bb_search_rollouts.argtypes = [vp, ip]
    L.bb_selfplay_rollouts.argtypes = [vp, ip]
    L.bb_sample_moves.argtypes = [vp, C.c_double, vp, vp, vp, vp, vp, vp, vp]
    L.bb_move_roots.argtypes = [vp, vp]
    L.bb_get_root_states.argtypes = [vp, vp]
    L.bb_selfplay_begin.argtypes = [vp, ip, C.c_double]
    L.bb_selfplay_set_starts.argtypes = [vp, ip, vp]
    L.bb_selfplay_set_temp_schedule.argtypes = [vp, ip, C.c_double]
    L.bb_selfplay_step.argtypes = [vp, ip]
    L.bb_selfplay_done.argtypes = [vp, C.POINTER(ip), C.POINTER(ip)]
    L.bb_examples_fetch.argtypes = [vp, ip, ip, vp, ip, vp, vp]
    L.bb_selfplay_headers.argtypes = [vp, ip, ip, vp]
    L.bb_reset_roots.argtypes = [vp]
    L.bb_node_view.argtypes = [vp, ip, ip, vp, vp, vp, vp, vp]
    L.bb_node_edges.argtypes = [vp, ip, ip, vp, vp, vp, vp, vp, vp]
    L.bb_examples_fetch_games.argtypes = [vp, ip, vp, vp, ip, vp, vp]
    L.bb_examples_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(vp)]
    L.bb_examples_to_batch.argtypes = [ip, ip, vp, ip, vp, vp, vp, vp, vp, vp]
    L.bb_examples_to_batch_sym.argtypes = [ip, ip, vp, ip, vp, vp, vp, vp, vp, vp, vp]
    L.bb_game_symmetries.argtypes = [ip]
    L.bb_examples_merge_workspace.argtypes = [ip, ip, C.POINTER(C.c_uint64)]
    L.bb_examples_merge.argtypes = [ip, ip, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, vp]
    L.bb_examples_merged_to_batch.argtypes = [ip, ip, vp, ip, vp, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp]
    L.bb_arena_create.argtypes = [vp, vp, ip, C.POINTER(vp)]
    L.bb_arena_begin.argtypes = [vp, ip, vp, vp, C.c_double]
    L.bb_arena_set_temp_schedule.argtypes = [vp, ip, C.c_double]
    L.bb_arena_step.argtypes = [vp, ip]
    L.bb_arena_status.argtypes = [vp, C.POINTER(ip)]
    L.bb_arena_fetch.argtypes = [vp, vp, vp, vp, vp]
    L.bb_arena_destroy.argtypes = [vp]
    L.bb_trainer_create.argtypes = [C.POINTER(TrainConfig), C.POINTER(NetWeights), C.POINTER(vp)]
    L.bb_trainer_destroy.argtypes = [vp]
    L.bb_trainer_set_loss.argtypes = [vp, ip, C.c_double]
    L.bb_trainer_step.argtypes = [vp, ip, vp, vp, vp, vp, C.c_double, ip, vp, vp]
    L.bb_trainer_epoch.argtypes = [vp, ip, vp, ip, ip, vp, vp, vp, C.c_double, vp, vp, vp]
    L.bb_trainer_param_count.argtypes = [vp, C.POINTER(C.c_int64)]
    L.bb_trainer_read.argtypes = [vp, ip, vp, C.c_int64]
    L.bb_trainer_eval.argtypes = [vp, ip, vp, ip, vp, vp, vp, vp, vp, vp, vp]
    L.bb_trainer_eval_tensors.argtypes = [vp, ip, vp, vp, vp, vp, vp, vp, vp]
    L.bb_examples_score_workspace.argtypes = [vp, ip, C.POINTER(C.c_uint64)]
    L.bb_examples_score.argtypes = [vp, ip, vp, ip, vp, vp, vp, vp, vp, vp, C.c_uint64, vp]
    for name in EXPORTS:
        if name != "bb_last_error":
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def last_error():
    return (lib().bb_last_error() or b"").decode()


def check(rc):
    """Map bb_status codes to the exception types the reference raises."""
    if rc >= 0:
        return rc
    msg = last_error()
    if rc == ERR_ARG:
        raise ValueError(msg)
    if rc == ERR_STATE:
        raise AssertionError(msg or "Primed for the correct input state.")
    if rc == ERR_NAN:
        raise ValueError(msg or "probabilities contain NaN")
    raise BlackbirdHipError(f"libblackbird_hip error {rc}: {msg}")


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_info_cache = {}


def game_info(game):
    if game not in _info_cache:
        gi = GameInfo()
        check(lib().bb_game_info_get(game, C.byref(gi)))
        _info_cache[game] = gi
    return _info_cache[game]


def game_symmetries(game):
    """bb_game_symmetries: how many board symmetries the game has for examples_to_batch_sym (Connect4 2, TicTacToe 8,
    DragonChess 1; symmetry 0 is the identity).  ValueError for an unknown game."""
    return check(lib().bb_game_symmetries(int(game)))


# ---- packed states (layout: include/blackbird_hip.h) -------------------------------------------------
GRID = {GAME_CONNECT4: (6, 7, 8), GAME_TICTACTOE: (3, 3, 4)}  # H, W, bit stride
STATE_DTYPE = {GAME_CONNECT4: np.dtype("<u8"), GAME_TICTACTOE: np.dtype("<u8"), GAME_DRAGONCHESS: np.dtype("u1")}


def pack_grid(game, boards, players, prevs=None):
    """boards [n,H,W,2] int8 (reference Board layout), players [n], prevs [n] (0 == None) -> uint64 [n,2]."""
    H, W, stride = GRID[game]
    boards = np.asarray(boards).reshape(-1, H, W, 2)
    n = boards.shape[0]
    out = np.zeros((n, 2), dtype=np.uint64)
    for r in range(H):
        for c in range(W):
            bit = np.uint64(r * stride + c)
            out[:, 0] |= (boards[:, r, c, 0] != 0).astype(np.uint64) << bit
            out[:, 1] |= (boards[:, r, c, 1] != 0).astype(np.uint64) << bit
    pl = np.asarray(players, dtype=np.uint64).reshape(n)
    pv = np.zeros(n, dtype=np.uint64) if prevs is None else np.asarray(prevs, dtype=np.uint64).reshape(n)
    out[:, 0] |= (pl & np.uint64(3)) << np.uint64(56)
    out[:, 0] |= (pv & np.uint64(3)) << np.uint64(58)
    return out


def unpack_grid(game, packed):
    """uint64 [n,2] -> (boards [n,H,W,2] int8, players [n], prevs [n])."""
    H, W, stride = GRID[game]
    packed = np.asarray(packed, dtype=np.uint64).reshape(-1, 2)
    n = packed.shape[0]
    boards = np.zeros((n, H, W, 2), dtype=np.int8)
    for r in range(H):
        for c in range(W):
            bit = np.uint64(r * stride + c)
            boards[:, r, c, 0] = (packed[:, 0] >> bit) & np.uint64(1)
            boards[:, r, c, 1] = (packed[:, 1] >> bit) & np.uint64(1)
    players = ((packed[:, 0] >> np.uint64(56)) & np.uint64(3)).astype(np.int8)
    prevs = ((packed[:, 0] >> np.uint64(58)) & np.uint64(3)).astype(np.int8)
    return boards, players, prevs


def pack_dc(boards, players, prevs=None, castles=None):
    """boards [n,8,8] piece codes, players [n], prevs [n] (0 == None), castles [n,4] -> uint8 [n,80]."""
    boards = np.asarray(boards).reshape(-1, 64)
    n = boards.shape[0]
    out = np.zeros((n, 80), dtype=np.uint8)
    out[:, :64] = boards.astype(np.int8).view(np.uint8)
    out[:, 64] = np.asarray(players, dtype=np.uint8).reshape(n)
    out[:, 65] = 0 if prevs is None else np.asarray(prevs, dtype=np.uint8).reshape(n)
    if castles is not None:
        out[:, 66:70] = (np.asarray(castles).reshape(n, 4) != 0).astype(np.uint8)
    return out


def unpack_dc(packed):
    packed = np.asarray(packed, dtype=np.uint8).reshape(-1, 80)
    boards = packed[:, :64].view(np.int8).reshape(-1, 8, 8).copy()
    return boards, packed[:, 64].astype(np.int8), packed[:, 65].astype(np.int8), packed[:, 66:70].astype(np.int8)


# ---- stateless batched game ops --------------------------------------------------------------------
def game_legal(game, states):
    gi = game_info(game)
    states = np.ascontiguousarray(states)
    n = states.shape[0]
    out = np.zeros((n, gi.A), dtype=np.uint8)
    check(lib().bb_game_legal(game, n, ptr(states), ptr(out)))
    return out


def game_apply(game, states, actions):
    states = np.ascontiguousarray(states).copy()
    n = states.shape[0]
    actions = np.ascontiguousarray(actions, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    check(lib().bb_game_apply(game, n, ptr(states), ptr(actions), ptr(status)))
    return states, status


def game_winner(game, states, prev_actions=None):
    states = np.ascontiguousarray(states)
    n = states.shape[0]
    prev = None if prev_actions is None else np.ascontiguousarray(prev_actions, dtype=np.int32)
    out = np.zeros(n, dtype=np.int8)
    check(lib().bb_game_winner(game, n, ptr(states), ptr(prev), ptr(out)))
    return out


def game_encode(game, states):
    gi = game_info(game)
    states = np.ascontiguousarray(states)
    n = states.shape[0]
    out = np.zeros((n, gi.H, gi.W, gi.C), dtype=np.int8)
    check(lib().bb_game_encode(game, n, ptr(states), ptr(out)))
    return out


def game_initial(game):
    gi = game_info(game)
    buf = np.zeros(gi.state_bytes, dtype=np.uint8)
    check(lib().bb_game_initial(game, ptr(buf)))
    return buf.view(STATE_DTYPE[game]).reshape(1, -1)


def example_dtype(game):
    gi = game_info(game)
    fields = [("game_id", "<u4"), ("ply", "<u2"), ("player", "u1"), ("z", "i1"), ("total", "<u4"),
              ("n_children", "<u4"), ("state", "u1", (gi.state_bytes,)), ("visits", "<u4", (gi.S,))]
    if not gi.dense:
        fields.append(("action", "<u2", (gi.S,)))
    dt = np.dtype(fields)
    assert dt.itemsize == gi.example_bytes, (dt.itemsize, gi.example_bytes)
    return dt


def examples_to_batch(game, n_records, records, n, index=None, boards=None, policy=None, value=None, bad=None, stream=0):
    """bb_examples_to_batch: rows `index[0..n)` (None: 0..n-1) of the device records -> float32 boards [n,H,W,C], policy
    [n,A], value [n] and the int32 count of rejected rows.  Every argument after `n` is a DEVICE address (an int, e.g.
    torch.Tensor.data_ptr(); None/0 = absent) on the current device; `stream` a hipStream_t handle.  Asynchronous."""
    check(lib().bb_examples_to_batch(int(game), int(n_records), C.c_void_p(records or None), int(n), C.c_void_p(index or None),
                                     C.c_void_p(boards or None), C.c_void_p(policy or None), C.c_void_p(value or None),
                                     C.c_void_p(bad or None), C.c_void_p(stream or None)))


def examples_to_batch_sym(game, n_records, records, n, index=None, sym=None, boards=None, policy=None, value=None, bad=None,
                          stream=0):
    """bb_examples_to_batch_sym: examples_to_batch with row k transformed by the game's symmetry sym[k] (uint8 [n] on the
    device, each < game_symmetries(game); None: the identity everywhere, i.e. examples_to_batch).  A row whose symmetry is
    out of range is written as zeros and counted in `bad`.  The same argument rules as examples_to_batch."""
    check(lib().bb_examples_to_batch_sym(int(game), int(n_records), C.c_void_p(records or None), int(n), C.c_void_p(index or None),
                                         C.c_void_p(sym or None), C.c_void_p(boards or None), C.c_void_p(policy or None),
                                         C.c_void_p(value or None), C.c_void_p(bad or None), C.c_void_p(stream or None)))


def examples_merge_workspace(game, n_records):
    """bb_examples_merge_workspace: the bytes of scratch memory examples_merge needs for n_records records.  Host only.
    ValueError for DragonChess (not covered), an unknown game or a negative count."""
    out = C.c_uint64(0)
    check(lib().bb_examples_merge_workspace(int(game), int(n_records), C.byref(out)))
    return int(out.value)


def examples_merge(game, n_records, records, group=None, rep=None, count=None, zsum=None, total=None, visits=None, n_groups=None,
                   bad=None, workspace=None, workspace_bytes=0, stream=0):
    """bb_examples_merge: the device records grouped by position (cells and side to move) and their targets summed per group
    -- group [n_records] int32, rep / count / zsum [n_records] int32, total [n_records] and visits [n_records, A] 64-bit, n_groups
    [1] and bad [1] int32 --, every argument after `n_records` a DEVICE address as in examples_to_batch, `workspace` of at least
    examples_merge_workspace bytes.  Asynchronous: n_groups (negative: an error code for check()) is valid once the stream has run."""
    p = lambda a: C.c_void_p(a or None)  # noqa: E731
    check(lib().bb_examples_merge(int(game), int(n_records), p(records), p(group), p(rep), p(count), p(zsum), p(total), p(visits),
                                  p(n_groups), p(bad), p(workspace), int(workspace_bytes), p(stream)))


def examples_merged_to_batch(game, n_records, records, n_groups, rep, count, zsum, total, visits, n, index=None, sym=None,
                             boards=None, policy=None, value=None, bad=None, stream=0):
    """bb_examples_merged_to_batch: examples_to_batch_sym over the groups examples_merge made of these records -- row k is group
    index[k] (None: group k) under symmetry sym[k] (None: as played).  The same argument rules as examples_to_batch."""
    p = lambda a: C.c_void_p(a or None)  # noqa: E731
    check(lib().bb_examples_merged_to_batch(int(game), int(n_records), p(records), int(n_groups), p(rep), p(count), p(zsum), p(total),
                                            p(visits), int(n), p(index), p(sym), p(boards), p(policy), p(value), p(bad), p(stream)))


def net_weights(H, W, flat):
    """(bb_net_weights, the arrays it points into) for a dict from blackbird_amd.weights.flatten(); the shape fields are
    taken from the arrays, so a network outside what an entry point supports reaches that entry point's own checks."""
    w = NetWeights()
    k0 = flat["conv0_k"]
    w.H, w.W, w.C, w.F = int(H), int(W), k0.shape[2], k0.shape[3]
    w.R, w.D, w.A = flat["blk_k"].shape[0], flat["v_d1_k"].shape[0], flat["p_d_b"].shape[0]
    keep = {}
    for name, _t in NetWeights._fields_[7:]:
        keep[name] = np.ascontiguousarray(flat[name], dtype=np.float32)
        setattr(w, name, keep[name].ctypes.data_as(_FP))
    return w, keep


def net_weights_device(H, W, C_, F, R, D, A, base, offsets):
    """A bb_net_weights whose blocks lie in DEVICE memory: block `name` starts offsets[name] float32 after the device address
    `base` (an int, e.g. torch.Tensor.data_ptr()).  For Engine.load_weights_device."""
    w = NetWeights()
    w.H, w.W, w.C, w.F, w.R, w.D, w.A = int(H), int(W), int(C_), int(F), int(R), int(D), int(A)
    for name, _t in NetWeights._fields_[7:]:
        setattr(w, name, C.cast(C.c_void_p(int(base) + 4 * int(offsets[name])), _FP))
    return w


def trainer_load_engine(h, engine, stream=0):
    """bb_trainer_load_engine: the trainer's current parameters into `engine` (an Engine that has had load_weights), packed on
    the device behind what `stream` holds.  Asynchronous for `stream`."""
    check(lib().bb_trainer_load_engine(h, engine.h, C.c_void_p(stream or None)))


def trainer_create(game, flat, H, W, optimizer, max_batch, device=0, momentum=0.9, alpha=0.2, epsilon=0.3, seed=0):
    """bb_trainer_create: a bb_trainer handle (c_void_p) over the weights `flat` (weights.flatten()) of an H x W game."""
    cfg = TrainConfig(game=int(game), optimizer=int(optimizer), max_batch=int(max_batch), device=int(device),
                      momentum=float(momentum), alpha=float(alpha), epsilon=float(epsilon), seed=int(seed) & (2 ** 64 - 1))
    w, _keep = net_weights(H, W, flat)
    h = C.c_void_p()
    check(lib().bb_trainer_create(C.byref(cfg), C.byref(w), C.byref(h)))
    return h


def trainer_destroy(h):
    if h is not None and h.value:
        lib().bb_trainer_destroy(h)


def trainer_set_loss(h, loss, l2=0.0):
    """bb_trainer_set_loss: LOSS_REFERENCE or LOSS_PER_EXAMPLE (with the coefficient `l2` of its L2 term) for the steps that follow."""
    check(lib().bb_trainer_set_loss(h, int(loss), float(l2)))


def trainer_step(h, n, boards, value, policy, noise=None, lr=0.0, apply=True, loss_out=None, stream=0):
    """bb_trainer_step: boards, value, policy, noise, loss_out are DEVICE addresses (ints; None/0 = absent).  Asynchronous."""
    check(lib().bb_trainer_step(h, int(n), C.c_void_p(boards or None), C.c_void_p(value or None), C.c_void_p(policy or None),
                                C.c_void_p(noise or None), float(lr), int(bool(apply)), C.c_void_p(loss_out or None),
                                C.c_void_p(stream or None)))


def trainer_epoch(h, n_records, records, n_batches, batch, order=None, sym=None, noise=None, lr=0.0, loss_out=None, bad=None,
                  stream=0):
    """bb_trainer_epoch: n_batches optimiser steps of `batch` rows each straight from the device records -- row j of batch i is
    record order[i * batch + j] (None: record i * batch + j) under symmetry sym[i * batch + j] (None: the identity).  records,
    order (int64), sym (uint8), noise (float32 [n_batches, A]; None: drawn), loss_out (float32 [n_batches, 4]) and bad (int32
    [1]) are DEVICE addresses (ints; None/0 = absent).  Asynchronous."""
    p = lambda a: C.c_void_p(a or None)  # noqa: E731
    check(lib().bb_trainer_epoch(h, int(n_records), p(records), int(n_batches), int(batch), p(order), p(sym), p(noise), float(lr),
                                 p(loss_out), p(bad), p(stream)))


def trainer_eval(h, n_records, records, n, index=None, sym=None, rows_out=None, flags_out=None, totals_out=None, bad=None, stream=0):
    """bb_trainer_eval: rows index[k] (None: record k) of the device records under sym[k] (None: the identity), scored with the
    trainer's current parameters.  records, index (int64), sym (uint8), rows_out (float32 [n, 3]), flags_out (uint8 [n]),
    totals_out (56 bytes, EVAL_TOTALS_DTYPE) and bad (int32 [1]) are DEVICE addresses (ints; None/0 = absent).  Asynchronous."""
    p = lambda a: C.c_void_p(a or None)  # noqa: E731
    check(lib().bb_trainer_eval(h, int(n_records), p(records), int(n), p(index), p(sym), p(rows_out), p(flags_out), p(totals_out),
                                p(bad), p(stream)))


def trainer_eval_tensors(h, n, boards, value, policy, rows_out=None, flags_out=None, totals_out=None, stream=0):
    """bb_trainer_eval_tensors: the same for rows given as bb_trainer_step's three device tensors.  Asynchronous."""
    p = lambda a: C.c_void_p(a or None)  # noqa: E731
    check(lib().bb_trainer_eval_tensors(h, int(n), p(boards), p(value), p(policy), p(rows_out), p(flags_out), p(totals_out), p(stream)))


def trainer_param_count(h):
    n = C.c_int64()
    check(lib().bb_trainer_param_count(h, C.byref(n)))
    return n.value


def trainer_read(h, what, count=None):
    """bb_trainer_read: a flat float32 array (count: the parameter count, or A for TRAIN_NOISE, when None)."""
    if count is None:
        count = trainer_param_count(h)
    out = np.zeros(int(count), dtype=np.float32)
    check(lib().bb_trainer_read(h, int(what), ptr(out), int(count)))
    return out


def temp_schedule(tempSchedule):
    """Model.SelfPlayTempSchedule / tempSchedule= of TestModelsBatched as (plies, lateTemp), or None for None.  ValueError for
    anything but a pair of an integer and a finite temperature >= 0 -- raised before any engine is made.  plies < 0 is the
    C ABI's "off": None."""
    if tempSchedule is None:
        return None
    try:
        plies, late = tempSchedule
    except (TypeError, ValueError):
        raise ValueError('tempSchedule must be a pair (plies, lateTemp), not {!r}'.format(tempSchedule)) from None
    if isinstance(plies, (bool, np.bool_)) or not isinstance(plies, (int, np.integer)):
        raise ValueError('tempSchedule: plies must be an integer, not {!r}'.format(plies))
    if isinstance(late, (bool, np.bool_)) or not isinstance(late, (int, float, np.integer, np.floating)) \
            or not (late >= 0 and np.isfinite(late)):
        raise ValueError('tempSchedule: lateTemp must be a finite temperature >= 0, not {!r}'.format(late))
    return (int(plies), float(late)) if plies >= 0 else None


def temp_at(temp, schedule, ply):
    """The temperature of the move out of ply `ply` under schedule (plies, lateTemp) or None."""
    return temp if schedule is None or ply < schedule[0] else schedule[1]


def fit_slots(game, n_slots, sims_per_move, *, mcts_kind=MCTS_DYNAMIC, max_depth=10, max_plies=None, max_games=None,
              node_capacity=0, device=0):
    """bb_fit_slots: (largest slot count <= n_slots whose pools fit the device's free memory, bytes per slot)."""
    if max_plies is None:
        max_plies = {GAME_CONNECT4: 42, GAME_TICTACTOE: 9}.get(game, 512)
    cfg = Config(game=game, n_slots=n_slots, mcts_kind=mcts_kind, max_depth=max_depth, evaluator=EVAL_NET,
                 sims_per_move=sims_per_move, max_plies=max_plies, max_games=max_games or n_slots, c_puct=1.0,
                 device=device, node_capacity=node_capacity)
    fit, per = C.c_int(), C.c_uint64()
    check(lib().bb_fit_slots(C.byref(cfg), C.byref(fit), C.byref(per)))
    return fit.value, per.value


# ---- engine ----------------------------------------------------------------------------------------------
class Engine:
    """One GPU-resident batch of search trees (bb_engine)."""

    def __init__(self, game, n_slots, sims_per_move, *, mcts_kind=MCTS_DYNAMIC, max_depth=10, evaluator=EVAL_NET,
                 c_puct=0.85, max_plies=None, max_games=None, seed=1234, hash_salt=0, first_game_id=0,
                 noise_on=False, alpha=0.2, epsilon=0.3, device=0, salt_per_game=False, node_capacity=0,
                 net_form=0, launch=0, general_net=False, track_ancestors=False, search_cache=False):
        """net_form: NET_FORM_AUTO / NET_FORM_F32 / NET_FORM_SPLIT (bb_config.net_form); launch: LAUNCH_AUTO / LAUNCH_LOCKSTEP /
        LAUNCH_ROUNDS / LAUNCH_WAVE (bb_config.launch; LAUNCH_WAVE is the search API's opt-in: run_sims_structure); general_net: a 16-filter network through the launch-per-layer kernels;
        search_cache: run_sims probes and fills the engine's evaluation cache where it searches in one launch with a network
        (bb_config.search_cache: same trees, fewer tower runs; bb_create refuses anything but 0 / 1)."""
        self.game = game
        self.info = game_info(game)
        if max_plies is None:
            max_plies = {GAME_CONNECT4: 42, GAME_TICTACTOE: 9}.get(game, 512)
        cfg = Config(game=game, n_slots=n_slots, mcts_kind=mcts_kind, max_depth=max_depth, evaluator=evaluator,
                     sims_per_move=sims_per_move, max_plies=max_plies, max_games=max_games or n_slots, c_puct=c_puct,
                     seed=seed, hash_salt=hash_salt, first_game_id=first_game_id, noise_on=int(noise_on), alpha=alpha,
                     epsilon=epsilon, device=device, salt_per_game=int(salt_per_game), node_capacity=node_capacity,
                     net_form=int(net_form), launch=int(launch), general_net=int(bool(general_net)),
                     track_ancestors=int(bool(track_ancestors)), search_cache=int(search_cache))
        self.cfg = cfg
        self.h = C.c_void_p()
        self.n_slots = n_slots
        self.max_plies = max_plies
        check(lib().bb_create(C.byref(cfg), C.byref(self.h)))
        self._weights_keep = None

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            lib().bb_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def load_weights(self, flat):
        """flat: dict from blackbird_amd.weights.flatten()."""
        w, self._weights_keep = net_weights(self.info.H, self.info.W, flat)
        check(lib().bb_load_weights(self.h, C.byref(w)))

    def load_weights_device(self, desc, stream=0):
        """bb_load_weights_device: `desc` a NetWeights whose pointers are device addresses on this engine's device (the
        current device; net_weights_device builds one), `stream` a hipStream_t handle.  The engine must have had load_weights
        with a network of the same shape: that call allocates the buffers this one fills.  What `desc` points into must stay
        alive until `stream` has passed this call (torch: record_stream)."""
        check(lib().bb_load_weights_device(self.h, C.byref(desc), C.c_void_p(stream or None)))

    def weights_image(self, which):
        """bb_weights_read: one operand buffer of the engine as a uint8 array -- `which` one of WEIGHTS_IMAGES (or its index):
        the float32 'w0', 'wt', 'epi', the 'head' array, 'x3' the bf16 images back to back (empty without them).  Layouts:
        csrc/net_pack.h."""
        k = WEIGHTS_IMAGES.index(which) if isinstance(which, str) else int(which)
        n = C.c_int64()
        check(lib().bb_weights_read(self.h, k, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        check(lib().bb_weights_read(self.h, k, ptr(out), out.nbytes, C.byref(n)))
        return out

    def counters(self):
        c = Counters()
        check(lib().bb_get_counters(self.h, C.byref(c)))
        return {n: getattr(c, n) for n, _ in Counters._fields_}

    def reset_counters(self):
        check(lib().bb_reset_counters(self.h))

    def synchronize(self):
        check(lib().bb_synchronize(self.h))

    def set_sims_per_move(self, sims):
        check(lib().bb_set_sims_per_move(self.h, int(sims)))

    def timing_enable(self, every_n):
        check(lib().bb_timing_enable(self.h, int(every_n)))

    def timing_read(self):
        m, mn, c = C.c_double(), C.c_double(), C.c_int()
        check(lib().bb_timing_read(self.h, C.byref(m), C.byref(mn), C.byref(c)))
        return m.value, mn.value, c.value

    def selfplay_mode(self):
        return check(lib().bb_selfplay_mode(self.h))

    def net_form(self):
        """0 float32-MFMA fused tower, 1 general-filter launches, 2 fused tower on the bf16 matrix pipe (float32 by operand
        splitting), 3 general-filter launches with such tower layers (bb_net_form)."""
        return check(lib().bb_net_form(self.h))

    def net_eval_structure(self, n):
        """bb_net_eval_structure: NET_EVAL_FUSED, or for the launch-per-layer network NET_EVAL_SMALL / NET_EVAL_BATCH -- how a
        net_eval call of n positions is cut into launches (the same bits either way).  Launches nothing."""
        out = C.c_int32(-1)
        check(lib().bb_net_eval_structure(self.h, int(n), C.byref(out)))
        return out.value

    def timing_net(self, iters=50, noise=True, ablate=0):
        ms = C.c_double()
        check(lib().bb_timing_net(self.h, int(iters), int(noise), int(ablate), C.byref(ms)))
        return ms.value

    def net_eval(self, states=None, planes=None, noise=False):
        A = self.info.A
        if states is not None:
            states = np.ascontiguousarray(states)
            n = states.shape[0]
        else:
            planes = np.ascontiguousarray(planes, dtype=np.int8)
            n = planes.shape[0]
        value = np.zeros(n, dtype=np.float32)
        logits = np.zeros((n, A), dtype=np.float32)
        policy = np.zeros((n, A), dtype=np.float32)
        check(lib().bb_net_eval(self.h, n, ptr(states), ptr(planes), ptr(value), ptr(logits), ptr(policy), int(noise)))
        return value, logits, policy

    def net_eval_keyed(self, game_ids, node_serials, states=None, planes=None):
        """bb_net_eval_keyed: the forward pass with the prior noise of (global game id, node serial) per position --
        exactly the priors a self-play kernel uses for that node."""
        A = self.info.A
        if states is not None:
            states = np.ascontiguousarray(states)
            n = states.shape[0]
        else:
            planes = np.ascontiguousarray(planes, dtype=np.int8)
            n = planes.shape[0]
        gids = np.ascontiguousarray(game_ids, dtype=np.uint32).reshape(n)
        sers = np.ascontiguousarray(node_serials, dtype=np.int32).reshape(n)
        value = np.zeros(n, dtype=np.float32)
        logits = np.zeros((n, A), dtype=np.float32)
        policy = np.zeros((n, A), dtype=np.float32)
        check(lib().bb_net_eval_keyed(self.h, n, ptr(states), ptr(planes), ptr(gids), ptr(sers), ptr(value), ptr(logits),
                                      ptr(policy)))
        return value, logits, policy

    def set_rng_stream(self, seed, first_game_id=0):
        check(lib().bb_set_rng_stream(self.h, C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint32(int(first_game_id) & 0xFFFFFFFF)))
        self.cfg.seed = int(seed) & (2 ** 64 - 1)
        self.cfg.first_game_id = int(first_game_id) & 0xFFFFFFFF

    def hash_eval(self, states):
        states = np.ascontiguousarray(states)
        n = states.shape[0]
        value = np.zeros(n, dtype=np.float32)
        policy = np.zeros((n, self.info.A), dtype=np.float32)
        check(lib().bb_hash_eval(self.h, n, ptr(states), ptr(value), ptr(policy)))
        return value, policy

    def set_roots(self, states, slots=None, game_ids=None):
        states = np.ascontiguousarray(states)
        n = states.shape[0]
        slots = None if slots is None else np.ascontiguousarray(slots, dtype=np.int32)
        gids = None if game_ids is None else np.ascontiguousarray(game_ids, dtype=np.uint32)
        check(lib().bb_set_roots(self.h, n, ptr(slots), ptr(states), ptr(gids)))

    def run_sims(self, sims, mask=None):
        if mask is None:
            check(lib().bb_run_sims(self.h, int(sims)))
        else:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            assert mask.shape[0] == self.n_slots
            check(lib().bb_run_sims_masked(self.h, int(sims), ptr(mask)))

    def run_sims_structure(self):
        """bb_run_sims_structure: LAUNCH_LOCKSTEP or LAUNCH_WAVE -- what run_sims launches for this engine as it stands (after
        load_weights): an engine that asked for LAUNCH_WAVE and cannot have it says so here, never silently."""
        out = C.c_int32(-1)
        check(lib().bb_run_sims_structure(self.h, C.byref(out)))
        return out.value

    def search_rollouts(self, on=True):
        """bb_search_rollouts: let a rollout engine created with launch=LAUNCH_WAVE search in one launch as well (the same trees
        bit for bit; run_sims_structure() reports it).  Accepted and without effect on any other engine."""
        check(lib().bb_search_rollouts(self.h, int(bool(on))))

    def selfplay_rollouts(self, on=True):
        """bb_selfplay_rollouts: let a rollout engine play selfplay_step in one launch per call, a wave per slot (the same
        records, headers and counters byte for byte; selfplay_mode() reports 6).  Accepted and without effect on any other engine."""
        check(lib().bb_selfplay_rollouts(self.h, int(bool(on))))

    def sample_moves(self, temp, u=None):
        n, S = self.n_slots, self.info.S
        u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        out = dict(action=np.zeros(n, np.int32), root_winrate=np.zeros(n, np.float32),
                   root_plays=np.zeros(n, np.int32), child_action=np.zeros((n, S), np.int32),
                   child_plays=np.zeros((n, S), np.int32), child_value=np.zeros((n, S), np.float32))
        check(lib().bb_sample_moves(self.h, float(temp), ptr(u), ptr(out["action"]), ptr(out["root_winrate"]),
                                    ptr(out["root_plays"]), ptr(out["child_action"]), ptr(out["child_plays"]),
                                    ptr(out["child_value"])))
        return out

    def move_roots(self, actions):
        actions = np.ascontiguousarray(actions, dtype=np.int32)
        assert actions.shape[0] == self.n_slots
        check(lib().bb_move_roots(self.h, ptr(actions)))

    def reset_roots(self):
        """bb_reset_roots: MCTS.ResetRoot for every slot."""
        check(lib().bb_reset_roots(self.h))

    def node_view(self, slot=0, node=-1):
        """bb_node_view: dict(child, plays, value [S], state (packed), flags, legal_mask, node)."""
        S = self.info.S
        child, plays, value = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.float32)
        state = np.zeros((1, self.info.state_bytes), dtype=np.uint8)
        info = np.zeros(3, np.int32)
        check(lib().bb_node_view(self.h, int(slot), int(node), ptr(child), ptr(plays), ptr(value), ptr(state), ptr(info)))
        return dict(child=child, plays=plays, value=value, state=state.view(STATE_DTYPE[self.game]), flags=int(info[0]),
                    legal_mask=int(np.uint32(info[1])), node=int(info[2]))

    def node_edges(self, slot=0, node=-1):
        """bb_node_edges: dict(action, child, plays, value [S] -- entry k is one child, action -1: none --, state (packed), flags,
        n_children, node).  Every game: the dense ones put action i at entry i."""
        S = self.info.S
        action, child = np.zeros(S, np.int32), np.zeros(S, np.int32)
        plays, value = np.zeros(S, np.int32), np.zeros(S, np.float32)
        state = np.zeros((1, self.info.state_bytes), dtype=np.uint8)
        info = np.zeros(3, np.int32)
        check(lib().bb_node_edges(self.h, int(slot), int(node), ptr(action), ptr(child), ptr(plays), ptr(value), ptr(state),
                                  ptr(info)))
        return dict(action=action, child=child, plays=plays, value=value, state=state.view(STATE_DTYPE[self.game]),
                    flags=int(info[0]), n_children=int(info[1]), node=int(info[2]))

    def root_states(self):
        buf = np.zeros((self.n_slots, self.info.state_bytes), dtype=np.uint8)
        check(lib().bb_get_root_states(self.h, ptr(buf)))
        return buf.view(STATE_DTYPE[self.game])

    def selfplay_begin(self, n_games, temp):
        check(lib().bb_selfplay_begin(self.h, int(n_games), float(temp)))
        self._n_games = int(n_games)

    def selfplay_set_starts(self, states):
        """bb_selfplay_set_starts: `states` = packed states [n, ...] (as set_roots takes them): game k of every later
        selfplay_begin starts from states[k % n].  None or an empty array clears the table (initial positions again).  A state
        a game cannot start from raises ValueError naming its index and the reason; the previous table then stays."""
        n = 0 if states is None else int(np.asarray(states).shape[0])
        if n == 0:
            check(lib().bb_selfplay_set_starts(self.h, 0, None))
            return
        states = np.ascontiguousarray(states)
        if states.nbytes != n * self.info.state_bytes:
            raise ValueError("start states: %d bytes for %d states of %d bytes each" % (states.nbytes, n, self.info.state_bytes))
        check(lib().bb_selfplay_set_starts(self.h, n, ptr(states)))

    def selfplay_set_temp_schedule(self, plies, temp_late=0.0):
        """bb_selfplay_set_temp_schedule: in every later selfplay_begin the move out of ply p (counted from the game's start
        position) is drawn at begin's temp while p < plies and at temp_late from there on.  plies < 0 (or None) turns it off."""
        check(lib().bb_selfplay_set_temp_schedule(self.h, -1 if plies is None else int(plies), float(temp_late)))

    def selfplay_step(self, plies=1):
        check(lib().bb_selfplay_step(self.h, int(plies)))

    def selfplay_done(self):
        d, f = C.c_int(), C.c_int()
        check(lib().bb_selfplay_done(self.h, C.byref(d), C.byref(f)))
        return bool(d.value), f.value

    def fetch_examples(self, first_game=0, n_games=None):
        n_games = self._n_games if n_games is None else n_games
        dt = example_dtype(self.game)
        cap = n_games * (self.max_plies + 1)
        rec = np.zeros(cap, dtype=dt)
        offs = np.zeros(n_games + 1, dtype=np.int32)
        win = np.zeros(n_games, dtype=np.int8)
        k = check(lib().bb_examples_fetch(self.h, first_game, n_games, ptr(rec), cap, ptr(offs), ptr(win)))
        return rec[:k], offs, win

    def selfplay_headers(self, first_game=0, n_games=None):
        """bb_selfplay_headers: int32 [n_games][4] = (n_examples, winner, plies, done)."""
        n_games = self._n_games if n_games is None else n_games
        hdr = np.zeros((n_games, 4), dtype=np.int32)
        check(lib().bb_selfplay_headers(self.h, int(first_game), int(n_games), ptr(hdr)))
        return hdr

    def fetch_games(self, game_ids, n_records=None):
        """bb_examples_fetch_games: the records of the listed (finished) games, compacted in list order."""
        ids = np.ascontiguousarray(game_ids, dtype=np.int32)
        cap = int(n_records) if n_records is not None else len(ids) * (self.max_plies + 1)
        rec = np.zeros(max(cap, 1), dtype=example_dtype(self.game))
        offs = np.zeros(len(ids) + 1, dtype=np.int32)
        win = np.zeros(len(ids), dtype=np.int8)
        k = check(lib().bb_examples_fetch_games(self.h, len(ids), ptr(ids), ptr(rec), cap, ptr(offs), ptr(win)))
        return rec[:k], offs, win

    def score_workspace(self, rows_per_chunk):
        """bb_examples_score_workspace: the bytes of scratch memory score_examples needs for chunks of rows_per_chunk rows.  Host
        only."""
        out = C.c_uint64(0)
        check(lib().bb_examples_score_workspace(self.h, int(rows_per_chunk), C.byref(out)))
        return int(out.value)

    def score_examples(self, n_records, records, n, index=None, rows_out=None, flags_out=None, totals_out=None, bad=None,
                       workspace=None, workspace_bytes=0, stream=0):
        """bb_examples_score: rows index[k] (None: record k) of the device records scored with the network this engine holds --
        any game, width and net form.  records, index (int64), rows_out (float32 [n, 3]), flags_out (uint8 [n]), totals_out (56
        bytes, EVAL_TOTALS_DTYPE), bad (int32 [1]) and workspace (score_workspace bytes for the chunk size wanted) are DEVICE
        addresses on the engine's device (ints; None/0 = absent).  Waits for the engine's own streams, then runs behind what
        `stream` holds; `stream` waits for the figures.  Asynchronous for `stream`."""
        p = lambda a: C.c_void_p(a or None)  # noqa: E731
        check(lib().bb_examples_score(self.h, int(n_records), p(records), int(n), p(index), p(rows_out), p(flags_out), p(totals_out),
                                      p(bad), p(workspace), int(workspace_bytes), p(stream)))

    def examples_device(self):
        """bb_examples_device: (records device pointer, bytes, record bytes, game header device pointer)."""
        p, hdr = C.c_void_p(), C.c_void_p()
        nb, rb = C.c_uint64(), C.c_uint64()
        check(lib().bb_examples_device(self.h, C.byref(p), C.byref(nb), C.byref(rb), C.byref(hdr)))
        return p.value, nb.value, rb.value, hdr.value


class Arena:
    """Head-to-head games of two engines on the device (bb_arena): `a` is model1, `b` model2, one game per slot index.  The
    engines are borrowed and must stay open -- and unused by anything else -- until close()."""

    def __init__(self, a, b, log_plies=0):
        self.a, self.b = a, b
        self.log_plies = int(log_plies)
        self.n_games = 0
        self.h = C.c_void_p()
        check(lib().bb_arena_create(a.h, b.h, self.log_plies, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            lib().bb_arena_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def begin(self, first, temp, start_states=None):
        """first: bool [n_games], a moves first in game i; start_states: packed states [n_games, ...] or None (initial position)."""
        first = np.ascontiguousarray(first, dtype=np.uint8)
        n = int(first.shape[0])
        if start_states is not None:
            start_states = np.ascontiguousarray(start_states)
            if start_states.nbytes != n * self.a.info.state_bytes:
                raise ValueError("start states: %d bytes for %d games of %d bytes each" % (start_states.nbytes, n, self.a.info.state_bytes))
        check(lib().bb_arena_begin(self.h, n, ptr(first), ptr(start_states), float(temp)))
        self.n_games = n

    def set_temp_schedule(self, plies, temp_late=0.0):
        """bb_arena_set_temp_schedule, before begin(): ply p of the match is sampled at begin's temp while p < plies, at temp_late
        from there on.  plies < 0 (or None) turns it off."""
        check(lib().bb_arena_set_temp_schedule(self.h, -1 if plies is None else int(plies), float(temp_late)))

    def step(self, plies=1):
        check(lib().bb_arena_step(self.h, int(plies)))

    def status(self):
        """Waits; the number of games still running.  Raises BlackbirdHipError when a tree outgrew its node pool, ValueError when a
        game stopped on NaN probabilities."""
        alive = C.c_int()
        check(lib().bb_arena_status(self.h, C.byref(alive)))
        return alive.value

    def fetch(self):
        """dict(result int8 [n], plies int32 [n], moves int32 [n, log_plies] (-1 padded), states (packed) [n, ...])."""
        n = self.n_games
        out = dict(result=np.zeros(n, np.int8), plies=np.zeros(n, np.int32), moves=np.full((n, self.log_plies), -1, np.int32))
        states = np.zeros((n, self.a.info.state_bytes), dtype=np.uint8)
        check(lib().bb_arena_fetch(self.h, ptr(out["result"]), ptr(out["plies"]), ptr(out["moves"]) if self.log_plies else None,
                                   ptr(states)))
        out["states"] = states.view(STATE_DTYPE[self.a.game])
        return out
