"""Support shared by the tests of merging duplicate positions (not collected): hand-built example records from
_lib.example_dtype and _lib.pack_grid -- no GPU is needed to make them --, the deliberately naive statement of a merge as a
Python dict loop, and the record sets the CPU and the GPU tests both use."""
import numpy as np

from blackbird_amd import _lib

C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
SHAPE = {C4: (6, 7, 4, 7, 8), TTT: (3, 3, 3, 9, 16)}  # H, W, K in a row, A, S
CELLS = np.uint64(0x00FFFFFFFFFFFFFF)


# ---- the rules, enough of them for legal random playouts -----------------------------------------------------------------------
def legal(game, cells):
    """cells [H, W] in {0, 1, 2} (Connect4: row 0 is the bottom) -> the legal actions"""
    H, W = cells.shape
    if game == C4:
        return [c for c in range(W) if cells[H - 1, c] == 0]
    return [i for i in range(H * W) if cells.reshape(-1)[i] == 0]


def play(game, cells, action, player):
    H, W = cells.shape
    out = cells.copy()
    if game == C4:
        out[int(np.flatnonzero(out[:, action] == 0)[0]), action] = player
    else:
        out[action // W, action % W] = player
    return out


def won(game, cells, player):
    H, W = cells.shape
    K = SHAPE[game][2]
    mine = cells == player
    for r in range(H):
        for c in range(W):
            for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
                rr, cc = r + (K - 1) * dr, c + (K - 1) * dc
                if 0 <= rr < H and 0 <= cc < W and all(mine[r + i * dr, c + i * dc] for i in range(K)):
                    return True
    return False


# ---- records -------------------------------------------------------------------------------------------------------------------
def record(game, cells, player, *, prev=0, z=0, visits=None, total=None, n_children=None, game_id=0, ply=0):
    """One example record: cells [H, W] in {0, 1, 2}, the side to move, and the targets.  visits: A counts (None: a terminal
    example, no visits); total: their sum unless given; n_children: the number of non-zero visits unless given."""
    H, W, _K, A, _S = SHAPE[game]
    r = np.zeros(1, dtype=_lib.example_dtype(game))
    boards = np.zeros((1, H, W, 2), dtype=np.int8)
    boards[0, ..., 0] = cells == 1
    boards[0, ..., 1] = cells == 2
    r["state"] = _lib.pack_grid(game, boards, [player], [prev]).view(np.uint8).reshape(1, -1)
    v = np.zeros(A, dtype=np.uint32) if visits is None else np.asarray(visits, dtype=np.uint32)
    r["visits"][0, :A] = v
    r["total"] = int(v.sum()) if total is None else total
    r["n_children"] = int((v > 0).sum()) if n_children is None else n_children
    r["game_id"], r["ply"], r["player"], r["z"] = game_id, ply, player, z
    return r[0]


def stack(rows, game):
    return np.array(rows, dtype=_lib.example_dtype(game))


def _visits(game, cells, rng):
    A = SHAPE[game][3]
    v = np.zeros(A, dtype=np.uint32)
    acts = legal(game, cells)
    v[acts] = rng.randint(0, 200, len(acts))
    return v


def playout_records(game, n, seed, distinct=False):
    """n records along random legal games from the empty board, each with random visits on its legal actions, a random outcome
    and the terminal example (no visits, total 0) at the end of its game; distinct: no position twice."""
    rng = np.random.RandomState(seed)
    H, W = SHAPE[game][:2]
    rows, seen, g = [], set(), 0
    while len(rows) < n:
        cells, player, prev, ply = np.zeros((H, W), dtype=np.int8), 1, 0, 0
        while len(rows) < n:
            over = won(game, cells, 3 - player) or not legal(game, cells)
            row = record(game, cells, player, prev=prev, z=int(rng.randint(-1, 2)), visits=None if over else _visits(game, cells, rng),
                         game_id=g, ply=ply)
            k = key_of(row)
            if not distinct or k not in seen:
                rows.append(row)
                seen.add(k)
            if over:
                break
            cells, prev = play(game, cells, int(rng.choice(legal(game, cells))), player), player
            player, ply = 3 - player, ply + 1
        g += 1
    return stack(rows, game)


def with_duplicates(game, rec, seed):
    """rec plus a copy of a third of its records -- the same state, targets of their own -- shuffled"""
    rng = np.random.RandomState(seed)
    extra = rec[rng.choice(len(rec), len(rec) // 3, replace=False)].copy()
    A = SHAPE[game][3]
    live = extra["total"] > 0
    extra["visits"][:, :A] = np.where((extra["visits"][:, :A] > 0) & live[:, None], rng.randint(1, 300, (len(extra), A)), 0)
    extra["total"] = extra["visits"].sum(axis=1)
    extra["z"] = rng.randint(-1, 2, len(extra))
    extra["game_id"] += 1000
    both = np.concatenate([rec, extra])
    return both[rng.permutation(len(both))]


def dict_loop_input(game, seed=3):
    """300 records: 225 from random legal playouts (the empty board and the openings repeat by themselves), a third of them
    copied with other targets, shuffled"""
    out = with_duplicates(game, playout_records(game, 225, seed), seed + 1)
    assert len(out) == 300
    return out


# ---- the naive statement ---------------------------------------------------------------------------------------------------------
def key_of(row):
    """the position key of one record, from its bytes: both players' cells and the side to move"""
    p1, p2 = (int(x) for x in np.frombuffer(np.asarray(row["state"]).tobytes(), dtype="<u8"))
    return (p1 & int(CELLS), p2 & int(CELLS), (p1 >> 56) & 3)


def dict_merge(game, rec):
    """merge_records_host as a loop over the records with a dict from key to group: Python integers, nothing vectorised"""
    _H, _W, _K, A, S = SHAPE[game]
    groups, group, rep, count, zsum, total, visits = {}, [], [], [], [], [], []
    for i, row in enumerate(rec):
        if int(row["n_children"]) > S:
            group.append(-1)
            continue
        k = key_of(row)
        if k not in groups:
            groups[k] = len(rep)
            rep.append(i)
            count.append(0)
            zsum.append(0)
            total.append(0)
            visits.append([0] * A)
        g = groups[k]
        group.append(g)
        count[g] += 1
        zsum[g] += int(row["z"])
        total[g] += int(row["total"])
        for a in range(A):
            visits[g][a] += int(row["visits"][a])
    return (np.array(group, dtype=np.int32).reshape(-1), np.array(rep, dtype=np.int32), np.array(count, dtype=np.int32),
            np.array(zsum, dtype=np.int32), np.array(total, dtype=np.uint64), np.array(visits, dtype=np.uint64).reshape(-1, A))


NAMES = ("group", "rep", "count", "zsum", "total", "visits")


def same_merge(got, want):
    """two results of a merge, array for array, exactly (64-bit sums compared as integers whatever their signedness)"""
    for g, w, what in zip(got, want, NAMES):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, g.shape, w.shape)
        assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), (what, int((g.astype(np.int64) != w.astype(np.int64)).sum()))


def rows_of(rec, merged):
    """the merged rows the definition gives, in float64 arithmetic rounded once: (value [G], policy [G, A])"""
    _group, _rep, count, zsum, total, visits = merged
    value = (zsum.astype(np.float64) / count.astype(np.float64)).astype(np.float32)
    tot = total.astype(np.float64)[:, None]
    policy = np.where(tot > 0, visits.astype(np.float64) / np.maximum(tot, 1.0), 0.0).astype(np.float32)
    return value, policy


# ---- the shapes of the GPU tests ---------------------------------------------------------------------------------------------------
def _positions(game, k, seed, terminal_last=False):
    """k different positions (cells, player, is it over), the last one a finished game if asked"""
    rec = playout_records(game, 400, seed, distinct=True)
    live, over = rec[rec["total"] > 0], rec[rec["total"] == 0]
    pick = list(live[:k - 1]) + [over[0] if terminal_last else live[k - 1]]
    assert len({key_of(r) for r in pick}) == k
    return pick


def copies(game, positions, n, seed, malformed=()):
    """n records cycling through `positions` (record i is a copy of position i % k with targets of its own); the records whose
    index is in `malformed` say n_children = S + 1"""
    rng = np.random.RandomState(seed)
    A, S = SHAPE[game][3:]
    out = stack([positions[i % len(positions)] for i in range(n)], game)
    live = out["total"] > 0
    out["visits"][:, :A] = np.where((out["visits"][:, :A] > 0) & live[:, None], rng.randint(1, 500, (n, A)), 0)
    out["total"] = out["visits"].sum(axis=1)
    out["z"] = rng.randint(-1, 2, n)
    out["game_id"], out["ply"] = np.arange(n), rng.randint(0, 40, n)
    for i in malformed:
        out["n_children"][i] = S + 1
    return out


def gpu_shapes(game):
    """name -> records: the shapes of tests/test_gpu_examples_merge.py (built once per game by its caller)"""
    one = _positions(game, 9, 11, terminal_last=True)
    two = copies(game, one[:1], 2, 2)
    two[1] = two[0]
    shapes = {
        "n=1": copies(game, one[:1], 1, 1),
        "n=2 identical": two,
        "n=5 one position": copies(game, one[1:2], 5, 3),
        "n=67 nine groups": copies(game, one, 67, 4, malformed=(30,)),
        "n=1000 three positions": copies(game, one[:3], 1000, 5),
    }
    if game == C4:
        shapes["n=1000 all distinct"] = playout_records(game, 1000, 6, distinct=True)
    return shapes
