"""The board symmetries of csrc/symmetry.h on the CPU.  A stand-alone program, compiled with the host compiler from the header
alone, prints NSYM and the four maps (cell, inverse cell, action, inverse action) of every game.  They must be permutations with
the inverses the header claims, a group with the identity at index 0, the images numpy gives (np.flip for Connect4, the eight
rot90 / flip images of the square for TicTacToe, in the order the header writes down) -- and symmetries of the RULES: along
random games of the oracle, the position reached by the mapped moves has the mapped legal moves, the same winner and the
cell-mapped input planes.  That last part is what pins the action map.  Then what needs the built library but no GPU: the two
new entry points are exported and bound, an empty batch is a no-op, bb_game_symmetries answers 2, 8, 1, and the host-side range
checks of DeviceExamples.batch(sym=...) and TrainWithDeviceExamples(augment=True)."""
import numpy as np
import pytest

from tests.host_cases import C4, DC, NSYM, SHAPE, TTT, maps  # noqa: F401  (maps: a fixture)

def test_counts(maps):
    assert {g: m["nsym"] for g, m in maps.items()} == NSYM


@pytest.mark.parametrize("game", [C4, TTT, DC])
def test_maps_are_permutations_with_their_inverses_and_a_group(maps, game):
    m = maps[game]
    H, W, A = SHAPE[game]
    for kind, size in (("cell", H * W), ("action", A)):
        fwd, inv = m[kind], m[kind + "_inv"]
        assert fwd.shape == inv.shape == (m["nsym"], size)
        ident = np.arange(size)
        assert np.array_equal(fwd[0], ident) and np.array_equal(inv[0], ident)  # index 0 is the identity
        for s in range(m["nsym"]):
            assert np.array_equal(np.sort(fwd[s]), ident) and np.array_equal(np.sort(inv[s]), ident)
            assert np.array_equal(inv[s][fwd[s]], ident) and np.array_equal(fwd[s][inv[s]], ident)
            assert np.array_equal(inv[s], fwd[m["inverse"][s]])
    # closed under composition, cell and action map together: "t after s" is one of the listed symmetries, in both maps
    pairs = [(tuple(m["cell"][s]), tuple(m["action"][s])) for s in range(m["nsym"])]
    assert len(set(pairs)) == m["nsym"] and len(set(p[0] for p in pairs)) == m["nsym"]
    for s in range(m["nsym"]):
        for t in range(m["nsym"]):
            assert (tuple(m["cell"][t][m["cell"][s]]), tuple(m["action"][t][m["action"][s]])) in pairs, (s, t)


def _image_by_maps(m, s, grid):
    """the board `grid` under symmetry s, once scattered by the cell map and once gathered by its inverse"""
    scattered = np.empty(grid.size, dtype=grid.dtype)
    scattered[m["cell"][s]] = grid.ravel()
    gathered = grid.ravel()[m["cell_inv"][s]]
    assert np.array_equal(scattered, gathered)
    return gathered.reshape(grid.shape)


def test_connect4_is_the_column_mirror(maps):
    m = maps[C4]
    g = np.arange(42).reshape(6, 7)
    assert np.array_equal(_image_by_maps(m, 0, g), g)
    assert np.array_equal(_image_by_maps(m, 1, g), np.flip(g, axis=1))
    assert np.array_equal(m["action"][1], 6 - np.arange(7)) and np.array_equal(m["action_inv"][1], 6 - np.arange(7))


def test_tictactoe_is_the_dihedral_group_in_the_order_the_header_gives(maps):
    m = maps[TTT]
    g = np.arange(9).reshape(3, 3)
    want = [g, g.T, np.flipud(g), np.rot90(g, 1), np.fliplr(g), np.rot90(g, -1), np.rot90(g, 2), np.rot90(g, 2).T]
    eight = {np.rot90(f, k).tobytes() for f in (g, np.fliplr(g)) for k in range(4)}
    assert len(eight) == 8 and {w.tobytes() for w in want} == eight  # the eight rot90 / flip images, each once
    for s in range(8):
        assert np.array_equal(_image_by_maps(m, s, g), want[s]), s
        assert np.array_equal(m["action"][s], m["cell"][s])  # an action is its cell
    assert list(m["inverse"]) == [0, 1, 2, 5, 4, 3, 6, 7]  # only the quarter turns are not their own inverses


# ---- against the rules: the oracle's game functions ----------------------------------------------------------------------
N_GAMES = {C4: 16, TTT: 48}  # random games; every position of them is looked at: a few hundred per game


def _random_games(orc, game, n_games, seed):
    """[(moves)] of random legal play from the start to the end of the game"""
    rng = np.random.RandomState(seed)
    games = []
    for _ in range(n_games):
        st, moves, prev = orc.new_state(game), [], None
        while orc.winner(game, st, prev) is None:
            prev = int(rng.choice(np.nonzero(orc.legal(game, st))[0]))
            assert orc.apply(game, st, prev) == 0
            moves.append(prev)
        games.append(moves)
    return games


@pytest.mark.parametrize("game", [C4, TTT])
def test_maps_are_symmetries_of_the_rules(orc, maps, game):
    m = maps[game]
    H, W, A = SHAPE[game]
    assert orc.dims(game)[:2] == (H, W) and orc.dims(game)[3] == A
    positions, wins = 0, set()
    for moves in _random_games(orc, game, N_GAMES[game], seed=11 + game):
        for s in range(m["nsym"]):
            act, cell = m["action"][s], m["cell"][s]
            a_st, b_st = orc.new_state(game), orc.new_state(game)  # the game as played; rebuilt from the mapped moves
            for ply in range(len(moves) + 1):
                prev = moves[ply - 1] if ply else None
                # legal moves: action a of the original is action act[a] of the image
                la, lb = orc.legal(game, a_st), orc.legal(game, b_st)
                mapped = np.empty_like(la)
                mapped[act] = la
                assert np.array_equal(lb, mapped), (s, ply)
                # the winner, by the last move and by the whole-board scan
                wa = orc.winner(game, a_st, prev)
                assert orc.winner(game, b_st, None if prev is None else int(act[prev])) == wa, (s, ply)
                assert orc.winner(game, b_st) == orc.winner(game, a_st), (s, ply)
                # input planes: cell i of the original is cell cell[i] of the image, plane by plane
                pa, pb = orc.encode(game, a_st)[0].reshape(H * W, -1), orc.encode(game, b_st)[0].reshape(H * W, -1)
                moved = np.empty_like(pa)
                moved[cell] = pa
                assert np.array_equal(pb, moved), (s, ply)
                if s == 0:
                    positions += 1
                    wins.add(wa)
                if ply < len(moves):
                    assert orc.apply(game, a_st, moves[ply]) == 0 and orc.apply(game, b_st, int(act[moves[ply]])) == 0
    assert positions >= 200 and {1, 2} <= wins  # both sides won somewhere: the winner check was not vacuous


def test_a_wrong_action_map_would_be_caught(orc, maps):
    """The rules check has teeth: Connect4's mirror with the identity as its action map fails it on the first asymmetric move."""
    st, img = orc.new_state(C4), orc.new_state(C4)
    assert orc.apply(C4, st, 0) == 0 and orc.apply(C4, img, 0) == 0
    pa, pb = orc.encode(C4, st)[0].reshape(42, -1), orc.encode(C4, img)[0].reshape(42, -1)
    moved = np.empty_like(pa)
    moved[maps[C4]["cell"][1]] = pa
    assert not np.array_equal(pb, moved)


# ---- the library, without a GPU ---------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_bound():
    from blackbird_amd import _lib
    for name in ("bb_examples_to_batch_sym", "bb_game_symmetries"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert callable(_lib.examples_to_batch_sym) and callable(_lib.game_symmetries)


def test_game_symmetries(maps):
    from blackbird_amd import _lib
    assert [_lib.game_symmetries(g) for g in (_lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS)] == [2, 8, 1]
    for g in (C4, TTT, DC):
        assert _lib.game_symmetries(g) == maps[g]["nsym"]
    for unknown in (3, -1, 99):
        assert _lib.lib().bb_game_symmetries(unknown) == _lib.ERR_ARG
        with pytest.raises(ValueError):
            _lib.game_symmetries(unknown)


def test_empty_batch_needs_no_gpu():
    from blackbird_amd import _lib
    for game in (_lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS):
        _lib.examples_to_batch_sym(game, 0, None, 0)
        _lib.examples_to_batch_sym(game, 5, None, 0, index=None, sym=None, boards=None, policy=None, value=None, bad=None, stream=0)
        assert _lib.lib().bb_examples_to_batch_sym(game, 5, None, 0, None, None, None, None, None, None, None) == _lib.OK
    with pytest.raises(ValueError):
        _lib.examples_to_batch_sym(_lib.GAME_CONNECT4, 5, None, -1)
    with pytest.raises(ValueError):
        _lib.examples_to_batch_sym(_lib.GAME_CONNECT4, 5, None, 3)  # no records (checked before anything is launched)


def test_batch_checks_a_host_sym_on_the_host():
    import torch
    from blackbird_amd import _lib
    from blackbird_amd.training import DeviceExamples
    for game, nsym in ((_lib.GAME_CONNECT4, 2), (_lib.GAME_TICTACTOE, 8), (_lib.GAME_DRAGONCHESS, 1)):
        ex = DeviceExamples.from_records(game, np.zeros(3, dtype=_lib.example_dtype(game)), "cpu")
        assert ex.symmetries == nsym
        for wrong in ([0, nsym, 0], [0, 0, 255], [-1, 0, 0], np.array([0, 0, nsym], dtype=np.uint8), torch.tensor([0, nsym, 0]),
                      [0.0, 1.0, 0.0]):
            with pytest.raises(ValueError):
                ex.batch(sym=wrong)
            with pytest.raises(ValueError):
                ex.batch([2, 1, 0], sym=wrong)
        with pytest.raises(ValueError):
            ex.batch([0, 1], sym=[0, 0, 0])           # one entry per output row
        t = ex.sym_tensor([nsym - 1, 0, 0])
        assert t.dtype == torch.uint8 and t.tolist() == [nsym - 1, 0, 0]
        with pytest.raises(_lib.BlackbirdHipError):  # a good sym, records on the host: there is no CPU path, and none is faked
            ex.batch(sym=[nsym - 1, 0, 0])
        gi = _lib.game_info(game)
        boards, value, policy = ex.batch(np.zeros(0, dtype=np.int64), sym=[])
        assert boards.shape == (0, gi.H, gi.W, gi.C) and value.shape == (0,) and policy.shape == (0, gi.A)


def test_augment_is_refused_for_dragonchess_before_any_device_call(tmp_path, monkeypatch):
    from blackbird_amd import Blackbird, DragonChess, _lib
    from blackbird_amd.training import DeviceExamples
    monkeypatch.chdir(tmp_path)

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "examples_to_batch_sym", no_device)
    monkeypatch.setattr(_lib, "examples_to_batch", no_device)
    monkeypatch.setattr(_lib, "Engine", no_device)
    cfg = {"blocks": 1, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}
    m = Blackbird.Model(DragonChess.BoardState, "dc", {"explorationRate": 0.85, "playLimit": 4}, cfg)
    monkeypatch.setattr(m, "_trainer_for", no_device)
    ex = DeviceExamples.from_records(_lib.GAME_DRAGONCHESS, np.zeros(4, dtype=_lib.example_dtype(_lib.GAME_DRAGONCHESS)), "cpu")
    state = np.random.get_state()
    for examples in (ex, None):
        with pytest.raises(ValueError, match="symmetry"):
            Blackbird.TrainWithDeviceExamples(m, 2, 0.01, examples=examples, augment=True)
    assert m.Version == 1 and np.array_equal(np.random.get_state()[1], state[1])  # nothing trained, nothing drawn
    m.Conn.Close()
