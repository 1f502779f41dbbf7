"""Oracle (oracle/orc_games.c) vs the hand-built wide DragonChess positions of tests/golden/boards_dc_wide.npz
(tests/make_golden.py part 'boards_dc_wide': the reference's own BoardState on positions with 64 .. 144 legal moves, and two
with more than the search tree's 144 edges per node), and the legal-move counts the GPU tests rely on."""
import os

import numpy as np
import pytest

S = 144  # DragonChess::S: edges per node (blackbird_amd/csrc/games.hip.h)


@pytest.fixture(scope="module")
def wide(golden_dir):
    return np.load(os.path.join(golden_dir, "boards_dc_wide.npz"), allow_pickle=False)


def _counts(g, pre=""):
    return np.diff(g[pre + "legal_off"])


def test_fixture_covers_the_legal_move_bands(wide):
    """A regenerated fixture cannot drift out of what the wide-node tests need: the edge counts at which a 64-lane pass
    begins or ends, counts inside the bands, both sides to move, king captures past edge 64, positions past S."""
    n = _counts(wide)
    for exact in (64, 65, 128, 129, S):
        assert exact in n, exact
    assert 1 <= ((n >= 66) & (n <= 127)).sum() and 1 <= ((n >= 130) & (n <= 143)).sum()
    assert n.max() == S and 10 <= len(n) <= 14
    w = n > 64
    turns = set(zip(wide["player"][w].tolist(), wide["prev"][w].tolist()))
    assert {(1, 1), (1, 2), (2, 1)} <= turns                      # White's first and second move, Black's move
    assert (wide["win_none"] == -1).all() and (wide["over_win_none"] == -1).all()
    cap = wide["first_king_capture"]
    assert ((cap >= 64) & w).sum() >= 2                            # terminal children in a second pass ...
    assert (wide["n_king_captures"][w] >= 2).any()
    assert any(cap[i] >= 64 and wide["n_king_captures"][i] == 2 and n[i] >= 130 for i in range(len(n)))
    over = _counts(wide, "over_")
    assert len(over) == 2 and 145 <= over.min() <= 160 and over.max() > 192
    assert set(wide["over_player"].tolist()) == {1, 2}
    # the narrow White-to-move position whose children are wide interior nodes
    i = wide["name"].tolist().index("walk3")
    assert n[i] == 3 and (wide["player"][i], wide["prev"][i]) == (1, 1)
    kids = wide["walk_children"]
    assert np.array_equal(kids[:, 0], wide["legal_idx"][wide["legal_off"][i]:wide["legal_off"][i + 1]])
    assert ((kids[:, 1] > 128) & (kids[:, 1] <= S)).all()


@pytest.mark.parametrize("pre", ["", "over_"])
def test_oracle_reproduces_the_wide_boards(orc, wide, pre):
    g = wide
    for i in range(len(g[pre + "player"])):
        st = orc.state_from_arrays(orc.DC, g[pre + "board"][i], g[pre + "player"][i], g[pre + "prev"][i] or None,
                                   g[pre + "castle"][i])
        la = orc.legal(orc.DC, st)
        want = g[pre + "legal_idx"][g[pre + "legal_off"][i]:g[pre + "legal_off"][i + 1]]
        assert np.array_equal(np.where(la == 1)[0], want) and set(np.unique(la)) <= {0.0, 1.0}, i
        w = orc.winner(orc.DC, st)
        assert (-1 if w is None else w) == g[pre + "win_none"][i]
        assert np.array_equal(orc.encode(orc.DC, st).ravel(), g[pre + "enc"][i])
        n_ok = 0
        for row in g[pre + "apply_ok"][i]:
            a, ok = int(row[0]), int(row[1])
            t = st.copy()
            assert (orc.apply(orc.DC, t, a) == 0) == bool(ok), (i, a)
            if ok:
                n_ok += 1
                assert t.player == row[2] and t.prev == row[3]
                assert list(t.castle) == [int(x) for x in row[4:8]]
                assert list(t.b[:64]) == [int(x) for x in row[8:72]]
        assert n_ok >= 3   # (legal moves of every pass are among the samples: make_golden.py)
        # every king capture the fixture counted ends the game for the oracle too, at the same edge
        caps = []
        for k, a in enumerate(want):
            t = st.copy()
            assert orc.apply(orc.DC, t, int(a)) == 0
            if orc.winner(orc.DC, t) is not None:
                caps.append(k)
        assert len(caps) == g[pre + "n_king_captures"][i] and (caps[0] if caps else -1) == g[pre + "first_king_capture"][i]
    if pre == "":
        i = g["name"].tolist().index("walk3")
        st = orc.state_from_arrays(orc.DC, g["board"][i], g["player"][i], g["prev"][i], g["castle"][i])
        for a, n_legal in g["walk_children"]:
            t = st.copy()
            assert orc.apply(orc.DC, t, int(a)) == 0 and (t.player, t.prev) == (2, 1)
            assert orc.legal(orc.DC, t).sum() == n_legal


def test_oracle_max_edges_is_the_engines_rule(orc, wide):
    """orc_cfg.max_edges restates the engine's bound: a node with more legal moves stays a leaf and every
    simulation that ends on it is counted; a search that meets no such node is the same with and without the bound."""
    g = wide
    over = orc.state_from_arrays(orc.DC, g["over_board"][1], g["over_player"][1], g["over_prev"][1], g["over_castle"][1])
    bounded = orc.make_cfg(orc.DC, evaluator=orc.EVAL_HASH, salt=7, max_edges=S)
    free = orc.make_cfg(orc.DC, evaluator=orc.EVAL_HASH, salt=7)
    sr = orc.Search(bounded, 0)
    with pytest.raises(ValueError):            # no child was ever played: np.random.choice / argmax has nothing to choose from
        sr.find_move(over, 1.0, 12, u=0.5)
    st = sr.stats()
    assert st.refused == 12 and st.sims == 12 and st.sum_depth == 0 and st.max_node_legal == 200 and st.nodes_reached == 0
    sr = orc.Search(free, 0)
    o = sr.find_move(over, 0, 12)
    assert o["plays"].sum() == 11 and sr.stats().refused == 0 and sr.stats().max_node_legal >= 200
    i = g["name"].tolist().index("b128")
    narrow = orc.state_from_arrays(orc.DC, g["board"][i], g["player"][i], g["prev"][i], g["castle"][i])
    a, b = orc.Search(bounded, 3), orc.Search(free, 3)
    oa, ob = a.find_move(narrow, 0, 150), b.find_move(narrow, 0, 150)
    assert b.stats().max_node_legal <= S and a.stats().refused == 0
    assert np.array_equal(oa["plays"], ob["plays"]) and np.array_equal(oa["winrates"], ob["winrates"]) and oa["action"] == ob["action"]
