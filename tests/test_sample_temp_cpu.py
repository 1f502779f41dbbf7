"""Move choice at temperatures other than 1, the part that needs no GPU: the yardstick of tests/test_gpu_sample_temp.py and of the
temp 0.1 arena cases is pinned here.

orc.sample_action against the reference's expression written in numpy (tests/temp_cases.py) over temperatures whose exponents
are integers (0.1 -> exactly 10.0, 0.5, and 1 / 2.0, 1 / 50.0) and NON-integers (0.3 -> 3.33.., 0.7 -> 1.42..: no integer
shortcut inside pow), on visit vectors with zeros, a single visited child, everything on the last child and counts up to 800
(800 ** 10 > 2 ** 53), at mid-interval draws and at draws 2^-40 either side of every boundary; the refusal where N ** (1 / temp)
overflows; orc.selfplay_game at temp 0.1 and 0 against a direct loop over Search.find_move; and that every draw the GPU tests
compare keeps 2^-40 from the boundaries of its cdf, so that those tests may ask for exact agreement."""
import numpy as np
import pytest

from tests import temp_cases as T
from tests import selfplay_cases as SC


@pytest.mark.parametrize("A", [7, 9])
@pytest.mark.parametrize("temp", T.TEMPS)
def test_sample_action_is_the_numpy_expression(orc, temp, A):
    n = {"mid": 0, "below": 0, "above": 0}
    for plays in T.visit_vectors(A):
        p = T.probabilities(plays, temp)
        assert np.isfinite(p).all() and p.sum() > 0
        for kind, k, u in T.draws(plays, temp):
            want = T.choice(p, u)
            assert orc.sample_action(plays, temp, u) == want, (plays, temp, kind, k, u)
            if kind != "above":
                assert want == k, (plays, temp, kind, k, u)       # (the draws are where they are meant to be)
            else:
                assert want > k and plays[want] > 0, (plays, temp, kind, k, u)
            n[kind] += 1
    assert min(n.values()) > 20, n


def test_visit_vectors_hold_the_edges():
    for A in (7, 9):
        vs = T.visit_vectors(A)
        assert any((v == 0).any() and (v > 0).sum() >= 3 for v in vs)            # zeros among the children
        assert any((v > 0).sum() == 1 and v[-1] == 0 for v in vs)                # a single non-zero child
        assert any((v > 0).sum() == 1 and v[-1] > 0 for v in vs)                 # all visits on the last child
        assert any(v.max() == 800 and v.max() ** 10 > 2.0 ** 53 for v in vs)
    # a single visited child: its own interval is the whole cdf, so only draws inside it exist
    assert [d[0] for d in T.draws(np.array([0, 0, 47.0, 0, 0, 0, 0]), 0.1)] == ["mid", "below"]


def test_temp_50_is_near_uniform_over_the_visited_children(orc):
    plays = np.array([0, 40, 1, 0, 5, 0, 2.0])
    p = T.probabilities(plays, 50.0)
    assert (p[plays == 0] == 0).all() and np.ptp(p[plays > 0]) < 0.02            # 0 ** 0.02 = 0
    assert [orc.sample_action(plays, 50.0, u) for u in (0.0, 0.3, 0.55, 0.8)] == [1, 2, 4, 6]


@pytest.mark.parametrize("plays,temp,what", [
    ([0, 1300, 5, 0, 0, 0, 0], 0.01, "nan"),              # 1300 ** 100 = inf: inf / inf
    ([3, 7, 9, 12, 0, 9, 8], T.OVERFLOW_TEMP, "nan"),     # what 48 simulations give: 7 ** 500 = inf
    ([1209, 1209, 0, 0, 0, 0, 0], 0.01, "sum"),           # each term is finite, their sum is not: every p is 0
    ([1209, 1, 1209, 4, 1209, 0, 0, 1, 1], 0.01, "sum"),
])
def test_overflow_is_refused(orc, plays, temp, what):
    plays = np.array(plays, dtype=np.float64)
    with np.errstate(over="ignore"):
        terms = np.array([c ** (1 / temp) for c in plays])
        total = sum(terms.tolist())
    assert total == np.inf and np.isfinite(terms).all() == (what == "sum")
    p = T.probabilities(plays, temp)
    with pytest.raises(ValueError, match="contain NaN" if what == "nan" else "do not sum to 1"):
        np.random.RandomState(0).choice(len(p), p=p)
    for u in (0.0, 0.3, 0.999):
        assert orc.sample_action(plays, temp, u) == -3
    # ... and through find_move: 48 simulations on Connect4's seven children give some child >= 7 visits
    if len(plays) == 7:
        s = orc.Search(orc.make_cfg(0, evaluator=orc.EVAL_HASH, salt=5))
        with pytest.raises(ValueError, match="NaN"):
            s.find_move(orc.new_state(0), T.OVERFLOW_TEMP, 48, u=0.5)
    # the largest finite case still samples
    assert orc.sample_action(np.array([4, 3, 0, 0, 0, 0, 0.0]), T.OVERFLOW_TEMP, 0.5) == 0


@pytest.mark.parametrize("temp", [0.1, 0.5, 0.0])
@pytest.mark.parametrize("og,sims,max_plies,games", [(0, 24, 42, 4), (1, 16, 9, 6), (2, 12, 8, 3)])
def test_selfplay_game_is_the_find_move_loop(orc, og, sims, max_plies, games, temp):
    """orc.selfplay_game at the exploitation temperature, at 0.5 and at temp 0 (as test_selfplay_starts_cpu pins it at temp 1)."""
    cfg = orc.make_cfg(og, evaluator=orc.EVAL_HASH, salt=4242, seed=99)
    for gid in range(1000, 1000 + games):
        want = orc.selfplay_game(cfg, gid, temp, sims, max_plies)
        got = SC.oracle_selfplay_from(orc, cfg, gid, orc.new_state(og), temp, sims, max_plies)
        assert got["n"] == want["n"] and got["winner"] == want["winner"], gid
        for k in ("boards", "pi", "player", "z", "actions"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (gid, k)
        assert got["stats"].sims == want["stats"].sims and got["stats"].sum_depth == want["stats"].sum_depth, gid
        # the recorded plays and draws are the ones the moves were chosen from
        assert np.array_equal(got["plays"] / got["plays"].sum(axis=1, keepdims=True), got["pi"][:-1])
        if temp != 0:
            assert [orc.sample_action(c, temp, u) for c, u in zip(got["plays"], got["u"])] == got["actions"].tolist()
    if temp == 0:   # no draw is consumed: another seed plays the same games
        other = orc.make_cfg(og, evaluator=orc.EVAL_HASH, salt=4242, seed=100)
        a, b = orc.selfplay_game(cfg, 1000, 0.0, sims, max_plies), orc.selfplay_game(other, 1000, 0.0, sims, max_plies)
        assert np.array_equal(a["actions"], b["actions"]) and np.array_equal(a["pi"], b["pi"])


# ---- the margins of every draw the GPU tests compare -------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", T.SELFPLAY_TEMPS)
@pytest.mark.parametrize("og", [0, 1, 2])
def test_lockstep_selfplay_draws_keep_their_margin(orc, og, temp):
    games = T.lockstep_games(orc, og, temp)
    assert len(games) == T.LOCKSTEP["n_games"]
    for k, o in enumerate(games):
        assert T.draw_margins(o, temp) >= T.MARGIN, (og, temp, k, T.draw_margins(o, temp))
        assert o["n"] >= 2 and len(o["plays"]) == len(o["u"]) == o["n"] - 1
    assert T.draw_margins(games[0], 0) == float("inf")
    if temp == 0.1:   # the temperature does change the games: this is not the temp 1 run again
        at_one = [SC.oracle_selfplay_from(orc, T.lockstep_cfg(orc, og, k), T.LOCKSTEP["first_id"] + k, orc.new_state(og), 1.0,
                                          T.LOCKSTEP["sims"], T.lockstep_max_plies(og)) for k in range(2)]
        assert any(a["actions"].tolist() != b["actions"].tolist() for a, b in zip(at_one, games))


@pytest.mark.parametrize("og", [0, 1])
def test_sample_moves_roots_and_keyed_draws_keep_their_margin(orc, og):
    rows = T.sample_oracle(orc, og)
    assert len(rows) == T.SAMPLE["n_slots"] and T.SAMPLE["n_slots"] % 4 != 0
    kinds = set()
    for i, (st, o) in enumerate(rows):
        assert o["root_plays"] == T.SAMPLE["sims"] and o["plays"].sum() in (T.SAMPLE["sims"] - 1, T.SAMPLE["sims"])
        kinds.add(int(orc.legal(og, st).sum()))
        # u = None at temp 0.1: the draw of (seed, game id i, ply 0)
        assert T.margin(o["plays"], 0.1, orc.u53(T.SAMPLE["seed"], i, 0)) >= T.MARGIN, i
        # the swept draws are 2^-40 from a boundary by construction, and from every other one by at least as much
        for temp in T.TEMPS:
            for _kind, _k, u in T.draws(o["plays"], temp):
                assert T.margin(o["plays"], temp, u) >= T.MARGIN * (1 - 2.0 ** -10), (i, temp, u)
        # 48 simulations: some child has >= 7 visits and the overflow temperature is refused
        assert o["plays"].max() >= 7 and orc.sample_action(o["plays"], T.OVERFLOW_TEMP, 0.5) == -3
    assert 1 in kinds and len(kinds) == 3            # one legal move, a full column / taken cells, the initial position
    per_temp = [sum(len(T.draws(o["plays"], temp)) for _st, o in rows) for temp in T.TEMPS]
    assert min(per_temp) >= 10 and sum(per_temp) >= T.SAMPLE_MIN_DRAWS, per_temp


def test_dragonchess_root_overflows_at_the_overflow_temperature(orc):
    o = orc.Search(orc.make_cfg(2, evaluator=orc.EVAL_HASH, salt=T.SAMPLE["salt"], seed=T.SAMPLE["seed"])).find_move(
        orc.new_state(2), 1.0, T.SAMPLE["sims"], u=0.5)
    assert o["plays"].max() >= 7 and orc.sample_action(o["plays"], T.OVERFLOW_TEMP, 0.5) == -3
    assert T.margin(o["plays"], 50.0, 0.5) >= T.MARGIN      # the one draw the GPU test compares on this root


@pytest.mark.parametrize("key,og", [("c4", 0), ("ttt", 1)])
def test_arena_oracle_draws_keep_their_margin(orc, key, og):
    """tests/test_gpu_arena.py::test_batched_arena_equals_two_searcher_oracle at temp 0.1: its uniforms against the oracle's plays."""
    from tests import arena_cases as AC
    trace = []
    AC.oracle_arena(orc, og, AC.hash_cfgs(orc, og), AC.SIMS, AC.FIRST, 0.1, np.random.RandomState(AC.UNIFORM_SEED).random_sample, trace)
    assert len(trace) >= len(AC.FIRST) * 5
    worst = min(T.margin(plays, 0.1, u) for plays, u in trace)
    assert worst >= T.MARGIN, worst
