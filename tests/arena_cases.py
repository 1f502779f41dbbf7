"""What tests/test_gpu_arena.py (-m gpu) and tests/test_sample_temp_cpu.py (no GPU) share about the arena's oracle case: the
two-searcher game loop over the oracle, the two hash-evaluator sides, first movers, play limits and the seed of the uniforms."""
import numpy as np

from blackbird_amd import _lib, arena
from blackbird_amd.DynamicMCTS import DynamicMCTS

FIRST = np.array([True, False, False, True, True, False, True, False, False, True, True])
SIMS = (30, 20)
UNIFORM_SEED = 5


def hash_cfgs(orc, og):
    """The two sides: different salts and exploration rates."""
    return (orc.make_cfg(og, evaluator=orc.EVAL_HASH, salt=11, c_puct=0.85, seed=77),
            orc.make_cfg(og, evaluator=orc.EVAL_HASH, salt=22, c_puct=1.3, seed=77))


def oracle_arena(orc, og, cfgs, sims, first, temp, draw, trace=None):
    """Blackbird.TestModels (Blackbird.py:177-216) for every game with two oracle searchers: the mover calls FindMove,
    BOTH call MoveRoot after every move; +1 / 0 / -1 from side 0's point of view.  Plies advance in step across games
    so that the uniforms are consumed in the batched arena's order (side 0's movers in game order, then side 1's).
    trace: a list that gets (the root's child plays, u) of every sampled move."""
    n = len(first)
    search = [[orc.Search(cfgs[k], g) for g in range(n)] for k in range(2)]
    state = [orc.new_state(og) for _ in range(n)]
    to0 = [bool(f) for f in first]
    alive = [True] * n
    result = [0] * n
    while any(alive):
        for k in range(2):
            movers = [g for g in range(n) if alive[g] and to0[g] == (k == 0)]
            us = draw(len(movers)) if (temp != 0 and movers) else [None] * len(movers)
            for g, u in zip(movers, us):
                r = search[k][g].find_move(state[g], temp, sims[k], u=-1.0 if u is None else float(u))
                state[g] = r["next"]
                if trace is not None and u is not None:
                    trace.append((r["plays"], float(u)))
        for g in range(n):
            if not alive[g]:
                continue
            search[0][g].move_root(state[g])
            search[1][g].move_root(state[g])
            to0[g] = not to0[g]
            w = orc.winner(og, state[g])
            if w is not None:
                alive[g] = False
                mine = 1 if first[g] else 2
                result[g] = 0 if w == 0 else (1 if w == mine else -1)
    return np.array(result)


# ---- players and engines of the device tests ------------------------------------------------------------------------------
class HashPlayer(DynamicMCTS):
    """DynamicMCTS on the deterministic validation evaluator; honours SearchLaunch like the stock searchers."""
    _EVALUATOR = _lib.EVAL_HASH

    def __init__(self, game, salt, c_puct=0.85, playLimit=24, node_capacity=None):
        DynamicMCTS.__init__(self, explorationRate=c_puct, playLimit=playLimit)
        self.Game, self.salt, self.node_capacity = game, salt, node_capacity

    def _make_engine(self, game_id, n_slots, sims, **kw):
        kw.setdefault('launch', self._search_launch())
        if self.node_capacity is not None:
            kw['node_capacity'] = self.node_capacity
        return _lib.Engine(game_id, n_slots=n_slots, sims_per_move=max(int(sims), 1), mcts_kind=self._KIND,
                           evaluator=_lib.EVAL_HASH, hash_salt=self.salt, c_puct=float(self.ExplorationRate), seed=77, **kw)


def searcher_engines(players, n_slots):
    """One engine per side, made as the arena makes them (arena._Searcher); numpy's seed fixes the engines' random streams."""
    out = []
    for k, p in enumerate(players):
        np.random.seed(100 + k)
        out.append(arena._Searcher(p, p.Game.GAME_ID, n_slots, p.PlayLimit, None).engine)
    return out
