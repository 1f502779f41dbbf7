"""Batched head-to-head evaluation: Blackbird.TestModels (Blackbird.py:177-216) for many games at once.

The reference plays one game at a time: a coin decides who starts, the player to move calls FindMove, BOTH players
call MoveRoot with the new state (tree reuse), until `state.Winner()` is set; the result is +1 / 0 / -1 from
model1's point of view.  Here all `numTests` games advance one ply per iteration: each searcher owns one engine with one
slot per game, searches exactly the slots where it is to move (`bb_run_sims_masked`: the other slots' trees are not
touched, as in the reference, where a model only searches on its own turns), and follows every move with MoveRoot.

Per game the sequence (FindMove on my turns, MoveRoot after every move) is the reference's; what differs from a serial
run is only the order in which random numbers are consumed across games, so results are identical for deterministic
settings (temp = 0, no prior noise) and identically distributed otherwise (tests/test_gpu_arena.py).

Two loops play this.  'host' (the default) is the loop written out in TestModelsBatched below: every ply it reads each side's
moves back and applies them through the batched game entry points.  'device' (opt-in: `loop='device'`, or the class attribute
MCTS.ArenaLoop as a preference) hands the same sequence to the engine library's arena (`_lib.Arena`, bb_arena_*): the games'
states, turns and results stay on the GPU, both sides' searches of a ply are in flight together, and the host looks at the
result once every few plies.  Per game it is the same sequence of operations, with the moves drawn from the engines' own
Philox streams (as `sample_moves(temp, None)` does), so `uniforms=` belongs to the host loop only; a RandomMCTS side and a side
that has only a wall-clock budget are played by the host loop too."""
import random
from time import time

import numpy as np

from . import _lib
from .RandomMCTS import RandomMCTS


class _Searcher(object):
    """One side of the arena: an MCTS / FixedMCTS / Model object turned into an engine with one slot per game."""

    def __init__(self, player, game_id, n_games, sims, seconds):
        self.player = player
        self.random = isinstance(player, RandomMCTS)
        self.engine = None
        self.sims = None if sims is None else int(sims)   # simulations per move (playLimit), or
        self.seconds = seconds                             # wall-clock budget per move (timeLimit) when sims is None
        if not self.random:
            plies = {_lib.GAME_CONNECT4: 43, _lib.GAME_TICTACTOE: 10}.get(game_id, 64)
            cap = player._MAX_NODES
            if self.sims is not None:
                cap = min(cap, self.sims * plies * player._max_depth() + 64)
            self.engine = player._make_engine(game_id, n_games, self.sims or 64, node_capacity=cap)
            player._after_engine_created(self.engine)  # a Model loads its weights here
            self.primed = np.zeros(n_games, dtype=bool)

    def search(self, mask):
        """_runMCTS (MCTS.py:284-303) on the slots of `mask`: playLimit simulations, or simulations in chunks until the
        move's wall-clock budget is spent (at least one chunk, so the root is always expanded)."""
        if self.sims is not None:
            self.engine.run_sims(self.sims, mask=mask)
            return
        end = time() + self.seconds
        while True:
            self.engine.run_sims(16, mask=mask)
            self.engine.synchronize()
            if time() >= end:
                break

    def close(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None


last_loop = None   # which loop the last TestModelsBatched call played through: 'host' or 'device'
_STEP_PLIES = 8    # device loop: plies enqueued between two looks at the result


def _device_loop_obstacle(model1, model2, playLimit, uniforms):
    """Why the device loop cannot play this match (a string), or None."""
    if uniforms is not None:
        return 'uniforms= belongs to the host loop: the device loop draws from the engines\' own streams'
    for name, m in (('model1', model1), ('model2', model2)):
        if isinstance(m, RandomMCTS):
            return '%s is a RandomMCTS, which the host loop plays' % name
        if playLimit is None and getattr(m, 'PlayLimit', None) is None and getattr(m, 'TimeLimit', None) is not None:
            return '%s has only a TimeLimit and no playLimit: a wall-clock budget is the host loop\'s' % name
    return None


def _choose_loop(model1, model2, playLimit, uniforms, loop):
    """'host' or 'device' for this call: an explicit loop='device' that cannot be had raises ValueError with the reason; the
    attribute model1.ArenaLoop = 'device' is a preference and falls back to the host loop.  Makes no engine."""
    explicit = loop is not None
    if loop is None:
        loop = getattr(model1, 'ArenaLoop', 'host')
    if loop not in ('host', 'device'):
        raise ValueError("the arena loop must be 'host' or 'device', not {!r}".format(loop))
    if loop == 'device':
        why = _device_loop_obstacle(model1, model2, playLimit, uniforms)
        if why is not None:
            if explicit:
                raise ValueError("loop='device' is not possible here: " + why)
            return 'host'
    return loop


def _device_arena(sides, game_id, temp, numTests, first, starts, schedule=None):
    """The match loop on the device: create, (schedule,) begin, step + status until nobody is alive, fetch."""
    arena = _lib.Arena(sides[0].engine, sides[1].engine, log_plies=0)
    try:
        if schedule is not None:
            arena.set_temp_schedule(*schedule)
        arena.begin(first, temp, starts)
        while True:
            arena.step(_STEP_PLIES)
            if arena.status() == 0:
                break
        return arena.fetch()['result'].astype(np.int32)
    finally:
        arena.close()


def TestModelsBatched(model1, model2, temp, numTests, playLimit=None, first=None, uniforms=None, loop=None, startStates=None,
                      tempSchedule=None):
    """Play `numTests` games of model1 against model2 concurrently; returns an int array of +1 / 0 / -1 (model1's
    wins / draws / losses), one entry per game, in game order.

    playLimit  simulations per move for both sides (default: each side's own PlayLimit; a side that only has a
               TimeLimit searches all its games together until that many seconds have passed, every move)
    first      optional bool array: model1 moves first in game i (default: `random.choice([True, False])` per game,
               drawn in game order like the reference does at the top of each game)
    uniforms   optional callable n -> float64[n] supplying np.random.choice's uniforms (default np.random.random_sample);
               host loop only
    loop       'host' or 'device' (module docstring); None takes model1.ArenaLoop as a preference.  `last_loop` says which
               loop played.  An explicit 'device' that is not possible raises ValueError naming the reason
    startStates  device loop only: a list of numTests GameStates the games start from instead of `Game()`
    tempSchedule (plies, lateTemp): ply p of the match -- 0 for each game's first move -- is played at `temp` while p < plies and
               at lateTemp from there on (0: the PUCT arg-max move): varied openings, then each side's best play.  Both loops;
               a RandomMCTS side takes no temperature.  ValueError, before any engine is made, for anything but a pair of an
               integer and a finite lateTemp >= 0"""
    global last_loop
    if numTests <= 0:
        raise ValueError('Use a positive integer for number of tests.')
    schedule = _lib.temp_schedule(tempSchedule)
    which = _choose_loop(model1, model2, playLimit, uniforms, loop)
    last_loop = which
    starts = None
    if startStates is not None and len(startStates) > 0:
        if which != 'device':
            raise ValueError("startStates= needs the device loop (loop='device')")
        if len(startStates) != numTests:
            raise ValueError('startStates must hold one state per game: %d for %d games' % (len(startStates), numTests))
        from .Blackbird import _packed_starts
        starts = _packed_starts(model1, startStates)
    game = model1.Game
    game_id = game.GAME_ID
    info = _lib.game_info(game_id)
    if first is None:
        first = np.array([random.choice([True, False]) for _ in range(numTests)], dtype=bool)
    first = np.asarray(first, dtype=bool)
    draw = uniforms if uniforms is not None else np.random.random_sample
    sides = []
    for m in (model1, model2):
        # FindMove's stop rule (MCTS.py:173-182): playLimit simulations and / or timeLimit seconds per move
        sims = playLimit if playLimit is not None else getattr(m, 'PlayLimit', None)
        seconds = getattr(m, 'TimeLimit', None)
        if sims is None and seconds is None and not isinstance(m, RandomMCTS):
            raise ValueError('Not enough information to decide a stop time.')
        sides.append(_Searcher(m, game_id, numTests, sims, seconds))
    try:
        if which == 'device':
            return _device_arena(sides, game_id, temp, numTests, first, starts, schedule)
        states = np.repeat(_lib.game_initial(game_id), numTests, axis=0)   # packed boards, host side
        alive = np.ones(numTests, dtype=bool)
        result = np.zeros(numTests, dtype=np.int32)
        to_move1 = first.copy()
        model1_player = np.where(first, 1, 2)
        ply = -1
        while alive.any():
            ply += 1                                              # every live game is on this ply of the match
            now = _lib.temp_at(temp, schedule, ply)
            actions = np.full(numTests, -1, dtype=np.int32)
            for k, side in enumerate(sides):
                mine = alive & (to_move1 if k == 0 else ~to_move1)
                if not mine.any():
                    continue
                idx = np.nonzero(mine)[0]
                if side.random:                                   # RandomMCTS.FindMove: a uniformly random legal move
                    legal = _lib.game_legal(game_id, states[idx])
                    for i, row in zip(idx, legal):
                        actions[i] = int(np.random.choice(np.nonzero(row)[0]))
                    continue
                eng = side.engine
                fresh = idx[~side.primed[idx]]                    # FindMove's `Root is None` branch
                if len(fresh):
                    eng.set_roots(states[fresh], slots=fresh, game_ids=fresh)
                    side.primed[fresh] = True
                side.search(mine)
                if eng.counters()['overflow']:
                    raise _lib.BlackbirdHipError('search tree outgrew the node pool')
                u = np.zeros(numTests, dtype=np.float64)
                if now != 0:
                    u[idx] = draw(len(idx))
                out = eng.sample_moves(now, u if now != 0 else None)
                if (out['action'][idx] < 0).any():
                    raise ValueError('probabilities contain NaN')
                actions[idx] = out['action'][idx]
            # apply the moves, then both sides follow with MoveRoot (Blackbird.py:198-200)
            idx = np.nonzero(alive)[0]
            new_states, status = _lib.game_apply(game_id, states[idx], actions[idx])
            if (status != 0).any():
                raise ValueError('Tried to make an illegal move.')
            states[idx] = new_states
            for side in sides:
                if side.random:
                    continue
                mv = np.where(alive & side.primed, actions, -1).astype(np.int32)
                side.engine.move_roots(mv)
            winners = _lib.game_winner(game_id, states[idx])   # state.Winner(): full scan, as Blackbird.py:202
            to_move1 = ~to_move1
            for i, w in zip(idx, winners):
                if w >= 0:                                         # Winner() is not None
                    alive[i] = False
                    result[i] = 0 if w == 0 else (1 if w == model1_player[i] else -1)
        return result
    finally:
        for side in sides:
            side.close()
