"""-m gpu: self-play with the rollout evaluator in one launch per bb_selfplay_step (bb_selfplay_rollouts: k_selfplay_wave_rollout,
k_dc_selfplay_wave_rollout; bb_selfplay_mode 6) against the lock-step loop it replaces.  A wave that keeps its slot for whole
plies runs, per slot, the lock-step sequence of operations from the same device functions, and a rollout's draws are keyed (game
id, simulation serial, 'ROLL', step), never by who computes them: so every case plays the same configuration twice, lock-step and
wave, and compares everything a caller can read -- records, game offsets, winners, headers, counters -- byte for byte.
Lock-step itself is held to the CPU oracle by tests/test_gpu_rollout.py; two cases are compared with the oracle directly here.
Only the cases of tests/rollout_cases.py are played; a lock-step run is made once per case and shared (never changed)."""
import pytest

from blackbird_amd import _lib
from tests import rollout_cases as RC
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu
WAVE_MODE = 6
COUNTERS = ("sims", "sum_depth", "nodes", "terminal_leaves", "games_finished", "plies", "examples")
BOTH = ["c4_fixed10", "dc_dynamic"]     # a dense and the wide game, Fixed and Dynamic: the cases run under every schedule


def _engine(name, wave, n_slots=None, **kw):
    key, fixed, max_depth, sims, n_games, slots, max_plies = RC.SELFPLAY[name]
    cfg = dict(n_slots=n_slots or slots, sims_per_move=sims, mcts_kind=_lib.MCTS_FIXED if fixed else _lib.MCTS_DYNAMIC,
               max_depth=max_depth, evaluator=_lib.EVAL_ROLLOUT, c_puct=RC.C_PUCT, seed=RC.SEED, max_games=n_games,
               max_plies=max_plies, first_game_id=RC.FIRST_GAME_ID)
    cfg.update(kw)
    eng = _lib.Engine(RC.GAMES[key], **cfg)
    assert eng.selfplay_mode() == 0                      # without the call: as before
    if wave:
        eng.selfplay_rollouts(True)
        assert eng.selfplay_mode() == WAVE_MODE
    return eng


def _finish(eng, n_games, step=8, between=None):
    """Play the begun games to the end in steps of `step` plies; between(k): called after step k.  Everything a caller can read.
    (One slot playing 24 Connect4 games one after another, a ply per step: at most 24 * 42 steps.)"""
    return SP.play_to_end(eng, n_games, step, 1.0, begin=False, steps_below=1100, between=between, headers=True)


def _play(name, wave, n_slots=None, step=8, **kw):
    eng = _engine(name, wave, n_slots, **kw)
    eng.selfplay_begin(RC.SELFPLAY[name][4], 1.0)
    out = _finish(eng, RC.SELFPLAY[name][4], step)
    eng.close()
    return out


_lock = {}


def _lockstep(name):
    """The lock-step run of a case (its own slot count, steps of 8 plies), played once; the caller must not change it."""
    if name not in _lock:
        _lock[name] = _play(name, False)
        c = _lock[name]["cnt"]
        assert c["overflow"] == 0 and c["games_finished"] == RC.SELFPLAY[name][4] and c["examples"] == len(_lock[name]["rec"])
    return _lock[name]


def _same(a, b, what):
    SP.assert_same_records(a, b, what, counters=COUNTERS, no_overflow=True)


# ---- 1. equality with lock-step and with the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.SELFPLAY))
def test_same_bytes_as_lockstep(name):
    """Fewer slots than games (slots are reused), slot counts that do not fill the workgroups' four waves, game ids from 1000."""
    _same(_lockstep(name), _play(name, True), name)


@pytest.mark.parametrize("name", BOTH)
def test_wave_selfplay_vs_oracle(orc, name):
    """The wave engine's games against the oracle's serial games, example by example, as
    tests/test_gpu_rollout.py::test_rollout_selfplay_vs_oracle compares the lock-step engine's; no compared value comes from a
    rollout that ran into the ply cap or found no legal move (RC.assert_rollouts_decided)."""
    out = _play(name, True)
    assert out["cnt"]["overflow"] == 0
    RC.assert_selfplay_is_the_oracles(orc, name, out["rec"], out["offs"], out["win"], out["cnt"])


# ---- 2. schedule independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots", [1, 5, 64])   # a single wave; a workgroup that is not full; more slots than games
@pytest.mark.parametrize("name", BOTH)
def test_slot_count_does_not_change_the_bytes(name, n_slots):
    # (the per-slot counters are summed, and every game's simulations are counted whichever slot plays it)
    _same(_lockstep(name), _play(name, True, n_slots=n_slots), (name, n_slots))


@pytest.mark.parametrize("step", [1, 3, 8])
@pytest.mark.parametrize("name", BOTH)
def test_step_size_does_not_change_the_bytes(name, step):
    _same(_lockstep(name), _play(name, True, step=step), (name, step))


@pytest.mark.parametrize("name", BOTH)
def test_every_slot_makes_exactly_plies_moves_per_step(name):
    """After every step of 3 plies the wave engine stands where the lock-step engine stands after the same steps: the same games
    finished with the same headers, the same number of moves made and of simulations run."""
    lock, wave = _engine(name, False), _engine(name, True)
    n_games = RC.SELFPLAY[name][4]
    seen = {id(lock): [], id(wave): []}
    for eng in (lock, wave):
        eng.selfplay_begin(n_games, 1.0)

        def note(k, eng=eng):
            c = eng.counters()
            seen[id(eng)].append((eng.selfplay_headers().tobytes(), c["plies"], c["sims"], c["games_finished"]))

        _finish(eng, n_games, 3, note)
        eng.close()
    a, b = seen[id(lock)], seen[id(wave)]
    assert len(a) == len(b) and len(a) > 3
    for k, (x, y) in enumerate(zip(a, b)):
        assert x == y, (name, "after step", k, x[1:], y[1:])
    assert a[0][1] == 3 * RC.SELFPLAY[name][5]   # (no game is over after three plies: every slot has made every move)


# ---- 3. the simulation count changes in mid-game ---------------------------------------------------------------------------------
def test_set_sims_per_move_between_steps():
    def run(wave):
        eng = _engine("c4_dynamic", wave)               # (created for 60 simulations per move: the node pool is sized for that)
        eng.selfplay_begin(12, 1.0)
        eng.selfplay_step(3)
        eng.set_sims_per_move(20)
        eng.selfplay_step(5)
        eng.set_sims_per_move(45)
        out = _finish(eng, 12, 4)
        eng.close()
        return out

    lock, wave = run(False), run(True)
    _same(lock, wave, "sims 60 -> 20 -> 45")
    assert lock["rec"].tobytes() != _lockstep("c4_dynamic")["rec"].tobytes()    # (the calls did change the games)
    assert lock["cnt"]["sims"] < _lockstep("c4_dynamic")["cnt"]["sims"]


# ---- 4. the host-side launch split -----------------------------------------------------------------------------------------------
# BB_SELFPLAY_WAVE_SIMS: the simulations per slot and launch, read once in bb_create where the other tuning switches are read.
# expected launches of a step of 8 plies: 8 x ceil(sims / cap) where a ply is longer than a launch, else ceil(8 / (cap // sims))
@pytest.mark.parametrize("name,cap,launches", [
    ("c4_fixed3", None, 1),     # 60 simulations per move, the kernel's own cap: the whole step
    ("c4_fixed3", 25, 24),      # a ply in three launches (25 + 25 + 10 and the move)
    ("c4_fixed3", 60, 8),       # a ply per launch
    ("c4_fixed3", 150, 4),      # two plies per launch
    ("ttt_dynamic", 100, 3),    # 30 per move: three plies per launch, the last launch two
    ("dc_dynamic", 5, 32),      # 16 per move: 5 + 5 + 5 + 1 and the move
    ("dc_dynamic", 40, 4),
])
def test_split_launches_give_the_same_bytes(monkeypatch, name, cap, launches):
    if cap is None:
        monkeypatch.delenv("BB_SELFPLAY_WAVE_SIMS", raising=False)
    else:
        monkeypatch.setenv("BB_SELFPLAY_WAVE_SIMS", str(cap))
    eng = _engine(name, True)
    eng.selfplay_begin(RC.SELFPLAY[name][4], 1.0)
    eng.timing_enable(1)
    eng.selfplay_step(8)
    assert eng.timing_read()[2] == launches, (name, cap)   # (every launch of this structure is bracketed)
    eng.timing_enable(0)
    out = _finish(eng, RC.SELFPLAY[name][4], 8)
    eng.close()
    _same(_lockstep(name), out, (name, cap))


# ---- 5. the switch itself --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c4_fixed10", "dc_fixed3"])
def test_switching_back_and_in_mid_run(name):
    eng = _engine(name, True)
    eng.selfplay_rollouts(False)
    assert eng.selfplay_mode() == 0
    eng.selfplay_begin(RC.SELFPLAY[name][4], 1.0)
    _same(_lockstep(name), _finish(eng, RC.SELFPLAY[name][4], 8), (name, "on, then off"))
    eng.close()
    eng = _engine(name, False)                         # lock-step and wave steps in turn: both leave what the other expects
    eng.selfplay_begin(RC.SELFPLAY[name][4], 1.0)
    flip = [False]

    def turn(k):
        flip[0] = not flip[0]
        eng.selfplay_rollouts(flip[0])
        assert eng.selfplay_mode() == (WAVE_MODE if flip[0] else 0)

    _same(_lockstep(name), _finish(eng, RC.SELFPLAY[name][4], 3, turn), (name, "alternating"))
    eng.close()


def test_bad_values_and_other_evaluators():
    eng = _engine("ttt_dynamic", True)
    for bad in (2, -1):
        assert _lib.lib().bb_selfplay_rollouts(eng.h, bad) == _lib.ERR_ARG
    assert eng.selfplay_mode() == WAVE_MODE
    eng.selfplay_rollouts()                            # (on=True is the default)
    assert eng.selfplay_mode() == WAVE_MODE and eng.run_sims_structure() == _lib.LAUNCH_LOCKSTEP   # bb_run_sims is not concerned
    eng.close()
    for game, launch in ((_lib.GAME_CONNECT4, _lib.LAUNCH_AUTO), (_lib.GAME_CONNECT4, _lib.LAUNCH_LOCKSTEP),
                         (_lib.GAME_DRAGONCHESS, _lib.LAUNCH_AUTO)):
        hashed = _lib.Engine(game, n_slots=3, sims_per_move=8, evaluator=_lib.EVAL_HASH, launch=launch, max_plies=12, max_games=3)
        before = hashed.selfplay_mode()
        hashed.selfplay_rollouts(True)                 # accepted, and nothing changes
        assert hashed.selfplay_mode() == before != WAVE_MODE
        hashed.close()


@pytest.mark.parametrize("on", [False, True])
def test_dragonchess_with_ancestors_is_still_refused(on):
    eng = _engine("dc_dynamic", on, track_ancestors=True)
    with pytest.raises(AssertionError, match="DragonChess self-play does not keep ancestor chains"):
        eng.selfplay_begin(6, 1.0)
    eng.close()
