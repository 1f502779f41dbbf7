"""The temperature schedule by ply (bb_selfplay_set_temp_schedule, bb_arena_set_temp_schedule, Model.SelfPlayTempSchedule,
tempSchedule=), the part that needs no GPU: the two symbols in header, library and bindings; the argument checks that come before any device call; the Python
validation, which raises before an engine exists; the statement of tests/temp_schedule_cases.py pinned to the constant-temperature
yardstick; and the margin condition for every case the GPU tests use."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from blackbird_amd import Blackbird, Connect4, _lib, arena
from tests import selfplay_cases as SC
from tests import temp_cases as T
from tests import temp_schedule_cases as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_in_header_library_and_bindings():
    text = open(os.path.join(ROOT, "include", "blackbird_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+bb_selfplay_set_temp_schedule\s*\(\s*bb_engine\s*\*\s*e\s*,\s*int\s+plies\s*,\s*double\s+temp_late\s*\)", code)
    assert re.search(r"\bint\s+bb_arena_set_temp_schedule\s*\(\s*bb_arena\s*\*\s*ar\s*,\s*int\s+plies\s*,\s*double\s+temp_late\s*\)", code)
    for name in ("bb_selfplay_set_temp_schedule", "bb_arena_set_temp_schedule"):
        assert "ply counts from the game's" in re.sub(r"\s+\*?\s*", " ", text[:text.index("int " + name)])[-2000:], name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name) and name in _lib.EXPORTS
        assert getattr(_lib.lib(), name).argtypes == [C.c_void_p, C.c_int, C.c_double]
    assert hasattr(_lib.Engine, "selfplay_set_temp_schedule") and hasattr(_lib.Arena, "set_temp_schedule")
    for fn in (arena.TestModelsBatched, Blackbird.TestModels, Blackbird.TestRandom,
               Blackbird.TestPrevious, Blackbird.TestGood):
        p = inspect.signature(fn).parameters
        assert "tempSchedule" in p and p["tempSchedule"].default is None, fn.__name__
    # self-play takes its schedule from the model (an attribute, like KeepDeviceExamples): the function's signature is not widened
    assert list(inspect.signature(Blackbird.GenerateTrainingSamples).parameters) == ["model", "nGames", "temp", "startStates"]
    src = inspect.getsource(Blackbird.Model.__init__)
    assert "self.SelfPlayTempSchedule = None" in src and "SelfPlayTempSchedule" in inspect.getsource(Blackbird.GenerateTrainingSamples)


def test_argument_checks_come_before_any_device_call():
    L = _lib.lib()
    for fn in (L.bb_selfplay_set_temp_schedule, L.bb_arena_set_temp_schedule):
        for plies, late in ((2, 0.0), (-1, 0.0), (0, 0.5), (2, -0.5), (2, float("nan")), (2, float("inf"))):
            assert fn(None, plies, late) == _lib.ERR_ARG and "null" in _lib.last_error(), (plies, late)


class _NoEngine(object):
    """A searcher that may not be turned into an engine: the validation has to raise first."""
    Game = Connect4.BoardState
    TimeLimit = None
    PlayLimit = 8
    SelfPlayTempSchedule = None

    def __getattr__(self, name):
        raise AssertionError("the call went on to " + name)


MALFORMED = [3, (3,), (1, 2.0, 3), "ab", (2.5, 0.1), ("2", 0.1), (True, 0.1), (2, -0.1), (2, float("nan")), (2, float("inf")),
             (2, -float("inf")), (2, "0.1"), (2, None), [None, 0.1]]


@pytest.mark.parametrize("bad", MALFORMED, ids=[repr(b) for b in MALFORMED])
def test_a_malformed_schedule_is_a_value_error_before_any_engine(bad):
    with pytest.raises(ValueError, match="tempSchedule"):
        _lib.temp_schedule(bad)
    with pytest.raises(ValueError, match="tempSchedule"):
        player = _NoEngine()
        player.SelfPlayTempSchedule = bad
        Blackbird.GenerateTrainingSamples(player, 3, 1.0)
    for loop in (None, "host", "device"):
        with pytest.raises(ValueError, match="tempSchedule"):
            arena.TestModelsBatched(_NoEngine(), _NoEngine(), 0.1, 2, loop=loop, tempSchedule=bad)
    with pytest.raises(ValueError, match="tempSchedule"):
        Blackbird.TestModels(_NoEngine(), _NoEngine(), 0.1, 1, tempSchedule=bad)


def test_well_formed_schedules():
    assert _lib.temp_schedule(None) is None
    assert _lib.temp_schedule((2, 0)) == (2, 0.0) and _lib.temp_schedule([np.int64(0), np.float32(0.5)]) == (0, 0.5)
    assert _lib.temp_schedule((-1, 0.3)) is None                    # the C ABI's "off"
    assert [_lib.temp_at(0.7, (2, 0.1), p) for p in range(4)] == [0.7, 0.7, 0.1, 0.1]
    assert [_lib.temp_at(0.7, (0, 0.1), p) for p in range(2)] == [0.1, 0.1] and _lib.temp_at(0.7, None, 5) == 0.7


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def _same_game(got, want, what):
    assert got["n"] == want["n"] and got["winner"] == want["winner"], what
    for k in ("boards", "pi", "player", "z", "actions", "plays", "u"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert got["stats"].sims == want["stats"].sims and got["stats"].sum_depth == want["stats"].sum_depth, what


@pytest.mark.parametrize("og", [0, 1, 2], ids=["c4", "ttt", "dc"])
def test_statement_with_equal_temperatures_and_with_no_early_ply_is_the_constant_temperature_yardstick(orc, og):
    L = T.LOCKSTEP
    for temp in (0.5, 0.0):
        for k, want in enumerate(T.lockstep_games(orc, og, temp)):
            cfg, gid = T.lockstep_cfg(orc, og, k), L["first_id"] + k
            for name, sched in (("late == temp", (temp, 2, temp)), ("plies = 0", (0.1, 0, temp)), ("never late", (temp, 10 ** 6, 0.3))):
                got = TS.oracle_selfplay_scheduled(orc, cfg, gid, orc.new_state(og), TS.temp_of(sched), L["sims"], T.lockstep_max_plies(og))
                _same_game(got, want, (og, temp, k, name))
                assert (got["temps"] == temp).all()


@pytest.mark.parametrize("name", sorted(TS.SCHEDULES))
@pytest.mark.parametrize("og", [0, 1, 2], ids=["c4", "ttt", "dc"])
def test_every_draw_of_the_gpu_cases_keeps_its_margin(orc, og, name):
    temp, plies, late = TS.SCHEDULES[name]
    games = TS.lockstep_games(orc, og, name)
    worst = min(TS.draw_margins(o) for o in games)
    print(og, name, "smallest margin", worst)
    assert worst >= T.MARGIN, (og, name, worst)
    for o in games:                                   # each move was played at the temperature the schedule gives its ply
        assert o["temps"].tolist() == [temp if p < plies else late for p in range(o["n"] - 1)]
    if 0 < plies < 10:                                # both phases are really played: some game is longer than the early phase
        assert max(o["n"] - 1 for o in games) > plies, (og, name)


def test_the_schedules_change_the_games(orc):
    """A schedule that the engine ignored would not be seen by a comparison against games it does not change."""
    for name in TS.SCHEDULES:
        temp, plies, late = TS.SCHEDULES[name]
        if plies >= 1000:
            continue
        const = [SC.oracle_selfplay_from(orc, T.lockstep_cfg(orc, 0, k), T.LOCKSTEP["first_id"] + k, orc.new_state(0), temp, T.LOCKSTEP["sims"], 42)
                 for k in range(T.LOCKSTEP["n_games"])]
        sched = TS.lockstep_games(orc, 0, name)
        assert any(not np.array_equal(a["actions"], b["actions"]) for a, b in zip(const, sched)), name


def test_the_case_from_start_positions_keeps_its_margin_and_counts_plies_from_the_start(orc):
    temp, plies, late = TS.SCHEDULES[TS.STARTS_CASE["name"]]
    games = TS.starts_games(orc)
    assert min(TS.draw_margins(o) for o in games) >= T.MARGIN
    for o in games:
        assert o["temps"].tolist() == [temp if p < plies else late for p in range(o["n"] - 1)]
    assert sum(o["n"] - 1 > plies for o in games) >= 4
