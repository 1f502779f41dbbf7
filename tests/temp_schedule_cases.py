"""What tests/test_temp_schedule_cpu.py (no GPU) and tests/test_gpu_temp_schedule.py (-m gpu) share about the temperature schedule
by ply (bb_selfplay_set_temp_schedule, bb_arena_set_temp_schedule): the schedules, the statement, the oracle's games and the
condition on their draws.

A schedule is (temp, plies, late): the move out of ply p is drawn at `temp` while p < plies and at `late` from there on.  The
statement is tests/selfplay_cases.py::oracle_selfplay_from's loop with the temperature chosen per move: the oracle's find_move
already takes its temperature per call.  The games are those of the lock-step case of tests/temp_cases.py (7 games on 3 slots, so
slots refill and a refilled slot starts again at the early temperature; 24 simulations; hash evaluator; DragonChess capped at 6
plies).  Every exponent 1 / temp is exact (0.5, 1.0, 0.1) or the temperature is 0; all of them but 1.0 are in temp_cases.TEMPS.

The condition (temp_cases.MARGIN = 2^-40, derived there): every move's draw keeps that relative distance from every inner boundary
of its cdf AT THAT MOVE'S OWN TEMPERATURE, so the GPU tests may demand exact agreement.  The seed is chosen so that it holds; the
CPU test asserts it for every case the GPU tests use."""
import numpy as np

from tests import selfplay_cases as SC
from tests import temp_cases as T

# id -> (temp, plies, late)
SCHEDULES = {
    "explore2_then_best": (0.5, 2, 0.0),
    "one_ply_at_1_then_0.1": (1.0, 1, 0.1),
    "best3_then_0.5": (0.0, 3, 0.5),
    "all_late": (0.1, 0, 0.5),              # every move is late: `temp` is never used
    "late_never_reached": (0.5, 1000, 0.0),
}
TWO = ("explore2_then_best", "one_ply_at_1_then_0.1")    # what every structure other than lock-step is held to
SEED = T.LOCKSTEP["seed"]


def temp_of(sched):
    temp, plies, late = sched
    return lambda ply: temp if ply < plies else late


def oracle_selfplay_scheduled(orc, cfg, game_id, start, temp_of_ply, play_limit, max_plies):
    """SC.oracle_selfplay_from with find_move(st, temp_of_ply(ply), ...): the same dict, and `temps`, each move's temperature."""
    game = cfg.game
    A = orc.dims(game)[3]
    search = orc.Search(cfg, game_id)
    search.drop_root()
    st = start.copy()
    boards, pi, player, actions, plays, us, temps = [], [], [], [], [], [], []
    winner, n = None, 0
    while winner is None and n < max_plies:
        temps.append(float(temp_of_ply(n)))
        o = search.find_move(st, temps[-1], play_limit, u=-1.0, ply=n)
        boards.append(orc.encode(game, st)[0])
        pi.append(o["prob"])
        player.append(st.player)
        actions.append(o["action"])
        plays.append(o["plays"])
        us.append(orc.u53(cfg.seed, game_id, n))
        st = o["next"]
        search.move_root(st)
        winner = orc.winner(game, st)
        n += 1
    boards.append(orc.encode(game, st)[0])
    pi.append(np.zeros(A))
    player.append(st.player)
    player = np.array(player, dtype=np.int8)
    w = -1 if winner is None else int(winner)
    z = np.zeros(n + 1, dtype=np.float32) if w <= 0 else np.where(player == w, 1.0, -1.0).astype(np.float32)
    return dict(n=n + 1, boards=np.stack(boards), pi=np.stack(pi), player=player, z=z,
                actions=np.array(actions, dtype=np.int32), winner=w, stats=search.stats(), plays=np.array(plays).reshape(n, A),
                u=np.array(us), temps=np.array(temps))


def draw_margins(o):
    """The smallest margin of any move of a scheduled oracle game, each at its own temperature (a move at 0 consumes no draw)."""
    return min([T.margin(c, t, u) for c, u, t in zip(o["plays"], o["u"], o["temps"]) if t != 0], default=float("inf"))


_games = {}


def lockstep_games(orc, og, name):
    """The oracle's games first_id .. first_id + 6 of the lock-step case under SCHEDULES[name], played once; not to be changed."""
    if (og, name) not in _games:
        L = T.LOCKSTEP
        _games[og, name] = [oracle_selfplay_scheduled(orc, T.lockstep_cfg(orc, og, k, seed=SEED), L["first_id"] + k, orc.new_state(og),
                                                      temp_of(SCHEDULES[name]), L["sims"], T.lockstep_max_plies(og))
                            for k in range(L["n_games"])]
    return _games[og, name]


# ---- a schedule together with caller-given start positions: "ply counts from the start position" ------------------------------
STARTS_CASE = dict(og=0, name="explore2_then_best", salt=4242, first_id=1000)   # Connect4; 7 games on 3 slots over SC.ACTIONS


def starts_states(orc):
    """The oracle's states of SC.ACTIONS[Connect4] (the action lists behind SC.starts_of, which needs a GPU)."""
    out = []
    for acts in SC.ACTIONS[SC.C4]:
        st = orc.new_state(0)
        for a in acts:
            assert orc.apply(0, st, a) == 0
        out.append(st)
    return out


def starts_games(orc):
    """Game k starts from state k % 4, mid-game, and its schedule counts plies from there; played once, not to be changed."""
    if "starts" not in _games:
        S, L = STARTS_CASE, T.LOCKSTEP
        starts = starts_states(orc)
        _games["starts"] = [oracle_selfplay_scheduled(
            orc, orc.make_cfg(0, evaluator=orc.EVAL_HASH, salt=S["salt"] + k, seed=SEED), S["first_id"] + k, starts[k % len(starts)],
            temp_of(SCHEDULES[S["name"]]), L["sims"], 42) for k in range(L["n_games"])]
    return _games["starts"]
