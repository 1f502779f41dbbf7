"""-m gpu: finished games read while other games are still being played.

The move tails (selfplay_move_body in csrc/tree.hip.h, its DragonChess twin in tree_dc.hip.h) write a game's last record,
back-fill z, fence, write the header words, fence, and only then set `done`, so that a reader between two launches may take
every game whose `done` is set.  Here every launch structure is harvested after every step the way
Blackbird.GenerateTrainingSamples and bench.py do it -- bb_selfplay_headers, then bb_examples_fetch_games (k_gather_examples)
of the newly finished games -- beside bb_examples_fetch and dist.engine_records_device at the same moment, and
tests/harvest_cases.py's ledger holds what was read to the headers, to the other readers and, at the end, to the final
fetch byte for byte (a); to the oracle's games and to a lock-step engine's (b).  Then the gather kernel's lists on paused
runs (c), its refusals (d), and the front end's own loop (e).  Every comparison is exact."""
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library is loaded, so that both use one HIP runtime: dist.py imports it late)

from blackbird_amd import Blackbird, Connect4, _lib, proto_wire, weights as W
from tests import harvest_cases as HC
from tests import model_cases as MC
from tests import selfplay_cases as SP
from tests.search_cases import assert_same_array

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C4, TTT, DC = SP.C4, SP.TTT, SP.DC
SIMS, FIRST_ID, SEED, SALT = 16, 500, 17, 4242
# slots (ragged: not whole workgroups), games (more than twice the slots: slots are refilled while finished games sit in the store)
SIZES = {C4: (19, 45), TTT: (21, 50), DC: (3, 8)}
MAX_PLIES = {C4: None, TTT: None, DC: 6}
ROLLOUT = dict(evaluator=_lib.EVAL_ROLLOUT, mcts_kind=_lib.MCTS_DYNAMIC, max_depth=10)
# name: (game, the structure bb_selfplay_mode must report, engine arguments, network blocks or None, bb_selfplay_rollouts)
CASES = {
    "c4-hash-lockstep": (C4, 0, dict(evaluator=_lib.EVAL_HASH, hash_salt=SALT, launch=_lib.LAUNCH_LOCKSTEP), None, False),
    "ttt-hash-lockstep": (TTT, 0, dict(evaluator=_lib.EVAL_HASH, hash_salt=SALT, launch=_lib.LAUNCH_LOCKSTEP), None, False),
    "c4-hash-rounds": (C4, 1, dict(evaluator=_lib.EVAL_HASH, hash_salt=SALT), None, False),    # what a dense game's hash engine plays
    "ttt-hash-rounds": (TTT, 1, dict(evaluator=_lib.EVAL_HASH, hash_salt=SALT), None, False),  # through unless told otherwise
    "dc-hash-lockstep": (DC, 0, dict(evaluator=_lib.EVAL_HASH, hash_salt=SALT), None, False),
    "c4-net-lockstep": (C4, 0, dict(evaluator=_lib.EVAL_NET, noise_on=True, launch=_lib.LAUNCH_LOCKSTEP), 2, False),
    "c4-net-rounds": (C4, 1, dict(evaluator=_lib.EVAL_NET, noise_on=True), 5, False),   # R = 5: the persistent kernel's fallback
    "c4-net-persistent": (C4, 3, dict(evaluator=_lib.EVAL_NET, noise_on=True), 2, False),
    "ttt-net-persistent": (TTT, 3, dict(evaluator=_lib.EVAL_NET, noise_on=True), 2, False),
    "dc-net-one-wave": (DC, 5, dict(evaluator=_lib.EVAL_NET, noise_on=True), 2, False),
    "ttt-rollout-wave": (TTT, 6, ROLLOUT, None, True),
    "c4-rollout-wave": (C4, 6, ROLLOUT, None, True),
}
HASHED = [k for k in CASES if "hash" in k]
NOT_LOCKSTEP = [k for k in CASES if CASES[k][1] != 0]


def _engine(name, lockstep=False, **kw):
    """The case's engine with its weights loaded; lockstep: its twin that plays the same games launch by launch."""
    game, mode, args, blocks, wave = CASES[name]
    n_slots, n_games = SIZES[game]
    cfg = dict(n_slots=n_slots, sims_per_move=SIMS, seed=SEED, max_games=n_games, first_game_id=FIRST_ID, alpha=SP.ALPHA,
               epsilon=SP.EPS, max_plies=MAX_PLIES[game])
    cfg.update(args)
    if lockstep:
        cfg["launch"] = _lib.LAUNCH_LOCKSTEP
    cfg.update(kw)
    eng = _lib.Engine(game, **cfg)
    if blocks is not None:
        gi = _lib.game_info(game)
        eng.load_weights(W.flatten(W.init_weights(gi.C, 16, blocks, 16, gi.A, seed=21, perturb=True)))
    if wave and not lockstep:
        eng.selfplay_rollouts(True)
    assert eng.selfplay_mode() == (0 if lockstep else mode), (name, eng.selfplay_mode())
    return eng


_harvested = {}


def _harvest_run(name, step):
    """The case played to the end in steps of `step` plies with the ledger fed after every step: (the ledger's run, the
    ledger).  Played once per (case, step); the callers must not change it."""
    if (name, step) not in _harvested:
        game = CASES[name][0]
        n_slots, n_games = SIZES[game]
        eng = _engine(name)
        try:
            led = HC.Ledger(n_games, n_slots, FIRST_ID)
            final = SP.play_to_end(eng, n_games, step, 1.0, between=lambda k: HC.harvest(eng, led, DEV), headers=True)
            assert final["cnt"]["overflow"] == 0 and final["cnt"]["games_finished"] == n_games, final["cnt"]
            mine = led.finish(final)
            mine["cnt"] = final["cnt"]
            print(f"mode {eng.selfplay_mode()}", end=" ")
            led.report(f"{name}, steps of {step}")
        finally:
            eng.close()
        _harvested[name, step] = (mine, led)
    return _harvested[name, step]


# ---- a. every launch structure, harvested after every step ------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_harvest_after_every_step(name, step):
    _mine, led = _harvest_run(name, step)
    led.assert_not_vacuous()


# ---- b. against something that is not the code under test -------------------------------------------------------------------------
_oracle = {}


def _oracle_games(orc, name):
    if name not in _oracle:
        game = CASES[name][0]
        max_plies = MAX_PLIES[game] or {C4: 42, TTT: 9}[game]
        cfg = orc.make_cfg(SP.OG[game], evaluator=orc.EVAL_HASH, salt=SALT, seed=SEED)
        _oracle[name] = [orc.selfplay_game(cfg, FIRST_ID + g, 1.0, SIMS, max_plies) for g in range(SIZES[game][1])]
    return _oracle[name]


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("name", HASHED)
def test_harvested_games_are_the_oracles(orc, name, step):
    """The records as fetch_games returned them in mid-run, game by game against the oracle's serial games: positions,
    visits / total, player, z, winner, length and header."""
    mine, _led = _harvest_run(name, step)
    game = CASES[name][0]
    lengths = set()
    for k, o in enumerate(_oracle_games(orc, name)):
        SP.assert_game_is_the_oracles(game, mine, k, o, FIRST_ID)
        lengths.add(o["n"])
    assert game == DC or len(lengths) > 3, lengths    # (the dense games end at different plies: slots are refilled out of step)


_lockstep = {}


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("name", NOT_LOCKSTEP)
def test_harvested_games_are_the_lockstep_engines(name, step):
    """What was harvested from a structure that plays many plies per launch against a second engine that plays the same seeds
    launch by launch and is read once, at the end."""
    mine, _led = _harvest_run(name, step)
    if name not in _lockstep:
        eng = _engine(name, lockstep=True)
        try:
            _lockstep[name] = SP.play_to_end(eng, SIZES[CASES[name][0]][1], 4, 1.0, headers=True)
        finally:
            eng.close()
    SP.assert_same_records(mine, _lockstep[name], name, counters=("sims", "games_finished", "examples"), no_overflow=True)


# ---- c. the gather kernel's lists -------------------------------------------------------------------------------------------------
SPARE = 3   # games the paused engines have room for beyond those they begin: their headers stay zero


def _paused(game):
    """A hash-evaluator run stopped when at least five games are done and others are not, on an engine with room for SPARE
    more games than it began; (engine, headers of every game it has room for, fetch_examples of the same)."""
    n_slots, n_games = SIZES[game]
    eng = _engine({C4: "c4-hash-lockstep", DC: "dc-hash-lockstep"}[game], max_games=n_games + SPARE)
    eng.selfplay_begin(n_games, 1.0)
    for _ in range(eng.max_plies * 2):
        eng.selfplay_step(1)
        if eng.selfplay_done()[1] >= 5:
            break
    hdr = eng.selfplay_headers(0, n_games + SPARE)
    return eng, hdr, eng.fetch_examples(0, n_games + SPARE)


def _lists(hdr, n_games):
    done = hdr[:, 3] != 0
    f, u = np.flatnonzero(done), np.flatnonzero(~done)
    assert len(f) >= 5 and (u < n_games).sum() >= 2 and (u >= n_games).sum() == SPARE, (f, u)
    rng = np.random.RandomState(3)
    beyond = u[u >= n_games]
    long_list = np.tile(np.concatenate([rng.permutation(f), u[:2], f[:1]]), 300 // (len(f) + 3) + 1)
    assert len(long_list) > 256
    return {
        "one": f[:1], "the last one": f[-1:], "ascending": f, "descending": f[::-1], "permuted": rng.permutation(f),
        "twice": [f[0], f[1], f[0]], "three times in a row": [f[1], f[1], f[1], f[2]], "nothing but one game": [f[3]] * 4,
        "unfinished first": [u[0], f[0], f[1]], "unfinished in the middle": [f[0], u[0], f[1]], "unfinished last": [f[0], f[1], u[0]],
        "several unfinished in a row": [u[1], u[0], f[2], u[0], u[1], u[2], f[0], u[3 % len(u)], u[0], f[4], u[1], u[1]],
        "only unfinished": u, "one unfinished": u[:1],
        "beyond the games begun": [f[0], beyond[0], beyond[1], f[1], beyond[2]], "only beyond the games begun": beyond,
        "longer than a block of threads": long_list,
    }


@pytest.mark.parametrize("game", [C4, DC], ids=["c4", "dc"])
def test_fetch_games_lists(game):
    """Every list against the answer assembled on the host from bb_examples_fetch of the same moment.  A game that is not done
    is a zero-length entry, a game listed twice two entries with the same rows: where `last g with off[g] <= rec` can go wrong."""
    assert _lib.game_info(game).example_bytes % 16 == 0     # the kernel copies in 16-byte units
    n_games = SIZES[game][1]
    eng, hdr, examples = _paused(game)
    try:
        for what, ids in _lists(hdr, n_games).items():
            ids = np.asarray(ids, dtype=np.int32)
            want = HC.expected_fetch_games(ids, hdr, examples)
            got = eng.fetch_games(ids)
            for g, w, part in zip(got, want, ("records", "offsets", "winners")):
                assert_same_array(g, w, (what, part))
            if "only" in what or what == "one unfinished":
                assert len(got[0]) == 0 and (got[2] == -2).all() and (got[1] == got[1][0]).all(), what
            else:
                assert len(got[0]) > 0, what
        assert len(examples[0]) > 0 and (examples[2] == -2).sum() >= 2 + SPARE
        # begun again: before any step the headers are zero and no game has a record
        eng.selfplay_begin(n_games, 1.0)
        assert not eng.selfplay_headers(0, n_games + SPARE).any()
        rec, offs, win = eng.fetch_games(np.arange(n_games + SPARE))
        assert len(rec) == 0 and not offs.any() and (win == -2).all()
    finally:
        eng.close()


# ---- d. refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_nothing_half_done():
    n_games = SIZES[C4][1]
    eng, hdr, examples = _paused(C4)
    try:
        done = np.flatnonzero(hdr[:, 3] != 0).astype(np.int32)
        ids = np.concatenate([done[::-1], [n_games - 1], done[:2]]).astype(np.int32)
        want = HC.expected_fetch_games(ids, hdr, examples)
        need = int(want[1][-1])

        def unchanged(after):
            for got, ref in ((eng.fetch_games(ids, need), want), (eng.fetch_examples(0, n_games + SPARE), examples)):
                for g, w in zip(got, ref):
                    assert_same_array(g, w, ("after", after))
            assert_same_array(eng.selfplay_headers(0, n_games + SPARE), hdr, ("headers after", after))

        unchanged("nothing")     # (a buffer of exactly the records needed is enough)
        for what, bad in (("id -1", [done[0], -1]), ("id max_games", [done[0], n_games + SPARE]), ("an empty list", [])):
            with pytest.raises(ValueError):
                eng.fetch_games(np.asarray(bad, dtype=np.int32))
            unchanged(what)
        # one record too few: the error of bb_examples_fetch for the same shortage
        with pytest.raises(_lib.BlackbirdHipError, match="records_out too small") as short:
            eng.fetch_games(ids, need - 1)
        assert "error %d" % _lib.ERR_CAPACITY in str(short.value)
        unchanged("a buffer one record short")
        all_rec = len(examples[0])
        buf = np.zeros(all_rec, dtype=_lib.example_dtype(C4))
        offs, win = np.zeros(n_games + SPARE + 1, dtype=np.int32), np.zeros(n_games + SPARE, dtype=np.int8)
        rc = _lib.lib().bb_examples_fetch(eng.h, 0, n_games + SPARE, _lib.ptr(buf), all_rec - 1, _lib.ptr(offs), _lib.ptr(win))
        assert rc == _lib.ERR_CAPACITY
        with pytest.raises(_lib.BlackbirdHipError, match="records_out too small"):
            _lib.check(rc)
        unchanged("bb_examples_fetch one record short")
    finally:
        eng.close()


# ---- e. the front end's loop ------------------------------------------------------------------------------------------------------
def test_generate_training_samples_stores_what_it_keeps(tmp_path, monkeypatch):
    """Blackbird.GenerateTrainingSamples harvests after every launch and stores blobs of what it harvested; the records it keeps
    on the device are a snapshot taken after the last game.  With more games than the engine has slots, the stored blobs must
    be, in number and content, the blobs of the kept records: z, visits / total in float64 and the planes, as blobs_of forms them."""
    monkeypatch.chdir(tmp_path)
    n_games, n_slots = 40, 12
    monkeypatch.setattr(Blackbird, "MAX_CONCURRENT_GAMES", n_slots)
    model = MC.model(Connect4.BoardState, "harvest", seed=5, play_limit=SIMS, eps=0.3, blocks=2)
    model.KeepDeviceExamples = True
    fetched = []
    try:
        eng = model._selfplay_engine(n_games)
        assert eng.n_slots == n_slots < n_games
        inner = eng.fetch_games

        def counted(ids, n_records=None):
            out = inner(ids, n_records)
            fetched.append((len(ids), eng.selfplay_done()[1]))
            return out

        monkeypatch.setattr(eng, "fetch_games", counted)
        Blackbird.GenerateTrainingSamples(model, n_games, 1.0)
        assert model._selfplay_engine(n_games) is eng     # (the run went through the engine that was watched)
        blobs = model.Conn.GetGames(model.Name, model.Version)
        rec = model.KeptDeviceExamples().records.cpu().numpy().reshape(-1).view(_lib.example_dtype(C4))
        print("harvests (games, finished by then):", fetched)
        assert sum(n for n, _fin in fetched) == n_games and len(fetched) >= 3 and fetched[0][1] < n_games
        assert len(np.unique(rec["game_id"])) == n_games and (rec["total"] == 0).sum() == n_games
        st = np.ascontiguousarray(rec["state"]).view(np.uint64).reshape(len(rec), 2)
        tot = rec["total"].astype(np.float64)
        pi = np.where(tot[:, None] > 0, rec["visits"][:, :7].astype(np.float64) / np.maximum(tot, 1.0)[:, None], 0.0)
        want = proto_wire.encode_states_batch(rec["z"].astype(np.float32), pi, _lib.game_encode(C4, st)[:, None])
        assert len(blobs) == len(want) == len(rec)
        assert sorted(bytes(b) for b in blobs) == sorted(bytes(b) for b in want)
        assert len({zlib.crc32(bytes(b)) for b in want}) > n_games    # (the blobs tell positions apart)
    finally:
        if getattr(model, "_batch_engine", None) is not None:
            model._batch_engine.close()
        model.Conn.Close()
