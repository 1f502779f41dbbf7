"""No GPU: the ledger of tests/harvest_cases.py on a run made by hand -- three games on two slots, harvested after each of four
steps with all three readers -- which it must accept, and the same run with one thing wrong at a time, each of which it must
reject by the assertion that is there for it (matched by its message).  Every assertion of the ledger has its case here."""
import numpy as np
import pytest

from tests.harvest_cases import Ledger, expected_fetch_games, no_games, z_of

FIRST = 700
DT = np.dtype([("game_id", "<u4"), ("ply", "<u2"), ("player", "u1"), ("z", "i1"), ("total", "<u4"), ("n_children", "<u4"),
               ("visits", "<u4", (4,))])
# game: (records, winner, the step after which it is done); game 2 follows game 0 on slot 0
GAMES = [(3, 1, 1), (5, 2, 2), (2, 0, 3)]
N_GAMES, N_SLOTS, STEPS = 3, 2, 4


def _game(g):
    n, w, _step = GAMES[g]
    r = np.zeros(n, dtype=DT)
    r["game_id"] = FIRST + g
    r["ply"] = np.arange(n)
    r["player"] = 1 + np.arange(n) % 2
    r["z"] = z_of(w, r["player"])
    r["total"] = 16
    r["total"][-1] = 0
    r["n_children"] = 4
    r["visits"] = 4 + g
    r["visits"][-1] = 0
    return r


def _headers(step):
    hdr = np.zeros((N_GAMES, 4), dtype=np.int32)
    for g, (n, w, at) in enumerate(GAMES):
        if at <= step:
            hdr[g] = (n, w, n - 1, 1)
    return hdr


def _fetch_examples(step, first=0, n=N_GAMES):
    hdr = _headers(step)
    parts, offs, win = [], [0], []
    for g in range(first, first + n):
        done = hdr[g, 3] != 0
        parts.append(_game(g) if done else np.zeros(0, dtype=DT))
        offs.append(offs[-1] + len(parts[-1]))
        win.append(hdr[g, 1] if done else -2)
    return np.concatenate(parts), np.array(offs, dtype=np.int32), np.array(win, dtype=np.int8)


def _feed_args(step):
    """Everything Ledger.feed takes after `step`, as fresh arrays."""
    hdr = _headers(step)
    ids = np.array([g for g, (_n, _w, at) in enumerate(GAMES) if at == step], dtype=np.int32)
    examples = _fetch_examples(step)
    fetched = expected_fetch_games(ids, hdr, examples) if len(ids) else no_games(DT)
    return dict(hdr=hdr, ids=ids, fetched=tuple(np.copy(a) for a in fetched), examples=examples,
                sub=(1, _fetch_examples(step, 1, 2)), device=examples[0].view(np.uint8).reshape(len(examples[0]), DT.itemsize).copy())


def _final():
    rec, offs, win = _fetch_examples(STEPS - 1)
    return dict(rec=rec, offs=offs, win=win, hdr=_headers(STEPS - 1))


def _drive(corrupt=None):
    led = Ledger(N_GAMES, N_SLOTS, FIRST)
    for step in range(STEPS):
        kw = _feed_args(step)
        if corrupt:
            corrupt(step, kw)
        led.feed(**kw)
    final = _final()
    if corrupt:
        corrupt("final", final)
    led.finish(final)
    return led


def test_the_ledger_accepts_a_correct_run():
    led = _drive()
    assert (led.harvests, led.overlapped, led.games_overlapped) == (3, 2, 2)   # (nothing runs beside the last game)
    assert (led.in_refilled_slot, led.refilled_since) == (1, 1)                # game 2, and game 0 before it
    led.assert_not_vacuous()
    run = led.as_run()
    assert run["rec"].tobytes() == _final()["rec"].tobytes() and run["hdr"].tolist() == _final()["hdr"].tolist()
    assert led.running(_headers(0)) == [0, 1] and led.running(_headers(1)) == [1, 2] and led.running(_headers(3)) == []
    assert led.unharvested(_headers(3)).tolist() == []
    assert Ledger(N_GAMES, N_SLOTS).unharvested(_headers(2)).tolist() == [0, 1]


def test_the_expected_answer_of_fetch_games():
    """expected_fetch_games, which the -m gpu tests hold the gather kernel to, on lists with a game twice and unfinished games."""
    hdr, ex = _headers(2), _fetch_examples(2)
    rec, offs, win = expected_fetch_games([1, 2, 0, 0, 2], hdr, ex)
    assert offs.tolist() == [0, 5, 5, 8, 11, 11] and win.tolist() == [2, -2, 1, 1, -2] and offs.dtype == np.int32
    assert rec.tobytes() == np.concatenate([_game(1), _game(0), _game(0)]).tobytes() and win.dtype == np.int8
    rec, offs, win = expected_fetch_games([2, 2], hdr, ex)
    assert len(rec) == 0 and rec.dtype == DT and offs.tolist() == [0, 0, 0] and win.tolist() == [-2, -2]


def test_z_of():
    assert z_of(1, [1, 2, 1]).tolist() == [1, -1, 1] and z_of(2, [1, 2, 1]).tolist() == [-1, 1, -1]
    assert z_of(0, [1, 2]).tolist() == [0, 0] and z_of(-1, [1, 2]).tolist() == [0, 0]   # a draw; the ply cap


# ---- one thing wrong at a time ---------------------------------------------------------------------------------------------------
def _at(step, fn):
    def corrupt(s, kw):
        if s == step:
            fn(kw)
    return corrupt


def _set(path, value):
    """kw[path[0]][path[1]]...[path[-1]] = value"""
    def fn(kw):
        x = kw
        for p in path[:-1]:
            x = x[p]
        x[path[-1]] = value
    return fn


def _z_still_zero(kw):
    kw["fetched"][0]["z"] = 0          # the harvest overtook the back-fill; the later readers show it filled in


def _harvest_again(kw):                # game 0 (done since step 1) once more at step 2, with its right records
    kw["ids"] = np.array([1, 0], dtype=np.int32)
    kw["fetched"] = expected_fetch_games(kw["ids"], kw["hdr"], kw["examples"])


def _harvest_early(kw):                # game 1 at step 1, when it is not done: fetch_games returns nothing for it
    kw["ids"] = np.array([0, 1], dtype=np.int32)
    kw["fetched"] = expected_fetch_games(kw["ids"], kw["hdr"], kw["examples"])


def _skip(kw):
    kw["ids"] = np.zeros(0, dtype=np.int32)
    kw["fetched"] = no_games(DT)


def _reader_reports_finished(kw):      # game 1 at step 1: a winner, and rows, for a game whose done is 0
    kw["examples"][2][1] = 2
    kw["sub"] = None
    kw["device"] = None


def _drop_last_row(kw):
    rec, offs, win = kw["fetched"]
    kw["fetched"] = (rec[:-1], offs, win)


def _one_row_less(kw):                 # consistent in itself, one row short of the header's count
    rec, offs, win = kw["fetched"]
    offs[-1] -= 1
    kw["fetched"] = (rec[:-1], offs, win)


def _reader_row_changed(kw):           # game 0's first row at step 2, a step after it was harvested (a refill that wrote there)
    kw["examples"][0]["visits"][0, 0] += 1
    kw["sub"] = None
    kw["device"] = None


def _reader_offsets(kw):
    kw["examples"][1][1] += 1
    kw["sub"] = None


def _no_examples(kw):
    kw["examples"] = None


CORRUPTIONS = {
    # those of the issue
    "z still 0 at harvest time": (_at(1, _z_still_zero), "z does not follow from the winner"),
    "header count changes after done": (_at(2, _set(("hdr", (0, 0)), 4)), "header changed after done"),
    "game harvested twice": (_at(2, _harvest_again), "harvested twice"),
    "game never harvested": (_at(2, _skip), "never harvested"),
    "record with the wrong game_id": (_at(2, _set(("fetched", 0, "game_id", 3), FIRST)), "wrong game_id"),
    "reader reports an unfinished game as finished": (_at(1, _reader_reports_finished), "unfinished games are not the headers'"),
    # the rest of the ledger's assertions
    "z of the loser's rows wrong": (_at(2, _set(("fetched", 0, "z", 0), 1)), "z does not follow from the winner"),
    "z in a drawn game": (_at(3, _set(("fetched", 0, "z", 1), -1)), "z does not follow from the winner"),
    "headers of another type": (_at(0, lambda kw: kw.update(hdr=kw["hdr"].astype(np.int64))), "headers"),
    "done turns off": (_at(2, _set(("hdr", (0, 3)), 0)), "done turned off"),
    "header winner changes after done": (_at(3, _set(("hdr", (1, 1)), 1)), "header changed after done"),
    "final header differs": (_at("final", _set(("hdr", (2, 2)), 5)), "header changed after done"),
    "offsets do not end at the record count": (_at(1, _drop_last_row), "harvest shape"),
    "harvested before done": (_at(1, _harvest_early), "harvested before done"),
    "a row less than the header says": (_at(1, _one_row_less), "record count is not the header's"),
    "winner is not the header's": (_at(1, _set(("fetched", 2, 0), 2)), "winner is not the header's"),
    "ply does not count up": (_at(2, _set(("fetched", 0, "ply", 4), 3)), "ply does not run"),
    "last record has visits": (_at(1, _set(("fetched", 0, "total", 2), 16)), "last record is not the terminal one"),
    "reader's winner differs": (_at(2, _set(("examples", 2, 0), 2)), "winners are not the headers'"),
    "reader's shape": (_at(2, lambda kw: kw.update(examples=_fetch_examples(2, 0, 2), sub=None, device=None)), "fetch_examples shape"),
    "reader's offsets": (_at(2, _reader_offsets), "offsets are not the headers' counts"),
    "reader shows a harvested row changed": (_at(2, _reader_row_changed), "not the records fetch_games returned"),
    "sub-range from game 0": (_at(2, lambda kw: kw.update(sub=(0, _fetch_examples(2, 0, 2)))), "sub-range"),
    "sub-range winners": (_at(2, _set(("sub", 1, 2, 0), -2)), "sub-range winners"),
    "sub-range offsets": (_at(2, _set(("sub", 1, 1, 2), 6)), "sub-range offsets"),
    "sub-range records": (_at(2, _set(("sub", 1, 0, "total", 0), 15)), "sub-range records"),
    "device view": (_at(2, _set(("device", (0, 0)), 1)), "device view"),
    "readers without fetch_examples": (_at(2, _no_examples), "compared with fetch_examples"),
    "final records differ": (_at("final", _set(("rec", "visits", (4, 1)), 9)), "harvested in mid-run vs the final fetch"),
    "final winners differ": (_at("final", _set(("win", 2), -1)), "harvested in mid-run vs the final fetch"),
    "final offsets differ": (_at("final", _set(("offs", 3), 11)), "harvested in mid-run vs the final fetch"),
}


@pytest.mark.parametrize("name", list(CORRUPTIONS))
def test_the_ledger_rejects(name):
    corrupt, message = CORRUPTIONS[name]
    with pytest.raises(AssertionError, match=message):
        _drive(corrupt)


def test_a_vacuous_run_is_refused():
    """One slot, one harvest at the end: everything agrees and nothing was shown."""
    led = Ledger(N_GAMES, N_SLOTS, FIRST)
    hdr, ex = _headers(3), _fetch_examples(3)
    led.feed(hdr, [0, 1, 2], expected_fetch_games([0, 1, 2], hdr, ex), examples=ex)
    led.finish(_final())
    with pytest.raises(AssertionError):
        led.assert_not_vacuous()
