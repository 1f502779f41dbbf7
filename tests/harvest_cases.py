"""Support for the tests that read finished games while other games are still being played (not collected).

The records of a finished game never change again, so whatever is harvested in mid-run must be, byte for byte, what the
final fetch of that game returns.  A Ledger is fed after every step -- the headers, the ids harvested, what fetch_games
returned for them and, where asked for, what the other readers returned at the same moment -- and asserts as it goes;
finish() holds what it collected against the state after the last step.  harvest() does the reading for an engine.
The ledger needs numpy alone (tests/test_harvest_cpu.py feeds it a run made by hand and every corruption it must reject);
records are any structured array with the fields game_id, ply, player, z and total."""
import numpy as np

from tests.search_cases import assert_same_array


def z_of(winner, player):
    """z of every record of a game from its winner (header word 1) and the records' side to move (Blackbird.py:260-264)."""
    player = np.asarray(player)
    if winner <= 0:
        return np.zeros(len(player), dtype=np.int8)
    return np.where(player == winner, 1, -1).astype(np.int8)


class Ledger:
    """n_games games on n_slots slots (game k + n_slots is the next game of game k's slot), global ids from first_game_id."""

    def __init__(self, n_games, n_slots, first_game_id=0):
        self.n_games, self.n_slots, self.first_game_id = int(n_games), int(n_slots), int(first_game_id)
        self.hdr = np.zeros((self.n_games, 4), dtype=np.int32)   # the headers as last seen
        self.games = {}                 # id -> (its records as harvested, its winner as harvested)
        self.harvests = 0               # non-empty ones
        self.overlapped = 0             # ... made while a begun game was still being played
        self.games_overlapped = 0       # the games of those
        self.in_refilled_slot = 0       # harvested games that were not the first of their slot
        self.refilled_since = 0         # harvested games whose slot had its next game by then

    # ---- headers ---------------------------------------------------------------------------------------------------------
    def see_headers(self, hdr):
        hdr = np.asarray(hdr)
        assert hdr.dtype == np.int32 and hdr.shape == (self.n_games, 4), ("headers", hdr.dtype, hdr.shape)
        was = self.hdr[:, 3] != 0
        off = np.flatnonzero(was & (hdr[:, 3] == 0))
        assert not len(off), ("done turned off", off.tolist())
        changed = np.flatnonzero(was & (hdr != self.hdr).any(axis=1))
        assert not len(changed), ("header changed after done", changed.tolist(), self.hdr[changed].tolist(), hdr[changed].tolist())
        self.hdr = hdr.copy()

    def unharvested(self, hdr):
        """The ids that are done in hdr and have not been harvested, ascending."""
        return np.array([g for g in np.flatnonzero(np.asarray(hdr)[:, 3] != 0) if int(g) not in self.games], dtype=np.int32)

    def running(self, hdr):
        """The ids of the games that have begun (the first of a slot, or the game after a finished one) and are not done."""
        done = np.asarray(hdr)[:, 3] != 0
        return [g for g in range(self.n_games) if not done[g] and (g < self.n_slots or done[g - self.n_slots])]

    # ---- one harvest -----------------------------------------------------------------------------------------------------
    def feed(self, hdr, ids, fetched, examples=None, sub=None, device=None):
        """hdr: selfplay_headers(0, n_games); ids: the games harvested now; fetched: fetch_games(ids) = (rec, offs, win);
        examples: fetch_examples(0, n_games) of the same moment; sub: (first_game > 0, fetch_examples(first_game, n)); device: the
        bytes of dist.engine_records_device (uint8 [n_records, record bytes])."""
        self.see_headers(hdr)
        hdr = self.hdr
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        rec, offs, win = fetched
        assert len(offs) == len(ids) + 1 and len(win) == len(ids) and offs[0] == 0 and offs[-1] == len(rec), \
            ("harvest shape", len(ids), len(offs), len(win), len(rec))
        running = self.running(hdr)
        for k, gid in enumerate(ids.tolist()):
            assert gid not in self.games, ("harvested twice", gid)
            assert hdr[gid, 3] != 0, ("harvested before done", gid)
            r = rec[offs[k]:offs[k + 1]]
            self.check_game(gid, r, int(win[k]))
            self.games[gid] = (r.copy(), int(win[k]))
            self.in_refilled_slot += gid >= self.n_slots
            self.refilled_since += gid + self.n_slots < self.n_games
        if len(ids):
            self.harvests += 1
            if running:
                self.overlapped += 1
                self.games_overlapped += len(ids)
        if examples is not None:
            self.check_readers(examples, sub, device)
        else:
            assert sub is None and device is None, "the other readers are compared with fetch_examples"

    def check_game(self, gid, r, win):
        """One game's records as harvested against its header: this is the moment the fences of the move tail exist for."""
        n, w = int(self.hdr[gid, 0]), int(self.hdr[gid, 1])
        assert len(r) == n >= 1, ("record count is not the header's", gid, len(r), n)
        assert win == w, ("winner is not the header's", gid, win, w)
        assert (r["game_id"] == self.first_game_id + gid).all(), ("wrong game_id", gid, r["game_id"].tolist())
        assert np.array_equal(r["ply"], np.arange(n)), ("ply does not run 0 .. n-1", gid, r["ply"].tolist())
        assert r["total"][-1] == 0, ("last record is not the terminal one", gid, int(r["total"][-1]))
        assert np.array_equal(r["z"], z_of(w, r["player"])), ("z does not follow from the winner", gid, w, r["z"].tolist(),
                                                             r["player"].tolist())

    def check_readers(self, examples, sub, device):
        rec, offs, win = examples
        hdr, done = self.hdr, self.hdr[:, 3] != 0
        assert len(win) == self.n_games and len(offs) == self.n_games + 1, ("fetch_examples shape", len(win), len(offs))
        assert np.array_equal(win == -2, ~done), ("fetch_examples: the unfinished games are not the headers'", win.tolist(),
                                                  done.tolist())
        assert np.array_equal(win[done], hdr[done, 1]), ("fetch_examples: winners are not the headers'", win.tolist())
        assert offs[0] == 0 and offs[-1] == len(rec) and np.array_equal(np.diff(offs), np.where(done, hdr[:, 0], 0)), \
            ("fetch_examples: offsets are not the headers' counts", np.asarray(offs).tolist(), len(rec))
        for gid in np.flatnonzero(done).tolist():
            if gid in self.games:    # (also a game harvested steps ago: its rows have not been touched since)
                assert rec[offs[gid]:offs[gid + 1]].tobytes() == self.games[gid][0].tobytes(), \
                    ("fetch_examples: not the records fetch_games returned", gid)
        if sub is not None:
            first, (srec, soffs, swin) = sub
            n = len(swin)
            assert 0 < first and first + n <= self.n_games and len(soffs) == n + 1, ("sub-range", first, n)
            assert_same_array(swin, win[first:first + n], "sub-range winners")
            assert_same_array(soffs, offs[first:first + n + 1] - offs[first], "sub-range offsets")
            assert_same_array(srec, rec[offs[first]:offs[first + n]], "sub-range records")
        if device is not None:
            assert np.asarray(device).tobytes() == rec.tobytes(), ("device view: not the bytes of fetch_examples",
                                                                   np.asarray(device).shape, len(rec))

    # ---- the end ---------------------------------------------------------------------------------------------------------
    def as_run(self):
        """What was harvested, put back in game order: rec, offs, win as fetch_examples returns them, and the last headers."""
        missing = [g for g in range(self.n_games) if g not in self.games]
        assert not missing, ("never harvested", missing)
        parts = [self.games[g][0] for g in range(self.n_games)]
        offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
        win = np.array([self.games[g][1] for g in range(self.n_games)], dtype=np.int8)
        return dict(rec=np.concatenate(parts), offs=offs, win=win, hdr=self.hdr.copy())

    def finish(self, final):
        """final: rec, offs, win of fetch_examples and hdr after the last step (selfplay_cases.play_to_end(headers=True))."""
        self.see_headers(final["hdr"])
        mine = self.as_run()
        for k in ("offs", "win", "rec"):
            assert_same_array(mine[k], final[k], ("harvested in mid-run vs the final fetch", k))
        return mine

    def report(self, what):
        print(f"{what}: {self.harvests} non-empty harvests, {self.overlapped} of them ({self.games_overlapped} games) while other "
              f"games were running; {self.in_refilled_slot} games in a refilled slot, {self.refilled_since} with their slot refilled")

    def assert_not_vacuous(self):
        """Conditions on the run's sizes: too few of these and the run has shown nothing about harvesting in mid-run."""
        assert self.harvests >= 3, self.harvests
        assert self.overlapped >= 1 and self.games_overlapped >= 1, (self.overlapped, self.games_overlapped)
        assert self.in_refilled_slot >= 1 and self.refilled_since >= 1, (self.in_refilled_slot, self.refilled_since)


# ---- reading an engine ---------------------------------------------------------------------------------------------------------
def no_games(dtype):
    """fetch_games of no game (the call itself refuses an empty list)."""
    return np.zeros(0, dtype=dtype), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int8)


def harvest(eng, ledger, device=None):
    """What Blackbird.GenerateTrainingSamples does between two launches -- headers, then fetch_games of the games that are newly
    done, into a buffer of exactly their records -- fed to the ledger with the other readers of the same moment: fetch_examples
    over all games and over a sub-range, and (device: a torch device name) dist.engine_records_device."""
    n = ledger.n_games
    hdr = eng.selfplay_headers(0, n)
    ids = ledger.unharvested(hdr)
    fetched = eng.fetch_games(ids, int(hdr[ids, 0].sum())) if len(ids) else no_games(ledger_dtype(eng))
    first = max(1, n // 3)
    view = None
    if device is not None:
        from blackbird_amd import dist
        assert eng.cfg.max_games == n   # (the device view covers the whole store)
        view = dist.engine_records_device(eng, device).cpu().numpy()
    ledger.feed(hdr, ids, fetched, examples=eng.fetch_examples(0, n), sub=(first, eng.fetch_examples(first, n - first - 1)),
                device=view)


def ledger_dtype(eng):
    from blackbird_amd import _lib
    return _lib.example_dtype(eng.game)


def expected_fetch_games(ids, hdr, examples):
    """What fetch_games(ids) must return, assembled from fetch_examples over games 0 .. len(hdr) - 1 of the same moment: the rows
    of game ids[k] at position k, offsets the running sum of the headers' counts (0 for a game that is not done), winner or -2."""
    rec, offs, win = examples
    ids = np.asarray(ids, dtype=np.int64)
    cnt = np.where(hdr[ids, 3] != 0, hdr[ids, 0], 0)
    parts = [rec[offs[g]:offs[g + 1]] for g in ids.tolist()]
    return (np.concatenate(parts) if parts else rec[:0], np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32),
            win[ids].astype(np.int8))
