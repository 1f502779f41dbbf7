"""bench.py's plain line and --dump-outputs: the dump's layout, 64 MB cap and fixed game set on synthetic records and a
stand-in engine (host only), and two short plain runs on the GPU in fresh child processes."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DC_RECORD = np.dtype([("game_id", "<u4"), ("ply", "<u2"), ("player", "u1"), ("z", "i1"), ("total", "<u4"),
                      ("n_children", "<u4"), ("state", "u1", (80,)), ("visits", "<u4", (144,)), ("action", "<u2", (144,))])


def _records(n_games, seed=1):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 200, n_games)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rec = np.zeros(offs[-1], DC_RECORD)
    rec["game_id"] = np.repeat(np.arange(n_games) + 4_000_000_000, counts)
    rec["ply"] = np.concatenate([np.arange(c) for c in counts])
    rec["visits"] = rng.integers(0, 800, rec["visits"].shape)
    rec["state"] = rng.integers(0, 256, rec["state"].shape)
    return rec, offs, np.arange(n_games) * 3, rng.integers(-1, 2, n_games).astype(np.int8)


def _load(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in glob.glob(os.path.join(d, "*.npy"))}


@pytest.mark.parametrize("n_games,budget,sampled", [(50, bench.DUMP_BYTES, False), (500, bench.DUMP_BYTES, True),
                                                    (500, 1 << 20, True)])
def test_dump_outputs_layout_cap_and_sample(tmp_path, n_games, budget, sampled):
    rec, offs, index, win = _records(n_games)
    kept, n = bench.dump_outputs(str(tmp_path / "a"), index, rec, offs, win, budget=budget)
    files = glob.glob(str(tmp_path / "a" / "*.npy"))
    assert sum(os.path.getsize(f) for f in files) <= budget
    d = _load(str(tmp_path / "a"))
    assert sorted(d) == sorted(["record_" + f for f in DC_RECORD.names] + ["game_index", "game_winner", "game_records"])
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert d["record_game_id"].dtype == np.float64
    assert n == n_games and len(d["game_index"]) == kept and 0 < kept <= n and (kept < n) == sampled
    assert np.all(np.diff(d["game_index"]) > 0)          # a sample keeps index order
    games = (d["game_index"] / 3).astype(np.int64)
    rows = np.concatenate([np.arange(offs[g], offs[g + 1]) for g in games])
    for f in DC_RECORD.names:                            # exact: every field fits its float type
        assert np.array_equal(d["record_" + f], rec[f][rows].astype(d["record_" + f].dtype)), f
    assert np.array_equal(d["game_records"], np.diff(offs)[games])
    assert np.array_equal(d["game_winner"], win[games])
    # the same records give the same files
    bench.dump_outputs(str(tmp_path / "b"), index, rec, offs, win, budget=budget)
    e = _load(str(tmp_path / "b"))
    assert all(np.array_equal(d[k], e[k]) for k in d)


def test_dump_outputs_no_games(tmp_path):
    rec = np.zeros(0, DC_RECORD)
    assert bench.dump_outputs(str(tmp_path), np.zeros(0, np.int64), rec, np.zeros(1, np.int32), np.zeros(0, np.int8)) == (0, 0)
    d = _load(str(tmp_path))
    assert len(d) == len(DC_RECORD.names) + 3 and all(len(a) == 0 for a in d.values())


class _FakeEngine:
    """The engine calls of bench.dump_games: game g of a batch finishes `done_at[g]` steps after selfplay_begin."""

    def __init__(self, done_at, rec, offs, win):
        self.done_at, self.rec, self.offs, self.win, self.t, self.n = done_at, rec, offs, win, 1000, 0

    def selfplay_begin(self, n, temp):
        self.t, self.n = 0, n

    def selfplay_done(self):
        return bool(np.all(self.done_at[:self.n] <= self.t)), 0

    def selfplay_headers(self, first, n):
        h = np.zeros((n, 4), np.int32)
        g = np.arange(first, first + n)
        h[:, 0] = np.diff(self.offs)[g]
        h[:, 3] = self.done_at[g] <= self.t
        return h

    def selfplay_step(self, k):
        self.t += k

    def counters(self):
        return {"overflow": 0}

    def fetch_games(self, ids, n_records):
        assert np.all(self.done_at[ids] <= self.t)
        rows = np.concatenate([np.arange(self.offs[g], self.offs[g + 1]) for g in ids])
        offs = np.concatenate([[0], np.cumsum(np.diff(self.offs)[ids])]).astype(np.int32)
        assert n_records == len(rows)
        return self.rec[rows], offs, self.win[ids]


def test_dump_games_plays_a_fresh_batch_to_the_end(tmp_path):
    rec, offs, _index, win = _records(40)
    done_at = np.random.default_rng(2).integers(0, 60, 40)
    eng = _FakeEngine(done_at, rec, offs, win)
    assert bench.dump_games(eng, str(tmp_path / "a"), 30, cap_steps=100) == (30, 30)
    assert eng.n == 30 and eng.t >= done_at[:30].max()
    d = _load(str(tmp_path / "a"))
    assert np.array_equal(d["game_index"], np.arange(30))
    assert np.array_equal(d["record_game_id"], rec["game_id"][:offs[30]].astype(np.float64))
    with pytest.raises(RuntimeError):                    # a batch that does not finish within the cap is an error
        bench.dump_games(_FakeEngine(done_at + 1000, rec, offs, win), str(tmp_path / "b"), 30, cap_steps=100)


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """A plain run: exactly --steps timed steps, the headline keys, none of the --full legs; --dump-outputs writes a batch of
    `slots` games, the same arrays in two runs."""
    slots = 512
    dumps = []
    for i in range(2):
        out = tmp_path / f"dump{i}"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                            "--prefill", "16", "--settle", "8", "--slots", str(slots), "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode == 0, p.stderr[-2000:]
        line = json.loads(p.stdout.strip().splitlines()[-1])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == 4 and sum(line["config"]["timed_launches"]) == 4 and line["ms_per_step"] > 0
        assert "cpu_baseline" not in line and "api" not in line
        assert sum(os.path.getsize(f) for f in glob.glob(str(out / "*.npy"))) <= bench.DUMP_BYTES
        d = _load(str(out))
        assert np.array_equal(d["game_index"], np.arange(slots))
        assert int(d["game_records"].sum()) == len(d["record_game_id"])
        assert np.all(d["record_visits"] / np.maximum(d["record_total"], 1.0)[:, None] <= 1.0)
        dumps.append(d)
    assert sorted(dumps[0]) == sorted(dumps[1])
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
