"""The shared comparators of tests/search_cases.py and tests/selfplay_cases.py on hand-made snapshots (no GPU, and no call into the built library: the support modules import blackbird_amd, which loads it lazily): an
equal pair passes, and a pair that differs from it in exactly one way fails -- or passes where the difference is one the caller
asked to ignore.  And play_to_end gives up, with an assertion, on an engine whose games never end."""
import numpy as np
import pytest

from tests import search_cases as S
from tests import selfplay_cases as SP

COUNTERS = dict(sims=40, nodes=33, overflow=0, evals=30, eval_cache_hits=0, eval_cache_probes=0)


def _snapshot():
    out = dict(action=np.array([3, 5], dtype=np.int32), root_winrate=np.array([0.5, 0.0], dtype=np.float32))
    rows = [dict(child=np.array([1, -1], dtype=np.int32), value=np.array([0.25, 0.0], dtype=np.float32), n_children=2),
            dict(child=np.array([-1, -1], dtype=np.int32), value=np.array([0.0, 0.0], dtype=np.float32), n_children=0)]
    return out, rows, dict(COUNTERS)


def _action(s):
    s[0]["action"][1] = 6


def _negative_zero(s):
    s[1][0]["value"][1] = -0.0


def _counter(s):
    s[2]["nodes"] += 1


def _missing_row(s):
    del s[1][1]


def _dtype(s):
    s[0]["action"] = s[0]["action"].astype(np.int64)


def _cache_counter(s):
    s[2]["evals"] -= 1


@pytest.mark.parametrize("change", [_action, _negative_zero, _counter, _missing_row, _dtype, _cache_counter])
def test_assert_same_fails_on_one_difference(change):
    a, b = _snapshot(), _snapshot()
    S.assert_same(a, b, "equal")
    change(b)
    with pytest.raises(AssertionError):
        S.assert_same(a, b, change.__name__)


def test_assert_same_ignores_only_the_named_counters():
    a, b = _snapshot(), _snapshot()
    _cache_counter(b)
    S.assert_same(a, b, "ignored", ignore_counters=S.CACHE_COUNTERS)
    _counter(b)
    with pytest.raises(AssertionError):
        S.assert_same(a, b, "another counter", ignore_counters=S.CACHE_COUNTERS)


def test_same_trio_holds_the_counter_identities():
    a, b, c = _snapshot(), _snapshot(), _snapshot()
    c[2].update(evals=20, eval_cache_hits=10, eval_cache_probes=30)
    S.same_trio((a, b, c), "trio")
    c[2]["eval_cache_hits"] = 9                      # probes != evals + hits
    with pytest.raises(AssertionError):
        S.same_trio((a, b, c), "trio")
    with pytest.raises(AssertionError):
        S.same_trio((a, b, c), "trio", probing=False)


REC = np.dtype([("game_id", "<u4"), ("ply", "<u2"), ("z", "i1"), ("visits", "<u4", (3,))])


def _run():
    rec = np.zeros(5, dtype=REC)
    rec["ply"] = [0, 1, 2, 0, 1]
    rec["visits"][:, 1] = 7
    return dict(rec=rec, offs=np.array([0, 3, 5], dtype=np.int32), win=np.array([1, -1], dtype=np.int8),
                hdr=np.array([[3, 1, 2, 1], [2, -1, 1, 1]], dtype=np.int32), cnt=dict(COUNTERS))


def _record_byte(r):
    r["rec"].view(np.uint8)[17] ^= 1


def _offset(r):
    r["offs"][1] = 2


def _winner(r):
    r["win"][1] = 0


def _header(r):
    r["hdr"][1, 2] = 2


def _offsets_dtype(r):
    r["offs"] = r["offs"].astype(np.int64)


def _sims(r):
    r["cnt"]["sims"] += 1


@pytest.mark.parametrize("change", [_record_byte, _offset, _winner, _header, _offsets_dtype, _sims])
def test_assert_same_records_fails_on_one_difference(change):
    a, b = _run(), _run()
    SP.assert_same_records(a, b, "equal", counters=("sims", "nodes"), no_overflow=True)
    change(b)
    with pytest.raises(AssertionError):
        SP.assert_same_records(a, b, change.__name__, counters=("sims", "nodes"), no_overflow=True)


def test_assert_same_records_compares_only_the_named_counters_and_overflow_on_request():
    a, b = _run(), _run()
    _sims(b)
    b["cnt"]["overflow"] = 1
    SP.assert_same_records(a, b, "no counters named")
    with pytest.raises(AssertionError):
        SP.assert_same_records(a, b, "overflow", no_overflow=True)


def test_assert_cache_counters():
    off = dict(sims=40, evals=30, eval_cache_hits=0, eval_cache_probes=0)
    on = dict(sims=40, evals=20, eval_cache_hits=10, eval_cache_probes=30)
    SP.assert_cache_counters(on, off)
    SP.assert_cache_counters(dict(off), off, probed=False)
    for key, value in (("eval_cache_probes", 31), ("evals", 21), ("sims", 41)):   # probes != evals + hits, ...
        with pytest.raises(AssertionError):
            SP.assert_cache_counters(dict(on, **{key: value}), off)
    with pytest.raises(AssertionError):
        SP.assert_cache_counters(on, dict(off, eval_cache_probes=1))
    with pytest.raises(AssertionError):
        SP.assert_cache_counters(on, off, probed=False)


class _NeverDone:
    max_plies = 9

    def __init__(self):
        self.begun, self.steps = None, 0

    def selfplay_begin(self, n_games, temp):
        self.begun = (n_games, temp)

    def selfplay_done(self):
        return False, 0

    def selfplay_step(self, plies):
        self.steps += 1


@pytest.mark.parametrize("steps_below, stops_at", [(None, 4 * (5 + 1)), (7, 7)])
def test_play_to_end_stops_at_its_bound(steps_below, stops_at):
    eng = _NeverDone()
    assert SP.step_bound(4, 9, 2) == 4 * (5 + 1)
    with pytest.raises(AssertionError, match="not over"):
        SP.play_to_end(eng, 4, 2, 1.0, steps_below=steps_below)
    assert eng.begun == (4, 1.0) and eng.steps == stops_at
