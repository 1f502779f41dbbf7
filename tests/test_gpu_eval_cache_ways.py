"""The two-way buckets of the Connect4 evaluation cache (net.hip.h: a bucket is two entries in one 128-byte line, a miss is
stored into the way games.hip.h eval_cache_pick_way names) change no result: whichever way an entry sits in, and whatever
was evicted for it, a hit returns the bits the tower would have produced.

The shapes are those of test_gpu_eval_cache.py (persistent kernel) and test_gpu_rounds_eval_cache.py (asynchronous rounds,
here LAUNCH_ROUNDS with general_net), whose helpers are used: records byte-identical with the cache on and off at the default
size, on tables so small that every bucket is fought over (2^10 entries = 512 buckets, and 2^11), and after a weight
reload on such a table.  More games than slots are played, so a refilled slot's first leaf is the initial position -- the
shallowest there is, which the kept way never gives up -- and the hit counter is non-zero even on the tiny tables.  No
test asserts a hit share: which probe finds which entry depends on timing."""
import pytest

from blackbird_amd import _lib
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu

ROUNDS = dict(launch=_lib.LAUNCH_ROUNDS, general_net=True)


def _play_persistent(eng, flat, n_games):
    return SP.play_loaded(eng, flat, n_games, 8, mode=None)


def _play_rounds(eng, flat, n_games):
    return SP.play_loaded(eng, flat, n_games, 4, mode=1, steps_below=4096)


def _rounds_on_off(monkeypatch, flat, slots, sims, n_games, log2):
    res = {}
    for cache in (True, False):
        eng = SP.c4_engine_under_cache(monkeypatch, cache, slots, sims, n_games, log2=log2, **ROUNDS)
        try:
            res[cache] = _play_rounds(eng, flat, n_games)
        finally:
            eng.close()
    SP.assert_same_records(res[True], res[False], ("rounds", log2))
    SP.assert_cache_counters(res[True]["cnt"], res[False]["cnt"])
    return res[True]["cnt"]


def _persistent_on_off(monkeypatch, flat, slots, sims, n_games, log2):
    res = {}
    for cache in (True, False):
        eng = SP.c4_engine_under_cache(monkeypatch, cache, slots, sims, n_games, log2=log2)
        try:
            assert eng.selfplay_mode() == 3
            res[cache] = _play_persistent(eng, flat, n_games)
        finally:
            eng.close()
    SP.assert_same_records(res[True], res[False], ("persistent", log2))
    SP.assert_cache_counters(res[True]["cnt"], res[False]["cnt"])
    return res[True]["cnt"]


@pytest.mark.parametrize("log2", [None, 10, 11], ids=["default", "2^10", "2^11"])
def test_persistent_same_records(monkeypatch, log2):
    on = _persistent_on_off(monkeypatch, SP.c4_weights(16, 4, seed=0), slots=128, sims=200, n_games=256, log2=log2)
    assert on["eval_cache_hits"] > 0


@pytest.mark.parametrize("log2", [None, 10, 11], ids=["default", "2^10", "2^11"])
def test_rounds_same_records(monkeypatch, log2):
    on = _rounds_on_off(monkeypatch, SP.c4_weights(16, 2), slots=256, sims=32, n_games=384, log2=log2)
    assert on["eval_cache_hits"] > 0


def test_rounds_two_streams_tiny_table(monkeypatch):
    """two slot-range views on two streams fight over 512 buckets"""
    on = _rounds_on_off(monkeypatch, SP.c4_weights(16, 2), slots=512, sims=32, n_games=768, log2=10)
    assert on["eval_cache_hits"] > 0


def test_persistent_no_stale_entries_tiny_table(monkeypatch):
    # entries made with weights A must not answer for weights B, in either way of a bucket
    fa, fb = SP.c4_weights(16, 4, seed=0), SP.c4_weights(16, 4, seed=1)
    eng = SP.c4_engine_under_cache(monkeypatch, True, 128, 200, 256, log2=10)
    try:
        first = _play_persistent(eng, fa, 256)
        after = _play_persistent(eng, fb, 256)
    finally:
        eng.close()
    assert first["cnt"]["eval_cache_hits"] > 0
    fresh = SP.c4_engine_under_cache(monkeypatch, False, 128, 200, 256)
    try:
        ref = _play_persistent(fresh, fb, 256)
    finally:
        fresh.close()
    SP.assert_same_records(after, ref, "persistent, after a reload")


def test_rounds_no_stale_entries_tiny_table(monkeypatch):
    fa, fb = SP.c4_weights(16, 2, seed=0), SP.c4_weights(16, 2, seed=1)
    eng = SP.c4_engine_under_cache(monkeypatch, True, 256, 32, 384, log2=10, **ROUNDS)
    try:
        first = _play_rounds(eng, fa, 384)
        after = _play_rounds(eng, fb, 384)
    finally:
        eng.close()
    assert first["cnt"]["eval_cache_hits"] > 0
    fresh = SP.c4_engine_under_cache(monkeypatch, False, 256, 32, 384, **ROUNDS)
    try:
        ref = _play_rounds(fresh, fb, 384)
    finally:
        fresh.close()
    SP.assert_same_records(after, ref, "rounds, after a reload")
