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
from tests import test_gpu_eval_cache as pk          # persistent kernel: _weights(seed), _engine, _play, _same
from tests import test_gpu_rounds_eval_cache as rd   # rounds: _weights(filters, blocks, seed), _engine, _play, _same, _on_off

pytestmark = pytest.mark.gpu

ROUNDS = dict(launch=_lib.LAUNCH_ROUNDS, general_net=True)


def _persistent_on_off(monkeypatch, flat, slots, sims, n_games, log2):
    res = {}
    for cache in (True, False):
        eng = pk._engine(monkeypatch, cache, slots, sims, n_games, log2=log2)
        try:
            assert eng.selfplay_mode() == 3
            res[cache] = pk._play(eng, flat, n_games)
        finally:
            eng.close()
    pk._same(res[True], res[False])
    on, off = res[True][3], res[False][3]
    print("log2", log2, "on:", {k: on[k] for k in ("sims", "evals", "eval_cache_hits", "eval_cache_probes")}, "off evals:", off["evals"])
    assert off["eval_cache_hits"] == 0 and off["eval_cache_probes"] == 0
    assert on["eval_cache_probes"] == on["evals"] + on["eval_cache_hits"] == off["evals"]
    assert on["sims"] == off["sims"]
    return on


@pytest.mark.parametrize("log2", [None, 10, 11], ids=["default", "2^10", "2^11"])
def test_persistent_same_records(monkeypatch, log2):
    on = _persistent_on_off(monkeypatch, pk._weights(0), slots=128, sims=200, n_games=256, log2=log2)
    assert on["eval_cache_hits"] > 0


@pytest.mark.parametrize("log2", [None, 10, 11], ids=["default", "2^10", "2^11"])
def test_rounds_same_records(monkeypatch, log2):
    on, _ = rd._on_off(monkeypatch, rd._weights(16, 2), slots=256, sims=32, n_games=384, log2=log2, **ROUNDS)
    assert on["eval_cache_hits"] > 0


def test_rounds_two_streams_tiny_table(monkeypatch):
    """two slot-range views on two streams fight over 512 buckets"""
    on, _ = rd._on_off(monkeypatch, rd._weights(16, 2), slots=512, sims=32, n_games=768, log2=10, **ROUNDS)
    assert on["eval_cache_hits"] > 0


def test_persistent_no_stale_entries_tiny_table(monkeypatch):
    # entries made with weights A must not answer for weights B, in either way of a bucket
    fa, fb = pk._weights(0), pk._weights(1)
    eng = pk._engine(monkeypatch, True, 128, 200, 256, log2=10)
    try:
        first = pk._play(eng, fa, 256)
        after = pk._play(eng, fb, 256)
    finally:
        eng.close()
    assert first[3]["eval_cache_hits"] > 0
    fresh = pk._engine(monkeypatch, False, 128, 200, 256)
    try:
        ref = pk._play(fresh, fb, 256)
    finally:
        fresh.close()
    pk._same(after, ref)


def test_rounds_no_stale_entries_tiny_table(monkeypatch):
    fa, fb = rd._weights(16, 2, seed=0), rd._weights(16, 2, seed=1)
    eng = rd._engine(monkeypatch, True, 256, 32, 384, log2=10, **ROUNDS)
    try:
        first = rd._play(eng, fa, 384)
        after = rd._play(eng, fb, 384)
    finally:
        eng.close()
    assert first[3]["eval_cache_hits"] > 0
    fresh = rd._engine(monkeypatch, False, 256, 32, 384, **ROUNDS)
    try:
        ref = rd._play(fresh, fb, 384)
    finally:
        fresh.close()
    rd._same(after, ref)
