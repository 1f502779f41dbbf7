"""The evaluation cache of the asynchronous-round self-play (Connect4; eval_probe.hip.h) changes no result.

Every network that does not fit the persistent kernel -- any wide one, a 16-filter one with too many blocks or under
LAUNCH_ROUNDS -- plays as rounds: the tree kernel posts the leaves that need the network, the network launches evaluate
them.  With the cache, and a network of the launch-per-layer kind (general_net), a probe kernel answers the posted leaves
whose position was evaluated before (value and priors from the table, the node's own prior noise drawn anew) and hands
only the rest to the network, whose heads store them.
A batch played with the cache must therefore store the very same bytes as one played without it, and

    eval_cache_probes == evals + eval_cache_hits == the evals of the run without the cache

(`evals` counts tower runs).  BB_EVAL_CACHE is read when an engine is created: one process compares both settings."""
import pytest

from blackbird_amd import _lib
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu

C4 = _lib.GAME_CONNECT4


def _play(eng, flat, n_games, plies_per_step=4):
    """as rounds"""
    return SP.play_loaded(eng, flat, n_games, plies_per_step, mode=1, steps_below=4096)


def _on_off(monkeypatch, flat, slots, sims, n_games, log2=None, probed=True, **kw):
    res = {}
    for cache in (True, False):
        eng = SP.c4_engine_under_cache(monkeypatch, cache, slots, sims, n_games, log2=log2, **kw)
        try:
            res[cache] = _play(eng, flat, n_games)
        finally:
            eng.close()
    SP.assert_same_records(res[True], res[False], "cache on and off")
    on, off = res[True]["cnt"], res[False]["cnt"]
    SP.assert_cache_counters(on, off, probed)
    return on, off


def test_same_records_wide_network(monkeypatch):
    """32 filters x 2 blocks (launch-per-layer kernels, tower layers in the split-operand form).  More games than slots: a
    refilled slot's first leaf is the initial position, which round 0 stored and a 2^26-entry table does not evict in a
    run this small -- so there are hits, whatever else repeats."""
    on, _ = _on_off(monkeypatch, SP.c4_weights(32, 2), slots=256, sims=32, n_games=384)
    assert on["eval_cache_hits"] > 0


@pytest.mark.parametrize("filters,kw", [
    (32, dict(net_form=_lib.NET_FORM_F32)),                              # k_gnet_conv layers
    (16, dict(net_form=_lib.NET_FORM_F32, general_net=True)),            # the same, 16 filters
    (16, dict(general_net=True)),                                        # k_gnet_conv_x3 layers, 16 filters
], ids=["wide-f32", "general16-f32", "general16-split"])
def test_same_records_both_net_forms(monkeypatch, filters, kw):
    """both net forms of the launch-per-layer path, at 32 and at 16 filters"""
    on, _ = _on_off(monkeypatch, SP.c4_weights(filters, 2), slots=256, sims=32, n_games=384, **kw)
    assert on["eval_cache_hits"] > 0


@pytest.mark.parametrize("net_form", [_lib.NET_FORM_AUTO, _lib.NET_FORM_F32], ids=["k_net_x3", "k_net_compact"])
def test_fused_16_filter_rounds_do_not_probe(monkeypatch, net_form):
    """The 16-filter network that falls through to rounds (LAUNCH_ROUNDS), in both of its forms: the cache stays out of it.
    Measured on one MI355X, 4096 games at 800 simulations per move (tools/bench_cache.py --launch-rounds --workload c2
    --steps 4 --warmup 1 --settle 4, three alternations): with the probe 75.8 ms per step against 60.5 ms without it, at
    36 % hits -- the fused tower of a 1.6-MFLOP network over two thirds of the leaves is hardly shorter, and the probe is
    one more launch in each of 800 rounds.  So the probe is kept for the launch-per-layer networks only; this case must
    still give the same records whatever BB_EVAL_CACHE says, and count no probes."""
    _on_off(monkeypatch, SP.c4_weights(16, 2), slots=256, sims=32, n_games=384, probed=False, launch=_lib.LAUNCH_ROUNDS,
            net_form=net_form)


@pytest.mark.parametrize("filters,kw", [(32, {}), (16, dict(general_net=True))], ids=["wide", "general16"])
def test_two_streams(monkeypatch, filters, kw):
    """>= 512 slots under LAUNCH_ROUNDS: two slot-range views on two streams probe and fill one table.  Which of two
    racing views finds the other's entry differs from run to run; records and the counter identity do not."""
    on, _ = _on_off(monkeypatch, SP.c4_weights(filters, 2), slots=512, sims=32, n_games=768, launch=_lib.LAUNCH_ROUNDS, **kw)
    assert on["eval_cache_probes"] > 0


def test_small_table(monkeypatch):
    # a table of 1024 entries: most probes land on an entry of another position (a miss), results unchanged
    _on_off(monkeypatch, SP.c4_weights(32, 2), slots=256, sims=32, n_games=384, log2=10)


def test_no_stale_entries(monkeypatch):
    # entries made with weights A must not answer for weights B
    fa, fb = SP.c4_weights(32, 2, seed=0), SP.c4_weights(32, 2, seed=1)
    eng = SP.c4_engine_under_cache(monkeypatch, True, 256, 32, 384)
    try:
        first = _play(eng, fa, 384)
        after = _play(eng, fb, 384)
    finally:
        eng.close()
    assert first["cnt"]["eval_cache_hits"] > 0
    fresh = SP.c4_engine_under_cache(monkeypatch, True, 256, 32, 384)
    try:
        ref = _play(fresh, fb, 384)
    finally:
        fresh.close()
    SP.assert_same_records(after, ref, "after a reload")


@pytest.mark.parametrize("filters,kw", [(32, {}), (16, dict(general_net=True))], ids=["wide", "general16"])
def test_schedule_independence_with_cache(monkeypatch, filters, kw):
    """The same games on one slot per game and on a quarter of the slots: a hit gives the bits the tower would have,
    whatever batch shape computed the stored entry."""
    flat = SP.c4_weights(filters, 2)
    res = []
    for slots in (256, 64):
        eng = SP.c4_engine_under_cache(monkeypatch, True, slots, 32, 256, **kw)
        try:
            res.append(_play(eng, flat, 256))
        finally:
            eng.close()
    SP.assert_same_records(res[0], res[1], "256 and 64 slots")
    assert res[0]["cnt"]["eval_cache_hits"] > 0 and res[1]["cnt"]["eval_cache_hits"] > 0


def test_full_size(monkeypatch):
    """BASELINE configs[4] (20 blocks x 256 filters), 4096 games, 8 simulations per move, a ply cap of 3 -- the set-up of
    test_gpu_fullsize.test_c5_network_full_size_in_search -- with and without the cache."""
    n, sims, cap = 4096, 8, 3
    flat = SP.c4_weights(256, 20)
    res = {}
    for cache in (True, False):
        SP.cache_env(monkeypatch, cache, None)
        eng = _lib.Engine(C4, n_slots=n, sims_per_move=sims, evaluator=_lib.EVAL_NET, seed=31, noise_on=True, alpha=0.2,
                          epsilon=0.3, max_games=n, max_plies=cap)
        try:
            eng.load_weights(flat)
            assert eng.net_form() == 3
            res[cache] = _play(eng, flat, n, plies_per_step=1)
        finally:
            eng.close()
    SP.assert_same_records(res[True], res[False], "full size")
    on, off = res[True]["cnt"], res[False]["cnt"]
    print("on:", on, "off:", off)
    assert on["games_finished"] == n and len(res[True]["rec"]) == n * (cap + 1)
    SP.assert_cache_counters(on, off)
    assert on["eval_cache_hits"] > 0
