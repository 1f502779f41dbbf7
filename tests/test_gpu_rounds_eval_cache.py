"""The evaluation cache of the asynchronous-round self-play (Connect4; eval_probe.hip.h) changes no result.

Every network that does not fit the persistent kernel -- any wide one, a 16-filter one with too many blocks or under
LAUNCH_ROUNDS -- plays as rounds: the tree kernel posts the leaves that need the network, the network launches evaluate
them.  With the cache, and a network of the launch-per-layer kind (general_net), a probe kernel answers the posted leaves
whose position was evaluated before (value and priors from the table, the node's own prior noise drawn anew) and hands
only the rest to the network, whose heads store them.
A batch played with the cache must therefore store the very same bytes as one played without it, and

    eval_cache_probes == evals + eval_cache_hits == the evals of the run without the cache

(`evals` counts tower runs).  BB_EVAL_CACHE is read when an engine is created: one process compares both settings."""
import numpy as np
import pytest

from blackbird_amd import _lib, weights as W

pytestmark = pytest.mark.gpu

C4 = _lib.GAME_CONNECT4


def _weights(filters, blocks, seed=0):
    return W.flatten(W.init_weights(3, filters, blocks, 16, 7, seed=seed))


def _engine(monkeypatch, cache, slots, sims, max_games, log2=None, **kw):
    monkeypatch.setenv("BB_EVAL_CACHE", "1" if cache else "0")
    if log2 is not None:
        monkeypatch.setenv("BB_EVAL_CACHE_LOG2", str(log2))
    else:
        monkeypatch.delenv("BB_EVAL_CACHE_LOG2", raising=False)
    return _lib.Engine(C4, n_slots=slots, sims_per_move=sims, evaluator=_lib.EVAL_NET, c_puct=0.85, seed=1234,
                       noise_on=True, alpha=0.2, epsilon=0.3, max_games=max_games, **kw)


def _play(eng, flat, n_games, plies_per_step=4):
    """load `flat`, play n_games to the end as rounds; (records, offsets, winners, counters)"""
    eng.load_weights(flat)
    assert eng.selfplay_mode() == 1
    eng.reset_counters()
    eng.selfplay_begin(n_games, 1.0)
    guard = 0
    while not eng.selfplay_done()[0]:
        eng.selfplay_step(plies_per_step)
        guard += 1
        assert guard < 4096
    rec, offs, win = eng.fetch_examples()
    cnt = eng.counters()
    assert cnt["overflow"] == 0
    return rec, offs, win, cnt


def _same(a, b):
    ra, oa, wa = a[:3]
    rb, ob, wb = b[:3]
    assert np.array_equal(oa, ob) and np.array_equal(wa, wb)
    assert ra.tobytes() == rb.tobytes()


def _on_off(monkeypatch, flat, slots, sims, n_games, log2=None, probed=True, **kw):
    res = {}
    for cache in (True, False):
        eng = _engine(monkeypatch, cache, slots, sims, n_games, log2=log2, **kw)
        try:
            res[cache] = _play(eng, flat, n_games)
        finally:
            eng.close()
    _same(res[True], res[False])
    on, off = res[True][3], res[False][3]
    print("on:", {k: on[k] for k in ("sims", "evals", "eval_cache_hits", "eval_cache_probes")},
          "off:", {k: off[k] for k in ("sims", "evals", "eval_cache_hits", "eval_cache_probes")})
    assert off["eval_cache_hits"] == 0 and off["eval_cache_probes"] == 0
    if probed:
        assert on["eval_cache_probes"] == on["evals"] + on["eval_cache_hits"]
    else:
        assert on["eval_cache_hits"] == 0 and on["eval_cache_probes"] == 0
    assert on["evals"] + on["eval_cache_hits"] == off["evals"]
    assert on["sims"] == off["sims"]
    return on, off


def test_same_records_wide_network(monkeypatch):
    """32 filters x 2 blocks (launch-per-layer kernels, tower layers in the split-operand form).  More games than slots: a
    refilled slot's first leaf is the initial position, which round 0 stored and a 2^26-entry table does not evict in a
    run this small -- so there are hits, whatever else repeats."""
    on, _ = _on_off(monkeypatch, _weights(32, 2), slots=256, sims=32, n_games=384)
    assert on["eval_cache_hits"] > 0


@pytest.mark.parametrize("filters,kw", [
    (32, dict(net_form=_lib.NET_FORM_F32)),                              # k_gnet_conv layers
    (16, dict(net_form=_lib.NET_FORM_F32, general_net=True)),            # the same, 16 filters
    (16, dict(general_net=True)),                                        # k_gnet_conv_x3 layers, 16 filters
], ids=["wide-f32", "general16-f32", "general16-split"])
def test_same_records_both_net_forms(monkeypatch, filters, kw):
    """both net forms of the launch-per-layer path, at 32 and at 16 filters"""
    on, _ = _on_off(monkeypatch, _weights(filters, 2), slots=256, sims=32, n_games=384, **kw)
    assert on["eval_cache_hits"] > 0


@pytest.mark.parametrize("net_form", [_lib.NET_FORM_AUTO, _lib.NET_FORM_F32], ids=["k_net_x3", "k_net_compact"])
def test_fused_16_filter_rounds_do_not_probe(monkeypatch, net_form):
    """The 16-filter network that falls through to rounds (LAUNCH_ROUNDS), in both of its forms: the cache stays out of it.
    Measured on one MI355X, 4096 games at 800 simulations per move (tools/bench_cache.py --launch-rounds --workload c2
    --steps 4 --warmup 1 --settle 4, three alternations): with the probe 75.8 ms per step against 60.5 ms without it, at
    36 % hits -- the fused tower of a 1.6-MFLOP network over two thirds of the leaves is hardly shorter, and the probe is
    one more launch in each of 800 rounds.  So the probe is kept for the launch-per-layer networks only; this case must
    still give the same records whatever BB_EVAL_CACHE says, and count no probes."""
    _on_off(monkeypatch, _weights(16, 2), slots=256, sims=32, n_games=384, probed=False, launch=_lib.LAUNCH_ROUNDS,
            net_form=net_form)


@pytest.mark.parametrize("filters,kw", [(32, {}), (16, dict(general_net=True))], ids=["wide", "general16"])
def test_two_streams(monkeypatch, filters, kw):
    """>= 512 slots under LAUNCH_ROUNDS: two slot-range views on two streams probe and fill one table.  Which of two
    racing views finds the other's entry differs from run to run; records and the counter identity do not."""
    on, _ = _on_off(monkeypatch, _weights(filters, 2), slots=512, sims=32, n_games=768, launch=_lib.LAUNCH_ROUNDS, **kw)
    assert on["eval_cache_probes"] > 0


def test_small_table(monkeypatch):
    # a table of 1024 entries: most probes land on an entry of another position (a miss), results unchanged
    _on_off(monkeypatch, _weights(32, 2), slots=256, sims=32, n_games=384, log2=10)


def test_no_stale_entries(monkeypatch):
    # entries made with weights A must not answer for weights B
    fa, fb = _weights(32, 2, seed=0), _weights(32, 2, seed=1)
    eng = _engine(monkeypatch, True, 256, 32, 384)
    try:
        first = _play(eng, fa, 384)
        after = _play(eng, fb, 384)
    finally:
        eng.close()
    assert first[3]["eval_cache_hits"] > 0
    fresh = _engine(monkeypatch, True, 256, 32, 384)
    try:
        ref = _play(fresh, fb, 384)
    finally:
        fresh.close()
    _same(after, ref)


@pytest.mark.parametrize("filters,kw", [(32, {}), (16, dict(general_net=True))], ids=["wide", "general16"])
def test_schedule_independence_with_cache(monkeypatch, filters, kw):
    """The same games on one slot per game and on a quarter of the slots: a hit gives the bits the tower would have,
    whatever batch shape computed the stored entry."""
    flat = _weights(filters, 2)
    res = []
    for slots in (256, 64):
        eng = _engine(monkeypatch, True, slots, 32, 256, **kw)
        try:
            res.append(_play(eng, flat, 256))
        finally:
            eng.close()
    _same(res[0], res[1])
    assert res[0][3]["eval_cache_hits"] > 0 and res[1][3]["eval_cache_hits"] > 0


def test_full_size(monkeypatch):
    """BASELINE configs[4] (20 blocks x 256 filters), 4096 games, 8 simulations per move, a ply cap of 3 -- the set-up of
    test_gpu_fullsize.test_c5_network_full_size_in_search -- with and without the cache."""
    n, sims, cap = 4096, 8, 3
    flat = _weights(256, 20)
    res = {}
    for cache in (True, False):
        monkeypatch.setenv("BB_EVAL_CACHE", "1" if cache else "0")
        monkeypatch.delenv("BB_EVAL_CACHE_LOG2", raising=False)
        eng = _lib.Engine(C4, n_slots=n, sims_per_move=sims, evaluator=_lib.EVAL_NET, seed=31, noise_on=True, alpha=0.2,
                          epsilon=0.3, max_games=n, max_plies=cap)
        try:
            eng.load_weights(flat)
            assert eng.net_form() == 3
            res[cache] = _play(eng, flat, n, plies_per_step=1)
        finally:
            eng.close()
    _same(res[True], res[False])
    on, off = res[True][3], res[False][3]
    print("on:", on, "off:", off)
    assert on["games_finished"] == n and len(res[True][0]) == n * (cap + 1)
    assert off["eval_cache_hits"] == 0 and off["eval_cache_probes"] == 0
    assert on["eval_cache_hits"] > 0
    assert on["eval_cache_probes"] == on["evals"] + on["eval_cache_hits"] == off["evals"]
    assert on["sims"] == off["sims"]
