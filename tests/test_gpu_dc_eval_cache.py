"""The evaluation cache of DragonChess self-play (mega_dc.hip.h, net.hip.h DragonChess entries) changes no result.

A hit replaces the network by the WideHead {value, R0, R1, m, 1/sum} stored when the same position was evaluated (the prior
noise is mixed in at the expansion, per node, either way), so a batch played with the cache must store the very same bytes as
one played without it, on both forms of the network.  BB_EVAL_CACHE is read when an engine is created: one process compares
both settings.  Ragged slot count (a workgroup holds four games) and slot reuse (more games than slots) throughout."""
import numpy as np
import pytest

from blackbird_amd import _lib, weights as W

pytestmark = pytest.mark.gpu

DC = _lib.GAME_DRAGONCHESS
SLOTS, GAMES, SIMS, PLIES = 37, 50, 48, 40


def _weights(seed):
    return W.flatten(W.init_weights(17, 16, 4, 16, 4032, seed=seed))


def _engine(monkeypatch, cache, noise=True, log2=None, net_form=_lib.NET_FORM_AUTO, launch=_lib.LAUNCH_AUTO):
    monkeypatch.setenv("BB_EVAL_CACHE", "1" if cache else "0")
    if log2 is not None:
        monkeypatch.setenv("BB_EVAL_CACHE_LOG2", str(log2))
    else:
        monkeypatch.delenv("BB_EVAL_CACHE_LOG2", raising=False)
    return _lib.Engine(DC, n_slots=SLOTS, sims_per_move=SIMS, evaluator=_lib.EVAL_NET, c_puct=0.85, seed=1234,
                       noise_on=noise, alpha=0.2, epsilon=0.3, max_games=GAMES, max_plies=PLIES, net_form=net_form,
                       launch=launch)


def _play(eng, flat, mode=5):
    """load `flat`, play GAMES games to the end; (records, offsets, winners, counters)"""
    eng.load_weights(flat)
    assert eng.selfplay_mode() == mode
    eng.reset_counters()
    eng.selfplay_begin(GAMES, 1.0)
    guard = 0
    while not eng.selfplay_done()[0]:
        eng.selfplay_step(8)
        guard += 1
        assert guard < 100
    rec, offs, win = eng.fetch_examples()
    cnt = eng.counters()
    assert cnt["overflow"] == 0
    return rec, offs, win, cnt


def _run(monkeypatch, flat, cache, **kw):
    mode = 0 if kw.get("launch") == _lib.LAUNCH_LOCKSTEP else 5
    eng = _engine(monkeypatch, cache, **kw)
    try:
        return _play(eng, flat, mode)
    finally:
        eng.close()


def _same(a, b):
    ra, oa, wa, _ = a
    rb, ob, wb, _ = b
    assert np.array_equal(oa, ob) and np.array_equal(wa, wb)
    assert ra.tobytes() == rb.tobytes()


@pytest.mark.parametrize("net_form", [_lib.NET_FORM_AUTO, _lib.NET_FORM_F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "no_noise"])
def test_same_records(monkeypatch, noise, net_form):
    flat = _weights(0)
    on = _run(monkeypatch, flat, True, noise=noise, net_form=net_form)
    off = _run(monkeypatch, flat, False, noise=noise, net_form=net_form)
    _same(on, off)
    con, coff = on[3], off[3]
    assert coff["eval_cache_hits"] == 0 and coff["eval_cache_probes"] == 0
    assert con["eval_cache_hits"] > 0
    # every network evaluation is probed; a hit is one tower run less
    assert con["eval_cache_probes"] == coff["evals"]
    assert con["eval_cache_probes"] == con["evals"] + con["eval_cache_hits"]
    assert con["sims"] == coff["sims"]


def test_small_table(monkeypatch):
    # a table of 1024 entries: most probes land on an entry of another position (a miss), results unchanged
    flat = _weights(0)
    on = _run(monkeypatch, flat, True, log2=10)
    off = _run(monkeypatch, flat, False)
    _same(on, off)
    assert on[3]["eval_cache_probes"] == on[3]["evals"] + on[3]["eval_cache_hits"] == off[3]["evals"]


def test_no_stale_entries(monkeypatch):
    # entries made with weights A must not answer for weights B
    fa, fb = _weights(0), _weights(1)
    eng = _engine(monkeypatch, True)
    try:
        _play(eng, fa)
        after = _play(eng, fb)
    finally:
        eng.close()
    _same(after, _run(monkeypatch, fb, True))
    _same(after, _run(monkeypatch, fb, False))


def test_lockstep_same(monkeypatch):
    # the launch-per-simulation structure (no cache) plays the same games as the cached one-wave-per-game kernel
    flat = _weights(0)
    _same(_run(monkeypatch, flat, True), _run(monkeypatch, flat, True, launch=_lib.LAUNCH_LOCKSTEP))
