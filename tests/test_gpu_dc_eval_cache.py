"""The evaluation cache of DragonChess self-play (mega_dc.hip.h, net.hip.h DragonChess entries) changes no result.

A hit replaces the network by the WideHead {value, R0, R1, m, 1/sum} stored when the same position was evaluated (the prior
noise is mixed in at the expansion, per node, either way), so a batch played with the cache must store the very same bytes as
one played without it, on both forms of the network.  BB_EVAL_CACHE is read when an engine is created: one process compares
both settings.  Ragged slot count (a workgroup holds four games) and slot reuse (more games than slots) throughout."""
import pytest

from blackbird_amd import _lib, weights as W
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu

DC = _lib.GAME_DRAGONCHESS
SLOTS, GAMES, SIMS, PLIES = 37, 50, 48, 40


def _weights(seed):
    return W.flatten(W.init_weights(17, 16, 4, 16, 4032, seed=seed))


def _engine(monkeypatch, cache, noise=True, log2=None, net_form=_lib.NET_FORM_AUTO, launch=_lib.LAUNCH_AUTO):
    return SP.net_engine_under_cache(monkeypatch, DC, cache, log2, n_slots=SLOTS, sims_per_move=SIMS, noise_on=noise,
                                     max_games=GAMES, max_plies=PLIES, net_form=net_form, launch=launch)


def _play(eng, flat, mode=5):
    return SP.play_loaded(eng, flat, GAMES, 8, mode=mode, steps_below=100)


def _run(monkeypatch, flat, cache, **kw):
    mode = 0 if kw.get("launch") == _lib.LAUNCH_LOCKSTEP else 5
    eng = _engine(monkeypatch, cache, **kw)
    try:
        return _play(eng, flat, mode)
    finally:
        eng.close()


@pytest.mark.parametrize("net_form", [_lib.NET_FORM_AUTO, _lib.NET_FORM_F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "no_noise"])
def test_same_records(monkeypatch, noise, net_form):
    flat = _weights(0)
    on = _run(monkeypatch, flat, True, noise=noise, net_form=net_form)
    off = _run(monkeypatch, flat, False, noise=noise, net_form=net_form)
    SP.assert_same_records(on, off)
    con, coff = on["cnt"], off["cnt"]
    SP.assert_cache_counters(con, coff)     # every network evaluation is probed; a hit is one tower run less
    assert con["eval_cache_hits"] > 0


def test_small_table(monkeypatch):
    # a table of 1024 entries: most probes land on an entry of another position (a miss), results unchanged
    flat = _weights(0)
    on = _run(monkeypatch, flat, True, log2=10)
    off = _run(monkeypatch, flat, False)
    SP.assert_same_records(on, off)
    assert on["cnt"]["eval_cache_probes"] == on["cnt"]["evals"] + on["cnt"]["eval_cache_hits"] == off["cnt"]["evals"]


def test_no_stale_entries(monkeypatch):
    # entries made with weights A must not answer for weights B
    fa, fb = _weights(0), _weights(1)
    eng = _engine(monkeypatch, True)
    try:
        _play(eng, fa)
        after = _play(eng, fb)
    finally:
        eng.close()
    SP.assert_same_records(after, _run(monkeypatch, fb, True))
    SP.assert_same_records(after, _run(monkeypatch, fb, False))


def test_lockstep_same(monkeypatch):
    # the launch-per-simulation structure (no cache) plays the same games as the cached one-wave-per-game kernel
    flat = _weights(0)
    SP.assert_same_records(_run(monkeypatch, flat, True), _run(monkeypatch, flat, True, launch=_lib.LAUNCH_LOCKSTEP))
