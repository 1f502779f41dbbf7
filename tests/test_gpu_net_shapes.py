"""-m gpu: the network over value-head width D (1 .. 64) and block count R, not only D = 16 and R <= 4.

bb_load_weights takes any D in 1 .. 64 and any R >= 0.  Every network path ends in head_one (net.hip.h), which puts dense unit d
on lane d behind `lane < D` and folds dense_2 over row 0 of the wave at D <= 16 and over the whole wave above; and
selfplay_structure (host_selfplay.hip.h) leaves the persistent kernels when the network does not fit their LDS copy: R > 4 or more
than 192 packed head parameters for Connect4 / TicTacToe (D >= 33), R > 8 or more than 12288 for DragonChess (D >= 41).
Here:
  * bb_net_eval against the oracle (1e-5, the bounds of test_gpu_gnet._check) over D and R, in every form of the network;
  * every dense unit reaches the value;
  * which structure plays at the exact-fit and first-fallback shapes, and that it plays the games of the lock-step launches
    (and, for three shapes, of the oracle's search);
  * a live engine that is given weights of another shape, and back;
  * the shapes bb_load_weights refuses.
tests/test_oracle_net.py holds the oracle itself against PyTorch at these widths."""
import ctypes

import numpy as np
import pytest

from blackbird_amd import _lib, weights as W
from tests.net_cases import eval_forms as _eval_forms, oracle_forward as _oracle, positions as _positions, within as _within
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu
ALPHA, EPS = 0.2, 0.3
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
OG = {C4: 0, TTT: 1}
GAME_IDS = {C4: "c4", TTT: "ttt", DC: "dc"}
N_POS = 7  # positions per bb_net_eval call (and 1: the first of them alone)


def _weights(game, R, D, F=16, seed=21):
    gi = _lib.game_info(game)
    return W.init_weights(gi.C, F, R, D, gi.A, seed=seed, perturb=True)


SHAPES = [(2, 1), (2, 15), (2, 16), (2, 17), (2, 32), (2, 33), (2, 64), (0, 16), (5, 16), (9, 16)]  # (R, D)


@pytest.mark.parametrize("game", [C4, TTT], ids=["c4", "ttt"])
@pytest.mark.parametrize("R,D", SHAPES, ids=[f"R{r}-D{d}" for r, d in SHAPES])
def test_net_eval_over_dense_width_and_blocks(orc, game, R, D):
    """The 16-filter network in its split-operand form, its float32-MFMA form and through the launch-per-layer kernels (in both
    of their forms), against the oracle.  The float32-MFMA tower and the launch-per-layer float32 kernels are the same fmaf
    chains and end in the same head_one: identical bits at every D."""
    st = _positions(game, N_POS, seed=100 * R + D)
    forms = [("split", {}, 2), ("f32", dict(net_form=_lib.NET_FORM_F32), 0),
             ("general f32", dict(general_net=True, net_form=_lib.NET_FORM_F32), 1),
             ("general split", dict(general_net=True), 3 if R else 1)]
    outs = _eval_forms(orc, game, W.flatten(_weights(game, R, D)), forms, st)
    for a, b in zip(outs["f32"], outs["general f32"]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("game", [C4, TTT], ids=["c4", "ttt"])
@pytest.mark.parametrize("R,D", SHAPES, ids=[f"R{r}-D{d}" for r, d in SHAPES])
def test_net_eval_32_filters_over_dense_width_and_blocks(orc, game, R, D):
    """the same widths and depths behind a 32-filter tower (k_gnet_heads -> head_one)"""
    st = _positions(game, N_POS, seed=100 * R + D)
    _eval_forms(orc, game, W.flatten(_weights(game, R, D, F=32)), [("32 filters", {}, 3 if R else 1)], st)


DC_SHAPES = [(2, 1), (2, 17), (2, 40), (2, 41), (2, 64), (9, 16)]


@pytest.mark.parametrize("R,D", DC_SHAPES, ids=[f"R{r}-D{d}" for r, d in DC_SHAPES])
def test_net_eval_dragonchess_over_dense_width_and_blocks(orc, R, D):
    """DragonChess (wide policy head; D = 40 is the last width that fits the one-wave-per-game kernel's head copy) in both net
    forms."""
    st = _positions(DC, N_POS, seed=100 * R + D)
    forms = [("split", {}, 2), ("f32", dict(net_form=_lib.NET_FORM_F32), 0)]
    _eval_forms(orc, DC, W.flatten(_weights(DC, R, D, seed=13)), forms, st)


UNITS = [(1, 0), (16, 0), (16, 15), (17, 0), (17, 16), (64, 0), (64, 63)]  # (D, d)


@pytest.mark.parametrize("game", [C4, TTT], ids=["c4", "ttt"])
@pytest.mark.parametrize("D,d", UNITS, ids=[f"D{D}-unit{d}" for D, d in UNITS])
def test_every_dense_unit_contributes(orc, game, D, d):
    """Dense unit d is made live (v_d1_b[d] = 1: its pre-activation is H*W + k[d] * pooled, open on the test positions) and
    dense_2 is scaled down so that tanh stays far from saturation.  Then v_d2_k[d] goes from 0 to 1/64: the oracle's value moves
    by at least 1e-3 on every position (asserted on the oracle: a property of these inputs), and the kernels must follow it
    within 1e-5 at both settings.  A head that drops lane D - 1, or reads lane D, fails here and nowhere else."""
    st = _positions(game, N_POS, seed=D)
    planes = _lib.game_encode(game, st)
    flats, refs = [], []
    for k in (0.0, 1.0 / 64):
        w = _weights(game, 1, D, seed=40 + D)
        w["value/dense_1/bias"][d] = 1.0
        w["value/dense_2/kernel"] *= np.float32(1.0 / 16)
        w["value/dense_2/kernel"][d, 0] = k
        flats.append(W.flatten(w))
        refs.append(_oracle(orc, game, flats[-1], planes))
    move = np.abs(refs[1][0] - refs[0][0])
    print(f"oracle values {refs[0][0]} -> {refs[1][0]}")
    assert move.min() >= 1e-3, "the chosen inputs do not make the unit visible"
    assert max(np.abs(refs[0][0]).max(), np.abs(refs[1][0]).max()) <= 0.9, "tanh is saturated on the chosen inputs"
    for name, kw in (("split", {}), ("f32", dict(net_form=_lib.NET_FORM_F32)),
                     ("general f32", dict(general_net=True, net_form=_lib.NET_FORM_F32))):
        eng = _lib.Engine(game, n_slots=4, sims_per_move=2, evaluator=_lib.EVAL_NET, **kw)
        try:
            for flat, ref in zip(flats, refs):
                eng.load_weights(flat)
                _within(eng.net_eval(states=st), ref, name)
        finally:
            eng.close()


# ---- which structure plays, and that it plays the same games -----------------------------------------------------------------
def _engine(game, n_slots, n_games, sims, seed, first_id, launch=_lib.LAUNCH_AUTO):
    return _lib.Engine(game, n_slots=n_slots, sims_per_move=sims, evaluator=_lib.EVAL_NET, seed=seed, max_games=n_games,
                       first_game_id=first_id, noise_on=True, alpha=ALPHA, epsilon=EPS, launch=launch,
                       max_plies=8 if game == DC else None)


def _play(eng, n_games):
    return SP.play_loaded(eng, None, n_games, 2, mode=None, steps_below=400, overflow_each_step=True)


def _selfplay(game, n_slots, n_games, sims, R, D, seed, first_id, launch=_lib.LAUNCH_AUTO):
    """A run (tests/selfplay_cases.py) with the dense width as a parameter, and its weights (flat) and bb_selfplay_mode (mode)."""
    flat = W.flatten(_weights(game, R, D))
    eng = _engine(game, n_slots, n_games, sims, seed, first_id, launch)
    try:
        eng.load_weights(flat)
        mode = eng.selfplay_mode()
        return dict(_play(eng, n_games), flat=flat, mode=mode)
    finally:
        eng.close()


SIZES = {C4: (19, 24, 16), TTT: (21, 30, 16), DC: (6, 8, 16)}  # slots (ragged: not whole workgroups), games (> slots), simulations a move
STRUCTURES = [(g, R, D, 3) for g in (C4, TTT) for R, D in ((0, 16), (4, 32), (4, 1))] + \
             [(g, R, D, 1) for g in (C4, TTT) for R, D in ((4, 33), (5, 16))] + \
             [(DC, 2, 40, 5), (DC, 8, 16, 5), (DC, 2, 41, 0), (DC, 9, 16, 0)]


@pytest.mark.parametrize("game,R,D,mode", STRUCTURES, ids=[f"{GAME_IDS[g]}-R{r}-D{d}-mode{m}" for g, r, d, m in STRUCTURES])
def test_structure_by_shape_plays_the_lockstep_games(game, R, D, mode):
    """(R, D) = (4, 32) fills the persistent kernel's head copy to the last float for TicTacToe (192 of 192; Connect4: 184), (2, 40)
    leaves DragonChess 8 of 12288: an LDS copy that overran would change a neighbour's operands and with them the games."""
    n_slots, n_games, sims = SIZES[game]
    a = _selfplay(game, n_slots, n_games, sims, R, D, 5, 300)
    assert a["mode"] == mode
    b = _selfplay(game, n_slots, n_games, sims, R, D, 5, 300, launch=_lib.LAUNCH_LOCKSTEP)
    assert b["mode"] == 0
    SP.assert_same_records(a, b, (game, R, D), counters=("sims",), no_overflow=True)


@pytest.mark.parametrize("game,R,D,mode", [(C4, 4, 32, 3), (TTT, 4, 32, 3), (C4, 5, 16, 1)], ids=["c4-exact-fit", "ttt-exact-fit", "c4-fallback"])
def test_structure_by_shape_matches_oracle_search(orc, game, R, D, mode):
    """example by example against the oracle's keyed-callback search, as test_queue_kernel_with_prior_noise_matches_oracle does"""
    gi = _lib.game_info(game)
    og = OG[game]
    n_slots, n_games, sims = SIZES[game]
    max_plies = {C4: 43, TTT: 10}[game]
    seed, first_id = 17, 500
    run = _selfplay(game, n_slots, n_games, sims, R, D, seed, first_id)
    flat, rec, offs, win, cnt, got = (run[k] for k in ("flat", "rec", "offs", "win", "cnt", "mode"))
    assert got == mode
    ev = _lib.Engine(game, n_slots=4, sims_per_move=2, evaluator=_lib.EVAL_NET, seed=seed, alpha=ALPHA, epsilon=EPS)
    ev.load_weights(flat)
    calls = {"with_policy": 0}

    def getpolicy(_ctx, stp, gid, serial, vp, pp):
        planes = orc.encode(og, stp.contents)
        v, _l, p = ev.net_eval_keyed([gid], [serial], planes=planes)
        vp[0] = float(v[0])
        if pp:
            calls["with_policy"] += 1
            for a in range(gi.A):
                pp[a] = float(p[0, a])

    cfg = orc.make_cfg(og, evaluator=orc.EVAL_CALLBACK_KEYED, seed=seed, cb2=orc.EVAL_CB2(getpolicy))
    sims_total = 0
    for gidx in range(n_games):
        o = orc.selfplay_game(cfg, first_id + gidx, 1.0, sims, max_plies - 1)
        r = rec[offs[gidx]:offs[gidx + 1]]
        assert len(r) == o["n"] and win[gidx] == o["winner"], gidx
        assert (r["game_id"] == first_id + gidx).all()
        tot = np.maximum(r["total"].astype(np.float64), 1.0)[:, None]
        assert np.array_equal(r["visits"][:, :gi.A] / tot, o["pi"]), gidx
        assert np.array_equal(r["player"], o["player"]) and np.array_equal(r["z"].astype(np.float32), o["z"])
        sims_total += o["stats"].sims
    ev.close()
    assert cnt["sims"] == sims_total and calls["with_policy"] > 0


@pytest.mark.parametrize("R,D", [(4, 33), (5, 16)], ids=["D33", "R5"])
def test_fallback_rounds_and_the_evaluation_cache(monkeypatch, R, D):
    """A Connect4 engine created for the persistent kernel owns an evaluation cache table; with a network that falls back to
    rounds it plays through the fused 16-filter tower, which leaves the table alone (test_gpu_rounds_eval_cache.py:
    test_fused_16_filter_rounds_do_not_probe).  Same records whatever BB_EVAL_CACHE says, and the counters of that test."""
    n_slots, n_games, sims = SIZES[C4]
    res = {}
    monkeypatch.delenv("BB_EVAL_CACHE_LOG2", raising=False)
    for cache in (True, False):
        if cache:
            monkeypatch.delenv("BB_EVAL_CACHE", raising=False)  # its default
        else:
            monkeypatch.setenv("BB_EVAL_CACHE", "0")
        res[cache] = _selfplay(C4, n_slots, n_games, sims, R, D, 5, 300)
        assert res[cache]["mode"] == 1
    SP.assert_same_records(res[True], res[False], (R, D))
    SP.assert_cache_counters(res[True]["cnt"], res[False]["cnt"], probed=False)


# ---- weights of another shape on a live engine -----------------------------------------------------------------------------------
@pytest.mark.parametrize("game,first,other,modes", [(C4, (4, 16), (5, 33), (3, 1)), (DC, (2, 16), (2, 41), (5, 0))], ids=["c4", "dc"])
def test_reload_another_shape_on_a_live_engine(game, first, other, modes):
    """first shape -> other shape -> first shape on ONE engine: the operand buffers are reallocated, the structure changes between
    two batches and back, and the evaluation cache must not carry anything over.  Every stage equals a fresh engine's."""
    n_slots, n_games, sims = SIZES[game]
    seed, first_id = 9, 40
    fa = W.flatten(_weights(game, *first, seed=3))
    fb = W.flatten(_weights(game, *other, seed=4))
    st = _positions(game, 7, seed=2)
    eng = _engine(game, n_slots, n_games, sims, seed, first_id)
    fresh = _engine(game, n_slots, n_games, sims, seed, first_id)
    try:
        eng.load_weights(fa)
        assert eng.selfplay_mode() == modes[0]
        run_a = _play(eng, n_games)
        eval_a = eng.net_eval(states=st)

        eng.load_weights(fb)
        fresh.load_weights(fb)
        assert eng.selfplay_mode() == modes[1] and fresh.selfplay_mode() == modes[1]
        for x, y in zip(eng.net_eval(states=st), fresh.net_eval(states=st)):
            assert np.array_equal(x, y)
        eng.set_rng_stream(seed, first_id)
        run_b = _play(eng, n_games)
        ref_b = _play(fresh, n_games)
        SP.assert_same_records(run_b, ref_b, "other shape", counters=("sims",))
        assert run_b["rec"].tobytes() != run_a["rec"].tobytes()  # (another network: other games)

        eng.load_weights(fa)
        assert eng.selfplay_mode() == modes[0]
        for x, y in zip(eng.net_eval(states=st), eval_a):
            assert np.array_equal(x, y)
        eng.set_rng_stream(seed, first_id)
        again = _play(eng, n_games)
        SP.assert_same_records(again, run_a, "first shape again", counters=("sims",))
    finally:
        eng.close()
        fresh.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _struct(gi, flat, **shape):
    """bb_net_weights built directly (weights.flatten cannot express F = 24, D = 0 ...): valid arrays, the given shape fields"""
    w = _lib.NetWeights()
    w.H, w.W, w.C, w.A = gi.H, gi.W, gi.C, gi.A
    w.F, w.R, w.D = flat["conv0_k"].shape[3], flat["blk_k"].shape[0], flat["v_d1_k"].shape[0]
    for k, v in shape.items():
        setattr(w, k, v)
    keep = []
    for name, _t in _lib.NetWeights._fields_[7:]:
        keep.append(np.ascontiguousarray(flat[name], dtype=np.float32))
        setattr(w, name, keep[-1].ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    return w, keep


def test_refused_shapes_leave_the_engine_as_it_was():
    gi = _lib.game_info(C4)
    flat = W.flatten(_weights(C4, 4, 16))
    st = _positions(C4, 5)
    eng = _lib.Engine(C4, n_slots=4, sims_per_move=2, evaluator=_lib.EVAL_NET)
    try:
        eng.load_weights(flat)
        before = eng.net_eval(states=st)
        mode = eng.selfplay_mode()
        big = W.flatten(_weights(C4, 4, 64, F=32))  # (arrays large enough for whatever a refused shape names)
        cases = [(s, ()) for s in (dict(F=24), dict(F=0), dict(D=0), dict(D=65), dict(R=-1))]
        cases += [(dict(), ("p_bn",)), (dict(R=4), ("blk_k",))]  # a block the shape needs, not given
        for shape, missing in cases:
            w, keep = _struct(gi, big, **shape)
            for name in missing:
                setattr(w, name, None)
                shape = dict(shape, missing=missing)
            rc = _lib.lib().bb_load_weights(eng.h, ctypes.byref(w))
            assert rc == _lib.ERR_ARG, (shape, rc)
            assert _lib.last_error(), shape
            with pytest.raises(ValueError):
                _lib.check(rc)
            after = eng.net_eval(states=st)
            assert all(np.array_equal(x, y) for x, y in zip(before, after)), shape
            assert eng.selfplay_mode() == mode and eng.net_form() == 2, shape
            del keep
        # without residual blocks there is nothing in blk_*: accepted with all three null, and the network they leave out of
        flat0 = W.flatten(_weights(C4, 0, 16))
        w, keep = _struct(gi, flat0)
        for name in ("blk_k", "blk_b", "blk_bn"):
            setattr(w, name, None)
        assert w.R == 0 and _lib.lib().bb_load_weights(eng.h, ctypes.byref(w)) == _lib.OK, _lib.last_error()
        got = eng.net_eval(states=st)
        eng.load_weights(flat0)
        assert all(np.array_equal(x, y) for x, y in zip(got, eng.net_eval(states=st)))
    finally:
        eng.close()
