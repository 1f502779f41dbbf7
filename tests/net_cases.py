"""What the -m gpu network tests share (not collected): random positions of every game, bb_net_eval against the oracle in several
forms of the network, and self-play with a network against the oracle's tree."""
import numpy as np

from blackbird_amd import _lib, weights as W
from tests import selfplay_cases as SP

TOL = 1e-5


def boards_for(game, rng, n):
    H, Wd, _ = _lib.GRID[game]
    cells = rng.randint(0, 3, size=(n, H, Wd))
    b = np.zeros((n, H, Wd, 2), dtype=np.int8)
    b[..., 0] = cells == 1
    b[..., 1] = cells == 2
    pl = rng.randint(1, 3, n)
    return b, pl


def dragonchess_positions(rng, n):
    """n packed DragonChess states: about a third of the squares hold a random piece, then player, previous player and castling
    flags (not reachable positions: inputs for the network)."""
    boards = np.zeros((n, 8, 8), dtype=np.int8)
    for i in range(n):
        m = rng.rand(8, 8) < 0.35
        boards[i][m] = rng.choice([-6, -5, -4, -3, -2, -1, 1, 2], m.sum())
    return _lib.pack_dc(boards, rng.randint(1, 3, n), rng.randint(0, 3, n), rng.randint(0, 2, (n, 4)))


def positions(game, n, seed=5):
    """n packed random positions of any game"""
    rng = np.random.RandomState(seed)
    if game == _lib.GAME_DRAGONCHESS:
        return dragonchess_positions(rng, n)
    b, pl = boards_for(game, rng, n)
    return _lib.pack_grid(game, b, pl)


def oracle_forward(orc, game, flat, planes):
    gi = _lib.game_info(game)
    F, R, D = flat["conv0_k"].shape[3], flat["blk_k"].shape[0], flat["v_d1_k"].shape[0]
    return orc.net_forward(orc.NetWeights(gi.H, gi.W, gi.C, F, R, D, gi.A, flat), planes)


def errors(got, ref):
    """(value, logits, policy) errors in the project's metric: absolute, logits relative to max(1, |logit|)"""
    (v, l, p), (ov, ol, op) = got, ref
    return (float(np.max(np.abs(v - ov))), float(np.max(np.abs(l - ol) / np.maximum(1.0, np.abs(ol)))),
            float(np.max(np.abs(p - op))))


def within(got, ref, what):
    ev, el, ep = errors(got, ref)
    print(f"{what}: value {ev:.2e} logits {el:.2e} policy {ep:.2e}")
    assert ev <= TOL and el <= TOL and ep <= TOL, what


def eval_forms(orc, game, flat, forms, st):
    """bb_net_eval of st and of st[:1] on one engine per form, each against the oracle (computed once); {name: outputs}"""
    planes = _lib.game_encode(game, st)
    ref = oracle_forward(orc, game, flat, planes)
    outs = {}
    for name, kw, net_form in forms:
        eng = _lib.Engine(game, n_slots=4, sims_per_move=2, evaluator=_lib.EVAL_NET, max_plies=8, **kw)
        try:
            eng.load_weights(flat)
            assert eng.net_form() == net_form, name
            outs[name] = eng.net_eval(states=st)
            one = eng.net_eval(states=st[:1])
        finally:
            eng.close()
        within(outs[name], ref, name)
        within(one, tuple(a[:1] for a in ref), name + ", n = 1")
        assert all(np.array_equal(a, b[:1]) for a, b in zip(one, outs[name])), name  # (a position alone: the same bits)
    return outs


def selfplay_vs_oracle_tree(orc, filters, blocks, game=_lib.GAME_CONNECT4, og=0, n_slots=8, n_games=6, sims=40, max_plies=43):
    gi = _lib.game_info(game)
    w = W.init_weights(gi.C, filters, blocks, 16, gi.A, seed=21)
    flat = W.flatten(w)
    eng = _lib.Engine(game, n_slots=n_slots, sims_per_move=sims, evaluator=_lib.EVAL_NET, seed=17, max_games=n_games)
    eng.load_weights(flat)
    out = SP.play_to_end(eng, n_games, 2, 1.0)
    rec, offs, win = out["rec"], out["offs"], out["win"]
    ev = _lib.Engine(game, n_slots=4, sims_per_move=2, evaluator=_lib.EVAL_NET)
    ev.load_weights(flat)

    def cb(_ctx, stp, vp, pp):
        planes = orc.encode(og, stp.contents)
        v, _l, p = ev.net_eval(planes=planes)
        vp[0] = float(v[0])
        if pp:
            for a in range(gi.A):
                pp[a] = float(p[0, a])

    cfg = orc.make_cfg(og, evaluator=orc.EVAL_CALLBACK, seed=17, cb=orc.EVAL_CB(cb))
    for gidx in range(n_games):
        o = orc.selfplay_game(cfg, gidx, 1.0, sims, max_plies - 1)
        r = rec[offs[gidx]:offs[gidx + 1]]
        assert len(r) == o["n"] and win[gidx] == o["winner"], gidx
        tot = np.maximum(r["total"].astype(np.float64), 1.0)[:, None]
        assert np.array_equal(r["visits"][:, :gi.A] / tot, o["pi"]), gidx
    eng.close()
    ev.close()
