"""-m gpu: the DragonChess search on nodes with 65 .. 144 edges -- where dc_expand deals more than one move per lane, the PUCT
loops of dc_phase_select take a second and a third pass of 64, and dc_choose_move / k_dc_sample / k_dc_node_edges /
dc_advance_root walk edge runs longer than a wave -- against the oracle's search of the same positions with the same evaluator
(tests/golden/boards_dc_wide.npz: hand-built positions, tests/make_golden.py 'boards_dc_wide').  Every comparison is exact.

Launch structures: the network cases run lock-step, in one launch (BB_LAUNCH_WAVE, the compact policy head) and in one launch with
the evaluation cache; the rollout case lock-step and in one launch (bb_search_rollouts).  DragonChess has no one-launch kernel for
the hash evaluator or for the float32-MFMA network form, so those cases run lock-step only (Engine.run_sims_structure says so).
The one-launch engines must equal the lock-step one byte for byte, and the lock-step one the oracle.

c_puct: the hash and network cases use 40, not 0.85 -- with priors of ~1/144 per edge and values in [0, 1] a search at 0.85 never
leaves the first edge it visits, and the edges of the later passes would compete but never win.
A position with more than S = 144 legal moves is refused by the tree (last part).  Below the widest roots a queen move
sometimes leaves Black more than 144 moves; the oracle is given the engine's rule (orc_cfg.max_edges = S, DESIGN.md 9: such a node
stays a leaf) and the engine's `overflow` must equal the oracle's count of simulations that ended on one.

C_FIXED: the Fixed case uses c_puct 4: an unvisited edge scores c * sq and a visited one at most 1 + c * sq / 2, so with
c * sq / 2 > 1 (sq >= 1) every unvisited edge beats every visited one and only the exact ties among the unvisited decide --
at 0.85 a visited edge with a high value is legitimately taken again before the last ones are tried."""
import ctypes as C
import functools

import numpy as np
import pytest

from blackbird_amd import DragonChess, _lib
from blackbird_amd import weights as W
from blackbird_amd.DynamicMCTS import DynamicMCTS
from tests import dc_wide_cases as WC
from tests import rollout_cases as RC

pytestmark = pytest.mark.gpu
DC = _lib.GAME_DRAGONCHESS
S = WC.S
LOCK, WAVE = _lib.LAUNCH_LOCKSTEP, _lib.LAUNCH_WAVE
C_WIDE = 40.0
C_FIXED = 4.0
ALPHA, EPS = 0.2, 0.3
ROLLOUT_POSITIONS = ("w65", "w129", "b134_kingcap", "b144")   # (every position's rollouts are decided; four keep the oracle quick)


def test_engine_constants_match():
    assert _lib.game_info(DC).S == S and _lib.game_info(DC).A == 4032


# ---- engines ------------------------------------------------------------------------------------------------------------------
def _engine(n_slots, evaluator, launch=LOCK, fixed=False, c_puct=WC.C_PUCT, **kw):
    kw.setdefault("node_capacity", 4096)   # 24 edges per node row: 98304 edges, room for ~600 nodes of 144
    return _lib.Engine(DC, n_slots=n_slots, sims_per_move=8, mcts_kind=_lib.MCTS_FIXED if fixed else _lib.MCTS_DYNAMIC,
                       max_depth=3 if fixed else 10, evaluator=evaluator, c_puct=c_puct, seed=WC.SEED, hash_salt=WC.SALT,
                       first_game_id=WC.FIRST_GAME_ID, launch=launch, max_plies=8, **kw)


@functools.lru_cache(maxsize=None)
def _weights():
    return W.flatten(W.init_weights(17, 16, 2, 16, 4032, seed=21, perturb=True))


def _net_engine(n_slots, launch=LOCK, **kw):
    eng = _engine(n_slots, _lib.EVAL_NET, launch, c_puct=C_WIDE, alpha=ALPHA, epsilon=EPS, **kw)
    eng.load_weights(_weights())
    return eng


def _net_callback(orc, ev, keyed_noise=None):
    """The oracle's evaluator callback: value and dense 4032-wide policy of bb_net_eval for the state it is asked about.
    keyed_noise = (seed, scale): the keyed callback, the priors of the legal moves mixed with orc_beta_noise of (game id, node
    serial, action) as dc_expand mixes them; scale (1.0: as is) moves every draw for the stability check."""
    def evaluate(stp, vp, pp, gid=None, serial=None):
        v, _l, p = ev.net_eval(planes=orc.encode(orc.DC, stp.contents))
        vp[0] = float(v[0])
        if pp:
            q = p[0].copy()
            if keyed_noise is not None:
                seed, scale = keyed_noise
                for a in np.flatnonzero(orc.legal(orc.DC, stp.contents)):
                    x = np.float32(orc.lib().orc_beta_noise(seed, gid, serial, int(a), ALPHA) * scale)
                    q[a] = np.float32(np.float32(np.float32(1.0) - np.float32(EPS)) * q[a]) + np.float32(np.float32(EPS) * x)
            C.memmove(pp, q.ctypes.data, 4 * 4032)

    if keyed_noise is None:
        return orc.EVAL_CB(lambda _ctx, stp, vp, pp: evaluate(stp, vp, pp))
    return orc.EVAL_CB2(lambda _ctx, stp, gid, serial, vp, pp: evaluate(stp, vp, pp, gid, serial))


# ---- comparisons ----------------------------------------------------------------------------------------------------------------
def _check_slot(out, s, legal, o, where, f64_rates=False):
    """Slot s of bb_sample_moves(temp 0) against the oracle's find_move result o: the compact child lists (actions ascending,
    every legal move, the rest of the row empty), plays, float32 win rates, root statistics, the chosen move."""
    k = len(legal)
    assert np.array_equal(out["child_action"][s, :k], legal) and (out["child_action"][s, k:] == -1).all(), where
    assert (out["child_plays"][s, k:] == 0).all() and (out["child_value"][s, k:] == 0).all(), where
    plays = out["child_plays"][s, :k]
    assert np.array_equal(plays.astype(np.float64), o["plays"][legal]), (where, plays, o["plays"][legal])
    n32 = plays.astype(np.float32)
    if f64_rates:   # the rollout evaluator's win rates are float64 divisions (tests/test_gpu_rollout.py)
        wr = np.where(plays > 0, out["child_value"][s, :k] / np.maximum(plays.astype(np.float64), 1), 0.0)
    else:
        wr = np.where(n32 > 0, out["child_value"][s, :k] / np.maximum(n32, 1), 0).astype(np.float64)
    assert np.array_equal(wr, o["winrates"][legal]), where
    assert o["plays"].sum() == o["plays"][legal].sum()
    assert out["root_plays"][s] == o["root_plays"], where
    assert out["root_winrate"][s] == np.float32(o["winrate"]), where
    assert out["action"][s] == o["action"], where


def _check_counters(cnt, stats, extra_sims=0):
    assert cnt["overflow"] == sum(st.refused for st in stats) + extra_sims   # (nodes wider than S below the root, if any)
    assert cnt["sims"] == sum(st.sims for st in stats) + extra_sims
    assert cnt["sum_depth"] == sum(st.sum_depth for st in stats)
    assert cnt["nodes"] == sum(st.nodes_reached for st in stats)
    assert cnt["terminal_leaves"] == sum(st.terminal_leaves for st in stats)


def _check_sampling(orc, eng, P, runs, which=None):
    """bb_sample_moves at temp 1 and 0.1 with given draws -- 0.0, 0.999999 and two that stop the cumulative sum at an edge
    past index 64 -- against orc.sample_action on the oracle's plays.  Returns how many draws landed past edge 64."""
    which = list(range(len(P))) if which is None else which
    past = 0
    for temp in (1.0, 0.1):
        plays = [runs[j]["o"]["plays"][P.legal[i]] for j, i in enumerate(which)]
        special = [WC.u_for_edges_past(pl, temp) for pl in plays]
        for kind in range(4):
            u = np.zeros(len(which))
            for j in range(len(which)):
                if kind < 2:
                    u[j] = (0.0, 0.999999)[kind]
                else:
                    sp = special[j]
                    u[j] = sp[min(kind - 2, len(sp) - 1)][0] if sp else (0.3, 0.7)[kind - 2]
            out = eng.sample_moves(temp, u)
            for j, i in enumerate(which):
                want = orc.sample_action(runs[j]["o"]["plays"], temp, float(u[j]))
                assert out["action"][j] == want, (P.names[i], temp, kind, u[j])
                if kind >= 2 and special[j]:
                    edge = int(np.flatnonzero(P.legal[i] == want)[0])
                    assert edge == special[j][min(kind - 2, len(special[j]) - 1)][1] and edge >= 64
                    past += 1
    return past


def _snap(eng):
    """What the launch structures must agree on byte for byte: bb_sample_moves at temp 0 and at temp 1 with fixed draws, the
    edges of every root and of every third of its children (bb_node_edges), the tree counters."""
    u = np.linspace(0.05, 0.95, eng.n_slots)
    outs = [eng.sample_moves(0.0), eng.sample_moves(1.0, u)]
    rows = []
    for s in range(eng.n_slots):
        root = eng.node_edges(s, -1)
        rows.append(root)
        rows += [eng.node_edges(s, int(c) & 0x3FFFFFFF) for c in root["child"][:root["n_children"]][::3] if c >= 0]
    cnt = eng.counters()
    return outs, rows, {k: cnt[k] for k in ("sims", "sum_depth", "nodes", "terminal_leaves", "overflow")}


def _same(a, b, what):
    for oa, ob in zip(a[0], b[0]):
        for k in oa:
            assert oa[k].tobytes() == ob[k].tobytes(), (what, k)
    assert len(a[1]) == len(b[1]), what
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), (what, "node", i, k)
    assert a[2] == b[2], (what, a[2], b[2])


def _check_node_edges(eng, s, out, n):
    """bb_node_edges of a root == bb_sample_moves' lists entry for entry; entries n .. S are -1 / CHILD_NONE / 0 / 0."""
    r = eng.node_edges(s, -1)
    assert r["n_children"] == n and r["flags"] & 1
    assert np.array_equal(r["action"], out["child_action"][s]) and np.array_equal(r["plays"], out["child_plays"][s])
    assert np.array_equal(r["value"], out["child_value"][s])
    assert (r["action"][n:] == -1).all() and (r["child"][n:] == -1).all()
    assert (r["plays"][n:] == 0).all() and (r["value"][n:] == 0).all()
    assert ((r["child"][:n] >= 0) == (r["plays"][:n] > 0)).all()   # a child exists once a simulation has taken its edge
    return r


# ---- Dynamic + hash evaluator: priors from the hash policy, normalised over 64 .. 144 legal moves ---------------------------------
def _hash_runs(orc, P):
    cfg = orc.make_cfg(orc.DC, max_edges=S, evaluator=orc.EVAL_HASH, c_puct=C_WIDE, salt=WC.SALT, seed=WC.SEED)
    return WC.oracle_run(orc, "hash", cfg, WC.sims_for(S, "dynamic"), P)


def test_dynamic_hash_vs_oracle(orc):
    P = WC.Positions()
    sims = WC.sims_for(S, "dynamic")
    assert sims >= 2 * P.n_legal.max() and sims <= 300
    runs = _hash_runs(orc, P)
    wide = [i for i in range(len(P)) if P.n_legal[i] > 64]
    for i in wide:   # (the oracle's own trees: edges of every pass were visited, so every pass has held the maximum)
        pl = runs[i]["o"]["plays"][P.legal[i]]
        assert all((pl[k:k + 64] > 0).any() for k in range(0, len(pl), 64)), P.names[i]
    eng = _engine(len(P), _lib.EVAL_HASH, c_puct=C_WIDE)
    assert eng.run_sims_structure() == LOCK
    eng.set_roots(P.packed(_lib), game_ids=P.lids)
    eng.run_sims(sims)
    out = eng.sample_moves(0.0)
    for i in range(len(P)):
        _check_slot(out, i, P.legal[i], runs[i]["o"], P.names[i])
        _check_node_edges(eng, i, out, P.n_legal[i])
    _check_counters(eng.counters(), [r["stats"] for r in runs])
    assert _check_sampling(orc, eng, P, runs) >= 2 * len(wide)
    eng.close()


def test_wide_positions_in_the_first_and_the_last_slot_of_five(orc):
    """Five slots (one workgroup of four waves and one more), the widest positions at both ends."""
    P = WC.Positions()
    which = [P.names.index(n) for n in ("b144", "walk3", "b64", "w65", "w142")]
    runs = [_hash_runs(orc, P)[i] for i in which]
    eng = _engine(5, _lib.EVAL_HASH, c_puct=C_WIDE)
    eng.set_roots(P.packed(_lib, which), game_ids=P.lids[which])
    eng.run_sims(WC.sims_for(S, "dynamic"))
    out = eng.sample_moves(0.0)
    for s, i in enumerate(which):
        _check_slot(out, s, P.legal[i], runs[s]["o"], P.names[i])
    _check_counters(eng.counters(), [r["stats"] for r in runs])
    eng.close()


# ---- Fixed (max depth 3), uniform priors, hash value: every unvisited edge ties exactly ---------------------------------------------
def test_fixed_uniform_priors_visit_edges_in_index_order(orc):
    """RefFixed of make_golden.py.  All unvisited edges of a node tie, so the float64 first-maximum rule -- within a lane's two
    or three edges and across the lanes -- decides every one of the first n_edges simulations: they take the edges in index
    order.  Checked directly after exactly n_edges simulations (one play each), then against the oracle after 10 more."""
    P = WC.Positions()
    sims = np.array([WC.sims_for(n, "fixed") for n in P.n_legal])
    cfg = orc.make_cfg(orc.DC, max_edges=S, kind=orc.FIXED, max_depth=3, evaluator=orc.EVAL_HASH, c_puct=C_FIXED, salt=WC.SALT,
                       seed=WC.SEED, priors_ones=True)
    runs = WC.oracle_run(orc, "fixed", cfg, sims, P)
    eng = _engine(len(P), _lib.EVAL_HASH, fixed=True, c_puct=C_FIXED)
    eng.set_roots(P.packed(_lib), game_ids=P.lids)
    done = np.zeros(len(P), dtype=np.int64)
    for target in sorted(set(P.n_legal.tolist())):      # slot i stops at n_legal[i] simulations: masked calls, narrowest first
        mask = (P.n_legal >= target).astype(np.uint8)
        step = target - int(done[mask == 1][0])
        eng.run_sims(step, mask=mask)
        done[mask == 1] += step
    assert np.array_equal(done, P.n_legal)
    out = eng.sample_moves(0.0)
    for i in range(len(P)):
        n = P.n_legal[i]
        assert np.array_equal(out["child_action"][i, :n], P.legal[i]), P.names[i]
        assert (out["child_plays"][i, :n] == 1).all() and out["root_plays"][i] == n, (P.names[i], out["child_plays"][i, :n])
    eng.run_sims(10)
    out = eng.sample_moves(0.0)
    for i in range(len(P)):
        _check_slot(out, i, P.legal[i], runs[i]["o"], P.names[i])
        _check_node_edges(eng, i, out, P.n_legal[i])
    _check_counters(eng.counters(), [r["stats"] for r in runs])
    _check_sampling(orc, eng, P, runs)
    eng.close()


# ---- rollout evaluator, Dynamic ---------------------------------------------------------------------------------------------------
def test_rollout_dynamic_vs_oracle_lockstep_and_one_launch(orc):
    P = WC.Positions()
    which = [P.names.index(n) for n in ROLLOUT_POSITIONS]
    sims = S + 6
    cfg = orc.make_cfg(orc.DC, max_edges=S, evaluator=orc.EVAL_ROLLOUT, c_puct=WC.C_PUCT, seed=WC.SEED)
    runs = WC.oracle_run(orc, "rollout", cfg, sims, P, which)
    for r in runs:
        RC.assert_rollouts_decided(r["stats"])
    snaps = []
    for launch in (LOCK, WAVE):
        eng = _engine(len(which), _lib.EVAL_ROLLOUT, launch)
        if launch == WAVE:
            eng.search_rollouts(True)
        assert eng.run_sims_structure() == launch
        eng.set_roots(P.packed(_lib, which), game_ids=P.lids[which])
        eng.run_sims(sims)
        snaps.append(_snap(eng))
        if launch == LOCK:
            out = eng.sample_moves(0.0)
            for s, i in enumerate(which):
                _check_slot(out, s, P.legal[i], runs[s]["o"], P.names[i], f64_rates=True)
                assert (out["child_plays"][s, :P.n_legal[i]] >= 1).all()   # uniform priors: every edge of every pass was taken
            _check_counters(eng.counters(), [r["stats"] for r in runs])
            _check_sampling(orc, eng, P, runs, which)
        eng.close()
    _same(snaps[0], snaps[1], "one launch")


# ---- network evaluator --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["split", "f32"])
def test_network_vs_oracle_on_gpu_values(orc, form):
    """The oracle's tree, fed bb_net_eval's value and dense policy for the same states through its callback evaluator, against
    the engine's: lock-step (the dense policy row through memory), one launch (the compact head: wide_prob for up to three
    moves per lane) and one launch with the evaluation cache.  The float32-MFMA form has the lock-step structure only."""
    P = WC.Positions()
    f32 = form == "f32"
    kw = dict(net_form=_lib.NET_FORM_F32) if f32 else {}
    sims = 160
    ev = _net_engine(2, **kw)
    cfg = orc.make_cfg(orc.DC, max_edges=S, evaluator=orc.EVAL_CALLBACK, c_puct=C_WIDE, seed=WC.SEED, cb=_net_callback(orc, ev))
    runs = WC.oracle_run(orc, "net_" + form, cfg, sims, P)
    ev.close()
    assert sum((r["o"]["plays"][P.legal[i]][64:] > 0).sum() for i, r in enumerate(runs)) >= 20   # later passes won simulations
    snaps = []
    for launch, cache in ((LOCK, False),) if f32 else ((LOCK, False), (WAVE, False), (WAVE, True)):
        eng = _net_engine(len(P), launch, search_cache=cache, **kw)
        assert eng.run_sims_structure() == launch
        eng.set_roots(P.packed(_lib), game_ids=P.lids)
        eng.run_sims(sims)
        snaps.append(_snap(eng))
        if launch == LOCK:
            out = eng.sample_moves(0.0)
            for i in range(len(P)):
                _check_slot(out, i, P.legal[i], runs[i]["o"], (form, P.names[i]))
            _check_counters(eng.counters(), [r["stats"] for r in runs])
        eng.close()
    for other, name in zip(snaps[1:], ("one launch", "one launch, cached")):
        _same(snaps[0], other, name)


def test_network_with_prior_noise_plays(orc):
    """Prior noise on: dc_expand draws one Beta per edge, the second and third entry of a lane included.  The oracle gets the
    same priors through its keyed callback -- bb_net_eval's clean policy mixed with orc_beta_noise of (game id, node serial,
    action); library powf there, v_log / v_exp here: 1e-5 -- so plays only, and only after the oracle's own search has been seen
    not to depend on 1e-5: its plays stay the same with every draw scaled by 1 +- 1e-4, and its two best PUCT scores at the
    root lie further apart than 1e-5."""
    P = WC.Positions()
    which = [P.names.index("b144")]
    i = which[0]
    sims = 120
    ev = _net_engine(2)
    runs = {}
    for scale in (1.0, 1.0 + 1e-4, 1.0 - 1e-4):
        cfg = orc.make_cfg(orc.DC, max_edges=S, evaluator=orc.EVAL_CALLBACK_KEYED, c_puct=C_WIDE, seed=WC.SEED,
                           cb2=_net_callback(orc, ev, keyed_noise=(WC.SEED, scale)))
        runs[scale] = WC.oracle_run(orc, ("noise", scale), cfg, sims, P, which)[0]["o"]
    o = runs[1.0]
    for scale, r in runs.items():
        assert np.array_equal(r["plays"], o["plays"]), scale
    # the root's PUCT scores as the oracle left them (priors: the root is node 0 of its game)
    st = P.orc_state(orc, i)
    _v, _l, p = ev.net_eval(planes=orc.encode(orc.DC, st))
    ev.close()
    legal = P.legal[i]
    nz = np.array([orc.lib().orc_beta_noise(WC.SEED, WC.FIRST_GAME_ID + int(P.lids[i]), 0, int(a), ALPHA) for a in legal])
    q = (1 - EPS) * p[0][legal].astype(np.float64) + EPS * nz
    score = o["winrates"][legal] + C_WIDE * (q / q.sum()) * np.sqrt(1.0 + o["plays"].sum()) / (1.0 + o["plays"][legal])
    top = np.sort(score)[::-1]
    assert top[0] - top[1] > 1e-5, top[:3]
    assert (o["plays"][legal][64:] > 0).sum() >= 3
    snaps = []
    for launch in (LOCK, WAVE):
        eng = _net_engine(1, launch, noise_on=True)
        assert eng.run_sims_structure() == launch
        eng.set_roots(P.packed(_lib, which), game_ids=P.lids[which])
        eng.run_sims(sims)
        out = eng.sample_moves(0.0)
        assert np.array_equal(out["child_action"][0, :len(legal)], legal)
        assert np.array_equal(out["child_plays"][0, :len(legal)].astype(np.float64), o["plays"][legal]), launch
        snaps.append(_snap(eng))
        eng.close()
    _same(snaps[0], snaps[1], "one launch, noise")


# ---- tree reuse and walking -----------------------------------------------------------------------------------------------------------
def test_move_roots_into_a_wide_child_and_reset_roots(orc):
    """From White's second move with three legal moves, every child Black's with 131 .. 134: search, bb_move_roots into the most
    visited child, search again (the wide node now sits behind a c_edges / c_off hint and came through dc_advance_root), against
    the oracle's move_root + find_move.  Then bb_reset_roots: the first root again, nothing forgotten."""
    P = WC.Positions()
    i = P.names.index("walk3")
    kids = dict(WC.fixture()["walk_children"].tolist())
    sims = 200
    cfg = orc.make_cfg(orc.DC, max_edges=S, evaluator=orc.EVAL_HASH, c_puct=C_WIDE, salt=WC.SALT, seed=WC.SEED)
    sr = orc.Search(cfg, WC.FIRST_GAME_ID + int(P.lids[i]))
    st = P.orc_state(orc, i)
    o1 = sr.find_move(st, 0, sims)
    assert kids[o1["action"]] > 128
    assert sr.move_root(o1["next"]) == 1
    o2 = sr.find_move(o1["next"], 0, sims)
    legal2 = np.flatnonzero(orc.legal(orc.DC, o1["next"])).astype(np.int32)
    assert len(legal2) == kids[o1["action"]] and (o2["plays"][legal2][64:] > 0).any() and (o2["plays"][legal2][128:] > 0).any()
    eng = _engine(1, _lib.EVAL_HASH, c_puct=C_WIDE, track_ancestors=True)
    eng.set_roots(P.packed(_lib, [i]), game_ids=P.lids[[i]])
    eng.run_sims(sims)
    out1 = eng.sample_moves(0.0)
    _check_slot(out1, 0, P.legal[i], o1, "first search")
    # the wide children through bb_node_edges, before any of them is the root
    root = _check_node_edges(eng, 0, out1, 3)
    for k in range(3):
        c = eng.node_edges(0, int(root["child"][k]) & 0x3FFFFFFF)
        assert c["n_children"] == kids[int(root["action"][k])] and c["plays"].sum() + 1 == root["plays"][k]
        assert (np.diff(c["action"][:c["n_children"]]) > 0).all() and (c["action"][c["n_children"]:] == -1).all()
    eng.move_roots([o1["action"]])
    out = eng.sample_moves(0.0)
    assert out["root_plays"][0] == o1["plays"][o1["action"]] and np.array_equal(out["child_action"][0, :len(legal2)], legal2)
    eng.run_sims(sims)
    out2 = eng.sample_moves(0.0)
    _check_slot(out2, 0, legal2, o2, "after move_roots")
    _check_node_edges(eng, 0, out2, len(legal2))
    _check_counters(eng.counters(), [sr.stats()])
    runs = [dict(o=o2)]
    P2 = type("Moved", (), dict(names=["moved"], legal=[legal2], __len__=lambda self: 1))()
    assert _check_sampling(orc, eng, P2, runs) >= 2
    # ResetRoot keeps the statistics: the first root with both searches' simulations, the wide child below it unchanged
    eng.reset_roots()
    top = eng.sample_moves(0.0)
    assert top["root_plays"][0] == 2 * sims and np.array_equal(top["child_action"][0, :3], P.legal[i])
    k = int(np.flatnonzero(P.legal[i] == o1["action"])[0])
    assert top["child_plays"][0, k] == out1["child_plays"][0, k] + sims
    r = _check_node_edges(eng, 0, top, 3)
    below = eng.node_edges(0, int(r["child"][k]) & 0x3FFFFFFF)
    for f in ("action", "plays", "value"):
        assert np.array_equal(below[f], out2["child_" + f][0]), f
    eng.close()


# ---- more legal moves than a node holds ---------------------------------------------------------------------------------------------
def _sample_moves_into(eng, temp, fill):
    """bb_sample_moves into host arrays that hold `fill` everywhere: what comes back was written by this call."""
    n = eng.n_slots
    out = dict(action=np.full(n, fill, np.int32), root_winrate=np.full(n, fill, np.float32), root_plays=np.full(n, fill, np.int32),
               child_action=np.full((n, S), fill, np.int32), child_plays=np.full((n, S), fill, np.int32),
               child_value=np.full((n, S), fill, np.float32))
    _lib.check(_lib.lib().bb_sample_moves(eng.h, float(temp), None, *(_lib.ptr(out[k]) for k in (
        "action", "root_winrate", "root_plays", "child_action", "child_plays", "child_value"))))
    return out


@pytest.mark.parametrize("case", ["hash_lockstep", "fixed_lockstep", "net_wave", "rollout_wave"])
def test_root_with_more_than_S_legal_moves_is_refused(orc, case):
    """Slots: 200 legal moves, 144, 129, 148.  bb_run_sims succeeds and counts every simulation of the two wide roots in
    `overflow`; bb_sample_moves reports "no tree" (-3) and empty rows for them; the slots between them and every row of theirs
    equal the oracle's search as if the neighbours were not there.  (Before dc_expand refused such a node, k_dc_sample wrote its
    145th .. 200th child into the next slot's rows, and past the arrays for the last slot.)"""
    P, O = WC.Positions(), WC.Positions("over_")
    assert O.n_legal.tolist() == [148, 200]
    mid = [P.names.index("b144"), P.names.index("w129")]
    packed = np.concatenate([O.packed(_lib, [1]), P.packed(_lib, mid), O.packed(_lib, [0])])
    lids = np.concatenate([[901], P.lids[mid], [902]])
    evaluator, fixed, launch = {"hash_lockstep": (_lib.EVAL_HASH, False, LOCK), "fixed_lockstep": (_lib.EVAL_HASH, True, LOCK),
                                "net_wave": (_lib.EVAL_NET, False, WAVE), "rollout_wave": (_lib.EVAL_ROLLOUT, False, WAVE)}[case]
    if case == "hash_lockstep":
        sims, runs = WC.sims_for(S, "dynamic"), [_hash_runs(orc, P)[i] for i in mid]
        eng = _engine(4, evaluator, launch, c_puct=C_WIDE)
    elif case == "fixed_lockstep":
        sims = 40
        cfg = orc.make_cfg(orc.DC, max_edges=S, kind=orc.FIXED, max_depth=3, evaluator=orc.EVAL_HASH, c_puct=C_FIXED, salt=WC.SALT,
                           seed=WC.SEED, priors_ones=True)
        runs = WC.oracle_run(orc, "fixed40", cfg, sims, P, mid)
        eng = _engine(4, evaluator, launch, fixed=True, c_puct=C_FIXED)
    elif case == "net_wave":
        sims = 60
        ev = _net_engine(2)
        cfg = orc.make_cfg(orc.DC, max_edges=S, evaluator=orc.EVAL_CALLBACK, c_puct=C_WIDE, seed=WC.SEED, cb=_net_callback(orc, ev))
        runs = WC.oracle_run(orc, "net60", cfg, sims, P, mid)
        ev.close()
        eng = _net_engine(4, launch)
    else:
        sims = 40
        cfg = orc.make_cfg(orc.DC, max_edges=S, evaluator=orc.EVAL_ROLLOUT, c_puct=WC.C_PUCT, seed=WC.SEED)
        runs = WC.oracle_run(orc, "rollout40", cfg, sims, P, mid)
        for r in runs:
            RC.assert_rollouts_decided(r["stats"])
        eng = _engine(4, evaluator, launch)
        eng.search_rollouts(True)
    assert eng.run_sims_structure() == launch
    eng.set_roots(packed, game_ids=lids)
    eng.run_sims(sims)                                   # succeeds
    cnt = eng.counters()
    assert cnt["overflow"] >= 2 * sims > 0               # every simulation of the two wide roots (exactly: _check_counters below)
    out = _sample_moves_into(eng, 0.0, -77)
    for s in (0, 3):
        assert out["action"][s] == _lib.ERR_STATE
        assert (out["child_action"][s] == -1).all() and (out["child_plays"][s] == 0).all() and (out["child_value"][s] == 0).all()
        r = eng.node_edges(s, -1)
        assert r["n_children"] == 0 and not (r["flags"] & 1) and (r["action"] == -1).all() and (r["plays"] == 0).all()
    for s, i in ((1, mid[0]), (2, mid[1])):
        _check_slot(out, s, P.legal[i], runs[s - 1]["o"], (case, P.names[i]), f64_rates=case == "rollout_wave")
        _check_node_edges(eng, s, out, P.n_legal[i])
    _check_counters(cnt, [r["stats"] for r in runs], extra_sims=2 * sims)
    eng.move_roots(np.array([-1, int(out["action"][1]), int(out["action"][2]), -1], dtype=np.int32))
    eng.run_sims(8)                                       # the refused roots stay refused, the others search on
    assert eng.counters()["overflow"] >= 2 * (sims + 8)
    assert _sample_moves_into(eng, 1.0, -77)["action"][[0, 3]].tolist() == [_lib.ERR_STATE, _lib.ERR_STATE]
    eng.close()


class _HashSearch(DynamicMCTS):
    """DynamicMCTS on the validation evaluator (as tests/test_gpu_dc_tree.py)."""
    def _make_engine(self, game_id, n_slots, sims, **kw):
        return _lib.Engine(game_id, n_slots=n_slots, sims_per_move=max(int(sims), 1), mcts_kind=self._KIND,
                           max_depth=self._max_depth(), evaluator=_lib.EVAL_HASH, hash_salt=WC.SALT,
                           c_puct=float(self.ExplorationRate), **kw)


def test_findmove_names_the_legal_move_count_and_S():
    O = WC.Positions("over_")
    m = _HashSearch(explorationRate=0.85, playLimit=6)
    with pytest.raises(_lib.BlackbirdHipError, match=r"200 legal moves.*S = 144"):
        m.FindMove(DragonChess.BoardState._from_packed(O.packed(_lib, [1])), 0)
    # a position the tree holds goes through the same front end (three simulations: the root, a child, a grandchild -- White's)
    P = WC.Positions()
    m = _HashSearch(explorationRate=0.85, playLimit=3)
    nxt, _v, prob = m.FindMove(DragonChess.BoardState._from_packed(P.packed(_lib, [P.names.index("b144")])), 0)
    assert (m.Root.LegalActions == 1).sum() == S and abs(prob.sum() - 1.0) < 1e-12 and m.Root.ChildPlays().sum() == 2
