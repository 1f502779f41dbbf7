"""-m gpu: example records scored with the network an engine holds (bb_examples_score, DeviceExamples.score_with,
Blackbird.EvaluateDeviceExamples(scorer='engine'); k_score_gather and k_score_rows of csrc/examples_score.hip.h).

The comparison route is Engine.net_eval(states=...) on the same states, which tests/test_gpu_net*.py hold to the oracle: its
float32 values and logits are the input of the float64 statement of tests/score_cases.py, so the network is not judged again;
the two new kernels are.  Per row the value equals net_eval's bit for bit (the same kernels; the cuts of a batch are documented
to give the same bits), se equals the float32 statement bit for bit, the flags are equal, and ce is within
tests/trainer_cases.close (1e-5 of max(1, largest |entry|)).  Counts are exact, and the two sums are the float64 sums of the
kernel's own float32 figures within 1e-12, as tests/test_gpu_trainer_eval.py holds them.

Records: a 4-game, 8-simulation self-play run under the hash evaluator per game, behind the hand-built corners of
score_cases.corners.  Against the trainer's scorer the two flag counts may differ on rows without room only -- the top two
logits closer than eval_cases.LOGIT_ROOM, |value| below VALUE_ROOM: the trainer's logits cannot be read through any entry point,
so this is the rule tests/test_gpu_trainer_eval.py compares bits under.  On the corners alone, under weights that leave every
row that room, the two scorers' flags are equal byte for byte (both call the one score_policy_serial).  Every test here fails without the entry point."""
import ctypes as C

import numpy as np
import pytest
import torch

from blackbird_amd import Blackbird, Connect4, DragonChess, _lib
from blackbird_amd import weights as W
from blackbird_amd.training import DeviceExamples, HipTrainer, eval_summary
from tests import eval_cases as EC
from tests import score_cases as SC
from tests import selfplay_cases as SP
from tests.trainer_cases import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C4, TTT, DC = SC.C4, SC.TTT, SC.DC
AUTO, F32 = _lib.NET_FORM_AUTO, _lib.NET_FORM_F32
_cache = {}


def _host_records(game):
    """the corners, then the self-play records; computed once and left unchanged"""
    if game not in _cache:
        kw = dict(max_plies=8) if game == DC else {}
        eng = _lib.Engine(game, n_slots=4, sims_per_move=8, evaluator=_lib.EVAL_HASH, hash_salt=5, seed=3, max_games=4, **kw)
        played = SP.play_to_end(eng, 4, 4, 1.0, steps_below=64)["rec"]
        eng.close()
        corners, at = SC.corners(game)
        assert len(played) >= 8
        _cache[game] = (np.concatenate([corners, played]), at)
    return _cache[game]


def _examples(game, well_formed=False):
    rec, at = _host_records(game)
    if well_formed:
        rec = rec[[r for r in range(len(rec)) if not SC.malformed(game, rec, r)]]
    return DeviceExamples.from_records(game, rec, DEV), rec, at


def _engine(game, F, R, form=AUTO, seed=7, **kw):
    gi = _lib.game_info(game)
    kw.setdefault("launch", _lib.LAUNCH_LOCKSTEP)           # (no evaluation cache to allocate: nothing here searches)
    eng = _lib.Engine(game, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET, net_form=form, **kw)
    eng.load_weights(W.flatten(W.init_weights(gi.C, F, R, 16, gi.A, seed=seed, perturb=True)))
    return eng


def _net_outputs(eng, game, rec, index):
    """net_eval's float32 (logits [n, A], values [n]) of the rows' states; zeros for malformed rows"""
    gi = _lib.game_info(game)
    index = np.asarray(index, dtype=np.int64)
    good = np.array([k for k, r in enumerate(index) if not SC.malformed(game, rec, int(r))], dtype=np.int64)
    logits, values = np.zeros((len(index), gi.A), dtype=np.float32), np.zeros(len(index), dtype=np.float32)
    if len(good):
        v, lg, _p = eng.net_eval(states=SP.states_of(game, rec[index[good]]))
        logits[good], values[good] = lg, v
    return logits, values


def _idx(index):
    return None if index is None else torch.tensor(np.asarray(index, dtype=np.int64), device=DEV)


def _check(game, got, want, what):
    rows, flags = got["per_row"].cpu().numpy(), got["flags"].cpu().numpy()
    assert rows.dtype == np.float32 and rows.shape == want["rows"].shape and flags.shape == want["flags"].shape
    assert np.array_equal(rows[:, 0].view(np.uint32), want["rows"][:, 0].astype(np.float32).view(np.uint32)), (what, "value")
    assert np.array_equal(rows[:, 1].view(np.uint32), want["rows"][:, 1].astype(np.float32).view(np.uint32)), (what, "se")
    assert np.array_equal(flags, want["flags"]), (what, "flags", flags, want["flags"])
    if len(rows):
        close(rows[:, 2], want["rows"][:, 2], (what, "ce"))
    assert not rows[~want["ok"]].any()
    for k in EC.COUNTS:
        assert got[k] == want["totals"][k], (what, k)
    own = SC.totals(rows, flags)                              # the kernel's own float32 figures, summed in float64
    for k in ("se_sum", "ce_sum"):
        print(what, k, "%.17g" % got[k], "float64 sum of the rows %.17g" % own[k])
        assert abs(got[k] - own[k]) <= 1e-12 * max(1.0, abs(own[k])), (what, k)
    return rows, flags


ENGINES = [(C4, 16, 0, AUTO), (C4, 16, 0, F32), (C4, 16, 2, AUTO), (C4, 16, 2, F32), (C4, 32, 1, AUTO), (C4, 32, 1, F32),
           (TTT, 16, 1, AUTO), (DC, 16, 1, AUTO), (DC, 16, 1, F32), (DC, 32, 1, AUTO)]


@pytest.mark.parametrize("game,F,R,form", ENGINES)
def test_rows_against_net_eval(game, F, R, form):
    ex, rec, at = _examples(game)
    eng = _engine(game, F, R, form)
    assert eng.net_form() == {(16, AUTO): 2, (16, F32): 0, (32, AUTO): 3, (32, F32): 1}[(F, form)]
    bad = 0
    for n in (0, 1, 5, 67):
        index = np.resize(np.arange(len(rec)), n)             # the corners first; 67 rows repeat the records
        want = SC.statement(game, *_net_outputs(eng, game, rec, index), rec, index)
        got = ex.score_with(eng, _idx(index), rows=True)
        _check(game, got, want, (game, F, R, form, n))
        bad += int((~want["ok"]).sum())
        if n == 0:
            assert got["rows"] == 0 and got["se_sum"] == 0.0 and np.isnan(got["value_mse"])
        if n == 67:
            assert want["totals"]["policy_rows"] > 8 and want["totals"]["top1"] < want["totals"]["policy_rows"]
    assert ex.bad() == bad and bad > 0
    whole = ex.score_with(eng, None, rows=True)               # index == NULL: every record in order
    _check(game, whole, SC.statement(game, *_net_outputs(eng, game, rec, np.arange(len(rec))), rec), (game, F, R, form, "all"))
    eng.close()


@pytest.mark.parametrize("game,F", [(C4, 16), (DC, 16), (C4, 32)])
def test_index_chunks_and_repeatability(game, F):
    ex, rec, at = _examples(game)
    eng = _engine(game, F, 1)
    nr = len(rec)
    base = ex.score_with(eng, None, rows=True)
    rows0, flags0 = base["per_row"].cpu().numpy(), base["flags"].cpu().numpy()
    before = ex.bad()
    # a permutation with repeats, every malformed kind in between
    rng = np.random.RandomState(9)
    order = np.concatenate([rng.permutation(nr), [at["tie"], at["tie"]]])
    wrong = {3: -1, 8: nr, 11: at["too_many"]}
    if game == DC:
        wrong[13] = at["bad_action"]
    index = order.copy()
    for k, r in wrong.items():
        index[k] = r
    got = ex.score_with(eng, _idx(index), rows=True)
    rows, flags = got["per_row"].cpu().numpy(), got["flags"].cpu().numpy()
    zero = np.array([SC.malformed(game, rec, int(r)) for r in index])
    assert zero[list(wrong)].all() and not rows[zero].any() and not flags[zero].any()
    keep = ~zero
    assert np.array_equal(rows[keep].view(np.uint32), rows0[index[keep]].view(np.uint32)) and np.array_equal(flags[keep], flags0[index[keep]])
    assert ex.bad() - before == int(zero.sum()) and got["rows"] == int(keep.sum())
    # chunks: a workspace for 3 rows with 7 rows against one chunk of 7; and the same call twice
    seven = _idx(index[:7])
    one = ex.score_with(eng, seven, rows=True, chunk_rows=7)
    for other in (ex.score_with(eng, seven, rows=True, chunk_rows=3), ex.score_with(eng, seven, rows=True, chunk_rows=7),
                  ex.score_with(eng, seven, rows=True, chunk_rows=1)):
        assert torch.equal(one["per_row"].view(torch.int32), other["per_row"].view(torch.int32)) and torch.equal(one["flags"], other["flags"])
        assert all(one[k] == other[k] for k in EC.COUNTS + ("se_sum", "ce_sum"))
    eng.close()


@pytest.mark.parametrize("game", [C4, TTT, DC])
def test_workspace_and_refusals(game):
    gi = _lib.game_info(game)
    eng = _engine(game, 16, 0)
    sizes = [eng.score_workspace(r) for r in range(0, 70)]
    assert sizes[0] == 0 and all(s % 16 == 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert all(sizes[r + 16] > sizes[r] for r in range(0, 54)) and sizes[1] >= gi.state_bytes + 4 * gi.A
    L, h = _lib.lib(), eng.h
    P = 0x10000                                               # (never read: every case returns before any device work)
    ok = dict(nrec=4, rec=P, n=2, index=P, rows=P, flags=P, tot=P, bad=P, ws=P, wsb=sizes[2])
    call = lambda **kw: (lambda a: L.bb_examples_score(h, a["nrec"], a["rec"], a["n"], a["index"], a["rows"], a["flags"], a["tot"],  # noqa: E731
                                                        a["bad"], a["ws"], a["wsb"], None))({**ok, **kw})
    for kw in (dict(n=-1), dict(nrec=-1), dict(tot=None), dict(rec=P + 8), dict(index=P + 4), dict(tot=P + 4), dict(rows=P + 2),
               dict(bad=P + 2), dict(ws=P + 8), dict(wsb=sizes[1] - 16), dict(wsb=0), dict(ws=None), dict(rec=None), dict(rows=None),
               dict(flags=None)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert _lib.last_error()
    out = C.c_uint64(0)
    assert L.bb_examples_score_workspace(h, -1, C.byref(out)) == _lib.ERR_ARG and L.bb_examples_score_workspace(h, 1, None) == _lib.ERR_ARG
    eng.close()
    # an engine without weights, and one whose evaluator is not the network: BB_ERR_WEIGHTS
    ex, _rec, _at = _examples(game)
    for bare in (_lib.Engine(game, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET, launch=_lib.LAUNCH_LOCKSTEP),
                 _lib.Engine(game, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_HASH)):
        with pytest.raises(_lib.BlackbirdHipError, match="error -6"):
            ex.score_with(bare)
        bare.close()
    assert ex.bad() == 0
    with pytest.raises(ValueError, match="game"):
        other = _engine(TTT if game == C4 else C4, 16, 0)
        try:
            ex.score_with(other)
        finally:
            other.close()


def test_a_score_moves_nothing_of_the_engine(monkeypatch):
    flat = SP.c4_weights(16, 1, seed=2)
    a, b = (SP.c4_engine_under_cache(monkeypatch, True, 4, 8, 4, log2=12) for _ in range(2))
    first = [SP.play_loaded(e, flat, 4, 4, mode=None) for e in (a, b)]
    SP.assert_same_runs(first[0], first[1], "first run")
    assert first[0]["cnt"]["eval_cache_probes"] > 0
    ex, _rec, _at = _examples(C4)
    before = a.counters()
    got = ex.score_with(a, rows=True)
    assert got["rows"] > 8 and a.counters() == before
    second = [SP.play_to_end(e, 4, 4, 1.0) for e in (a, b)]
    SP.assert_same_runs(second[0], second[1], "after a score")          # (records, offsets, winners; sims and depths)
    assert second[0]["cnt"]["eval_cache_hits"] > 0                      # the table of the first run is still there
    a.close()
    b.close()


def test_against_the_trainers_scorer():
    ex, rec, _at = _examples(C4, well_formed=True)
    w0 = W.init_weights(3, 16, 2, 16, 7, seed=5, perturb=True)
    tr = HipTrainer(w0, device=DEV, seed=1)
    theirs = tr.evaluate_records(ex, rows=True)
    for form in (AUTO, F32):
        eng = _lib.Engine(C4, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET, net_form=form, launch=_lib.LAUNCH_LOCKSTEP)
        eng.load_weights(W.flatten(w0))
        mine = ex.score_with(eng, rows=True)
        for k in ("rows", "policy_rows", "decided"):
            assert mine[k] == theirs[k] == SC.totals(mine["per_row"].cpu().numpy(), mine["flags"].cpu().numpy())[k], k
        for k in ("value_mse", "policy_ce"):
            print(form, k, "engine %.9g trainer %.9g" % (mine[k], theirs[k]))
            assert abs(mine[k] - theirs[k]) <= 1e-5 * abs(theirs[k]) + 1e-6, k
        logits, values = _net_outputs(eng, C4, rec, np.arange(len(rec)))
        top = np.sort(logits, axis=1)
        fm, ft = mine["flags"].cpu().numpy().astype(int), theirs["flags"].cpu().numpy().astype(int)
        differ = (fm ^ ft) != 0
        top1_differs, sign_differs = ((fm ^ ft) & _lib.ROW_TOP1) != 0, ((fm ^ ft) & _lib.ROW_SIGN_OK) != 0
        print(form, "rows whose flags differ:", int(differ.sum()), "top1", int(top1_differs.sum()), "sign_ok", int(sign_differs.sum()))
        assert not ((fm ^ ft) & ~(_lib.ROW_TOP1 | _lib.ROW_SIGN_OK)).any()
        assert ((top[:, -1] - top[:, -2])[top1_differs] <= EC.LOGIT_ROOM).all() and (np.abs(values)[sign_differs] <= EC.VALUE_ROOM).all()
        assert abs(mine["top1"] - theirs["top1"]) <= int(top1_differs.sum()) and abs(mine["sign_ok"] - theirs["sign_ok"]) <= int(sign_differs.sum())
        eng.close()
    assert ex.bad() == 0
    tr.close()


@pytest.mark.parametrize("game", [C4, TTT])
def test_both_scorers_set_the_same_flags_on_the_corners(game):
    """The hand-built corners -- 'terminal' (total 0), 'tie' (two top shares), z in {-1, 0, 1}, 'too_many' (malformed) -- scored
    with the same 16-filter weights by the trainer's scorer and by an engine in the float32 form: the flags bytes are equal row
    by row, no row left out.  The two networks round differently (1e-5), so a TOP1 or SIGN_OK bit may differ only where two
    logits, or the value and 0, lie that close; the float64 statement (eval_cases.forward, on the CPU) shows that no corner
    does under init_weights(seed=2, perturb=True) with 2 blocks: the smallest gap between the top two logits is 0.0578
    (Connect4; TicTacToe 0.590) and the smallest |value| 0.0110 (TicTacToe; Connect4 0.349), both asserted > 1e-3 here.  The
    values are negative, so SIGN_OK is set on the z = -1 row and clear on the z = 1 rows."""
    gi = _lib.game_info(game)
    rec, at = SC.corners(game)
    ex = DeviceExamples.from_records(game, rec, DEV)
    w0 = W.init_weights(gi.C, 16, 2, 16, gi.A, seed=2, perturb=True)
    good = np.array([r for r in range(len(rec)) if not SC.malformed(game, rec, r)])
    value, logits = EC.forward(w0, EC.host_rows(game, rec[good])[0])
    top = np.sort(logits, axis=1)
    print(game, "smallest top-two logit gap %.4g, smallest |value| %.4g" % ((top[:, -1] - top[:, -2]).min(), np.abs(value).min()))
    assert (top[:, -1] - top[:, -2]).min() > 1e-3 and np.abs(value).min() > 1e-3
    want = np.zeros(len(rec), dtype=np.uint8)
    want[good] = SC.statement(game, logits, value, rec, good)["flags"]
    tr = HipTrainer(w0, device=DEV, seed=1)
    eng = _lib.Engine(game, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET, net_form=F32, launch=_lib.LAUNCH_LOCKSTEP)
    eng.load_weights(W.flatten(w0))
    assert eng.net_form() == 0
    theirs = tr.evaluate_records(ex, rows=True)["flags"].cpu().numpy()
    mine = ex.score_with(eng, rows=True)["flags"].cpu().numpy()
    eng.close()
    tr.close()
    print(game, "trainer", theirs, "engine", mine, "statement", want)
    assert np.array_equal(mine, theirs), (mine, theirs)
    assert np.array_equal(mine, want) and mine[at["too_many"]] == 0 and ex.bad() == 2      # (one malformed row, met by each scorer)
    assert mine[at["terminal"]] & _lib.ROW_COUNTED and not mine[at["terminal"]] & _lib.ROW_HAS_POLICY
    assert {int(z) for z in rec["z"][good]} == {-1, 0, 1} and (mine[good] & _lib.ROW_SIGN_OK).any()


def _cfg(backend, filters=16, hip_games=None):
    training = {"optimizer": "adam"}
    if backend:
        training["backend"] = backend
    if hip_games:
        training["hip_games"] = hip_games
    return {"blocks": 1, "filters": filters, "eval": {"dense": 16}, "hasTeacher": False,
            "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.0}}, "training": training}


def _same(a, b):
    return all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a) and set(a) == set(b)


def _fresh_score(game, weights, ex):
    eng = _lib.Engine(game, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET, launch=_lib.LAUNCH_LOCKSTEP)
    eng.load_weights(W.flatten(weights))
    out = ex.score_with(eng)
    eng.close()
    return out


@pytest.mark.parametrize("game,board,cfg", [(DC, DragonChess.BoardState, _cfg("hip", 16, "all")), (C4, Connect4.BoardState, _cfg(None, 32))])
def test_front_end_scores_with_the_evaluation_engine(tmp_path, monkeypatch, game, board, cfg):
    monkeypatch.chdir(tmp_path)
    ex, _rec, _at = _examples(game, well_formed=True)
    model = Blackbird.Model(board, "scored", {"explorationRate": 0.85, "playLimit": 8}, cfg)
    state = np.random.get_state()
    got = Blackbird.EvaluateDeviceExamples(model, ex, scorer="engine")
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]       # numpy's generator is left where it was
    assert model._trainer is None and model._eval_engine is not None           # no trainer is made
    assert got["rows"] == len(ex) and got["policy_rows"] > 0 and set(got) == set(eval_summary(0, 0, 0, 0, 0, 0.0, 0.0))
    assert _same(got, _fresh_score(game, model._weights, ex))
    assert _same(got, Blackbird.EvaluateDeviceExamples(model, ex, batchSize=5, scorer="engine"))     # chunks of 5 rows
    np.random.seed(5)
    Blackbird.TrainWithDeviceExamples(model, 4, 0.01, examples=ex)
    trained = Blackbird.EvaluateDeviceExamples(model, ex, scorer="engine")
    assert not _same(trained, got) and _same(trained, _fresh_score(game, model._trainer.export(), ex))
    with pytest.raises(ValueError, match="scorer"):
        Blackbird.EvaluateDeviceExamples(model, ex, scorer="bogus")
    if game == C4:
        with pytest.raises(ValueError, match="records source"):
            Blackbird.EvaluateDeviceExamples(model, ex.merged(), scorer="engine")


def test_front_end_trainer_scorer_is_what_it_was(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ex, _rec, _at = _examples(C4, well_formed=True)
    model = Blackbird.Model(Connect4.BoardState, "kept", {"explorationRate": 0.85, "playLimit": 8}, _cfg("hip"))
    plain = Blackbird.EvaluateDeviceExamples(model, ex)
    assert type(model._trainer) is HipTrainer
    assert _same(plain, Blackbird.EvaluateDeviceExamples(model, ex, scorer="trainer")) and _same(plain, model._trainer.evaluate_records(ex))
    engine = Blackbird.EvaluateDeviceExamples(model, ex, scorer="engine")
    for k in ("rows", "policy_rows", "decided"):
        assert engine[k] == plain[k]
    assert abs(engine["policy_ce"] - plain["policy_ce"]) <= 1e-5 * abs(plain["policy_ce"]) + 1e-6
