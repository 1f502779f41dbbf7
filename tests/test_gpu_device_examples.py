"""-m gpu: training from self-play examples that stay on the GPU.

bb_examples_to_batch (csrc/examples.hip.h) through training.DeviceExamples against the host statement of the same three
tensors -- planes by bb_game_encode, pi = visits / total in float64 as GenerateTrainingSamples' blobs_of forms it, then
float32, z as float32 -- BIT for bit: real self-play records of all three games (hash evaluator, no weights needed),
hand-built records for the corners (total == 0, the float64 division, spare slots, a full and an empty compact child
list), malformed input (contained: zero rows and a count, every access in bounds by construction), and the front end:
Model.KeepDeviceExamples + Blackbird.TrainWithDeviceExamples, which must train exactly as the host path does."""
import numpy as np
import pytest

from blackbird_amd import Blackbird, Connect4, _lib
from blackbird_amd.training import DeviceExamples, Trainer, epoch_order
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
SELFPLAY = {C4: dict(n_games=8, sims=16), TTT: dict(n_games=8, sims=16), DC: dict(n_games=2, sims=8, max_plies=6)}
TOL = 1e-5  # tests/test_train_parity.py


def expected(game, rec):
    """(boards, value, policy) of host records, formed on the host."""
    gi = _lib.game_info(game)
    st = np.ascontiguousarray(rec["state"]).view(_lib.STATE_DTYPE[game]).reshape(len(rec), -1)
    boards = _lib.game_encode(game, st).astype(np.float32)
    tot = rec["total"].astype(np.float64)
    if gi.dense:
        visits = rec["visits"][:, :gi.A].astype(np.float64)
    else:  # Blackbird.GenerateTrainingSamples.blobs_of
        visits = np.zeros((len(rec), gi.A), dtype=np.float64)
        live = np.arange(gi.S)[None, :] < rec["n_children"][:, None]
        rows = np.nonzero(live)[0]
        visits[rows, rec["action"][live]] = rec["visits"][live]
    pi = np.where(tot[:, None] > 0, visits / np.maximum(tot, 1.0)[:, None], 0.0)
    return boards, rec["z"].astype(np.float32), pi.astype(np.float32)


def same(got, want, rows=None):
    for g, w, what in zip(got, want, ("boards", "value", "policy")):
        g = g.cpu().numpy()
        w = w if rows is None else w[rows]
        assert g.dtype == np.float32 and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, int((g != w).sum()))


_played = {}


def played(game):
    """One finished self-play run per game, shared by the tests (left unchanged): host records, what the host forms from
    them, and the device snapshot taken from the engine -- after which the engine starts another run, so that a snapshot
    that still looked into the engine's store would show."""
    if game not in _played:
        cfg = SELFPLAY[game]
        eng = _lib.Engine(game, n_slots=cfg["n_games"], sims_per_move=cfg["sims"], evaluator=_lib.EVAL_HASH, hash_salt=5, seed=3,
                          max_games=cfg["n_games"], max_plies=cfg.get("max_plies"))
        rec = SP.play_to_end(eng, cfg["n_games"], 4, 1.0, steps_below=64)["rec"].copy()
        ex = DeviceExamples.from_engine(eng, DEV)
        eng.set_rng_stream(99, 1000)
        eng.selfplay_begin(cfg["n_games"], 1.0)
        eng.selfplay_step(2)
        eng.synchronize()
        eng.close()
        _played[game] = (rec, expected(game, rec), ex)
    return _played[game]


@pytest.mark.parametrize("game", [C4, TTT, DC])
def test_real_records_bit_exact(game):
    rec, want, ex = played(game)
    n = len(rec)
    assert len(ex) == n >= SELFPLAY[game]["n_games"] * 2 and ex.records.is_cuda
    assert ex.records.cpu().numpy().tobytes() == rec.tobytes()
    terminal = rec["total"] == 0
    assert terminal.sum() == SELFPLAY[game]["n_games"] and (rec["total"] > 0).any()  # every game's terminal example is there
    assert not want[2][terminal].any() and want[2][~terminal].any()
    same(ex.batch(), want)                                   # index = None: every record, in order
    rng = np.random.RandomState(1)
    perm = rng.permutation(n)
    same(ex.batch(perm), want, perm)
    import torch
    same(ex.batch(torch.from_numpy(perm).to(DEV)), want, perm)  # an index that is on the device already
    same(ex.batch([n - 1]), want, [n - 1])                   # a batch of one
    for rows in (5, 257):                                    # not a multiple of what a block covers; more than one block
        idx = rng.randint(0, n, rows)
        same(ex.batch(idx), want, idx)
    assert ex.bad() == 0
    # the same through from_records and cat, and any single output alone
    half = DeviceExamples.cat([DeviceExamples.from_records(game, rec[:3], DEV), DeviceExamples.from_records(game, rec[3:], DEV)])
    same(half.batch(perm), want, perm)
    gi = _lib.game_info(game)
    pol = torch.full((n, gi.A), 7.0, dtype=torch.float32, device=DEV)
    _lib.examples_to_batch(game, n, ex.records.data_ptr(), n, policy=pol.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(pol.cpu().numpy(), want[2])
    val = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    _lib.examples_to_batch(game, n, ex.records.data_ptr(), n, value=val.data_ptr())
    assert np.array_equal(val.cpu().numpy(), want[1])
    with pytest.raises(ValueError):
        _lib.examples_to_batch(game, n, ex.records.data_ptr(), n)  # all three outputs absent


def _blank(game, n):
    rec = np.zeros(n, dtype=_lib.example_dtype(game))
    rec["state"] = _lib.game_initial(game).view(np.uint8).reshape(1, -1)
    rec["game_id"] = 7
    rec["ply"] = np.arange(n)
    rec["player"] = 1
    return rec


BIG = 2 ** 24 + 1


def test_the_chosen_pair_tells_a_float32_division_from_the_float64_one():
    """(2^24 - 1) / (2^24 + 1): float32 operands first (2^24 + 1 rounds to 2^24) gives 1 - 2^-24, the float64 quotient
    rounds to 1 - 2^-23."""
    v, t = np.array([BIG - 2], dtype=np.uint32), np.array([BIG], dtype=np.uint32)
    in64 = (v.astype(np.float64) / t.astype(np.float64)).astype(np.float32)
    in32 = v.astype(np.float32) / t.astype(np.float32)
    assert in64[0] != in32[0] and in64[0] == np.float32(1 - 2.0 ** -23)


@pytest.mark.parametrize("game", [C4, TTT])
def test_hand_built_dense_records(game):
    gi = _lib.game_info(game)
    rec = _blank(game, 6)
    rec["n_children"] = gi.A
    rec["z"] = [0, 1, -1, 1, -1, 0]
    rec["visits"][0, :3] = [4, 5, 6]                 # total == 0: a zero row whatever the visits say
    rec["visits"][1, :2] = [1, 2]
    rec["total"][1] = 3
    rec["visits"][2, 0] = BIG
    rec["total"][2] = BIG
    rec["visits"][3, 0] = BIG - 2                    # pins the double division (see the test above)
    rec["total"][3] = BIG
    rec["visits"][4, :gi.A] = np.arange(1, gi.A + 1)
    rec["visits"][4, gi.A:] = 1000 + np.arange(gi.S - gi.A)   # spare slots: must not appear anywhere
    rec["total"][4] = rec["visits"][4, :gi.A].sum()
    rec["visits"][5, gi.A - 1] = 3                   # the last action
    rec["total"][5] = 3
    assert gi.S > gi.A
    ex = DeviceExamples.from_records(game, rec, DEV)
    want = expected(game, rec)
    got = ex.batch()
    same(got, want)
    pol = got[2].cpu().numpy()
    assert not pol[0].any()
    assert np.array_equal(pol[1, :3], np.array([1 / 3, 2 / 3, 0], dtype=np.float64).astype(np.float32))
    assert pol[2, 0] == np.float32(1.0) and pol[3, 0] == np.float32(1 - 2.0 ** -23)
    assert pol[4].max() < 1 and abs(float(pol[4].astype(np.float64).sum()) - 1) < 1e-6
    assert np.array_equal(got[1].cpu().numpy(), rec["z"].astype(np.float32))
    assert ex.bad() == 0


def _dc_records():
    gi = _lib.game_info(DC)
    S, A = gi.S, gi.A
    rec = _blank(DC, 5)
    rng = np.random.RandomState(2)
    rec["action"] = 0xFFFF                          # what the engine leaves beyond n_children
    acts = rng.permutation(np.arange(1, A - 1))[:S].astype(np.uint16)
    acts[3], acts[S - 1] = 0, A - 1                 # both ends of the row
    for r in (0, 2, 4):                             # full child lists, distinct actions
        rec["n_children"][r] = S
        rec["action"][r] = np.roll(acts, r)
        rec["visits"][r] = rng.randint(1, 50, S)
        rec["total"][r] = rec["visits"][r].sum()
    rec["z"] = [1, -1, 0, 1, -1]
    rec["visits"][1, :4] = [9, 9, 9, 9]             # no children: nothing of these may show
    rec["total"][1] = 36
    rec["n_children"][3] = 2                        # a short list
    rec["action"][3, :2] = [A - 1, 0]
    rec["visits"][3, :2] = [BIG - 2, 2]
    rec["total"][3] = BIG
    return rec


def test_hand_built_dragonchess_records():
    gi = _lib.game_info(DC)
    rec = _dc_records()
    ex = DeviceExamples.from_records(DC, rec, DEV)
    want = expected(DC, rec)
    got = ex.batch()
    same(got, want)
    pol = got[2].cpu().numpy()
    assert (pol[0] != 0).sum() == gi.S
    assert pol[0, 0] == np.float32(rec["visits"][0, 3] / rec["total"][0]) and pol[0, gi.A - 1] != 0
    assert not pol[1].any()
    assert pol[3, gi.A - 1] == np.float32(1 - 2.0 ** -23) and (pol[3] != 0).sum() == 2
    assert ex.bad() == 0


def test_malformed_input_is_contained():
    """Zero rows and a count -- no fault is provoked: the kernel checks an index, a child count and an action before it uses
    them, so every access stays inside the buffers whatever they say."""
    import torch
    # indices outside the records, below DeviceExamples' own range check
    rec, want, ex = played(C4)
    gi = _lib.game_info(C4)
    n_rec = len(rec)
    idx = np.array([0, n_rec, 1, -1, n_rec - 1], dtype=np.int64)
    good = np.array([0, 2, 4])
    d_idx = torch.from_numpy(idx).to(DEV)
    boards = torch.full((5, gi.H, gi.W, gi.C), 7.0, dtype=torch.float32, device=DEV)
    policy = torch.full((5, gi.A), 7.0, dtype=torch.float32, device=DEV)
    value = torch.full((5,), 7.0, dtype=torch.float32, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.examples_to_batch(C4, n_rec, ex.records.data_ptr(), 5, d_idx.data_ptr(), boards.data_ptr(), policy.data_ptr(),
                           value.data_ptr(), bad.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert int(bad.item()) == 2
    for t, w in zip((boards, value, policy), want):
        t = t.cpu().numpy()
        assert not t[[1, 3]].any() and np.array_equal(t[good], w[idx[good]])
    with pytest.raises(IndexError):
        ex.batch(idx)                               # ... which refuses them before anything is launched
    # a dense record that claims more children than a row has
    r2 = rec[:3].copy()
    r2["n_children"][1] = gi.S + 1
    e2 = DeviceExamples.from_records(C4, r2, DEV)
    got = [t.cpu().numpy() for t in e2.batch()]
    for t, w in zip(got, want):
        assert not t[1].any() and np.array_equal(t[[0, 2]], w[[0, 2]])
    assert e2.bad() == 1
    # DragonChess: an action beyond the policy row, a child count beyond the record; the same for an index out of range
    gd = _lib.game_info(DC)
    rd = _dc_records()
    wd = expected(DC, rd)
    rd["action"][1, 0] = gd.A
    rd["n_children"][1] = 1
    rd["n_children"][3] = gd.S + 1
    e3 = DeviceExamples.from_records(DC, rd, DEV)
    got = [t.cpu().numpy() for t in e3.batch()]
    for t, w in zip(got, wd):
        assert not t[[1, 3]].any() and np.array_equal(t[[0, 2, 4]], w[[0, 2, 4]])
    assert e3.bad() == 2
    pol = torch.full((3, gd.A), 7.0, dtype=torch.float32, device=DEV)
    d_idx = torch.tensor([4, 5, 0], dtype=torch.int64, device=DEV)
    _lib.examples_to_batch(DC, 5, e3.records.data_ptr(), 3, d_idx.data_ptr(), policy=pol.data_ptr(), bad=e3._bad.data_ptr())
    pol = pol.cpu().numpy()
    assert not pol[1].any() and np.array_equal(pol[[0, 2]], wd[2][[4, 0]]) and e3.bad() == 3


# ---- the front end ------------------------------------------------------------------------------------------------
def _cfg(epsilon=0.3):
    return {"blocks": 4, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
            "policy": {"dirichlet": {"alpha": 0.2, "epsilon": epsilon}}, "training": {"optimizer": "adam"}}


def _close(got, want, what):
    scale = max(1.0, float(np.max(np.abs(want))))
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))))
    print(what, "err", err, "scale", scale)
    assert err <= TOL * scale, (what, err, scale)


def test_keep_device_examples_and_train_with_them(tmp_path, monkeypatch):
    import torch
    monkeypatch.chdir(tmp_path)
    mcts = {"explorationRate": 0.85, "playLimit": 16}
    # the attribute left False: nothing is kept, sqlite receives the games
    plain = Blackbird.Model(Connect4.BoardState, "plain", mcts, _cfg())
    assert plain.KeepDeviceExamples is False
    np.random.seed(21)
    Blackbird.GenerateTrainingSamples(plain, 8, 1.0)
    blobs_plain = plain.Conn.GetGames(plain.Name, plain.Version)
    assert plain.KeptDeviceExamples() is None and plain._kept_examples == []
    with pytest.raises(ValueError):
        Blackbird.TrainWithDeviceExamples(plain, 16, 0.01)
    assert plain.Version == 1
    plain._batch_engine.close()
    plain.Conn.Close()
    # switched on: the same games go to sqlite (same numpy seed, same initial weights), and as many records stay on the GPU
    model = Blackbird.Model(Connect4.BoardState, "kept", mcts, _cfg())
    model.KeepDeviceExamples = True
    np.random.seed(21)
    Blackbird.GenerateTrainingSamples(model, 8, 1.0)
    blobs = model.Conn.GetGames(model.Name, model.Version)
    assert sorted(blobs) == sorted(blobs_plain) and len(blobs) >= 8 * 8
    kept = model.KeptDeviceExamples()
    assert len(kept) == len(blobs) and kept.records.is_cuda
    # ... the very examples: the blobs are (z, pi in float64, planes) of the kept records
    want = expected(C4, kept.records.cpu().numpy().reshape(-1).view(_lib.example_dtype(C4)))
    exs = [Blackbird.ExampleState.FromSerialized(b) for b in blobs]
    key = lambda b, z, p: (np.asarray(b, np.float32).tobytes(), float(z), np.asarray(p, np.float32).tobytes())
    assert sorted(key(e.Board, e.MctsEval[0], e.MctsPolicy) for e in exs) == sorted(key(*row) for row in zip(*want))
    # a second run accumulates
    Blackbird.GenerateTrainingSamples(model, 8, 1.0)
    n_all = len(model.Conn.GetGames(model.Name, model.Version))
    assert len(model.KeptDeviceExamples()) == n_all > len(blobs)
    # training
    x = _lib.game_encode(C4, _lib.game_initial(C4))
    before = model.getEvaluation(x)              # (creates the engine behind getEvaluation with the OLD weights)
    w_old = {k: v.copy() for k, v in model._weights.items()}
    calls = {"changed": 0, "put": 0}

    def counted(obj, name, key):
        inner = getattr(obj, name)

        def wrapper(*args):
            calls[key] += 1
            return inner(*args)
        monkeypatch.setattr(obj, name, wrapper)
    counted(model, "_weights_changed", "changed")
    counted(model.Conn, "PutModel", "put")
    Blackbird.TrainWithDeviceExamples(model, 16, 0.01)
    assert model.Version == 2 and calls == {"changed": 1, "put": 1}
    assert model.batchCount == n_all // 16 >= 8
    assert model.Conn.GetLastVersion(Connect4.BoardState.GameType, "kept") == 2
    assert model._kept_examples == [] and model.KeptDeviceExamples() is None   # the old version's examples are dropped
    assert any(not np.array_equal(model._weights[k], w_old[k]) for k in w_old)
    # the engines hold the trained weights: their outputs are the trainer's forward pass of the exported weights
    planes = np.concatenate([x, want[0][:6].astype(np.int8)])
    tr = Trainer(model._weights, device=DEV)
    with torch.no_grad():
        tv, tl = tr.forward(torch.tensor(planes.astype(np.float32), device=DEV))
    tv, tl = tv.cpu().numpy(), tl.cpu().numpy()
    after = model.getEvaluation(x)
    assert after != before and abs(float(after) - float(tv[0])) <= TOL
    ev, el, _ep = model._eval_engine.net_eval(planes=planes)
    assert np.max(np.abs(ev - tv)) <= TOL and np.max(np.abs(el - tl) / np.maximum(1.0, np.abs(tl))) <= TOL
    bv, bl, _bp = model._batch_engine.net_eval(planes=planes)     # the self-play engine too
    assert np.array_equal(bv, ev) and np.array_equal(bl, el)
    pol = model.getPolicy(x)
    assert pol.shape == (7,) and abs(float(pol.sum()) - 1) < 1e-4
    with pytest.raises(ValueError):
        Blackbird.TrainWithDeviceExamples(model, 16, 0.01)        # nothing kept for version 2
    model._batch_engine.close()
    model.Conn.Close()


def test_same_training_as_the_host_path(tmp_path, monkeypatch):
    """Two batches of 16 of the same records in the same epoch order: the device path against the host statement
    (_records_to_examples' stacking fed to Network.train batch by batch).  epsilon = 0: the loss draws no noise.  The
    inputs are bit-identical, so only PyTorch's own reductions can differ: 1e-5, the bound tests/test_train_parity.py
    holds the GPU trainer to after two steps."""
    monkeypatch.chdir(tmp_path)
    rec = played(C4)[0][:40]                      # 40 examples: an epoch of two whole batches
    mcts = {"explorationRate": 0.85, "playLimit": 16}
    a = Blackbird.Model(Connect4.BoardState, "dev", mcts, _cfg(0))
    b = Blackbird.Model(Connect4.BoardState, "host", mcts, _cfg(0))
    assert a.epsilon == 0 and all(np.array_equal(a._weights[k], b._weights[k]) for k in a._weights)
    w0 = {k: v.copy() for k, v in a._weights.items()}
    np.random.seed(5)
    Blackbird.TrainWithDeviceExamples(a, 16, 0.01, examples=DeviceExamples.from_records(C4, rec, DEV))
    np.random.seed(5)
    order = epoch_order(len(rec), 16)
    assert len(order) == 32
    exs = Blackbird._records_to_examples(Connect4.BoardState, rec)
    for i in range(2):
        batch = [exs[j] for j in order[i * 16:(i + 1) * 16]]
        b.train(np.vstack([e.Board for e in batch]), np.hstack([e.MctsEval for e in batch]),
                np.vstack([e.MctsPolicy for e in batch]), 0.01)
    assert a.batchCount == b.batchCount == 2
    assert sorted(a._weights) == sorted(b._weights)
    moved = 0
    for k in sorted(b._weights):
        _close(a._weights[k], b._weights[k], k)
        moved += not np.array_equal(b._weights[k], w0[k])
    assert moved > len(w0) // 2
    a.Conn.Close()
    b.Conn.Close()
