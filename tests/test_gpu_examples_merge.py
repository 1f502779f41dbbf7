"""-m gpu: duplicate positions merged on the device (bb_examples_merge, bb_examples_merged_to_batch, csrc/examples_merge.hip.h;
training.MergedExamples, TrainWithDeviceExamples(merge=True)).

The statement is training.merge_records_host -- the numpy definition tests/test_examples_merge_cpu.py holds against a dict loop --
and every comparison is exact, array for array: all sums are integers, and a merged row is a float64 quotient rounded once.  The
shapes are the smallest at which the kernels can go wrong (tests/merge_cases.py): one record, one group, a set that crosses a
wave and holds a malformed record and a terminal group, a thousand records on three table slots, a thousand distinct ones in
a table of 2048."""
import numpy as np
import pytest
import torch

from blackbird_amd import Blackbird, Connect4, TicTacToe, _lib
from blackbird_amd.training import DeviceExamples, epoch_order, merge_records_host
from tests import merge_cases as MC
from tests import model_cases as M
from tests import selfplay_cases as SP
from tests.host_cases import maps  # noqa: F401  (a fixture: the maps of csrc/symmetry.h from the stand-alone program)
from tests.merge_cases import C4, TTT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMES = [C4, TTT]
BOARD_CLS = {C4: Connect4.BoardState, TTT: TicTacToe.BoardState}

_shapes = {}


def shapes(game):
    """name -> (records, the host statement of their merge), built once per game and left unchanged"""
    if game not in _shapes:
        _shapes[game] = {name: (rec, merge_records_host(game, rec)) for name, rec in MC.gpu_shapes(game).items()}
    return _shapes[game]


def arrays(m):
    return [t.cpu().numpy() for t in (m.group, m.rep, m.count, m.zsum, m.total, m.visits)]


def numpy3(t):
    return tuple(x.cpu().numpy() for x in t)


@pytest.mark.parametrize("game", GAMES)
def test_every_shape_against_the_host_statement(game):
    seen = {}
    for name, (rec, want) in shapes(game).items():
        m = DeviceExamples.from_records(game, rec, DEV).merged()
        MC.same_merge(arrays(m), want)
        assert len(m) == len(want[1]) and m.bad() == int((want[0] < 0).sum()), name
        assert np.array_equal(m.counts().cpu().numpy(), want[2])
        seen[name] = (len(rec), len(m), m.bad())
    assert seen["n=1"] == (1, 1, 0) and seen["n=2 identical"] == (2, 1, 0) and seen["n=5 one position"] == (5, 1, 0)
    assert seen["n=67 nine groups"] == (67, 9, 1) and seen["n=1000 three positions"] == (1000, 3, 0)
    rec, want = shapes(game)["n=67 nine groups"]
    assert want[4][8] == 0 and want[2][8] == 7 and want[0][30] == -1  # the terminal group, the malformed record
    if game == C4:
        assert seen["n=1000 all distinct"] == (1000, 1000, 0)


@pytest.mark.parametrize("game", GAMES)
def test_two_runs_give_the_same_bits(game):
    rec, _want = shapes(game)["n=1000 three positions"]
    ex = DeviceExamples.from_records(game, rec, DEV)
    a, b = ex.merged(), ex.merged()
    for x, y in zip(arrays(a), arrays(b)):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(numpy3(a.batch()), numpy3(b.batch())):
        assert x.tobytes() == y.tobytes()


def same(got, want):
    for g, w, what in zip(got, want, ("boards", "value", "policy")):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, int((g != w).sum()))


def identity_rows(game, rec, want):
    """the merged rows of the definition: planes of rep[g] (bb_game_encode), the float64 quotients rounded once"""
    st = np.ascontiguousarray(rec["state"]).view(_lib.STATE_DTYPE[game]).reshape(len(rec), -1)
    boards = _lib.game_encode(game, st[want[1]]).astype(np.float32)
    value, policy = MC.rows_of(rec, want)
    return boards, value, policy


def permuted(m, ident, index, sym):
    """rows `index` of the identity merged batch, cells and actions permuted by the maps m (tests/test_gpu_examples_sym.py)"""
    ib, iv, ip = ident
    H, W, C = ib.shape[1:]
    boards, policy = np.empty((len(index), H, W, C), np.float32), np.empty((len(index), ip.shape[1]), np.float32)
    for k, (g, s) in enumerate(zip(index, sym)):
        cells = np.empty((H * W, C), np.float32)
        cells[m["cell"][s]] = ib[g].reshape(H * W, C)
        boards[k] = cells.reshape(H, W, C)
        policy[k, m["action"][s]] = ip[g]
    return boards, iv[np.asarray(index)], policy


@pytest.mark.parametrize("game", GAMES)
def test_merged_batch_rows(maps, game):  # noqa: F811
    rec, want = shapes(game)["n=67 nine groups"]
    m = DeviceExamples.from_records(game, rec, DEV).merged()
    ident = identity_rows(game, rec, want)
    assert ident[2].any() and not ident[2][8].any() and len(set(ident[1].tolist())) > 2  # pooled targets, not all 0 or +-1
    same(numpy3(m.batch()), ident)
    index = np.array([8, 0, 3, 3, 7, 1, 0, 2, 6, 5, 4, 8, 3])  # a permutation of the groups with repeats
    same(numpy3(m.batch(index)), tuple(x[index] for x in ident))
    nsym = maps[game]["nsym"]
    assert m.symmetries == nsym
    for s in range(nsym):
        sym = np.full(len(index), s)
        same(numpy3(m.batch(index, sym=sym)), permuted(maps[game], ident, index, sym))
    sym = (np.arange(len(index)) * 3 + 1) % nsym   # neighbouring rows under different symmetries
    same(numpy3(m.batch(index, sym=sym)), permuted(maps[game], ident, index, sym))
    same(numpy3(m.batch(index, sym=torch.from_numpy(sym.astype(np.uint8)).to(DEV))), permuted(maps[game], ident, index, sym))
    flipped = numpy3(m.batch(sym=np.full(len(m), nsym - 1)))
    assert (flipped[0] != ident[0]).any() and (flipped[2] != ident[2]).any() and np.array_equal(flipped[1], ident[1])
    assert m.bad() == 1  # the malformed record the merge left out, and no rejected row


@pytest.mark.parametrize("game", GAMES)
def test_no_duplicates_is_the_plain_batch(game):
    rec = MC.playout_records(game, 300, 9, distinct=True)
    ex = DeviceExamples.from_records(game, rec, DEV)
    m = ex.merged()
    assert len(m) == len(ex) == 300 and (rec["total"] == 0).any()
    assert np.array_equal(m.rep.cpu().numpy(), np.arange(300)) and (m.counts() == 1).all()
    plain = numpy3(ex.batch())
    assert plain[2].any() and plain[1].any()
    for got, want in zip(numpy3(m.batch()), plain):
        assert got.tobytes() == want.tobytes()
    idx = np.random.RandomState(3).randint(0, 300, 41)
    sym = np.random.RandomState(4).randint(0, m.symmetries, 41)
    for got, want in zip(numpy3(m.batch(idx, sym=sym)), numpy3(ex.batch(idx, sym=sym))):
        assert got.tobytes() == want.tobytes()
    assert m.bad() == 0 and ex.bad() == 0


@pytest.mark.parametrize("game", GAMES)
def test_malformed_rows_are_zeros_and_counted(maps, game):  # noqa: F811
    rec, want = shapes(game)["n=67 nine groups"]
    m = DeviceExamples.from_records(game, rec, DEV).merged()
    ident = identity_rows(game, rec, want)
    nsym, n = maps[game]["nsym"], 9
    index = np.array([3, 0, 5, 5, 1, 9, 4, -1, 2])      # 9 and -1: no such group (67 records, nine groups)
    sym = (np.arange(n) + 1) % nsym
    sym[[2, 6]] = nsym, 255                              # not symmetries of the game
    wrong = [2, 5, 6, 7]
    good = np.array([k for k in range(n) if k not in wrong])
    idx = torch.from_numpy(index).to(DEV)                # (the front end's own range checks are not what is tested)
    b, v, p = numpy3(m._batch(idx, torch.from_numpy(sym.astype(np.uint8)).to(DEV)))
    for t in (b, v, p):
        assert not t[wrong].any()
    same((b[good], v[good], p[good]), permuted(maps[game], ident, index[good], sym[good]))
    assert m.bad() == 1 + 4  # the merge's malformed record, and each bad row exactly once
    # a rep outside the records counts as malformed too, and never becomes an address
    m.rep[2] = 67
    m.rep[4] = -5
    b, v, p = numpy3(m.batch())
    keep = np.array([g for g in range(9) if g not in (2, 4)])
    for t in (b, v, p):
        assert not t[[2, 4]].any()
    same((b[keep], v[keep], p[keep]), tuple(x[keep] for x in ident))
    assert m.bad() == 1 + 4 + 2
    with pytest.raises(IndexError):
        m.batch([9])
    with pytest.raises(ValueError):
        m.batch([0], sym=[nsym])


def test_real_selfplay_records():
    n_games = 64
    eng = _lib.Engine(C4, n_slots=n_games, sims_per_move=32, evaluator=_lib.EVAL_HASH, hash_salt=9, seed=4, max_games=n_games)
    rec = SP.play_to_end(eng, n_games, 4, 1.0, steps_below=64)["rec"].copy()
    ex = DeviceExamples.from_engine(eng, DEV)
    eng.close()
    assert len(ex) == len(rec) and ex.records.cpu().numpy().tobytes() == rec.tobytes()
    m = ex.merged()
    want = merge_records_host(C4, rec)
    MC.same_merge(arrays(m), want)
    assert len(m) < len(ex) and m.bad() == 0
    counts, group = m.counts().cpu().numpy(), m.group.cpu().numpy()
    assert rec["ply"][0] == 0 and counts[group[0]] == n_games  # the empty board, once per game
    print("real records: %d records, %d groups, largest groups %s" % (len(ex), len(m), np.sort(counts)[::-1][:5].tolist()))
    same(numpy3(m.batch()), identity_rows(C4, rec, want))


# ---- the front end: TrainWithDeviceExamples(merge=...) ---------------------------------------------------------------------------
def _model(game, name):
    return M.model(BOARD_CLS[game], name, seed=None, play_limit=8, eps=0, blocks=1)


def _same_weights(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert np.array_equal(a[k], b[k]), k


def _train_records(game):
    """30 records in 19 groups: merged, an epoch of two whole batches of 8; unmerged, of three"""
    pos = MC._positions(game, 19, 13)
    rec = MC.copies(game, pos, 30, 14)
    assert len(merge_records_host(game, rec)[1]) == 19
    return rec


@pytest.fixture
def repeatable_torch(tmp_path, monkeypatch):
    """Bit-for-bit comparisons between two runs of the PyTorch trainer: its switch for run-to-run repeatable convolutions, for
    the test only, and one untimed training call of the same shapes first (tests/test_gpu_examples_sym.py)."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)

    def warm(game):
        m = _model(game, "warm")
        Blackbird.TrainWithDeviceExamples(m, 8, 0.01, examples=DeviceExamples.from_records(game, _train_records(game), DEV))
        m.Conn.Close()
    return warm


@pytest.mark.parametrize("game", GAMES)
def test_merge_true_is_the_hand_written_loop(repeatable_torch, game):
    repeatable_torch(game)
    rec = _train_records(game)
    a, b, c = _model(game, "merge"), _model(game, "loop"), _model(game, "plain")
    _same_weights(a._weights, b._weights)
    np.random.seed(5)
    torch.manual_seed(5)
    Blackbird.TrainWithDeviceExamples(a, 8, 0.01, examples=DeviceExamples.from_records(game, rec, DEV), merge=True)
    merged = DeviceExamples.from_records(game, rec, DEV).merged()
    np.random.seed(5)
    torch.manual_seed(5)
    order = merged.index_tensor(epoch_order(len(merged), 8))
    assert len(merged) == 19 and len(order) == 16
    trainer = b._trainer_for(merged.info.C)
    for i in range(2):
        boards, value, policy = merged._batch(order[i * 8:(i + 1) * 8])
        trainer.step_tensors(boards, value, policy, 0.01)
    assert merged.bad() == 0 and a.batchCount == 2
    _same_weights(a._weights, trainer.export())
    # ... and merging did change what was trained on
    np.random.seed(5)
    torch.manual_seed(5)
    Blackbird.TrainWithDeviceExamples(c, 8, 0.01, examples=DeviceExamples.from_records(game, rec, DEV))
    assert c.batchCount == 3 and any(not np.array_equal(a._weights[k], c._weights[k]) for k in a._weights)
    for model in (a, b, c):
        model.Conn.Close()


def test_merge_with_augment_is_the_hand_written_loop(repeatable_torch):
    repeatable_torch(C4)
    rec = _train_records(C4)
    a, b = _model(C4, "both"), _model(C4, "loop")
    _same_weights(a._weights, b._weights)
    np.random.seed(6)
    torch.manual_seed(6)
    Blackbird.TrainWithDeviceExamples(a, 8, 0.01, examples=DeviceExamples.from_records(C4, rec, DEV), merge=True, augment=True)
    merged = DeviceExamples.from_records(C4, rec, DEV).merged()
    np.random.seed(6)
    torch.manual_seed(6)
    order = epoch_order(len(merged), 8)
    sym = np.random.randint(merged.symmetries, size=len(order))  # the same draw, right after the order
    assert sym.any() and not sym.all()
    trainer = b._trainer_for(merged.info.C)
    for i in range(2):
        boards, value, policy = merged.batch(order[i * 8:(i + 1) * 8], sym[i * 8:(i + 1) * 8])
        trainer.step_tensors(boards, value, policy, 0.01)
    _same_weights(a._weights, trainer.export())
    a.Conn.Close()
    b.Conn.Close()


def test_merge_false_trains_as_the_default_does(repeatable_torch):
    repeatable_torch(C4)
    rec = _train_records(C4)[:20]  # an epoch of two whole batches of 8
    a, b = _model(C4, "plain"), _model(C4, "off")
    w0 = {k: v.copy() for k, v in a._weights.items()}
    states = []
    for model, kw in ((a, {}), (b, {"merge": False})):
        np.random.seed(5)
        torch.manual_seed(5)
        Blackbird.TrainWithDeviceExamples(model, 8, 0.01, examples=DeviceExamples.from_records(C4, rec, DEV), **kw)
        states.append(np.random.get_state())
    assert a.batchCount == b.batchCount == 2
    _same_weights(a._weights, b._weights)
    assert any(not np.array_equal(a._weights[k], w0[k]) for k in w0)
    assert np.array_equal(states[0][1], states[1][1]) and states[0][2:] == states[1][2:]  # numpy's generator: consumed alike
    a.Conn.Close()
    b.Conn.Close()
