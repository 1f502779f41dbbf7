"""-m gpu: training batches in another orientation, formed on the device (bb_examples_to_batch_sym, csrc/examples.hip.h).

The statement is "the identity batch, cells and actions permuted by the maps of csrc/symmetry.h" -- the maps as
tests/test_symmetry_cpu.py prints and checks them on the CPU -- and every comparison is exact: nothing here rounds differently
from the kernel without a symmetry.  Records are real self-play records of the hash evaluator, the terminal examples included.
The same rows are held against the rules on the device as well (the position rebuilt by bb_game_apply from the mapped moves of
the record's game), so the kernel's planes and policy belong to a position the game can reach, whatever the test's numpy says."""
import numpy as np
import pytest
import torch

from blackbird_amd import Blackbird, Connect4, TicTacToe, _lib
from blackbird_amd.training import DeviceExamples, epoch_order
from tests import model_cases as M
from tests import selfplay_cases as SP
from tests.host_cases import maps  # noqa: F401  (a fixture: the header's maps from the stand-alone program)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
SELFPLAY = {C4: dict(n_games=32, sims=8), TTT: dict(n_games=32, sims=8), DC: dict(n_games=2, sims=8, max_plies=6)}
BOARD_CLS = {C4: Connect4.BoardState, TTT: TicTacToe.BoardState}

_played = {}


def played(game):
    """One finished self-play run per game, shared by the tests and left unchanged: (host records, game offsets, device
    examples, the identity batch through the OLD entry point as numpy (boards, value, policy))."""
    if game not in _played:
        cfg = SELFPLAY[game]
        eng = _lib.Engine(game, n_slots=cfg["n_games"], sims_per_move=cfg["sims"], evaluator=_lib.EVAL_HASH, hash_salt=9, seed=4,
                          max_games=cfg["n_games"], max_plies=cfg.get("max_plies"))
        out = SP.play_to_end(eng, cfg["n_games"], 4, 1.0, steps_below=64)
        rec, offs = out["rec"].copy(), out["offs"].copy()
        eng.close()
        ex = DeviceExamples.from_records(game, rec, DEV)
        assert (rec["total"] == 0).sum() == cfg["n_games"] and (rec["total"] > 0).any()  # the terminal examples are there
        _played[game] = (rec, offs, ex, old_entry_point(game, ex))
    return _played[game]


def _outputs(game, n, fill=7.0):
    gi = _lib.game_info(game)
    return (torch.full((n, gi.H, gi.W, gi.C), fill, dtype=torch.float32, device=DEV),
            torch.full((n,), fill, dtype=torch.float32, device=DEV),
            torch.full((n, gi.A), fill, dtype=torch.float32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))


def old_entry_point(game, ex, index=None):
    """(boards, value, policy, bad) of bb_examples_to_batch, as numpy"""
    n = len(ex) if index is None else len(index)
    idx = None if index is None else torch.from_numpy(np.asarray(index, dtype=np.int64)).to(DEV)
    b, v, p, bad = _outputs(game, n)
    _lib.examples_to_batch(game, len(ex), ex.records.data_ptr(), n, None if idx is None else idx.data_ptr(), b.data_ptr(),
                           p.data_ptr(), v.data_ptr(), bad.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return b.cpu().numpy(), v.cpu().numpy(), p.cpu().numpy(), int(bad.item())


def new_entry_point(game, ex, index, sym, boards=True, value=True, policy=True):
    """(boards, value, policy, bad) of bb_examples_to_batch_sym, as numpy; an output switched off is passed as NULL and comes
    back as the untouched fill"""
    n = len(ex) if index is None else len(index)
    idx = None if index is None else torch.from_numpy(np.asarray(index, dtype=np.int64)).to(DEV)
    s = None if sym is None else torch.from_numpy(np.asarray(sym, dtype=np.uint8)).to(DEV)
    b, v, p, bad = _outputs(game, n)
    _lib.examples_to_batch_sym(game, len(ex), ex.records.data_ptr(), n, None if idx is None else idx.data_ptr(),
                               None if s is None else s.data_ptr(), b.data_ptr() if boards else None,
                               p.data_ptr() if policy else None, v.data_ptr() if value else None, bad.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    return b.cpu().numpy(), v.cpu().numpy(), p.cpu().numpy(), int(bad.item())


def statement(m, ident, index, sym):
    """the identity batch `ident` (every record, in order), rows `index`, cells and actions permuted by the maps m"""
    ib, iv, ip = ident[:3]
    n = len(index)
    boards, policy = np.empty((n,) + ib.shape[1:], np.float32), np.empty((n,) + ip.shape[1:], np.float32)
    H, W, C = ib.shape[1:]
    for k, (r, s) in enumerate(zip(index, sym)):
        cells = np.empty((H * W, C), np.float32)
        cells[m["cell"][s]] = ib[r].reshape(H * W, C)
        boards[k] = cells.reshape(H, W, C)
        policy[k, m["action"][s]] = ip[r]
    return boards, iv[np.asarray(index)], policy


def same(got, want):
    for g, w, what in zip(got, want, ("boards", "value", "policy")):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, int((g != w).sum()))


@pytest.mark.parametrize("game", [C4, TTT, DC])
def test_no_symmetry_and_all_zero_reproduce_the_old_entry_point(game):
    rec, _offs, ex, ident = played(game)
    n = len(rec)
    assert ident[3] == 0 and ident[2].any() and ident[0].any()
    for sym in (None, np.zeros(n, dtype=np.uint8)):
        got = new_entry_point(game, ex, None, sym)
        same(got, ident)
        assert got[3] == 0
    idx = np.random.RandomState(2).randint(0, n, 37)
    want = old_entry_point(game, ex, idx)
    for sym in (None, np.zeros(37, dtype=np.uint8)):
        got = new_entry_point(game, ex, idx, sym)
        same(got, want)
        assert got[3] == want[3] == 0
    # the front end: batch() with and without sym
    for sym in (None, np.zeros(37, dtype=np.uint8), torch.zeros(37, dtype=torch.uint8, device=DEV)):
        b, v, p = ex.batch(idx, sym=sym)
        same((b.cpu().numpy(), v.cpu().numpy(), p.cpu().numpy()), want)
    assert ex.bad() == 0 and ex.symmetries == {C4: 2, TTT: 8, DC: 1}[game]


def _cases(n_rec, nsym):
    """(index, sym): n = 1, 5 and 67 rows -- a Connect4 row is 134 floats and a TicTacToe row 37, so rows straddle 256-thread
    blocks and waves --, the index out of order and with repeats, neighbouring rows under different symmetries, every symmetry
    at every n"""
    rng = np.random.RandomState(6)
    out = []
    for s in range(nsym):
        out.append((np.array([n_rec - 1 - s]), np.array([s])))
        idx = rng.randint(0, n_rec, 5)
        idx[3] = idx[0]
        out.append((idx, (np.arange(5) * (nsym - 1) + s) % nsym))
    idx = rng.randint(0, n_rec, 67)
    idx[40:45] = idx[11]
    out.append((idx, (np.arange(67) + 1) % nsym))
    out.append((idx[::-1].copy(), (np.arange(67) * 3 + 2) % nsym))
    return out


@pytest.mark.parametrize("game", [C4, TTT])
def test_every_symmetry_against_the_statement(maps, game):  # noqa: F811
    rec, _offs, ex, ident = played(game)
    m = maps[game]
    seen = set()
    for idx, sym in _cases(len(rec), m["nsym"]):
        assert len(idx) == 1 or ((np.diff(sym) != 0).all() and len(set(idx)) < len(idx) and (np.diff(idx) < 0).any())
        got = new_entry_point(game, ex, idx, sym)
        same(got, statement(m, ident, idx, sym))
        assert got[3] == 0
        b, v, p = ex.batch(idx, sym=sym)  # and through the front end
        same((b.cpu().numpy(), v.cpu().numpy(), p.cpu().numpy()), got)
        seen |= {(len(idx), int(s)) for s in sym}
    assert seen == {(n, s) for n in (1, 5, 67) for s in range(m["nsym"])}
    # the statement is not the identity: a mirrored row differs from the row as played somewhere
    idx = np.arange(len(rec))
    flipped = new_entry_point(game, ex, idx, np.full(len(rec), m["nsym"] - 1))
    assert (flipped[0] != ident[0]).any() and (flipped[2] != ident[2]).any() and np.array_equal(flipped[1], ident[1])
    assert ex.bad() == 0


def _moves(game, rec, offs):
    """[moves of game g]: the action between consecutive records of a game, read off the stone that appeared"""
    gi = _lib.game_info(game)
    st = np.ascontiguousarray(rec["state"]).view(_lib.STATE_DTYPE[game]).reshape(len(rec), -1)
    occ = _lib.unpack_grid(game, st)[0].sum(axis=-1)
    out = []
    for g in range(len(offs) - 1):
        o = occ[offs[g]:offs[g + 1]]
        new = (o[1:] - o[:-1]).reshape(len(o) - 1, -1)
        assert (new.sum(axis=1) == 1).all() and (new >= 0).all()
        cell = new.argmax(axis=1)
        out.append(cell % gi.W if game == C4 else cell)
    return out


@pytest.mark.parametrize("game", [C4, TTT])
def test_against_the_rules_on_the_device(maps, game):  # noqa: F811
    rec, offs, ex, ident = played(game)
    m = maps[game]
    nsym, n_games, n_rec = m["nsym"], len(offs) - 1, len(rec)
    moves = _moves(game, rec, offs)
    # rebuilt[s][k]: the position of record k under symmetry s, played from the start by the mapped moves of its game
    cur = np.repeat(_lib.game_initial(game), nsym * n_games, axis=0).reshape(nsym, n_games, -1)
    rebuilt = np.zeros((nsym, n_rec, cur.shape[-1]), dtype=cur.dtype)
    for ply in range(max(len(mv) for mv in moves) + 1):
        live = [g for g in range(n_games) if ply <= len(moves[g])]
        for g in live:
            rebuilt[:, offs[g] + ply] = cur[:, g]
        go = [g for g in live if ply < len(moves[g])]
        if go:
            acts = np.array([[m["action"][s][moves[g][ply]] for g in go] for s in range(nsym)], dtype=np.int32)
            nxt, status = _lib.game_apply(game, cur[:, go].reshape(nsym * len(go), -1), acts.reshape(-1))
            assert not status.any()
            cur[:, go] = nxt.reshape(nsym, len(go), -1)
    st = np.ascontiguousarray(rec["state"]).view(_lib.STATE_DTYPE[game]).reshape(n_rec, -1)
    cells = np.uint64(0x00FFFFFFFFFFFFFF)
    assert np.array_equal(rebuilt[0] & cells, st & cells)  # the moves were read correctly: the identity rebuilds the records
    for s in range(nsym):
        b, _v, p, bad = new_entry_point(game, ex, None, np.full(n_rec, s))
        assert bad == 0
        assert np.array_equal(b, _lib.game_encode(game, rebuilt[s]).astype(np.float32)), s
        legal = _lib.game_legal(game, rebuilt[s])
        assert not p[legal == 0].any() and p.any(), s


@pytest.mark.parametrize("game", [C4, TTT])
def test_null_outputs(maps, game):  # noqa: F811
    rec, _offs, ex, _ident = played(game)
    nsym = maps[game]["nsym"]
    rng = np.random.RandomState(8)
    idx, sym = rng.randint(0, len(rec), 21), rng.randint(0, nsym, 21)
    full = new_entry_point(game, ex, idx, sym)
    assert np.unique(sym).size > 1
    for off in range(3):
        keep = [k != off for k in range(3)]
        got = new_entry_point(game, ex, idx, sym, boards=keep[0], value=keep[1], policy=keep[2])
        for k in range(3):
            assert np.array_equal(got[k], full[k]) if keep[k] else (got[k] == 7.0).all(), (off, k)
    with pytest.raises(ValueError):
        new_entry_point(game, ex, idx, sym, boards=False, value=False, policy=False)


@pytest.mark.parametrize("game", [C4, TTT, DC])
def test_a_symmetry_the_game_does_not_have_is_a_bad_row(maps, game):  # noqa: F811
    rec, _offs, ex, ident = played(game)
    m = maps[game]
    nsym, n = m["nsym"], 9
    idx = np.array([3, 0, 5, 5, 1, 2, 4, 0, 3])
    sym = (np.arange(n) + 1) % nsym
    sym[[2, 6]] = nsym, 255
    good = np.array([k for k in range(n) if k not in (2, 6)])
    b, v, p, bad = new_entry_point(game, ex, idx, sym)
    assert bad == 2  # each bad row counts exactly once
    for t in (b, v, p):
        assert not t[[2, 6]].any()
    if game == DC:
        want = [ident[k][idx[good]] for k in range(3)]
    else:
        want = statement(m, ident, idx[good], sym[good])
    same((b[good], v[good], p[good]), want)
    # the front end leaves a device tensor to the kernel and reports it in bad(); a host array it refuses itself
    mine = DeviceExamples(game, ex.records)
    tb, tv, tp = mine.batch(idx, sym=torch.from_numpy(sym.astype(np.uint8)).to(DEV))
    same((tb.cpu().numpy(), tv.cpu().numpy(), tp.cpu().numpy()), (b, v, p))
    assert mine.bad() == 2
    with pytest.raises(ValueError):
        mine.batch(idx, sym=sym)
    assert mine.bad() == 2


def test_dragonchess_all_zero_is_the_old_entry_point_and_one_is_bad():
    rec, _offs, ex, ident = played(DC)
    n = min(len(rec), 6)
    idx = np.arange(n)[::-1].copy()
    want = old_entry_point(DC, ex, idx)
    got = new_entry_point(DC, ex, idx, np.zeros(n, dtype=np.uint8))
    same(got, want)
    assert got[3] == 0 and want[2].any()
    sym = np.zeros(n, dtype=np.uint8)
    sym[1] = 1
    got = new_entry_point(DC, ex, idx, sym)
    assert got[3] == 1
    keep = np.arange(n) != 1
    for g, w in zip(got[:3], want[:3]):
        assert not g[1].any() and np.array_equal(g[keep], w[keep])


# ---- the front end: TrainWithDeviceExamples(augment=...) ----------------------------------------------------------------
def _model(game, name):
    return M.model(BOARD_CLS[game], name, seed=None, play_limit=8, eps=0, blocks=1)


def _same_weights(a, b):
    assert sorted(a) == sorted(b)
    worst = max((float(np.max(np.abs(a[k].astype(np.float64) - b[k]))), k) for k in sorted(a))
    print("largest difference between the two sets of weights: %.3g at %s" % worst)
    for k in sorted(a):
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture
def repeatable_torch(tmp_path, monkeypatch):
    """The comparisons below are bit for bit between two runs of the PyTorch trainer, so its convolutions must be run-to-run
    repeatable: PyTorch's own switch for that, for the test only, and one untimed training call of the same shapes first, so
    that neither compared run is the process's first meeting with a convolution shape (when the library picks its kernels)."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)

    def warm(game):
        m = _model(game, "warm")
        Blackbird.TrainWithDeviceExamples(m, 16, 0.01, examples=DeviceExamples.from_records(game, played(game)[0][:40], DEV))
        m.Conn.Close()
    return warm


def test_augment_false_trains_as_the_default_does(repeatable_torch):
    repeatable_torch(C4)
    rec = played(C4)[0][:40]  # 40 examples: an epoch of two whole batches of 16
    a, b = _model(C4, "plain"), _model(C4, "off")
    _same_weights(a._weights, b._weights)
    w0 = {k: v.copy() for k, v in a._weights.items()}
    states = []
    for model, kw in ((a, {}), (b, {"augment": False})):
        np.random.seed(5)
        torch.manual_seed(5)
        Blackbird.TrainWithDeviceExamples(model, 16, 0.01, examples=DeviceExamples.from_records(C4, rec, DEV), **kw)
        states.append(np.random.get_state())
    assert a.batchCount == b.batchCount == 2
    _same_weights(a._weights, b._weights)
    assert any(not np.array_equal(a._weights[k], w0[k]) for k in w0)
    assert np.array_equal(states[0][1], states[1][1]) and states[0][2:] == states[1][2:]  # numpy's generator: consumed alike
    a.Conn.Close()
    b.Conn.Close()


@pytest.mark.parametrize("game", [C4, TTT])
def test_augment_true_is_the_hand_written_loop(repeatable_torch, game):
    repeatable_torch(game)
    rec = played(game)[0][:40]
    nsym = _lib.game_symmetries(game)
    a, b, c = _model(game, "aug"), _model(game, "loop"), _model(game, "plain")
    _same_weights(a._weights, b._weights)
    np.random.seed(5)
    torch.manual_seed(5)
    Blackbird.TrainWithDeviceExamples(a, 16, 0.01, examples=DeviceExamples.from_records(game, rec, DEV), augment=True)
    # by hand: the same two draws, then batch(index, sym) and step_tensors
    ex = DeviceExamples.from_records(game, rec, DEV)
    np.random.seed(5)
    torch.manual_seed(5)
    order = epoch_order(len(rec), 16)
    sym = np.random.randint(nsym, size=len(order))
    assert len(order) == 32 and sym.any() and sym.max() < nsym  # not all zero: the case cannot pass vacuously
    trainer = b._trainer_for(ex.info.C)
    for i in range(2):
        boards, value, policy = ex.batch(order[i * 16:(i + 1) * 16], sym[i * 16:(i + 1) * 16])
        trainer.step_tensors(boards, value, policy, 0.01)
    assert ex.bad() == 0 and a.batchCount == 2
    _same_weights(a._weights, trainer.export())
    # ... and augmenting did change what was trained on
    np.random.seed(5)
    torch.manual_seed(5)
    Blackbird.TrainWithDeviceExamples(c, 16, 0.01, examples=DeviceExamples.from_records(game, rec, DEV))
    assert any(not np.array_equal(a._weights[k], c._weights[k]) for k in a._weights)
    for model in (a, b, c):
        model.Conn.Close()
