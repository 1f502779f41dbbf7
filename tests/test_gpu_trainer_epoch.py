"""-m gpu: a whole epoch of HIP training steps straight from example records (bb_trainer_epoch, csrc/train.hip.h's records
source; training.HipTrainer.epoch_records; Blackbird.TrainWithDeviceExamples on the hip backend).

The yardstick is the per-batch loop the epoch replaces -- DeviceExamples._batch (bb_examples_to_batch_sym) + step_tensors
(bb_trainer_step) --, and the comparison is exact: the records source hands the kernels the floats the batch tensors would have
held, in the same order, so parameters, both optimiser slots, the drawn noise and the four loss words are the same BITS.  One
batch per game is also held to the float64 statement of the training graph (tests/trainer_cases.py) on rows decoded on the
host, by that file's 1e-5 rule.  Shapes are the smallest at which the kernels can go wrong: batches of 1, 6 and 17 rows (17
crosses the 16-way strided sum of the label sum L), one and three batches, no tower blocks and two."""
import numpy as np
import pytest
import torch

from blackbird_amd import Blackbird, Connect4, TicTacToe, _lib
from blackbird_amd import weights as W
from blackbird_amd.training import DeviceExamples, HipTrainer, epoch_order
from tests import eval_cases as EC
from tests import merge_cases as MC
from tests import model_cases as M
from tests.merge_cases import C4, TTT
from tests.trainer_cases import ALPHA, EPS, close, close_live, statement

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMES = [C4, TTT]
BOARD_CLS = {C4: Connect4.BoardState, TTT: TicTacToe.BoardState}
LR = 1e-2

_records = {}


def records(game):
    """40 records along random legal games (terminal examples included), built once per game and left unchanged"""
    if game not in _records:
        rec = MC.playout_records(game, 40, 21)
        assert (rec["total"] == 0).any() and (rec["total"] > 0).any()
        _records[game] = rec
    return _records[game]


def _trainer(game, R, kind, seed=11, max_batch=17, w_seed=3):
    A = MC.SHAPE[game][3]
    w0 = W.init_weights(3, 16, R, 16, A, seed=w_seed, perturb=True)
    return HipTrainer(w0, alpha=ALPHA, epsilon=EPS, optimizer=kind, momentum=0.9, device=DEV, seed=seed, max_batch=max_batch), w0


def _state(tr, losses):
    """everything a step leaves behind, on the host"""
    return tr.export(), tr.slots(), tr.last_noise(), losses.cpu().numpy()


def _same_bits(a, b):
    assert a[3].shape == b[3].shape and np.array_equal(a[3], b[3]), ("losses", a[3], b[3])
    assert np.array_equal(a[2], b[2]), "noise"
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), ("parameters", k)
    for sa, sb, what in zip(a[1], b[1], "mv"):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), ("slot", what, k)


def _loop(tr, ex, order, sym, batch, noise=None):
    """the hand-written per-batch loop; returns the [n_batches, 4] losses"""
    out = []
    for i in range(int(order.numel()) // batch):
        rows = slice(i * batch, (i + 1) * batch)
        boards, value, policy = ex._batch(order[rows], None if sym is None else sym[rows])
        total, parts = tr.step_tensors(boards, value, policy, LR, noise=None if noise is None else noise[i])
        out.append(torch.stack([total] + parts))
    return torch.stack(out)


def _order_and_sym(ex, rows, with_sym, seed):
    rng = np.random.RandomState(seed)
    order = rng.randint(0, len(ex), rows)
    if rows > 1:
        order[-1] = order[0]                     # a repeat for certain; the draw is not sorted
    sym = rng.randint(0, ex.symmetries, rows) if with_sym else None
    if with_sym and rows > 1:
        sym[0], sym[-1] = 0, ex.symmetries - 1   # the repeated record under two orientations
    return ex.index_tensor(order), None if sym is None else ex.sym_tensor(sym)


# ---- 1. the same bits as the loop ------------------------------------------------------------------------------------------
CASES = [(C4, 2, "adam", 6, 3, True), (C4, 0, "momentum", 17, 1, False), (C4, 2, "sgd", 1, 3, True), (C4, 0, "adam", 17, 3, True),
         (C4, 2, "momentum", 6, 1, False), (C4, 0, "sgd", 6, 3, False), (TTT, 2, "adam", 17, 3, True),
         (TTT, 0, "momentum", 6, 3, True), (TTT, 2, "sgd", 17, 1, False), (TTT, 0, "adam", 1, 1, True),
         (TTT, 2, "momentum", 1, 3, False), (TTT, 0, "sgd", 6, 1, True)]


@pytest.mark.parametrize("game,R,kind,batch,n_batches,with_sym", CASES)
def test_epoch_is_the_per_batch_loop(game, R, kind, batch, n_batches, with_sym):
    ex = DeviceExamples.from_records(game, records(game), DEV)
    order, sym = _order_and_sym(ex, batch * n_batches, with_sym, 7 + batch)
    one, w0 = _trainer(game, R, kind)
    two, _w = _trainer(game, R, kind)
    losses = one.epoch_records(ex, order, batch, LR, sym=sym)
    assert tuple(losses.shape) == (n_batches, 4) and losses.device.type == "cuda"
    got, want = _state(one, losses), _state(two, _loop(two, ex, order, sym, batch))
    _same_bits(got, want)
    assert ex.bad() == 0 and np.isfinite(got[3]).all() and got[2].any()          # the noise was drawn
    assert any(not np.array_equal(got[0][k], w0[k]) for k in w0)                 # ... and the epoch trained
    one.close()
    two.close()


# ---- 2. malformed input: contained, counted, and equal to the loop over rows of zeros ------------------------------------------
@pytest.mark.parametrize("game", GAMES)
def test_malformed_rows_are_zero_rows_and_counted(game):
    """Nothing here can fault: every such value is checked on the device before it becomes an address (examples.hip.h), and the
    assertion is on the contained result -- the epoch equals bb_trainer_step on what bb_examples_to_batch_sym writes for the same
    rows, which is zeros for each of them."""
    gi = _lib.game_info(game)
    nsym = _lib.game_symmetries(game)
    rec = MC.copies(game, MC._positions(game, 5, 12), 12, 13, malformed=(3,))     # record 3 says n_children = S + 1
    ex = DeviceExamples.from_records(game, rec, DEV)
    batch, n_batches, n = 6, 2, 12
    order = np.array([0, 3, 5, len(rec), 7, 1, 2, -1, 9, 10, 11, 4], dtype=np.int64)
    sym = np.zeros(n, dtype=np.uint8)
    sym[2], sym[8], sym[10] = nsym - 1, 1, nsym                                     # row 10: not a symmetry of the game
    d_order, d_sym = torch.from_numpy(order).to(DEV), torch.from_numpy(sym).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    one, _w = _trainer(game, 2, "adam")
    two, _w = _trainer(game, 2, "adam")
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    losses = torch.zeros((n_batches, 4), dtype=torch.float32, device=DEV)
    _lib.trainer_epoch(one._h, len(rec), ex.records.data_ptr(), n_batches, batch, d_order.data_ptr(), d_sym.data_ptr(), None, LR,
                       losses.data_ptr(), bad.data_ptr(), stream)
    assert int(bad.item()) == 4
    # the loop over the batch tensors of the same rows
    boards = torch.full((n, gi.H, gi.W, gi.C), 7.0, dtype=torch.float32, device=DEV)
    value = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    policy = torch.full((n, gi.A), 7.0, dtype=torch.float32, device=DEV)
    bad2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.examples_to_batch_sym(game, len(rec), ex.records.data_ptr(), n, d_order.data_ptr(), d_sym.data_ptr(), boards.data_ptr(),
                               policy.data_ptr(), value.data_ptr(), bad2.data_ptr(), stream)
    assert int(bad2.item()) == 4
    for k in (1, 3, 7, 10):
        assert not boards[k].any() and not policy[k].any() and not value[k].any()
    losses2 = torch.zeros((n_batches, 4), dtype=torch.float32, device=DEV)
    for i in range(n_batches):
        rows = slice(i * batch, (i + 1) * batch)
        _lib.trainer_step(two._h, batch, boards[rows].data_ptr(), value[rows].data_ptr(), policy[rows].data_ptr(), None, LR, True,
                          losses2[i].data_ptr(), stream)
    _same_bits(_state(one, losses), _state(two, losses2))
    one.close()
    two.close()


# ---- 3. against the float64 statement ----------------------------------------------------------------------------------------
def _host_rows(game, rec):
    """(planes, value, policy) of records as the host forms them: bb_game_encode's planes, pi = visits / total in float64"""
    gi = _lib.game_info(game)
    st = np.ascontiguousarray(rec["state"]).view(_lib.STATE_DTYPE[game]).reshape(len(rec), -1)
    tot = rec["total"].astype(np.float64)
    pi = np.where(tot[:, None] > 0, rec["visits"][:, :gi.A].astype(np.float64) / np.maximum(tot, 1.0)[:, None], 0.0)
    return _lib.game_encode(game, st), rec["z"].astype(np.float64), pi


@pytest.mark.parametrize("all_terminal", [False, True], ids=["with the terminal example", "all terminal"])
@pytest.mark.parametrize("game", GAMES)
def test_one_batch_against_the_statement(game, all_terminal):
    rec = MC.stack(MC._positions(game, 6, 15, terminal_last=True), game)          # five live positions and a finished game
    rec["z"] = [1, -1, 0, 1, -1, 1]
    if all_terminal:                                                               # no visits anywhere: L = 0
        rec["visits"], rec["total"], rec["n_children"] = 0, 0, 0
    assert rec["total"][-1] == 0 and (rec["total"][:-1] > 0).all() != all_terminal
    ex = DeviceExamples.from_records(game, rec, DEV)
    tr, w0 = _trainer(game, 2, "sgd")
    A = MC.SHAPE[game][3]
    noise = np.random.RandomState(16).beta(ALPHA, 1 - ALPHA, size=(1, A)).astype(np.float32)
    losses = tr.epoch_records(ex, None, 6, LR, noise=noise).cpu().numpy()
    boards, ev, pl = _host_rows(game, rec)
    r_total, r_parts, r_grads = statement({k: np.asarray(v, dtype=np.float64) for k, v in w0.items()}, boards, ev, pl, noise[0], EPS)
    assert losses.shape == (1, 4) and np.array_equal(tr.last_noise(), noise[0]) and ex.bad() == 0
    close(losses[0, 0], r_total, (game, "loss"))
    for got, want, name in zip(losses[0, 1:], r_parts, ("lossEvaluation", "lossPolicy", "lossParam")):
        close(got, want, (game, name))
    if all_terminal:
        assert losses[0, 2] == 0.0
    grads = tr._named(_lib.TRAIN_GRADS)
    for k in r_grads:
        close(grads[k], r_grads[k], (game, "grad", k))
    tr.close()


def test_live_epoch_is_the_loop_and_its_first_step_the_statement():
    """Two batches at live inputs (tests/test_trainer_liveness_cpu.py: with the weights of the cases above the value head is
    saturated or its ReLUs are off): the epoch is the per-batch loop bit for bit, and the loop's first step is held to the float64
    statement per tensor within tol * max|data gradient| + 2**-23 * max|want|, tol = min(8 f, 1e-5), f the float32 statement's
    error on the CPU (tests/trainer_cases.py: float32_figure).  Measured on the MI355X: f 2.9e-6, the kernel 7.8e-7, tol 1e-5."""
    ref = EC.epoch_live_case()
    game, batch, noise = ref["game"], EC.EPOCH_LIVE_CASE[3], ref["noise"]
    ex = DeviceExamples.from_records(game, ref["rec"], DEV)
    order = ex.index_tensor(ref["order"])
    one, two = (HipTrainer(ref["w"], alpha=ALPHA, epsilon=EPS, optimizer="adam", momentum=0.9, device=DEV, seed=11, max_batch=17)
                for _k in range(2))
    losses = one.epoch_records(ex, order, batch, LR, noise=noise)
    out = []
    for i in range(2):
        boards, value, policy = ex._batch(order[i * batch:(i + 1) * batch], None)
        total, parts = two.step_tensors(boards, value, policy, LR, noise=torch.from_numpy(noise[i]).to(DEV))
        out.append(torch.stack([total] + parts))
        if i == 0:
            assert np.array_equal(boards.cpu().numpy(), ref["rows"][0]) and np.array_equal(value.cpu().numpy(), ref["rows"][1])
            grads = two._named(_lib.TRAIN_GRADS)
    _same_bits(_state(one, losses), _state(two, torch.stack(out)))
    assert ex.bad() == 0 and np.array_equal(one.last_noise(), noise[1])
    r_total, r_parts, r_grads, r_data, _live = ref["want"]
    first = out[0].cpu().numpy()
    close(first[0], r_total, "loss")
    for got, want, name in zip(first[1:], r_parts, ("lossEvaluation", "lossPolicy", "lossParam")):
        close(got, want, name)
    worst = 0.0
    for k in r_grads:
        close(grads[k], r_grads[k], ("grad", k))
        worst = max(worst, close_live(grads[k], r_grads[k], float(np.abs(r_data[k]).max()), ref["tol"], ("live grad", k)))
    print("float32 statement %.3g kernel %.3g tolerance %.3g" % (ref["figure"], worst, ref["tol"]))
    one.close()
    two.close()


# ---- 4. repeatability ----------------------------------------------------------------------------------------------------------
def test_the_same_epoch_twice_gives_the_same_bits():
    ex = DeviceExamples.from_records(C4, records(C4), DEV)
    order, sym = _order_and_sym(ex, 3 * 17, True, 31)
    runs = []
    for _run in range(2):
        tr, _w = _trainer(C4, 2, "adam", seed=21)
        runs.append(_state(tr, tr.epoch_records(ex, order, 17, LR, sym=sym)))
        tr.close()
    _same_bits(*runs)
    assert not np.array_equal(runs[0][3][0], runs[0][3][1])


# ---- 5. the front end --------------------------------------------------------------------------------------------------------
def _hip_model(game, name):
    cfg = M.net_config(1, 0.3)
    cfg["training"]["backend"] = "hip"
    return Blackbird.Model(BOARD_CLS[game], name, {"explorationRate": 0.85, "playLimit": 8}, cfg)


@pytest.fixture
def epoch_calls(monkeypatch):
    """how often HipTrainer.epoch_records ran"""
    calls, real = [], HipTrainer.epoch_records

    def counted(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)

    monkeypatch.setattr(HipTrainer, "epoch_records", counted)
    return calls


def test_train_with_device_examples_is_the_hand_written_loop(tmp_path, monkeypatch, epoch_calls):
    monkeypatch.chdir(tmp_path)
    np.random.seed(31)
    play = _hip_model(C4, "play")
    play.KeepDeviceExamples = True
    Blackbird.GenerateTrainingSamples(play, 8, 1.0)
    kept = play.KeptDeviceExamples()
    assert len(kept) >= 40
    records_40 = kept.records[:40].clone()                                          # an epoch of five whole batches of 8
    w0 = {k: v.copy() for k, v in play._weights.items()}
    for augment in (False, True):
        a, b = _hip_model(C4, "epoch%d" % augment), _hip_model(C4, "loop%d" % augment)
        for m in (a, b):
            m._weights = {k: v.copy() for k, v in w0.items()}
        version = a.Version
        np.random.seed(5)
        Blackbird.TrainWithDeviceExamples(a, 8, LR, examples=DeviceExamples(C4, records_40), augment=augment, fused=True)
        after = np.random.get_state()
        assert len(epoch_calls) == 1 + augment and type(a._trainer) is HipTrainer
        assert a.Version == version + 1 and a.batchCount == 5
        ex = DeviceExamples(C4, records_40)
        np.random.seed(5)
        order = ex.index_tensor(epoch_order(len(ex), 8))
        sym = ex.sym_tensor(np.random.randint(ex.symmetries, size=len(order))) if augment else None
        trainer = b._trainer_for(ex.info.C)                                        # (its noise seed comes from numpy's generator)
        _loop(trainer, ex, order, sym, 8)
        mine = np.random.get_state()
        assert np.array_equal(after[1], mine[1]) and after[2:] == mine[2:]         # numpy's generator: consumed alike
        want = trainer.export()
        assert sorted(a._weights) == sorted(want)
        for k in want:
            assert np.array_equal(a._weights[k], want[k]), (augment, k)
        assert any(not np.array_equal(want[k], w0[k]) for k in w0)
        for m in (a, b):
            m.Conn.Close()
    # merge=True still trains, through the per-batch loop, and so does a call that does not ask for the epoch (fused is opt-in:
    # it measured no faster than the loop, README)
    for name, kw in (("merged", dict(merge=True, fused=True)), ("default", {})):
        c = _hip_model(C4, name)
        c._weights = {k: v.copy() for k, v in w0.items()}
        np.random.seed(5)
        Blackbird.TrainWithDeviceExamples(c, 8, LR, examples=DeviceExamples(C4, records_40), **kw)
        assert len(epoch_calls) == 2 and c.batchCount >= 1 and any(not np.array_equal(c._weights[k], w0[k]) for k in w0)
        c.Conn.Close()
    play._batch_engine.close()
    play.Conn.Close()


# ---- 6. argument errors ------------------------------------------------------------------------------------------------------
def test_epoch_arguments():
    ex = DeviceExamples.from_records(C4, records(C4), DEV)
    tr, w0 = _trainer(C4, 0, "sgd", max_batch=8)
    order = ex.index_tensor(np.arange(16))
    with pytest.raises(ValueError, match="DeviceExamples"):
        tr.epoch_records(ex.merged(), order, 8, LR)
    with pytest.raises(ValueError, match="game"):
        tr.epoch_records(DeviceExamples.from_records(TTT, records(TTT), DEV), order, 8, LR)
    with pytest.raises(ValueError, match="max_batch"):
        tr.epoch_records(ex, order[:9], 9, LR)
    with pytest.raises(ValueError):
        tr.epoch_records(DeviceExamples.from_records(C4, records(C4), "cpu"), order.cpu(), 8, LR)
    with pytest.raises(ValueError):
        tr.epoch_records(ex, order[:12], 8, LR)                                    # no whole number of batches
    with pytest.raises(ValueError):
        tr.epoch_records(ex, order, 8, LR, sym=torch.zeros(3, dtype=torch.uint8, device=DEV))
    raw = dict(h=tr._h, n_records=len(ex), records=ex.records.data_ptr(), n_batches=2, batch=8, order=order.data_ptr(), lr=LR)
    for wrong in (dict(n_batches=-1), dict(batch=0), dict(batch=9), dict(n_records=-1), dict(records=None),
                  dict(records=ex.records.data_ptr() + 8), dict(lr=float("inf")), dict(order=order.data_ptr() + 4)):
        with pytest.raises(ValueError):
            _lib.trainer_epoch(**{**raw, **wrong})
    empty = tr.epoch_records(ex, order[:0], 8, LR)                                  # an empty epoch
    assert tuple(empty.shape) == (0, 4)
    _lib.trainer_epoch(**{**raw, "n_batches": 0, "records": None})
    after = tr.export()
    for k in w0:
        assert np.array_equal(after[k], w0[k]), k
    assert ex.bad() == 0
    tr.close()
