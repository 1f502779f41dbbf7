"""-m gpu: scoring example records with the trainer's device parameters (bb_trainer_eval / bb_trainer_eval_tensors,
csrc/train_eval.hip.h; training.HipTrainer.evaluate_records / evaluate_tensors; Blackbird.EvaluateDeviceExamples).

The yardstick is the float64 statement of tests/eval_cases.py under the `close` rule of tests/trainer_cases.py (1e-5 relative to
max(1, largest |entry|)); the two sources of the kernel are held to each other bit for bit.  Shapes are the smallest at which the
kernel can go wrong: no tower block, one, two and nine (the two activation buffers change roles per layer), dense widths 1, 16
and 64, and row counts 0, 1, 2, 3, 4, 5 and 130: none, the one row a workgroup takes, and more than one workgroup."""
import numpy as np
import pytest
import torch

from blackbird_amd import Blackbird, Connect4, TicTacToe, _lib
from blackbird_amd import weights as W
from blackbird_amd.training import DeviceExamples, HipTrainer, Trainer
from tests import eval_cases as EC
from tests import merge_cases as MC
from tests import model_cases as M
from tests.merge_cases import C4, TTT
from tests.trainer_cases import ALPHA, EPS, close, close_live

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAME = {"connect4": C4, "tictactoe": TTT}
BOARD_CLS = {C4: Connect4.BoardState, TTT: TicTacToe.BoardState}
LR = 1e-2
SUMS = ("se_sum", "ce_sum")
MEANS = ("value_mse", "policy_ce", "top1_rate", "sign_rate")


def _trainer(game, R, D=16, eps=EPS, kind="adam", seed=11, max_batch=17, w_seed=3):
    A = MC.SHAPE[game][3]
    w0 = W.init_weights(3, 16, R, D, A, seed=w_seed, perturb=True)
    return HipTrainer(w0, alpha=ALPHA, epsilon=eps, optimizer=kind, momentum=0.9, device=DEV, seed=seed, max_batch=max_batch), w0


def _examples(game):
    return DeviceExamples.from_records(game, EC.records(game), DEV)


_index = EC.index      # n record numbers: the tied-visits record, a terminal example, then the others; None for all 130


def _decoded(ex, index=None, sym=None):
    """the rows as bb_examples_to_batch_sym writes them (tests/test_gpu_device_examples.py holds those to the host), in float64"""
    return tuple(t.cpu().numpy().astype(np.float64) for t in ex._batch(index, sym))


def _check(got, want, what):
    """one evaluation (rows=True) against the statement: per-row figures, flags where the statement has room, totals"""
    n = len(want["rows"])
    per_row, flags = got["per_row"].cpu().numpy(), got["flags"].cpu().numpy()
    assert per_row.shape == (n, 3) and flags.shape == (n,)
    if n:
        close(per_row, want["rows"], (what, "rows"))
    has, top1, decided, sign_ok, counted = EC.bits(flags)
    assert counted.all() and np.array_equal(has, want["has"]) and np.array_equal(decided, want["decided"])
    assert not top1[~has].any() and not sign_ok[~decided].any() and (per_row[~has, 2] == 0).all()
    top1_room, sign_room = want["has"] & want["top1_room"], want["decided"] & want["sign_room"]
    out1, out3 = int((want["has"] & ~want["top1_room"]).sum()), int((want["decided"] & ~want["sign_room"]).sum())
    print(what, "rows left out of the flag comparison: bit 1 %d, bit 3 %d of %d" % (out1, out3, n))
    assert out1 <= 0.1 * n and out3 <= 0.1 * n
    assert np.array_equal(top1[top1_room], want["top1"][top1_room]) and np.array_equal(sign_ok[sign_room], want["sign_ok"][sign_room])
    tot = want["totals"]
    for k in ("rows", "policy_rows", "decided"):
        assert got[k] == tot[k], (what, k)
    assert got["top1"] == int(top1.sum()) and abs(got["top1"] - tot["top1"]) <= out1
    assert got["sign_ok"] == int(sign_ok.sum()) and abs(got["sign_ok"] - tot["sign_ok"]) <= out3
    for k in SUMS:
        close(got[k], tot[k], (what, k))
    if tot["rows"]:
        close(got["value_mse"], tot["se_sum"] / tot["rows"], (what, "value_mse"))
    if tot["policy_rows"]:
        close(got["policy_ce"], tot["ce_sum"] / tot["policy_rows"], (what, "policy_ce"))
        assert got["top1_rate"] == got["top1"] / got["policy_rows"]
    if tot["decided"]:
        assert got["sign_rate"] == got["sign_ok"] / got["decided"]


def _same(a, b):
    """two evaluations (rows=True), bit for bit"""
    assert torch.equal(a["per_row"], b["per_row"]) and torch.equal(a["flags"], b["flags"])
    for k in EC.COUNTS + SUMS:
        assert a[k] == b[k], k


# ---- 1. against the float64 statement ----------------------------------------------------------------------------------------------
CASES = [("connect4", 0, 16, 2), ("connect4", 0, 16, 3), ("connect4", 9, 64, 2), ("connect4", 9, 64, 130),
         ("connect4", 1, 1, 1), ("connect4", 1, 1, 5), ("connect4", 1, 1, 130), ("tictactoe", 2, 16, 1), ("tictactoe", 2, 16, 0),
         ("tictactoe", 9, 64, 1), ("tictactoe", 9, 64, 2), ("tictactoe", 9, 64, 4), ("tictactoe", 2, 16, 130)]


@pytest.mark.parametrize("name,R,D,n", CASES)
def test_rows_and_totals_against_the_statement(name, R, D, n):
    game = GAME[name]
    ex = _examples(game)
    index = _index(game, n)
    idx = None if index is None else ex.index_tensor(index)
    tr, w0 = _trainer(game, R, D)
    got = tr.evaluate_records(ex, idx, rows=True)
    want = EC.statement(w0, *_decoded(ex, idx))
    assert len(want["rows"]) == n
    if n >= 2:   # the tied-visits record and a terminal example are among the rows: the first maximum, and a row without a label
        rec = EC.records(game)[[1] if index is None else index[:1]]
        A = MC.SHAPE[game][3]
        assert (rec["visits"][0, :A] == rec["visits"][0, :A].max()).sum() == 2 and not want["has"].all() and want["has"].any()
    _check(got, want, (name, R, D, n))
    assert ex.bad() == 0
    tr.close()


# ---- 1b. at live inputs, column by column -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EC.LIVE_CASES, ids=str)
def test_live_rows_against_the_statement(case):
    """At the weights of CASES the Connect4 value head saturates (value +-1, se in {0, 1, 4}) and the three columns are compared
    jointly at the scale of the largest cross entropy.  Here the rows are live (tests/test_trainer_liveness_cpu.py) and value, se
    and ce are each held to tol * max|column| + 2**-23 * max|column|, tol = min(8 f, 1e-5), f the error of that column of the same
    statement evaluated in float32 on the CPU, relative to the column's largest |entry|.
    Measured on the MI355X, f / the kernel's error in the same measure / tol, for value, se, ce:
      connect4 R0 D1 n1      1.3e-7/5.3e-7/1.0e-6   4.7e-8/4.4e-7/3.7e-7   7.5e-8/7.5e-8/6.0e-7
      connect4 R9 D64 n1     9.9e-9/7.8e-8/8.0e-8   5.6e-8/5.6e-8/4.4e-7   9.0e-8/8.6e-8/7.2e-7
      connect4 R2 D1 n2      1.3e-7/1.6e-7/1.0e-6   1.9e-7/1.0e-7/1.5e-6   7.1e-8/1.4e-7/5.6e-7
      tictactoe R2 D64 n2    5.4e-7/6.4e-8/4.4e-6   1.6e-6/2.2e-7/1e-5     8.9e-8/3.5e-8/7.1e-7
      tictactoe R9 D1 n2     1.3e-6/2.1e-7/1e-5     5.5e-7/8.8e-8/4.4e-6   2.3e-8/4.2e-8/1.8e-7
      tictactoe R0 D64 n130  6.4e-7/5.3e-7/5.1e-6   4.5e-7/4.2e-7/3.6e-6   1.7e-7/1.2e-7/1.4e-6
    With one row f is the rounding of a single number (9.9e-9 is a sixth of a unit in the last place), so there the bound is
    mostly its 2**-23 term: se of connect4 R0 D1 n1 is at 4.4e-7 against 3.7e-7 + 1.2e-7."""
    _name, _R, _D, n, _ws = case
    ref = EC.live_case(case)
    ex = _examples(ref["game"])
    idx = None if ref["index"] is None else ex.index_tensor(ref["index"])
    tr = HipTrainer(ref["w"], alpha=ALPHA, epsilon=EPS, optimizer="adam", momentum=0.9, device=DEV, seed=11, max_batch=17)
    got = tr.evaluate_records(ex, idx, rows=True)
    rows = _decoded(ex, idx)
    assert np.array_equal(rows[0], ref["rows"][0]) and np.array_equal(rows[1], ref["rows"][1])   # the rows the host decoded
    want = EC.statement(ref["w"], *rows)
    assert len(want["rows"]) == n
    _check(got, want, case)                                                                       # the joint rule still holds
    per_row = got["per_row"].cpu().numpy()
    for c, column in enumerate(EC.COLUMNS):
        scale = float(np.abs(want["rows"][:, c]).max())
        rel = close_live(per_row[:, c], want["rows"][:, c], scale, ref["tol"][c], (case, column))
        print(case, column, "float32 statement %.3g kernel %.3g tolerance %.3g" % (ref["figure"][c], rel, ref["tol"][c]))
    assert (np.abs(per_row[:, 0]) < 0.95).any() and (np.abs(want["rows"][:, 0]) < 0.95).any()    # not the saturated +-1
    assert ex.bad() == 0
    tr.close()


# ---- 2. the two sources, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,R", [("connect4", 2), ("tictactoe", 1)])
def test_records_and_tensors_give_the_same_bits(name, R):
    game = GAME[name]
    ex = _examples(game)
    rng = np.random.RandomState(8)
    nsym = ex.symmetries
    assert nsym == {C4: 2, TTT: 8}[game]
    order = np.concatenate([rng.permutation(len(ex)), rng.randint(0, len(ex), 31), [5, 5, 5]])      # a permutation, and repeats
    sym = np.concatenate([np.arange(len(order) - 3) % nsym, [0, nsym - 1, 1]])                       # every orientation
    index, syms = ex.index_tensor(order), ex.sym_tensor(sym)
    tr, w0 = _trainer(game, R)
    a = tr.evaluate_records(ex, index, syms, rows=True)
    b = tr.evaluate_tensors(*ex._batch(index, syms), rows=True)
    _same(a, b)
    assert a["rows"] == len(order) and 0 < a["policy_rows"] < a["rows"]
    # ... and the orientation matters to what is read, not to the definition: the statement on the turned rows
    _check(a, EC.statement(w0, *_decoded(ex, index, syms)), (name, "turned"))
    # no index, no symmetry: the records in order
    _same(tr.evaluate_records(ex, rows=True), tr.evaluate_tensors(*ex._batch(None), rows=True))
    assert ex.bad() == 0
    tr.close()


# ---- 3. malformed rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", [C4, TTT])
def test_malformed_rows_are_zeros_counted_and_in_no_total(game):
    """Nothing here can fault: every such value is checked on the device before it becomes an address (examples.hip.h)."""
    nsym = _lib.game_symmetries(game)
    rec = MC.copies(game, MC._positions(game, 5, 12), 12, 13, malformed=(3,))      # record 3 says n_children = S + 1
    ex = DeviceExamples.from_records(game, rec, DEV)
    order = np.array([0, 3, 5, len(rec), 7, 1, 2, -1, 9, 10, 11, 4, 6], dtype=np.int64)
    sym = np.zeros(len(order), dtype=np.uint8)
    sym[2], sym[8], sym[10] = nsym - 1, 1, nsym                                     # row 10: not a symmetry of the game
    wrong = [1, 3, 7, 10]
    good = [k for k in range(len(order)) if k not in wrong]
    d_order, d_sym = torch.from_numpy(order).to(DEV), torch.from_numpy(sym).to(DEV)
    tr, w0 = _trainer(game, 2)
    got = tr.evaluate_records(ex, d_order, d_sym, rows=True)
    assert ex.bad() == 4
    per_row, flags = got["per_row"].cpu().numpy(), got["flags"].cpu().numpy()
    assert not per_row[wrong].any() and not flags[wrong].any() and (flags[good] & _lib.ROW_COUNTED).all()
    only = tr.evaluate_records(ex, d_order[good].contiguous(), d_sym[good].contiguous(), rows=True)
    assert torch.equal(only["per_row"], got["per_row"][good]) and torch.equal(only["flags"], got["flags"][good])
    for k in EC.COUNTS:
        assert got[k] == only[k], k
    assert got["rows"] == len(good)
    for k, col in zip(SUMS, (1, 2)):      # the same floats in another strided order: double sums of at most 13 terms
        assert abs(got[k] - only[k]) <= 1e-12 * max(1.0, abs(only[k])) and abs(got[k] - per_row[good, col].astype(np.float64).sum()) <= 1e-12 * max(1.0, abs(only[k]))
    assert ex.bad() == 4
    tr.close()


# ---- 4. the forward pass of the step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,R,D", [("connect4", 2, 16), ("tictactoe", 9, 64)])
def test_squared_error_is_the_steps_loss_evaluation(name, R, D):
    game = GAME[name]
    ex = _examples(game)
    tr, _w0 = _trainer(game, R, D, eps=0.0)
    index = ex.index_tensor(np.arange(3, 20))                                        # 17 rows = max_batch
    boards, value, policy = ex._batch(index)
    got = tr.evaluate_records(ex, index)
    _loss, parts, _grads = tr.gradients(boards.cpu().numpy(), value.cpu().numpy(), policy.cpu().numpy())
    mine = got["se_sum"] / 17
    print(name, "se_sum / n %.9g lossEvaluation %.9g relative difference %.3g" % (mine, parts[0], abs(mine - parts[0]) / parts[0]))
    assert got["rows"] == 17 and abs(mine - parts[0]) <= 1e-6 * parts[0]
    # a batch of one row: lossEvaluation = (float)((double)le[0] / 1.0) is that row's own squared error, so the step's forward pass
    # and the scorer's must give the same float32 -- they are one text (csrc/train.hip.h: tr_conv_fwd, tr_head_*)
    one = tr.evaluate_records(ex, index[:1], rows=True)
    _loss, parts, _grads = tr.gradients(boards[:1].cpu().numpy(), value[:1].cpu().numpy(), policy[:1].cpu().numpy())
    se = float(one["per_row"][0, 1])
    print(name, "one row: se %.9g lossEvaluation %.9g" % (se, parts[0]))
    assert one["rows"] == 1 and se > 0 and parts[0] == se
    tr.close()


# ---- 5. evaluation moves nothing ----------------------------------------------------------------------------------------------------
def _buffers(tr):
    return [_lib.trainer_read(tr._h, what) for what in (_lib.TRAIN_PARAMS, _lib.TRAIN_SLOT_M, _lib.TRAIN_SLOT_V, _lib.TRAIN_GRADS)]


def test_evaluation_writes_no_trainer_state():
    ex = _examples(C4)
    boards, value, policy = ex._batch(ex.index_tensor(np.arange(17)))
    tr, _w0 = _trainer(C4, 2)
    tr.step_tensors(boards, value, policy, LR)                                       # slots, gradients and noise are not zero
    before, noise = _buffers(tr), tr.last_noise()
    assert all(b.any() for b in before) and noise.any()
    tr.evaluate_records(ex, rows=True)
    tr.evaluate_tensors(boards, value, policy)
    after = _buffers(tr)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(tr.last_noise(), noise)
    tr.close()


@pytest.mark.parametrize("kind", ["adam", "momentum"])
def test_training_with_evaluations_in_between_trains_the_same_bits(kind):
    """the noise a step draws is keyed by the trainer's step counter: an evaluation must not advance it"""
    ex = _examples(C4)
    one, _w = _trainer(C4, 2, kind=kind, seed=21)
    two, _w = _trainer(C4, 2, kind=kind, seed=21)
    for i in range(3):
        batch = ex._batch(ex.index_tensor(np.arange(17 * i, 17 * i + 17)))
        la, _parts = one.step_tensors(*batch, LR)
        if i < 2:
            one.evaluate_records(ex)
            one.evaluate_tensors(*batch)
        lb, _parts = two.step_tensors(*batch, LR)
        assert float(la) == float(lb) and np.array_equal(one.last_noise(), two.last_noise()) and one.last_noise().any()
    for a, b in zip(_buffers(one), _buffers(two)):
        assert np.array_equal(a, b)
    one.close()
    two.close()


# ---- 6. the current weights, without an export ------------------------------------------------------------------------------------
def test_evaluation_sees_the_weights_a_step_left():
    ex = _examples(TTT)
    tr, w0 = _trainer(TTT, 2)
    index = ex.index_tensor(np.arange(2))
    rows = _decoded(ex, index)
    first = tr.evaluate_records(ex, index, rows=True)
    tr.step_tensors(*ex._batch(ex.index_tensor(np.arange(17))), LR)
    got = tr.evaluate_records(ex, index, rows=True)
    _check(got, EC.statement(tr.export(), *rows), "after a step")
    _check(first, EC.statement(w0, *rows), "before it")
    assert np.abs(got["per_row"].cpu().numpy() - first["per_row"].cpu().numpy()).max() > 1e-3
    tr.close()


# ---- 7. repeatable; no rows ---------------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bits_and_no_rows_give_zero_totals():
    ex = _examples(C4)
    tr, _w0 = _trainer(C4, 9, 64)
    _same(tr.evaluate_records(ex, rows=True), tr.evaluate_records(ex, rows=True))
    for got in (tr.evaluate_records(ex, ex.index_tensor(np.zeros(0, dtype=np.int64)), rows=True),
                tr.evaluate_tensors(torch.zeros((0, 6, 7, 3)), torch.zeros(0), torch.zeros((0, 7)), rows=True)):
        assert tuple(got["per_row"].shape) == (0, 3) and tuple(got["flags"].shape) == (0,)
        assert all(got[k] == 0 for k in EC.COUNTS + SUMS) and all(np.isnan(got[k]) for k in MEANS)
    totals = torch.full((56,), 255, dtype=torch.uint8, device=DEV)
    _lib.trainer_eval(tr._h, 0, None, 0, totals_out=totals.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    assert not totals.cpu().numpy().any()
    # without rows_out / flags_out the per-row figures go to the trainer's own scratch: the same totals
    want = tr.evaluate_records(ex)
    _lib.trainer_eval(tr._h, len(ex), ex.records.data_ptr(), len(ex), totals_out=totals.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    tot = totals.cpu().numpy().view(_lib.EVAL_TOTALS_DTYPE)[0]
    for k in EC.COUNTS + SUMS:
        assert tot[k].item() == want[k], k
    tr.close()


# ---- 8. argument errors -------------------------------------------------------------------------------------------------------------
def test_arguments():
    ex = _examples(C4)
    tr, _w0 = _trainer(C4, 0)
    index = ex.index_tensor(np.arange(8))
    with pytest.raises(ValueError, match="DeviceExamples"):
        tr.evaluate_records(ex.merged())
    with pytest.raises(ValueError, match="game"):
        tr.evaluate_records(_examples(TTT))
    with pytest.raises(ValueError):
        tr.evaluate_records(DeviceExamples.from_records(C4, EC.records(C4), "cpu"))
    with pytest.raises(ValueError):
        tr.evaluate_records(ex, index, sym=torch.zeros(3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        tr.evaluate_records(ex, index.to(torch.int32))
    rows = torch.zeros((8, 3), dtype=torch.float32, device=DEV)
    totals = torch.zeros(64, dtype=torch.uint8, device=DEV)
    raw = dict(h=tr._h, n_records=len(ex), records=ex.records.data_ptr(), n=8, index=index.data_ptr(), rows_out=rows.data_ptr(),
               totals_out=totals.data_ptr())
    for wrong in (dict(n=-1), dict(n_records=-1), dict(records=None), dict(records=ex.records.data_ptr() + 8),
                  dict(index=index.data_ptr() + 4), dict(rows_out=rows.data_ptr() + 2), dict(totals_out=None),
                  dict(totals_out=totals.data_ptr() + 4), dict(bad=ex._bad.data_ptr() + 2), dict(h=None)):
        with pytest.raises(ValueError):
            _lib.trainer_eval(**{**raw, **wrong})
    boards, value, policy = ex._batch(index)
    raw = dict(h=tr._h, n=8, boards=boards.data_ptr(), value=value.data_ptr(), policy=policy.data_ptr(), totals_out=totals.data_ptr())
    for wrong in (dict(n=-1), dict(boards=None), dict(value=value.data_ptr() + 2), dict(policy=None), dict(totals_out=None),
                  dict(totals_out=totals.data_ptr() + 4)):
        with pytest.raises(ValueError):
            _lib.trainer_eval_tensors(**{**raw, **wrong})
    assert ex.bad() == 0 and not totals.cpu().numpy().any()
    tr.close()


# ---- 9. the front end ---------------------------------------------------------------------------------------------------------------
def _model(backend, name):
    cfg = M.net_config(1, 0.3)
    cfg["training"]["backend"] = backend
    return Blackbird.Model(BOARD_CLS[C4], name, {"explorationRate": 0.85, "playLimit": 16}, cfg)


def test_evaluate_device_examples_on_both_backends(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    np.random.seed(31)
    play = _model("hip", "play")
    play.KeepDeviceExamples = True
    Blackbird.GenerateTrainingSamples(play, 64, 1.0)
    kept = play.KeptDeviceExamples()
    train, held = kept.split_games(0.25, 3)
    assert len(train) + len(held) == len(kept) and len(held) >= 16 * 7
    w0 = {k: v.copy() for k, v in play._weights.items()}
    out = {}
    for backend in ("hip", "torch"):
        m = _model(backend, backend)
        m._weights = {k: v.copy() for k, v in w0.items()}
        version, batches, state = m.Version, m.batchCount, np.random.get_state()
        out[backend] = Blackbird.EvaluateDeviceExamples(m, examples=held, batchSize=100)      # (chunks of 100: more than one)
        after = np.random.get_state()
        assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]
        assert type(m._trainer) is {"hip": HipTrainer, "torch": Trainer}[backend]
        assert m.Version == version and m.batchCount == batches and sorted(m._weights) == sorted(w0)
        for k in w0:
            assert np.array_equal(m._weights[k], w0[k]), k
        assert all(not torch.is_tensor(v) for v in out[backend].values())
        m.Conn.Close()
    hip, tor = out["hip"], out["torch"]
    assert hip["rows"] == len(held) and 0 < hip["policy_rows"] < hip["rows"] and hip["decided"] > 0
    for k in EC.COUNTS:
        assert hip[k] == tor[k], (k, hip[k], tor[k])
    for k in SUMS + MEANS:
        close(hip[k], tor[k], k)
    # the kept examples of the model's Version, when none are given
    mine = Blackbird.EvaluateDeviceExamples(play)
    assert mine["rows"] == len(kept)
    play._batch_engine.close()
    play.Conn.Close()
