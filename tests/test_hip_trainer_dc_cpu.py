"""The HIP training step for DragonChess (training.HipTrainer over bb_trainer_*, k_train_*_wide of csrc/train.hip.h), the part
that needs no GPU:

  * NetworkConfig['training']['hip_games']: 'dense' by default (backend 'hip' alone still refuses a DragonChess network, in the
    words tests/test_hip_trainer_cpu.py pins), 'all', and anything else refused;
  * bb_trainer_create's checks for the game, which precede every device call: 32 filters, one block more than the LDS of a CU
    holds, dense 65, weights of another game's shape -- and the largest covered shape passes them (and then fails for want of a
    GPU), which holds training.HIP_TRAINER_DC_BLOCKS to train_max_blocks<DragonChess>() from both sides;
  * the entry points a DragonChess trainer refuses, on no trainer at all: unchanged;
  * the batch maker of tests/dc_trainer_cases.py, and trainer_cases.statement on such a batch against training.Trainer on the
    CPU at one block: the reference tests/test_gpu_hip_trainer_dc.py holds the kernels to is itself held to something."""
import ctypes as C

import numpy as np
import pytest

from blackbird_amd import _lib, training
from blackbird_amd import weights as W
from tests import dc_trainer_cases as DCC
from tests.trainer_cases import ALPHA, EPS, assert_live, close, statement

DC = _lib.GAME_DRAGONCHESS


# ---- the front end --------------------------------------------------------------------------------------------------------
def _net(tmp_path, monkeypatch, training_cfg, name, blocks=1, filters=16, dense=16):
    monkeypatch.chdir(tmp_path)
    from blackbird_amd.Network import Network
    from blackbird_amd.NetworkFactory import NetworkFactory
    cfg = {"blocks": blocks, "filters": filters, "eval": {"dense": dense}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": training_cfg}
    return Network(name, NetworkFactory(cfg, DCC.A, inputShape=(DCC.H, DCC.Wd, DCC.C)))


def test_hip_games_key(tmp_path, monkeypatch):
    assert training.HIP_GAMES == ("dense", "all")
    for cfg in ({"optimizer": "adam", "backend": "hip"}, {"optimizer": "adam", "backend": "hip", "hip_games": "dense"}):
        net = _net(tmp_path, monkeypatch, cfg, "dense_%d" % len(cfg))
        with pytest.raises(ValueError, match="Connect4 or TicTacToe"):      # today's refusal, in today's words
            net._trainer_for(17)
        assert net._trainer is None
    for bad in ("dragonchess", "", None, True):
        net = _net(tmp_path, monkeypatch, {"optimizer": "adam", "backend": "hip", "hip_games": bad}, "bad_%s" % bad)
        with pytest.raises(ValueError, match="hip_games"):
            net._trainer_for(17)
    # a bad value is refused whatever the backend; a good one does not disturb the PyTorch trainer
    with pytest.raises(ValueError, match="hip_games"):
        _net(tmp_path, monkeypatch, {"optimizer": "adam", "hip_games": "some"}, "bad_torch")._trainer_for(17)
    tr = _net(tmp_path, monkeypatch, {"optimizer": "sgd", "hip_games": "all"}, "torch_all")._trainer_for(17)
    assert type(tr) is training.Trainer and (tr.C, tr.A) == (17, 4032)


def test_hip_games_all_admits_the_shape_and_names_the_limits(tmp_path, monkeypatch):
    w = DCC.weights(1, 16, 1)
    assert not training.hip_trainer_supports(w) and not training.hip_trainer_supports(w, "dense")
    assert training.hip_trainer_supports(w, "all")
    assert training.hip_trainer_supports(DCC.weights(training.HIP_TRAINER_DC_BLOCKS, 64, 1), "all")
    assert not training.hip_trainer_supports(DCC.weights(training.HIP_TRAINER_DC_BLOCKS + 1, 16, 1), "all")
    assert not training.hip_trainer_supports(DCC.weights(1, 65, 1), "all")
    assert not training.hip_trainer_supports(W.init_weights(17, 32, 1, 16, 4032, seed=1), "all")
    with pytest.raises(ValueError, match="hip_games"):
        training.hip_trainer_supports(w, "most")
    assert DCC.R_MAX == training.HIP_TRAINER_DC_BLOCKS and "0 to %d blocks" % DCC.R_MAX in training.HIP_TRAINER_LIMITS_ALL
    both = {"optimizer": "adam", "backend": "hip", "hip_games": "all"}
    deep = _net(tmp_path, monkeypatch, both, "deep_1", blocks=DCC.R_MAX + 1)
    with pytest.raises(ValueError, match="DragonChess \\(0 to %d blocks" % DCC.R_MAX):
        deep._trainer_for(17)
    wide = _net(tmp_path, monkeypatch, both, "wide_1", filters=32)
    with pytest.raises(ValueError, match="16 filters"):
        wide._trainer_for(17)
    if _lib.lib().bb_device_count() <= 0:          # within the limits the trainer is made: without a GPU that fails loudly
        with pytest.raises((_lib.BlackbirdHipError, RuntimeError)):
            _net(tmp_path, monkeypatch, both, "ok_1")._trainer_for(17)


# ---- bb_trainer_create ------------------------------------------------------------------------------------------------------
def _create(filters=16, blocks=1, dense=16, planes=DCC.C, actions=DCC.A, board=(DCC.H, DCC.Wd)):
    flat = W.flatten(W.init_weights(planes, filters, blocks, dense, actions, seed=1))
    return _lib.trainer_create(DC, flat, board[0], board[1], _lib.OPT_ADAM, 4)


@pytest.mark.parametrize("bad", [dict(filters=32), dict(blocks=DCC.R_MAX + 1), dict(dense=65), dict(dense=0),
                                 dict(planes=3, actions=7, board=(6, 7)), dict(planes=3), dict(actions=7)])
def test_create_refuses_what_is_outside_the_scope(bad):
    """BB_ERR_ARG (ValueError through the bindings) with or without a GPU: the checks precede every device call."""
    with pytest.raises(ValueError):
        _create(**bad)


def test_the_refusal_names_the_largest_block_count():
    with pytest.raises(ValueError, match="0\\.\\.%d blocks" % DCC.R_MAX):
        _create(blocks=DCC.R_MAX + 1)


def test_the_largest_shape_passes_the_argument_checks():
    if _lib.lib().bb_device_count() > 0:
        h = _create(blocks=DCC.R_MAX, dense=64)
        assert _lib.trainer_param_count(h) == sum(v.size for v in W.init_weights(DCC.C, 16, DCC.R_MAX, 64, DCC.A).values())
        _lib.trainer_destroy(h)
    else:
        with pytest.raises(_lib.BlackbirdHipError) as e:       # not a ValueError: every argument check lies behind it
            _create(blocks=DCC.R_MAX, dense=64)
        assert not isinstance(e.value, ValueError)


def test_records_source_and_scorer_on_no_trainer():
    L = _lib.lib()
    assert L.bb_trainer_epoch(None, 0, None, 0, 1, None, None, None, 0.01, None, None, None) == _lib.ERR_ARG
    assert L.bb_trainer_eval(None, 0, None, 0, None, None, None, None, None, None, None) == _lib.ERR_ARG
    assert L.bb_trainer_eval_tensors(None, 0, None, None, None, None, None, None, None) == _lib.ERR_ARG
    out = np.zeros(4, np.float32)
    assert L.bb_trainer_read(None, _lib.TRAIN_NOISE, _lib.ptr(out), 4) == _lib.ERR_ARG and not out.any()
    assert L.bb_trainer_load_engine(None, None, None) == _lib.ERR_ARG
    assert L.bb_trainer_destroy(None) == _lib.OK
    assert C.sizeof(_lib.TrainConfig) > 0


# ---- the batch maker and the statement ---------------------------------------------------------------------------------------
def test_batch_maker():
    boards, ev, pl, noise = DCC.make_batch(5, 3)
    assert boards.shape == (5, 8, 8, 17) and boards.dtype == np.int8 and pl.shape == (5, 4032) and noise.shape == (4032,)
    assert all(boards[j, :, :, 16].any() for j in range(5)) and set(np.unique(boards[..., 16])) <= {-1, 1}
    assert boards[..., :12].sum(axis=-1).max() == 1 and boards[..., :12].any()
    assert not pl[-1].any()
    for j in range(4):
        assert (pl[j] != 0).sum() == 10 and abs(pl[j].sum() - 1) < 1e-12 and all(pl[j, a] > 0 for a in DCC.EDGE_ACTIONS)
    assert ((noise > 0) & (noise < 1)).all()
    again = DCC.make_batch(5, 3)
    assert all(np.array_equal(a, b) for a, b in zip((boards, ev, pl, noise), again))
    full = DCC.make_batch(5, 3, terminal_last=False)
    assert full[2][-1].any() and np.array_equal(full[0], boards) and np.array_equal(full[2][:-1], pl[:-1])
    assert not DCC.make_batch(5, 3, zero_labels=True)[2].any()


@pytest.mark.parametrize("eps", [EPS, 0.0])
def test_statement_agrees_with_the_pytorch_trainer(eps):
    """The float64 statement against training.Trainer (float32 conv2d autograd, CPU) at one block: the loss terms and every
    gradient under the `close` rule."""
    w0 = DCC.weights(1, 16, 4)
    batch = DCC.make_batch(3, 21)
    noise = batch[3] if eps else None
    total, parts, grads = statement(w0, batch[0], batch[1], batch[2], noise, eps)
    tr = training.Trainer(w0, alpha=ALPHA, epsilon=eps, optimizer="sgd", device="cpu")
    t_total, t_parts, t_grads = tr.gradients(batch[0], batch[1], batch[2], noise=np.zeros(DCC.A) if noise is None else noise)
    close(t_total, total, ("loss", eps))
    for got, want in zip(t_parts, parts):
        close(got, want, ("term", eps))
    assert set(t_grads) == set(grads) and len(grads) == 18 + 8
    for k in grads:
        assert t_grads[k].shape == grads[k].shape
        close(t_grads[k].numpy(), grads[k], ("grad", k, eps))
    assert grads["resTower/conv_block/conv/kernel"].shape == (3, 3, 17, 16) and grads["policy/policy/kernel"].shape == (2, 4032)


def test_the_live_case_is_live():
    """trainer_cases.assert_live on the statement at the live case, and the three slices a 16-channel or 16-action mapping
    would leave unwritten carry a data gradient there."""
    ref = DCC.live_case()
    R, D, B, _ws, _bs = DCC.LIVE_CASE
    assert_live(ref["want"], B, D, False, DCC.LIVE_CASE)
    assert all(r.any() for r in ref["batch"][2])               # no terminal row
    for k, s in DCC.LIVE_SLICES.items():
        assert np.abs(ref["want"][3][k][s]).max() >= 1e-3, k
    assert 0 < ref["tol"] <= 1e-5
