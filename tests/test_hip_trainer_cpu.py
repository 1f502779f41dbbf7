"""The HIP training backend (training.HipTrainer, bb_trainer_*), the part that needs no GPU:

  * `statement`: the reference's training graph (NetworkFactory.py:37-245) for ANY dense game and network shape, in float64
    as shifted-window einsum contractions in NHWC (no conv2d), and `RefOptimizer`, the TF1 update rules in numpy -- what
    tests/test_gpu_hip_trainer.py holds the kernels to.  Checked here against the statement of tests/test_train_parity.py
    (tied to Connect4, two blocks) at that file's shape, to 1e-12;
  * bb_trainer_create's argument checks, which come before any device call, and its loud failure without a GPU;
  * the front end: the default configuration still builds the PyTorch trainer, and a shape outside the kernels' scope with
    backend 'hip' is refused, not silently trained by PyTorch."""
import ctypes as C

import numpy as np
import pytest

from blackbird_amd import _lib
from blackbird_amd import weights as W
from tests import trainer_cases as tp
from tests.trainer_cases import GAMES, RefOptimizer, make_batch, statement

# ---- the statement against the existing one ----------------------------------------------------------------------------
def test_statement_agrees_with_the_connect4_statement():
    w0 = W.init_weights(tp.C, tp.F, tp.R, tp.D, tp.A, seed=3, perturb=True)
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w0.items()}
    batch = tp._batch(40)
    mine = make_batch(tp.H, tp.Wd, tp.A, tp.B, 40)
    for a, b in zip(batch, mine):            # the generalised batch maker draws what the original draws
        assert np.array_equal(a, b)
    total, parts, grads = statement(w64, *batch, tp.EPS)
    r_total, r_parts, r_grads = tp._ref_grads(w64, batch)
    assert abs(total - r_total) <= 1e-12 and np.max(np.abs(np.array(parts) - np.array(r_parts))) <= 1e-12
    assert set(grads) == set(r_grads) and len(grads) == 18 + 8 * tp.R
    for k in grads:
        assert np.max(np.abs(grads[k] - r_grads[k])) <= 1e-12, k
    for kind in ("adam", "momentum", "sgd"):
        a, b, w_a, w_b = RefOptimizer(kind, 0.9), tp._RefOptimizer(kind, 0.9), w64, w64
        for _step in range(2):
            w_a, w_b = a.apply(w_a, grads, 1e-2), b.apply(w_b, grads, 1e-2)
            for k in w_a:
                assert np.max(np.abs(w_a[k] - np.asarray(w_b[k], dtype=np.float64))) <= 1e-12, (kind, k)


def test_unflatten_inverts_flatten():
    for (C_, R, D, A) in ((3, 0, 1, 7), (3, 2, 16, 9), (3, 9, 64, 7)):
        w = W.init_weights(C_, 16, R, D, A, seed=2, perturb=True)
        flat = W.flatten(w)
        fields = W.flat_fields(C_, 16, R, D, A)
        assert [n for n, _s in fields] == [n for n, _t in _lib.NetWeights._fields_[7:]]
        vec = np.concatenate([flat[n].ravel() for n, _s in fields])
        back = W.unflatten(vec, C_, 16, R, D, A)
        assert list(back) == list(w)
        for k in w:
            assert back[k].shape == w[k].shape and np.array_equal(back[k], w[k]), k
        if R in (0, 2):  # the PyTorch trainer's flat tensor (Trainer.load_into's descriptor points into it): the same vector
            from blackbird_amd.training import Trainer
            t_flat, offsets = Trainer(w, device="cpu")._flat_device()
            assert t_flat.dtype.is_floating_point and t_flat.element_size() == 4 and np.array_equal(t_flat.numpy(), vec)
            sums = np.cumsum([0] + [flat[n].size for n, _s in fields])
            assert offsets == {n: int(at) for (n, _s), at in zip(fields, sums)} and sums[-1] == vec.size


# ---- bb_trainer_create: arguments, and no GPU ---------------------------------------------------------------------------
def _create(game="connect4", filters=16, blocks=2, dense=16, optimizer=_lib.OPT_ADAM, max_batch=8, board=None, **kw):
    gid, H, Wd, A = GAMES[game] if game in GAMES else (game, 6, 7, 7)
    if board:
        H, Wd = board
    flat = W.flatten(W.init_weights(3, filters, blocks, dense, A, seed=1))
    return _lib.trainer_create(gid, flat, H, Wd, optimizer, max_batch, **kw)


@pytest.mark.parametrize("bad", [
    dict(game=_lib.GAME_DRAGONCHESS), dict(game=7), dict(filters=32), dict(blocks=10), dict(dense=65), dict(optimizer=3),
    dict(optimizer=-1), dict(max_batch=0), dict(max_batch=-4), dict(board=(3, 3)), dict(game="tictactoe", board=(6, 7)),
    dict(epsilon=1.5), dict(alpha=0.0)])
def test_create_refuses_what_is_outside_the_scope(bad):
    """BB_ERR_ARG (ValueError through the bindings) with or without a GPU: the checks precede every device call."""
    with pytest.raises(ValueError):
        _create(**bad)


def test_create_refuses_null_arguments_and_missing_blocks():
    L = _lib.lib()
    cfg = _lib.TrainConfig(game=_lib.GAME_CONNECT4, optimizer=_lib.OPT_SGD, max_batch=4, alpha=0.2, epsilon=0.3)
    w, _keep = _lib.net_weights(6, 7, W.flatten(W.init_weights(3, 16, 1, 4, 7)))
    h = C.c_void_p()
    assert L.bb_trainer_create(None, C.byref(w), C.byref(h)) == _lib.ERR_ARG
    assert L.bb_trainer_create(C.byref(cfg), None, C.byref(h)) == _lib.ERR_ARG
    assert L.bb_trainer_create(C.byref(cfg), C.byref(w), None) == _lib.ERR_ARG
    w.blk_k = None
    assert L.bb_trainer_create(C.byref(cfg), C.byref(w), C.byref(h)) == _lib.ERR_ARG and not h.value
    # the other entry points on no trainer at all
    n = C.c_int64()
    out = np.zeros(4, np.float32)
    assert L.bb_trainer_step(None, 1, None, None, None, None, 0.01, 1, None, None) == _lib.ERR_ARG
    assert L.bb_trainer_param_count(None, C.byref(n)) == _lib.ERR_ARG
    assert L.bb_trainer_read(None, _lib.TRAIN_PARAMS, _lib.ptr(out), 4) == _lib.ERR_ARG
    assert L.bb_trainer_destroy(None) == _lib.OK


def test_create_fails_loudly_without_a_gpu():
    if _lib.lib().bb_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.BlackbirdHipError):
        _create()
    from blackbird_amd.training import HipTrainer
    with pytest.raises((_lib.BlackbirdHipError, RuntimeError)):
        HipTrainer(W.init_weights(3, 16, 1, 4, 7), device="cuda")


# ---- the front end --------------------------------------------------------------------------------------------------------
def _net(tmp_path, monkeypatch, training, filters=16, actions=7, shape=(6, 7, 3), name="n_1"):
    monkeypatch.chdir(tmp_path)
    from blackbird_amd.Network import Network
    from blackbird_amd.NetworkFactory import NetworkFactory
    cfg = {"blocks": 1, "filters": filters, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": training}
    return Network(name, NetworkFactory(cfg, actions, inputShape=shape))


@pytest.mark.parametrize("training", [{"optimizer": "adam"}, {"optimizer": "sgd", "backend": "torch"}])
def test_default_backend_is_the_pytorch_trainer(tmp_path, monkeypatch, training):
    from blackbird_amd.training import Trainer
    net = _net(tmp_path, monkeypatch, training)
    tr = net._trainer_for(3)
    assert type(tr) is Trainer and tr.kind == training["optimizer"] and net._trainer_for(3) is tr


def test_hip_backend_refuses_shapes_outside_its_scope(tmp_path, monkeypatch):
    """No silent fallback: the message names the limits."""
    wide = _net(tmp_path, monkeypatch, {"optimizer": "adam", "backend": "hip"}, filters=32, name="wide_1")
    with pytest.raises(ValueError, match="16 filters"):
        wide._trainer_for(3)
    dc = _net(tmp_path, monkeypatch, {"optimizer": "adam", "backend": "hip"}, actions=4032, shape=(8, 8, 17), name="dc_1")
    with pytest.raises(ValueError, match="Connect4 or TicTacToe"):
        dc._trainer_for(17)
    odd = _net(tmp_path, monkeypatch, {"optimizer": "adam", "backend": "triton"}, name="odd_1")
    with pytest.raises(ValueError, match="backend"):
        odd._trainer_for(3)
