"""-m gpu: the training step as HIP kernels (training.HipTrainer over bb_trainer_*, csrc/train.hip.h) against the float64
statement of the reference's graph in tests/trainer_cases.py (tests/test_hip_trainer_cpu.py checks it): the loss terms and the gradient of every variable, two
optimiser steps per optimiser, the shapes where the kernels can go wrong, bit-repeatability, the device-drawn noise, the same
training as the PyTorch trainer over real self-play records, and the front end.

Tolerance: 1e-5 relative to max(1, largest |entry|) of each tensor (the `_close` rule of tests/test_train_parity.py).  No
gradient tensor reaches 1, so that is an absolute 1e-5, and at weights drawn by init_weights alone the value head saturates and
whole ReLU layers are off: the live tests (test_gradients_live, test_two_steps_live) hold the same kernels, at inputs whose
every backward pass is multiplied by something, to a bound measured from float32 arithmetic (tests/trainer_cases.py)."""

import numpy as np
import pytest
import torch

from blackbird_amd import Blackbird, Connect4, _lib
from blackbird_amd import weights as W
from blackbird_amd.training import DeviceExamples, HipTrainer, Trainer
from tests.trainer_cases import (ALPHA, EPS, GAMES, LIVE_CASES, LIVE_LR, TWO_STEP_CASE, RefOptimizer, assert_live, close, close_live,
                                 float32_figure, live_case, live_tol, make_batch, statement)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _w64(w):
    return {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}


def _trainer(w0, kind="adam", eps=EPS, seed=11, max_batch=130):
    return HipTrainer(w0, alpha=ALPHA, epsilon=eps, optimizer=kind, momentum=0.9, device=DEV, seed=seed, max_batch=max_batch)


def _check_gradients(tr, here, batch, eps, what, noise="given"):
    """One gradient-only step of `tr` on `batch` against the statement at the weights `here`; returns the gradients."""
    boards, ev, pl, nz = batch
    total, parts, grads = tr.gradients(boards, ev, pl, noise=nz if noise == "given" else None)
    r_total, r_parts, r_grads = statement(here, boards, ev, pl, nz if noise == "given" else None, eps)
    close(total, r_total, (what, "loss"))
    for got, want, name in zip(parts, r_parts, ("lossEvaluation", "lossPolicy", "lossParam")):
        close(got, want, (what, name))
    assert set(grads) == set(r_grads)
    for k in r_grads:
        g = grads[k].cpu().numpy()
        assert g.shape == r_grads[k].shape and g.dtype == np.float32, (what, k, g.shape)
        close(g, r_grads[k], (what, "grad", k))
    return grads


@pytest.mark.parametrize("kind", ["adam", "momentum", "sgd"])
def test_two_steps_match_the_statement(kind):
    _g, H, Wd, A = GAMES["connect4"]
    w0 = W.init_weights(3, 16, 2, 16, A, seed=3, perturb=True)
    tr = _trainer(w0, kind)
    assert (tr.kind, tr.momentum, tr.alpha, tr.epsilon) == (kind, 0.9, ALPHA, EPS)
    assert (tr.C, tr.F, tr.R, tr.D, tr.A) == (3, 16, 2, 16, A)
    ref_opt = RefOptimizer(kind, 0.9)
    lr = 1e-2
    for step in range(2):  # the second step exercises the optimiser's slots (m, v, beta powers / the accumulator)
        batch = make_batch(H, Wd, A, 6, 40 + step)
        here = _w64(tr.export())
        grads = _check_gradients(tr, here, batch, EPS, (kind, step))
        # The update rule is checked on the gradients the step actually used (tests/test_train_parity.py: Adam maps g to
        # g / (|g| + 3.2e-7) on its first step, which turns the rounding of a float32 gradient near zero into percents of lr
        # -- that conditioning belongs to the optimiser, not to either implementation).  The step recomputes exactly these
        # gradients: the kernels are bit-repeatable (test_repeatable).
        g64 = {k: v.cpu().numpy().astype(np.float64) for k, v in grads.items()}
        total, parts = tr.step(batch[0], batch[1], batch[2], lr, noise=batch[3])
        assert isinstance(total, float) and len(parts) == 3
        want_w = ref_opt.apply(here, g64, lr)
        new = tr.export()
        assert list(new) == list(w0)
        for k in want_w:
            close(new[k], want_w[k], (kind, step, "weights", k))
            if k in g64 and np.abs(g64[k]).max() > 1e-6:
                assert not np.array_equal(new[k], here[k].astype(np.float32)), (kind, step, "did not move", k)
            if k.endswith("moving_mean") or k.endswith("moving_variance"):
                assert np.array_equal(new[k], w0[k]), k
    m, v = tr.slots()
    for k in g64:
        if kind == "adam":
            close(m[k], ref_opt.m[k], (kind, "m", k))
            close(v[k], ref_opt.v[k], (kind, "v", k))
        elif kind == "momentum":
            close(m[k], ref_opt.m[k], (kind, "accumulator", k))
        else:
            assert not m[k].any() and not v[k].any()
    tr.close()


# every value of each axis at least once; R in {0, 9} crossed with B in {1, 130}
SHAPES = [("connect4", 0, 16, 1), ("connect4", 0, 16, 130), ("connect4", 9, 16, 1), ("connect4", 9, 16, 130),
          ("connect4", 1, 1, 6), ("connect4", 4, 64, 50), ("tictactoe", 2, 16, 6), ("tictactoe", 9, 64, 130),
          ("tictactoe", 0, 1, 1)]


@pytest.mark.parametrize("game,R,D,B", SHAPES)
def test_gradients_over_shapes(game, R, D, B):
    _g, H, Wd, A = GAMES[game]
    w0 = W.init_weights(3, 16, R, D, A, seed=5 + R, perturb=True)
    tr = _trainer(w0, "sgd")
    _check_gradients(tr, _w64(w0), make_batch(H, Wd, A, B, 60 + B), EPS, (game, R, D, B))
    after = tr.export()
    for k in w0:                                   # apply = 0 moves nothing
        assert np.array_equal(after[k], w0[k]), k
    tr.close()


def _check_gradients_live(tr, here, batch, want, tol, what):
    """One gradient-only step of `tr` on `batch` against `want` = statement(here, ..., parts=True) under the live rule: per
    tensor |got - want| <= tol * max|data gradient| + 2**-23 * max|want|.  Returns (gradients, largest relative error)."""
    boards, ev, pl, nz = batch
    total, parts, grads = tr.gradients(boards, ev, pl, noise=nz)
    r_total, r_parts, r_grads, r_data, _live = want
    close(total, r_total, (what, "loss"))
    for got, ref, name in zip(parts, r_parts, ("lossEvaluation", "lossPolicy", "lossParam")):
        close(got, ref, (what, name))
    assert set(grads) == set(r_grads)
    worst = 0.0
    for k in r_grads:
        g = grads[k].cpu().numpy()
        assert g.shape == r_grads[k].shape and g.dtype == np.float32, (what, k, g.shape)
        close(g, r_grads[k], (what, "grad", k))          # today's rule still holds
        worst = max(worst, close_live(g, r_grads[k], float(np.abs(r_data[k]).max()), tol, (what, "live grad", k)))
    return grads, worst


@pytest.mark.parametrize("case", LIVE_CASES, ids=str)
def test_gradients_live(case):
    """The gradient of every variable at inputs where every backward pass is live (tests/test_trainer_liveness_cpu.py), per tensor
    within tol * max|data gradient| + 2**-23 * max|want| of the float64 statement, tol = min(8 f, 1e-5) with f the error of the
    same statement evaluated in float32 on the CPU (largest over the tensors, each relative to its largest |data gradient|).
    Measured on the MI355X (f on its host CPU; it depends on the CPU's float32 summation order, the kernel's error does not),
    f / the kernel's error in the same measure / tol:
      tictactoe R2 D16 B6      2.5e-6 / 2.8e-6 / 1e-5       connect4 R0 D16 B1, no label  4.7e-7 / 5.5e-7 / 3.7e-6
      connect4 R0 D16 B1       6.5e-7 / 1.4e-6 / 5.2e-6     tictactoe R0 D1 B1, no label  6.6e-6 / 1.9e-6 / 1e-5
      connect4 R1 D1 B6        9.8e-6 / 5.0e-6 / 1e-5       connect4 R2 D64 B2            1.5e-6 / 1.1e-6 / 1e-5
      connect4 R9 D16 B1       6.4e-7 / 1.2e-6 / 5.1e-6     connect4 R9 D16 B2            2.7e-5 / 9.4e-6 / 1e-5 (the cap)
      tictactoe R9 D64 B2      3.6e-6 / 3.8e-6 / 1e-5       tictactoe R0 D16 B130         2.5e-6 / 4.0e-6 / 1e-5
    The kernel is nowhere more than 2.2 float32-statement errors from the statement."""
    game, _R, _D, B, _ws, _bs, terminal_last = case
    ref = live_case(case)
    w0 = ref["w"]
    tr = _trainer(w0, "sgd")
    grads, worst = _check_gradients_live(tr, _w64(w0), ref["batch"], ref["want"], ref["tol"], case)
    print(case, "float32 statement %.3g kernel %.3g tolerance %.3g" % (ref["figure"], worst, ref["tol"]))
    if B == 1 and terminal_last:                       # the one row has no label: the policy head's data gradient is exactly 0
        n_l2 = np.float32(sum(1 for k in grads if "bias" not in k))
        for k, g in grads.items():
            if k.startswith("policy/"):
                assert np.array_equal(g.cpu().numpy(), np.zeros_like(w0[k]) if "bias" in k else w0[k] / n_l2), k
    after = tr.export()
    for k in w0:                                       # apply = 0 moves nothing
        assert np.array_equal(after[k], w0[k]), k
    tr.close()


@pytest.mark.parametrize("kind", ["adam", "momentum", "sgd"])
def test_two_steps_live(kind):
    """test_two_steps_match_the_statement at the live two-step case: both steps' gradients under the rule of test_gradients_live
    (the second at the weights the first step left, its tolerance measured there), the update and the slots as before, and
    value/dense_2/kernel -- which a saturated tanh leaves where it is -- moved by each step."""
    game, _R, _D, B, _ws, b_seed, terminal_last = TWO_STEP_CASE
    _g, H, Wd, A = GAMES[game]
    ref = live_case(TWO_STEP_CASE)
    w0 = ref["w"]
    tr = _trainer(w0, kind)
    ref_opt = RefOptimizer(kind, 0.9)
    for step in range(2):
        here32 = tr.export()
        here = _w64(here32)
        if step == 0:
            batch, want, figure = ref["batch"], ref["want"], ref["figure"]
        else:
            batch = make_batch(H, Wd, A, B, b_seed + 1, terminal_last=terminal_last)
            want = statement(here32, *batch, EPS, parts=True)
            assert_live(want, B, _D, False, (kind, step))
            figure = float32_figure(here32, batch, EPS, want)
        grads, worst = _check_gradients_live(tr, here, batch, want, live_tol(figure), (kind, step))
        print(kind, step, "float32 statement %.3g kernel %.3g tolerance %.3g" % (figure, worst, live_tol(figure)))
        g64 = {k: v.cpu().numpy().astype(np.float64) for k, v in grads.items()}
        tr.step(batch[0], batch[1], batch[2], LIVE_LR, noise=batch[3])
        want_w = ref_opt.apply(here, g64, LIVE_LR)
        new = tr.export()
        for k in want_w:
            close(new[k], want_w[k], (kind, step, "weights", k))
            # the same update from the same float32 gradients: what is left is the rounding of p - step, half a unit in the
            # last place of the weight (the step's own few-ulp error is lr times smaller); four of them allowed
            assert np.abs(new[k] - want_w[k]).max() <= 2.0 ** -22 * np.abs(want_w[k]).max(), (kind, step, "weights", k)
            if k in g64:
                assert not np.array_equal(new[k], here32[k]), (kind, step, "did not move", k)
            else:
                assert np.array_equal(new[k], w0[k]), k
        assert (new["value/dense_2/kernel"] != here32["value/dense_2/kernel"]).any()
    m, v = tr.slots()
    for k in g64:
        if kind == "adam":
            close(m[k], ref_opt.m[k], (kind, "m", k))
            close(v[k], ref_opt.v[k], (kind, "v", k))
        elif kind == "momentum":
            close(m[k], ref_opt.m[k], (kind, "accumulator", k))
        else:
            assert not m[k].any() and not v[k].any()
    tr.close()


def test_no_noise_is_plain_log_softmax():
    _g, H, Wd, A = GAMES["connect4"]
    w0 = W.init_weights(3, 16, 2, 16, A, seed=3, perturb=True)
    tr = _trainer(w0, "sgd", eps=0.0)
    _check_gradients(tr, _w64(w0), make_batch(H, Wd, A, 6, 44), 0.0, "eps0", noise=None)
    assert not tr.last_noise().any()               # epsilon = 0: no draw
    tr.close()


def test_zero_policy_labels_leave_the_l2_part_only():
    _g, H, Wd, A = GAMES["connect4"]
    w0 = W.init_weights(3, 16, 2, 16, A, seed=3, perturb=True)
    tr = _trainer(w0, "sgd")
    batch = make_batch(H, Wd, A, 6, 45, zero_labels=True)
    grads = _check_gradients(tr, _w64(w0), batch, EPS, "zero labels")
    n_l2 = np.float32(sum(1 for k in grads if "bias" not in k))
    for k, g in grads.items():
        if k.startswith("policy/"):
            want = np.zeros_like(w0[k]) if "bias" in k else w0[k] / n_l2
            assert np.array_equal(g.cpu().numpy(), want), k
    tr.close()


def _run_steps(w0, seed, noises=(None, None, None)):
    _g, H, Wd, A = GAMES["connect4"]
    tr = _trainer(w0, "adam", seed=seed)
    losses, drawn = [], []
    for step, nz in enumerate(noises):
        boards, ev, pl, _nz = make_batch(H, Wd, A, 6, 70 + step)
        total, parts = tr.step(boards, ev, pl, 1e-2, noise=nz)
        losses.append([total] + parts)
        drawn.append(tr.last_noise())
    out = (tr.export(), tr.slots(), np.array(losses), drawn)
    tr.close()
    return out


def _same_bits(a, b):
    assert np.array_equal(a[2], b[2]), "losses"
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), ("parameters", k)
    for sa, sb in zip(a[1], b[1]):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), ("slots", k)


def test_repeatable_and_noise_readback():
    w0 = W.init_weights(3, 16, 2, 16, 7, seed=3, perturb=True)
    one, two = _run_steps(w0, 21), _run_steps(w0, 21)
    _same_bits(one, two)                           # no sum depends on scheduling
    assert np.isfinite(one[2]).all() and not np.array_equal(one[2][0], one[2][1])
    for a, b in zip(one[3], two[3]):
        assert np.array_equal(a, b)
    # a twin that is GIVEN the draws the first one made computes the same bits
    twin = _run_steps(w0, 999, noises=one[3])
    _same_bits(one, twin)
    other = _run_steps(w0, 22)                     # another seed: other draws
    assert not np.array_equal(other[3][0], one[3][0])


def test_drawn_noise_is_beta():
    _g, H, Wd, A = GAMES["connect4"]
    tr = _trainer(W.init_weights(3, 16, 0, 1, A, seed=1), "sgd", seed=5, max_batch=2)
    boards, ev, pl, _nz = make_batch(H, Wd, A, 2, 80)
    dev = [torch.tensor(np.asarray(x, dtype=np.float32), device=DEV) for x in (boards, ev, pl)]
    draws = []
    for _step in range(200):
        tr._launch(dev[0], dev[1], dev[2], None, 0.0, False)
        draws.append(tr.last_noise())
    draws = np.array(draws)
    assert draws.shape == (200, A) and (draws >= 0).all() and (draws <= 1).all()
    # Beta(0.2, 0.8): standard deviation 0.283, so the mean of 1400 draws has standard error 0.0076; five of them
    print("mean of the draws", draws.mean())
    assert abs(float(draws.mean()) - ALPHA) <= 0.04
    assert all(not np.array_equal(draws[i], draws[i + 1]) for i in range(199))
    tr.close()


def test_step_arguments():
    _g, H, Wd, A = GAMES["connect4"]
    tr = _trainer(W.init_weights(3, 16, 1, 4, A, seed=1), "sgd", max_batch=4)
    b = torch.zeros((4, H, Wd, 3), dtype=torch.float32, device=DEV)
    v = torch.zeros(4, dtype=torch.float32, device=DEV)
    p = torch.zeros((4, A), dtype=torch.float32, device=DEV)
    ok = dict(n=4, boards=b.data_ptr(), value=v.data_ptr(), policy=p.data_ptr(), lr=0.01, apply=False)
    _lib.trainer_step(tr._h, **ok)
    for bad in (dict(n=0), dict(n=-1), dict(n=5), dict(boards=None), dict(value=None), dict(policy=None),
                dict(boards=b.data_ptr() + 2), dict(policy=p.data_ptr() + 1), dict(noise=p.data_ptr() + 3),
                dict(loss_out=v.data_ptr() + 2), dict(lr=float("nan"))):
        with pytest.raises(ValueError):
            _lib.trainer_step(tr._h, **{**ok, **bad})
    n = _lib.trainer_param_count(tr._h)
    assert n == tr.count == sum(x.size for x in W.flatten(tr.export()).values())
    for what, count in ((_lib.TRAIN_PARAMS, n - 1), (_lib.TRAIN_GRADS, n + 1), (_lib.TRAIN_NOISE, n), (9, n), (-1, n)):
        with pytest.raises(ValueError):
            _lib.trainer_read(tr._h, what, count)
    out = np.zeros(4, np.float32)
    assert _lib.lib().bb_trainer_read(tr._h, _lib.TRAIN_PARAMS, None, n) == _lib.ERR_ARG
    assert _lib.lib().bb_trainer_param_count(tr._h, None) == _lib.ERR_ARG and not out.any()
    with pytest.raises(ValueError):
        tr.step(np.zeros((5, H, Wd, 3)), np.zeros(5), np.zeros((5, A)), 0.01)   # more than max_batch
    torch.cuda.synchronize()
    tr.close()
    for device in (-1, _lib.lib().bb_device_count()):   # the ordinal is checked against the devices present
        with pytest.raises(ValueError):
            _lib.trainer_create(_lib.GAME_CONNECT4, W.flatten(W.init_weights(3, 16, 1, 4, A)), H, Wd, _lib.OPT_SGD, 4, device=device)


# ---- the front end --------------------------------------------------------------------------------------------------------
def _cfg(backend, epsilon=0.0, blocks=4, filters=16):
    training = {"optimizer": "adam"}
    if backend:
        training["backend"] = backend
    return {"blocks": blocks, "filters": filters, "eval": {"dense": 16}, "hasTeacher": False,
            "policy": {"dirichlet": {"alpha": 0.2, "epsilon": epsilon}}, "training": training}


def test_same_training_as_the_pytorch_trainer(tmp_path, monkeypatch):
    """Two batches of 50 real self-play records through Blackbird.TrainWithDeviceExamples, once per backend, from the same
    weights and numpy seed; epsilon = 0, so neither draws noise."""
    monkeypatch.chdir(tmp_path)
    mcts = {"explorationRate": 0.85, "playLimit": 16}
    a = Blackbird.Model(Connect4.BoardState, "hip", mcts, _cfg("hip"))
    b = Blackbird.Model(Connect4.BoardState, "torch", mcts, _cfg(None))
    assert a.epsilon == 0 and all(np.array_equal(a._weights[k], b._weights[k]) for k in a._weights)
    w0 = {k: v.copy() for k, v in a._weights.items()}
    a.KeepDeviceExamples = True
    np.random.seed(31)
    Blackbird.GenerateTrainingSamples(a, 64, 1.0)
    kept = a.KeptDeviceExamples()
    assert len(kept) >= 100
    ex = DeviceExamples(_lib.GAME_CONNECT4, kept.records[:120].clone())   # an epoch of two whole batches of 50
    x = _lib.game_encode(_lib.GAME_CONNECT4, _lib.game_initial(_lib.GAME_CONNECT4))
    a.getEvaluation(x)                                                     # the engine behind it holds the OLD weights
    for model in (a, b):
        np.random.seed(5)
        Blackbird.TrainWithDeviceExamples(model, 50, 0.01, examples=ex)
    assert type(a._trainer) is HipTrainer and type(b._trainer) is Trainer
    assert a.batchCount == b.batchCount == 2 and sorted(a._weights) == sorted(b._weights)
    moved = 0
    for k in sorted(b._weights):
        close(a._weights[k], b._weights[k], k)
        moved += not np.array_equal(a._weights[k], w0[k])
    assert moved > len(w0) // 2
    # the engine after the reload computes the network of the exported weights
    planes = np.concatenate([x, kept.batch(np.arange(6))[0].cpu().numpy().astype(np.int8)])
    after = a._eval_engine.net_eval(planes=planes)
    fresh_engine = _lib.Engine(_lib.GAME_CONNECT4, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET)
    fresh_engine.load_weights(W.flatten(a._weights))
    fresh = fresh_engine.net_eval(planes=planes)
    for got, want in zip(after, fresh):
        assert np.array_equal(got, want)
    fresh_engine.close()
    a._batch_engine.close()
    a.Conn.Close()
    b.Conn.Close()


def test_front_end(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from blackbird_amd.Network import Network
    from blackbird_amd.NetworkFactory import NetworkFactory
    net = Network("h_1", NetworkFactory(_cfg("hip", 0.3, blocks=1), 7, inputShape=(6, 7, 3)))
    boards, ev, pl, _nz = make_batch(6, 7, 7, 4, 90)
    w_old = {k: v.copy() for k, v in net._weights.items()}
    net.train(boards, ev, pl, 0.01)
    assert type(net._trainer) is HipTrainer and net.batchCount == 1
    assert any(not np.array_equal(net._weights[k], w_old[k]) for k in w_old)
    with pytest.raises(NotImplementedError):
        net.train(boards, ev, pl, teacher=object())
    assert net.loadModel("h_1") and net._trainer is None          # parameters and slots of the old weights are dropped
    with pytest.raises(ValueError, match="16 filters"):
        Network("w_1", NetworkFactory(_cfg("hip", blocks=1, filters=32), 7, inputShape=(6, 7, 3)))._trainer_for(3)
    with pytest.raises(ValueError, match="Connect4 or TicTacToe"):
        Network("d_1", NetworkFactory(_cfg("hip", blocks=1), 4032, inputShape=(8, 8, 17)))._trainer_for(17)
