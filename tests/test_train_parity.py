"""one Network.train step (blackbird_amd/training.py, PyTorch-ROCm float32, NCHW conv2d) against an
INDEPENDENT statement of the reference's training graph (/root/reference/src/NetworkFactory.py:37-245) written here in
float64 as shifted-window einsum contractions in NHWC with a hand-written optimiser in numpy:

  * the three loss terms (value MSE :187-188, the BxB policy cross term :190-194, the unweighted L2 mean over non-bias
    trainables :196-201), with the graph's shared Beta noise and batch-wide normalisation (:176-182) inside;
  * d loss / d variable for EVERY trainable variable;
  * the variables after one and two optimiser steps for adam / momentum / sgd (TF1 update rules, :234-242).

Tolerance 1e-5 (BASELINE.json north_star) relative to the largest entry of each tensor.  TensorFlow itself is not
installable here, so this pins the implementation to the published formulas, not to TF's binaries ("parity unpinned by
the reference").  The CPU variant runs in the `not gpu` suite; the `gpu` variant runs the same step on the
MI355X and also checks that the engine's logits after the weight reload are those of the exported weights."""
import numpy as np
import pytest
import torch

from blackbird_amd import weights as W
from blackbird_amd.training import Trainer
from tests.trainer_cases import ALPHA, EPS, A, C, D, F, H, R, TOL, Wd, _batch, _close, _ref_grads, _RefOptimizer

def _check_step(device, kind):
    w0 = W.init_weights(C, F, R, D, A, seed=3, perturb=True)
    tr = Trainer(w0, alpha=ALPHA, epsilon=EPS, optimizer=kind, momentum=0.9, device=device)
    ref_opt = _RefOptimizer(kind, 0.9)
    lr = 1e-2
    for step in range(2):  # the second step exercises the optimiser's slots (m, v, beta powers / the accumulator)
        batch = _batch(40 + step)
        here = {k: np.asarray(v, dtype=np.float64) for k, v in tr.export().items()}
        total, parts, grads = tr.gradients(*batch)
        r_total, r_parts, r_grads = _ref_grads(here, batch)
        _close(total, r_total, (kind, step, "loss"))
        for got, want, name in zip(parts, r_parts, ("lossEvaluation", "lossPolicy", "lossParam")):
            _close(got, want, (kind, step, name))
        assert set(grads) == set(r_grads)
        for k in r_grads:
            _close(grads[k].detach().cpu().numpy(), r_grads[k], (kind, step, "grad", k))
        # The update rule is checked on the gradients the step actually used: Adam maps g to g / (|g| + 3.2e-7) on its
        # first step, which turns the 1e-8 rounding of a float32 gradient near zero into percents of lr -- that
        # conditioning belongs to the optimiser (TF's float32 kernels have it too), not to either implementation.
        g64 = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in grads.items()}
        tr.step(batch[0], batch[1], batch[2], lr, noise=batch[3])
        want_w = ref_opt.apply(here, g64, lr)
        new = tr.export()
        for k in want_w:
            _close(new[k], want_w[k], (kind, step, "weights", k))
            if k in g64 and np.abs(g64[k]).max() > 1e-6:
                assert not np.array_equal(new[k], here[k].astype(np.float32)), (kind, step, "did not move", k)
    return tr


@pytest.mark.parametrize("kind", ["adam", "momentum", "sgd"])
def test_train_step_matches_independent_statement_cpu(kind):
    _check_step("cpu", kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["adam", "momentum", "sgd"])
def test_train_step_matches_independent_statement_gpu(kind, orc):
    tr = _check_step("cuda", kind)
    # the engine after the reload computes the network of the exported weights (and the oracle agrees within 1e-5)
    from blackbird_amd import _lib
    game = _lib.GAME_CONNECT4
    flat = W.flatten(tr.export())
    boards = _batch(7)[0]
    a = _lib.Engine(game, n_slots=2, sims_per_move=2, evaluator=_lib.EVAL_NET)
    a.load_weights(W.flatten(W.init_weights(C, F, R, D, A, seed=3, perturb=True)))
    before = a.net_eval(planes=boards)
    a.load_weights(flat)                      # what Model._weights_changed does after train()
    after = a.net_eval(planes=boards)
    b = _lib.Engine(game, n_slots=2, sims_per_move=2, evaluator=_lib.EVAL_NET)
    b.load_weights(flat)
    fresh = b.net_eval(planes=boards)
    assert not np.array_equal(before[1], after[1])
    for x, y in zip(after, fresh):
        assert np.array_equal(x, y)
    ov, ol, op = orc.net_forward(orc.NetWeights(H, Wd, C, F, R, D, A, flat), boards)
    assert np.max(np.abs(after[0] - ov)) <= TOL and np.max(np.abs(after[1] - ol) / np.maximum(1.0, np.abs(ol))) <= TOL
    # and the trainer's own forward (the graph that was differentiated) is that network too
    with torch.no_grad():
        tv, tl = tr.forward(torch.tensor(boards.astype(np.float32), device=tr.device))
    assert np.max(np.abs(tv.cpu().numpy() - after[0])) <= TOL
    assert np.max(np.abs(tl.cpu().numpy() - after[1]) / np.maximum(1.0, np.abs(after[1]))) <= TOL
    a.close()
    b.close()


def test_teacher_is_refused_and_reload_resets_the_trainer(tmp_path, monkeypatch):
    """train(teacher=...) must not silently drop the term; loadModel must not leave a stale optimiser."""
    monkeypatch.chdir(tmp_path)
    from blackbird_amd.Network import Network
    from blackbird_amd.NetworkFactory import NetworkFactory
    cfg = {"blocks": 1, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}
    net = Network("t_1", NetworkFactory(cfg, 7, inputShape=(6, 7, 3)))
    with pytest.raises(NotImplementedError):
        net.train(np.zeros((2, 6, 7, 3), np.int8), np.zeros(2), np.zeros((2, 7)), teacher=object())
    net._trainer = object()  # stands for a trainer built from older weights
    assert net.loadModel("t_1") and net._trainer is None
