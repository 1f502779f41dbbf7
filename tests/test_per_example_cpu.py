"""No GPU: the per-example policy loss (NetworkConfig['training']['loss'] = 'per_example') in the PyTorch trainer against the
float64 statement of tests/per_example_cases.py, the validation of the two new keys in every layer that reads them, and the
learning case that is the reason for the option: the reference loss trains every row towards the batch's summed label, this one
towards its own.

Tolerance: tests/trainer_cases.close -- 1e-5 of max(1, largest |entry|) per tensor, the rule of tests/test_train_parity.py.
Every test here fails without the feature: Trainer takes no `loss` argument and bb_trainer_set_loss does not exist."""
import numpy as np
import pytest
import torch

from blackbird_amd import _lib
from blackbird_amd import weights as W
from blackbird_amd.training import HipTrainer, Trainer
from tests import per_example_cases as PE
from tests.trainer_cases import GAMES, make_batch

L2 = 1e-4


# ---- the loss and every gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,R,D,B", [("connect4", 2, 16, 6), ("tictactoe", 1, 64, 5)])
@pytest.mark.parametrize("labels", ["terminal row", "all terminal"])
def test_trainer_matches_the_statement(game, R, D, B, labels):
    _g, H, Wd, A = GAMES[game]
    w0 = W.init_weights(3, 16, R, D, A, seed=3 + R, perturb=True)
    boards, ev, pl, _nz = make_batch(H, Wd, A, B, 40 + B, zero_labels=labels == "all terminal")
    assert not pl[-1].any() and pl[0].any() == (labels == "terminal row")
    tr = Trainer(w0, optimizer="sgd", device="cpu", loss="per_example", l2=L2)
    assert (tr.loss_kind, tr.l2) == ("per_example", L2)
    grads = PE.check_against_statement(tr, PE.w64(w0), (boards, ev, pl), L2, (game, labels))
    _total, terms, _g2 = tr.gradients(boards, ev, pl)
    want_l2 = L2 * sum(0.5 * float((np.asarray(v, dtype=np.float64) ** 2).sum()) for k, v in w0.items()
                       if "bias" not in k and "moving" not in k)
    PE.close(terms[2], want_l2, (game, labels, "lossParam, by hand"))
    if labels == "all terminal":
        assert terms[1] == 0.0
        plain = Trainer(w0, optimizer="sgd", device="cpu", loss="per_example", l2=0.0)
        _t, terms0, g0 = plain.gradients(boards, ev, pl)
        assert terms0[1] == 0.0 and terms0[2] == 0.0
        for k, g in g0.items():                       # no label anywhere: the policy head has exactly no gradient
            if k.startswith("policy/"):
                assert not g.any(), k
            else:
                assert g.any(), k
        for k in grads:                               # ... and with the L2 term its gradient is l2 * v alone
            if k.startswith("policy/") and "bias" not in k:
                PE.close(grads[k], L2 * np.asarray(w0[k], dtype=np.float64), (game, "l2 * v", k))


def test_a_terminal_row_adds_nothing_to_the_policy_loss():
    """The batch with its terminal row and the batch without it have the same sum over the labelled rows: n * lossPolicy agrees."""
    _g, H, Wd, A = GAMES["connect4"]
    w0 = W.init_weights(3, 16, 1, 16, A, seed=4, perturb=True)
    boards, ev, pl, _nz = make_batch(H, Wd, A, 6, 46)
    tr = Trainer(w0, device="cpu", loss="per_example", l2=L2)
    with_row = tr.gradients(boards, ev, pl)[1][1]
    without = tr.gradients(boards[:5], ev[:5], pl[:5])[1][1]
    PE.close(6 * with_row, 5 * without, "n * lossPolicy")


def test_the_reference_loss_is_the_default_and_unchanged():
    _g, H, Wd, A = GAMES["connect4"]
    w0 = W.init_weights(3, 16, 1, 16, A, seed=4, perturb=True)
    boards, ev, pl, nz = make_batch(H, Wd, A, 6, 47)
    a, b = Trainer(w0, device="cpu"), Trainer(w0, device="cpu", loss="reference", l2=0.5)     # (l2 is not read)
    assert a.loss_kind == "reference"
    ta, pa, ga = a.gradients(boards, ev, pl, noise=nz)
    tb, pb, gb = b.gradients(boards, ev, pl, noise=nz)
    assert ta == tb and pa == pb and all(torch.equal(ga[k], gb[k]) for k in ga)
    pe = Trainer(w0, device="cpu", loss="per_example").gradients(boards, ev, pl)
    assert pe[1][0] == pa[0] and pe[1][1] != pa[1]                   # the value term is shared, the policy term is another


# ---- validation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(loss="per-example"), dict(loss=None), dict(loss=1), dict(l2=-1e-4), dict(l2=float("nan")),
                                 dict(l2=float("inf")), dict(l2=-float("inf")), dict(l2="much"), dict(l2=1e39)])
def test_both_trainers_refuse_a_bad_loss_or_l2(bad):
    w0 = W.init_weights(3, 16, 1, 4, 7, seed=1)
    kw = {"loss": "per_example", **bad}
    with pytest.raises(ValueError, match="l2" if "l2" in bad else "loss"):
        Trainer(w0, device="cpu", **kw)
    with pytest.raises(ValueError, match="l2" if "l2" in bad else "loss"):       # before any device call: with or without a GPU
        HipTrainer(w0, device="cuda", **kw)
    if "l2" in bad:                                                                # ... whichever loss is chosen
        with pytest.raises(ValueError, match="l2"):
            Trainer(w0, device="cpu", **bad)


def test_noise_is_refused_in_per_example_mode():
    _g, H, Wd, A = GAMES["connect4"]
    w0 = W.init_weights(3, 16, 1, 4, A, seed=1)
    boards, ev, pl, nz = make_batch(H, Wd, A, 4, 48)
    tr = Trainer(w0, device="cpu", loss="per_example")
    before = tr.export()
    with pytest.raises(ValueError, match="noise"):
        tr.gradients(boards, ev, pl, noise=nz)
    with pytest.raises(ValueError, match="noise"):
        tr.step(boards, ev, pl, 0.01, noise=nz)
    t = [torch.tensor(np.asarray(x, dtype=np.float32)) for x in (boards, ev, pl, nz)]
    with pytest.raises(ValueError, match="noise"):
        tr.step_tensors(t[0], t[1], t[2], 0.01, noise=t[3])
    after = tr.export()
    assert tr.t == 0 and all(np.array_equal(after[k], before[k]) for k in before)
    tr.step(boards, ev, pl, 0.01)                                                  # without one it steps
    assert tr.t == 1


def test_the_library_refuses_a_bad_loss_before_any_device_call():
    """bb_trainer_set_loss checks its two numbers before it looks at the trainer, so the refusal names what is wrong with or
    without a GPU; a null trainer is refused too."""
    L = _lib.lib()
    assert (_lib.LOSS_REFERENCE, _lib.LOSS_PER_EXAMPLE) == (0, 1)
    for loss, l2, word in ((2, 0.0, "unknown loss"), (-1, 0.0, "unknown loss"), (1, -1e-4, "l2"), (1, float("nan"), "l2"),
                           (1, float("inf"), "l2"), (0, -1.0, "l2"), (1, 1e39, "l2"), (1, 1e-4, "null trainer"),
                           (0, 0.0, "null trainer")):
        assert L.bb_trainer_set_loss(None, loss, l2) == _lib.ERR_ARG, (loss, l2)
        assert word in _lib.last_error(), (loss, l2, _lib.last_error())
        with pytest.raises(ValueError, match=word):
            _lib.trainer_set_loss(None, loss, l2)


def _net(tmp_path, monkeypatch, training, name):
    monkeypatch.chdir(tmp_path)
    from blackbird_amd.Network import Network
    from blackbird_amd.NetworkFactory import NetworkFactory
    cfg = {"blocks": 1, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
           "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": training}
    return Network(name, NetworkFactory(cfg, 7, inputShape=(6, 7, 3)))


def test_the_front_end_reads_and_validates_the_keys(tmp_path, monkeypatch):
    tr = _net(tmp_path, monkeypatch, {"optimizer": "adam"}, "d_1")._trainer_for(3)
    assert type(tr) is Trainer and (tr.loss_kind, tr.l2) == ("reference", 1e-4)
    tr = _net(tmp_path, monkeypatch, {"optimizer": "adam", "loss": "per_example"}, "p_1")._trainer_for(3)
    assert (tr.loss_kind, tr.l2) == ("per_example", 1e-4)
    tr = _net(tmp_path, monkeypatch, {"optimizer": "sgd", "loss": "per_example", "l2": 0}, "p_2")._trainer_for(3)
    assert (tr.loss_kind, tr.l2, tr.kind) == ("per_example", 0.0, "sgd")
    for training, word in (({"loss": "alphazero"}, "loss"), ({"loss": "per_example", "l2": -1.0}, "l2"),
                           ({"loss": "per_example", "l2": float("nan")}, "l2"), ({"l2": -1.0}, "l2"),
                           ({"backend": "hip", "loss": "cross"}, "loss")):
        net = _net(tmp_path, monkeypatch, {"optimizer": "adam", **training}, "bad_1")
        with pytest.raises(ValueError, match=word):
            net._trainer_for(3)
        assert net._trainer is None
    net = _net(tmp_path, monkeypatch, {"optimizer": "adam", "loss": "per_example", "l2": 1e-3}, "t_1")
    boards, ev, pl, _nz = make_batch(6, 7, 7, 4, 49)
    w_old = {k: v.copy() for k, v in net._weights.items()}
    net.train(boards, ev, pl, 0.01)                                                # Network.train draws no noise of its own
    assert net.batchCount == 1 and any(not np.array_equal(net._weights[k], w_old[k]) for k in w_old)


# ---- why the option exists ------------------------------------------------------------------------------------------------------
def test_the_per_example_loss_learns_each_rows_own_move():
    """8 distinct TicTacToe boards with one-hot labels on 3 distinct actions (3, 3 and 2 rows each), Adam, lr 1e-2, l2 1e-4, 200
    steps: the per-example loss puts every row's own move first, and its cross entropy falls.  The reference loss on the same data
    is printed, not asserted: it stays at the size of the largest label class (3 of 8; cross entropy about 1.09)."""
    w0, boards, ev, labels = PE.learning_case()
    t = [torch.tensor(x.astype(np.float32)) for x in (boards, ev, labels)]
    tr = Trainer(w0, optimizer="adam", device="cpu", loss="per_example", l2=1e-4)
    start = tr.evaluate_tensors(*t)
    assert start["policy_rows"] == 8
    for _step in range(200):
        tr.step_tensors(t[0], t[1], t[2], 1e-2)
    end = tr.evaluate_tensors(*t)
    print("per_example: top1 %d -> %d of 8, policy_ce %.4g -> %.4g" % (start["top1"], end["top1"], start["policy_ce"], end["policy_ce"]))
    ref = Trainer(w0, optimizer="adam", device="cpu", epsilon=0.3)
    torch.manual_seed(5)
    for _step in range(200):
        ref.step_tensors(t[0], t[1], t[2], 1e-2)
    after = ref.evaluate_tensors(*t)
    print("reference:   top1 %d -> %d of 8, policy_ce %.4g -> %.4g" % (start["top1"], after["top1"], start["policy_ce"], after["policy_ce"]))
    assert end["top1"] == 8 and end["policy_ce"] < start["policy_ce"]
