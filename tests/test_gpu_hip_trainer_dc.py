"""-m gpu: the DragonChess training step as HIP kernels (training.HipTrainer over bb_trainer_*; k_train_prep_wide and
k_train_grad with its wide policy head, csrc/train.hip.h) against the float64 statement of tests/trainer_cases.py on the batches of
tests/dc_trainer_cases.py (tests/test_hip_trainer_dc_cpu.py checks both): the loss terms and the gradient of every variable
over the shapes, at live inputs, two steps per optimiser, bit-repeatability, the drawn noise, an all-terminal batch, the same
training as the PyTorch trainer over real self-play records, the hand-off to an engine, the front end and the refusals.

Tolerance: tests/trainer_cases.close -- 1e-5 of max(1, largest |entry|) per tensor; the live case adds close_live under
live_tol (8 float32-statement errors, capped at 1e-5).  Every one of these tests fails without the feature: HipTrainer raises
ValueError for 17 planes and 4032 actions."""
import numpy as np
import pytest
import torch

from blackbird_amd import _lib
from blackbird_amd import weights as W
from blackbird_amd.training import DeviceExamples, HipTrainer, Trainer
from tests import dc_trainer_cases as DCC
from tests import selfplay_cases as SP
from tests.trainer_cases import ALPHA, EPS, RefOptimizer, close, close_live, statement

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DC = _lib.GAME_DRAGONCHESS
AUTO, F32 = _lib.NET_FORM_AUTO, _lib.NET_FORM_F32


def _w64(w):
    return {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}


def _trainer(w0, kind="adam", eps=EPS, seed=11, max_batch=17):
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


# R in {0, 1, 2, R_max} (the activation buffers change roles per layer; R_max fills the LDS of a CU), D in {1, 16, 64}, B in
# {1 -- the one row is the terminal example --, 2, 6, 17}
SHAPES = [(0, 1, 1), (1, 16, 2), (2, 64, 6), (DCC.R_MAX, 16, 17)]


@pytest.mark.parametrize("eps", [EPS, 0.0])
@pytest.mark.parametrize("R,D,B", SHAPES)
def test_gradients_over_shapes(R, D, B, eps):
    w0 = DCC.weights(R, D, 5 + R)
    tr = _trainer(w0, "sgd", eps=eps)
    assert (tr.C, tr.F, tr.R, tr.D, tr.A, tr.wide) == (17, 16, R, D, 4032, True)
    batch = DCC.make_batch(B, 60 + B)
    _check_gradients(tr, _w64(w0), batch, eps, (R, D, B, eps), noise="given" if eps else None)
    if eps == 0.0:
        assert not tr.last_noise().any()            # epsilon = 0: no draw
    else:
        assert np.array_equal(tr.last_noise(), batch[3].astype(np.float32))
    after = tr.export()
    for k in w0:                                    # apply = 0 moves nothing
        assert np.array_equal(after[k], w0[k]), k
    tr.close()


def test_gradients_live():
    """The gradient of every variable at the live case of tests/dc_trainer_cases.py (R 1, D 16, B 2, every row labelled;
    test_the_live_case_is_live asserts trainer_cases.assert_live on the statement alone), under the rule of
    tests/test_gpu_hip_trainer.py::test_gradients_live: per tensor within tol * max|data gradient| + 2**-23 * max|want| of the
    float64 statement, tol = min(8 f, 1e-5) with f the error of the float32 statement on the CPU.  The slices a 16-channel or a
    16-actions-a-thread mapping would miss -- conv_block/conv/kernel[:, :, 16, :], policy/policy/kernel[:, 4016:] and
    policy/policy/bias[4016:] -- are non-zero in the statement and held to the same bound on their own.
    Measured on the MI355X (f on its host CPU), f / the kernel's error in the same measure / tol: 1.24e-6 / 4.18e-6 / 9.95e-6;
    the three slices alone: 2.2e-6, 7.7e-8 and 7.4e-7."""
    ref = DCC.live_case()
    w0, batch, want, tol = ref["w"], ref["batch"], ref["want"], ref["tol"]
    tr = _trainer(w0, "sgd")
    total, parts, grads = tr.gradients(batch[0], batch[1], batch[2], noise=batch[3])
    r_total, r_parts, r_grads, r_data, _live = want
    close(total, r_total, "live loss")
    for got, r, name in zip(parts, r_parts, ("lossEvaluation", "lossPolicy", "lossParam")):
        close(got, r, ("live", name))
    assert set(grads) == set(r_grads)
    worst = 0.0
    for k in r_grads:
        g = grads[k].cpu().numpy()
        close(g, r_grads[k], ("live grad", k))
        worst = max(worst, close_live(g, r_grads[k], float(np.abs(r_data[k]).max()), tol, ("live grad", k)))
    for k, s in DCC.LIVE_SLICES.items():
        g, r = grads[k].cpu().numpy()[s], r_grads[k][s]
        assert np.abs(r_data[k][s]).max() >= 1e-3 and g.any(), k
        worst = max(worst, close_live(g, r, float(np.abs(r_data[k][s]).max()), tol, ("live slice", k)))
    print("live: float32 statement %.3g kernel %.3g tolerance %.3g" % (ref["figure"], worst, tol))
    tr.close()


@pytest.mark.parametrize("kind", ["adam", "momentum", "sgd"])
def test_two_steps_match_the_statement(kind):
    w0 = DCC.weights(2, 16, 3)
    tr = _trainer(w0, kind)
    assert (tr.kind, tr.momentum, tr.alpha, tr.epsilon) == (kind, 0.9, ALPHA, EPS)
    ref_opt = RefOptimizer(kind, 0.9)
    lr = 1e-2
    for step in range(2):  # the second step exercises the optimiser's slots
        batch = DCC.make_batch(6, 40 + step)
        here = _w64(tr.export())
        grads = _check_gradients(tr, here, batch, EPS, (kind, step))
        # the update rule is checked on the gradients the step used (tests/test_gpu_hip_trainer.py says why); the step recomputes
        # exactly these: the kernels are bit-repeatable (test_repeatable_and_noise_readback)
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


def _run_steps(w0, seed, noises=(None, None, None)):
    tr = _trainer(w0, "adam", seed=seed)
    losses, drawn, grads = [], [], []
    for step, nz in enumerate(noises):
        boards, ev, pl, _nz = DCC.make_batch(6, 70 + step)
        total, parts = tr.step(boards, ev, pl, 1e-2, noise=nz)
        losses.append([total] + parts)
        drawn.append(tr.last_noise())
        grads.append(_lib.trainer_read(tr._h, _lib.TRAIN_GRADS))
    out = (tr.export(), tr.slots(), np.array(losses), drawn, grads)
    tr.close()
    return out


def _same_bits(a, b):
    assert np.array_equal(a[2], b[2]), "losses"
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), ("parameters", k)
    for sa, sb in zip(a[1], b[1]):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), ("slots", k)
    for ga, gb in zip(a[4], b[4]):
        assert np.array_equal(ga, gb), "gradients"


def test_repeatable_and_noise_readback():
    w0 = DCC.weights(2, 16, 3)
    one, two = _run_steps(w0, 21), _run_steps(w0, 21)
    _same_bits(one, two)                           # no sum depends on scheduling
    assert np.isfinite(one[2]).all() and not np.array_equal(one[2][0], one[2][1])
    for a, b in zip(one[3], two[3]):
        assert np.array_equal(a, b)
    twin = _run_steps(w0, 999, noises=one[3])      # a twin that is GIVEN the draws the first one made computes the same bits
    _same_bits(one, twin)


def test_drawn_noise():
    """4032 draws in (0, 1) a step, read back as drawn, another draw on the next step and under another seed; their mean is
    Beta(0.2, 0.8)'s 0.2 (standard deviation 0.283: the mean of 4032 draws has standard error 0.0045; five of them)."""
    w0 = DCC.weights(0, 1, 1)
    boards, ev, pl, _nz = DCC.make_batch(2, 80)
    draws = []
    for seed in (5, 5, 6):
        tr = _trainer(w0, "sgd", seed=seed, max_batch=2)
        for _step in range(2):
            tr.gradients(boards, ev, pl)
            draws.append(tr.last_noise())
        tr.close()
    for d in draws:
        assert d.shape == (4032,) and d.dtype == np.float32 and ((d > 0) & (d < 1)).all()
        print("mean of the draws", d.mean())
        assert abs(float(d.mean()) - ALPHA) <= 0.0225
    assert np.array_equal(draws[0], draws[2]) and np.array_equal(draws[1], draws[3])     # the same seed: the same stream
    assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[0], draws[4])
    # a step that is GIVEN the drawn noise has the loss of the step that drew it
    tr = _trainer(w0, "sgd", seed=5, max_batch=2)
    drew = tr.gradients(boards, ev, pl)[:2]
    given = tr.gradients(boards, ev, pl, noise=draws[0])[:2]
    assert drew == given
    tr.close()


def test_zero_policy_labels_leave_the_l2_part_only():
    w0 = DCC.weights(2, 16, 3)
    tr = _trainer(w0, "sgd")
    batch = DCC.make_batch(6, 45, zero_labels=True)
    grads = _check_gradients(tr, _w64(w0), batch, EPS, "zero labels")
    n_l2 = np.float32(sum(1 for k in grads if "bias" not in k))
    for k, g in grads.items():
        if k.startswith("policy/"):
            want = np.zeros_like(w0[k]) if "bias" in k else w0[k] / n_l2
            assert np.array_equal(g.cpu().numpy(), want), k
    tr.close()


# ---- real records, the front end, the hand-off -----------------------------------------------------------------------------
def _cfg(backend, hip_games=None, epsilon=0.0, blocks=1, handoff=None):
    training = {"optimizer": "adam"}
    if backend:
        training["backend"] = backend
    if hip_games:
        training["hip_games"] = hip_games
    if handoff:
        training["handoff"] = handoff
    return {"blocks": blocks, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
            "policy": {"dirichlet": {"alpha": 0.2, "epsilon": epsilon}}, "training": training}


def _network(name, cfg):
    from blackbird_amd.Network import Network
    from blackbird_amd.NetworkFactory import NetworkFactory
    return Network(name, NetworkFactory(cfg, DCC.A, inputShape=(DCC.H, DCC.Wd, DCC.C)))


def _records():
    """A 4-game, 8-simulation self-play run of at most 8 plies under the deterministic evaluator, as device examples."""
    eng = _lib.Engine(DC, n_slots=4, sims_per_move=8, evaluator=_lib.EVAL_HASH, hash_salt=5, seed=3, max_games=4, max_plies=8)
    SP.play_to_end(eng, 4, 4, 1.0, steps_below=64)
    ex = DeviceExamples.from_engine(eng, DEV)
    eng.close()
    return ex


def test_same_training_as_the_pytorch_trainer(tmp_path, monkeypatch):
    """Two batches of real DragonChess records through DeviceExamples.batch and step_tensors, once per backend, from the same
    weights; epsilon = 0, so neither draws noise."""
    monkeypatch.chdir(tmp_path)
    ex = _records()
    n = len(ex)
    B = min(n // 2, 12)
    assert B >= 8 and ex.bad() == 0
    a = _network("dc_1", _cfg("hip", "all"))
    b = _network("dc_1", _cfg(None))                       # (loads the weights the first one saved)
    w0 = {k: v.copy() for k, v in a._weights.items()}
    assert all(np.array_equal(w0[k], b._weights[k]) for k in w0)
    ta, tb = a._trainer_for(17), b._trainer_for(17)
    assert type(ta) is HipTrainer and ta.wide and type(tb) is Trainer
    labelled = 0
    for i in range(2):
        boards, value, policy = ex.batch(np.arange(i * B, (i + 1) * B))
        labelled += int((policy != 0).any(dim=1).sum())
        assert boards[..., 16].any()
        la = ta.step_tensors(boards, value, policy, 0.01)
        lb = tb.step_tensors(boards, value, policy, 0.01)
        close(float(la[0]), float(lb[0]), ("loss", i))
    assert labelled >= B
    wa, wb = ta.export(), tb.export()
    moved = 0
    for k in sorted(wb):
        close(wa[k], wb[k], k)
        moved += not np.array_equal(wa[k], w0[k])
    assert moved > len(w0) // 2
    ta.close()


@pytest.mark.parametrize("handoff", [None, "device"])
def test_front_end(tmp_path, monkeypatch, handoff):
    """Network.train on a DragonChess network with backend 'hip' and hip_games 'all', under both hand-offs: the engine behind
    getEvaluation computes the network of the trained weights."""
    monkeypatch.chdir(tmp_path)
    net = _network("f_1", _cfg("hip", "all", epsilon=0.3, handoff=handoff))
    boards, ev, pl, _nz = DCC.make_batch(4, 90)
    w_old = {k: v.copy() for k, v in net._weights.items()}
    net.getEvaluation(boards[:1])                           # the engine holds the OLD weights
    net.train(boards, ev, pl, 0.01)
    assert type(net._trainer) is HipTrainer and net.batchCount == 1
    w_new = net._weights
    assert any(not np.array_equal(w_new[k], w_old[k]) for k in w_old)
    after = net._eval_engine.net_eval(planes=boards)
    fresh = _lib.Engine(DC, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET, max_plies=4)
    fresh.load_weights(W.flatten(w_new))
    for got, want in zip(after, fresh.net_eval(planes=boards)):
        assert np.array_equal(got, want)
    fresh.close()
    with pytest.raises(ValueError, match="Connect4 or TicTacToe"):       # without the second key: today's refusal
        _network("g_1", _cfg("hip"))._trainer_for(17)


@pytest.mark.parametrize("net_form", [AUTO, F32])
def test_load_into_is_the_host_route(net_form):
    w0 = DCC.weights(2, 16, 11)
    tr = _trainer(w0, "adam", max_batch=4)
    boards, ev, pl, nz = DCC.make_batch(4, 91)
    tr.step(boards, ev, pl, 0.01, noise=nz)
    a = _lib.Engine(DC, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET, net_form=net_form, max_plies=4)
    b = _lib.Engine(DC, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET, net_form=net_form, max_plies=4)
    try:
        a.load_weights(W.flatten(tr.export()))              # the host route
        b.load_weights(W.flatten(w0))                       # ... and B holds the weights from before the step
        tr.load_into(b)
        for k in _lib.WEIGHTS_IMAGES:
            x, y = a.weights_image(k), b.weights_image(k)
            assert x.shape == y.shape and np.array_equal(x, y), k
        for x, y, name in zip(a.net_eval(planes=boards), b.net_eval(planes=boards), ("value", "logits", "policy")):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    finally:
        a.close()
        b.close()
        tr.close()


def test_refusals_leave_the_trainer_working(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    w0 = DCC.weights(1, 16, 2)
    tr = _trainer(w0, "sgd", max_batch=4)
    boards, ev, pl, nz = DCC.make_batch(4, 92)
    ex = _records()
    order = ex.index_tensor(np.arange(4))

    def still_steps(what):
        before = tr.export()
        total, _parts = tr.step(boards, ev, pl, 0.01, noise=nz)
        after = tr.export()
        assert np.isfinite(total) and any(not np.array_equal(after[k], before[k]) for k in before), what

    with pytest.raises(ValueError, match="records source"):
        tr.epoch_records(ex, order, 4, 0.01)
    still_steps("epoch_records")
    with pytest.raises(ValueError, match="records source"):
        tr.evaluate_records(ex)
    still_steps("evaluate_records")
    with pytest.raises(ValueError, match="records source"):
        tr.evaluate_tensors(*ex.batch(np.arange(4)))
    still_steps("evaluate_tensors")
    # the library's own refusals, below the Python checks
    t = torch.zeros(8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="DragonChess"):
        _lib.trainer_epoch(tr._h, len(ex), ex.records.data_ptr(), 1, 4, order.data_ptr(), bad=ex._bad.data_ptr())
    with pytest.raises(ValueError, match="DragonChess"):
        _lib.trainer_eval(tr._h, len(ex), ex.records.data_ptr(), 4, totals_out=t.data_ptr())
    with pytest.raises(ValueError, match="DragonChess"):
        _lib.trainer_eval_tensors(tr._h, 0, None, None, None, totals_out=t.data_ptr())
    still_steps("the library's refusals")
    big = DCC.make_batch(5, 93)
    with pytest.raises(ValueError, match="max_batch"):
        tr.step(big[0], big[1], big[2], 0.01, noise=big[3])
    still_steps("a batch above max_batch")
    with pytest.raises(ValueError):
        _lib.trainer_read(tr._h, _lib.TRAIN_NOISE, 16)       # the noise of this game is A = 4032 floats
    assert tr.last_noise().shape == (4032,)
    tr.close()

    # fused=True: the epoch call does not cover the game, and says so before anything is trained
    from blackbird_amd import Blackbird, DragonChess
    model = Blackbird.Model(DragonChess.BoardState, "fused", {"explorationRate": 0.85, "playLimit": 8}, _cfg("hip", "all"))
    w_before = {k: v.copy() for k, v in model._weights.items()}
    np.random.seed(5)
    with pytest.raises(ValueError, match="records source"):
        Blackbird.TrainWithDeviceExamples(model, 4, 0.01, examples=ex, fused=True)
    assert model.batchCount == 0 and all(np.array_equal(model._weights[k], w_before[k]) for k in w_before)
    np.random.seed(5)
    Blackbird.TrainWithDeviceExamples(model, 4, 0.01, examples=ex)          # the per-batch loop trains it
    assert model.batchCount == len(ex) // 4 and type(model._trainer) is HipTrainer
    assert any(not np.array_equal(model._weights[k], w_before[k]) for k in w_before)
    model.Conn.Close()
