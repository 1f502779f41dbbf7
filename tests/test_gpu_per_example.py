"""-m gpu: the per-example policy loss as HIP kernels (training.HipTrainer(loss='per_example') over bb_trainer_set_loss; the
BB_LOSS_PER_EXAMPLE instantiations of k_train_prep / k_train_prep_wide and k_train_grad, csrc/train.hip.h) against the float64
statement of tests/per_example_cases.py: the loss terms and the gradient of every variable over the shapes where the kernels
can go wrong, at live inputs, two steps per optimiser, the PyTorch trainer on the same batches, bit-repeatability, the epoch
straight from records, the step's reported terms against the scorer, the untouched reference loss, and the front end.

Tolerance: tests/trainer_cases.close -- 1e-5 of max(1, largest |entry|) per tensor; the live cases add close_live under live_tol
(8 errors of the float32 statement, capped at 1e-5).  Every test here fails without the feature: HipTrainer takes no `loss`
argument and bb_trainer_set_loss does not exist."""
import numpy as np
import pytest
import torch

from blackbird_amd import Blackbird, Connect4, TicTacToe, _lib
from blackbird_amd import weights as W
from blackbird_amd.training import DeviceExamples, HipTrainer, Trainer
from tests import dc_trainer_cases as DCC
from tests import merge_cases as MC
from tests import model_cases as M
from tests import per_example_cases as PE
from tests.merge_cases import C4, TTT
from tests.trainer_cases import ALPHA, EPS, GAMES, TWO_STEP_CASE, RefOptimizer, close, live_case, live_tol, make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L2 = 1e-4
LR = 1e-2
BOARD_CLS = {C4: Connect4.BoardState, TTT: TicTacToe.BoardState}


def _trainer(w0, kind="sgd", l2=L2, seed=11, max_batch=130, **kw):
    kw.setdefault("loss", "per_example")
    return HipTrainer(w0, alpha=ALPHA, epsilon=EPS, optimizer=kind, momentum=0.9, device=DEV, seed=seed, max_batch=max_batch, l2=l2, **kw)


def _dense_batch(game, B, seed, **kw):
    _g, H, Wd, A = GAMES[game]
    return make_batch(H, Wd, A, B, seed, **kw)[:3]


# ---- 1. the loss terms and every gradient, over the shapes ------------------------------------------------------------------------
# Connect4: every R in {0, 2, 9}, D in {1, 16, 64}, B in {1, 6, 130} at least once, R in {0, 9} crossed with B in {1, 130}; the one
# row of a B = 1 batch is the terminal example in the first case and a labelled row in the third.  130 rows: the slab sums.
DENSE_SHAPES = [("connect4", 0, 16, 1, True), ("connect4", 0, 16, 130, True), ("connect4", 9, 16, 1, False),
                ("connect4", 9, 16, 130, True), ("connect4", 2, 1, 6, True), ("connect4", 2, 64, 6, True),
                ("tictactoe", 2, 16, 6, True), ("tictactoe", 9, 64, 130, True)]


@pytest.mark.parametrize("game,R,D,B,terminal_last", DENSE_SHAPES)
def test_gradients_over_shapes(game, R, D, B, terminal_last):
    A = GAMES[game][3]
    w0 = W.init_weights(3, 16, R, D, A, seed=5 + R, perturb=True)
    tr = _trainer(w0)
    assert (tr.loss_kind, tr.l2, tr.R, tr.D, tr.A) == ("per_example", L2, R, D, A)
    batch = _dense_batch(game, B, 60 + B, terminal_last=terminal_last)
    grads = PE.check_against_statement(tr, PE.w64(w0), batch, L2, (game, R, D, B))
    assert not tr.last_noise().any()                      # nothing is drawn
    if B == 1 and terminal_last:                          # no label at all: the policy head's gradient is l2 * v, bit for bit
        for k, g in grads.items():
            if k.startswith("policy/"):
                assert np.array_equal(g, np.zeros_like(w0[k]) if "bias" in k else np.float32(L2) * w0[k]), k
    after = tr.export()
    for k in w0:                                          # apply = 0 moves nothing
        assert np.array_equal(after[k], w0[k]), k
    tr.close()


# DragonChess: R in {0, 1}, D 16, B in {1, 4}.  tests/dc_trainer_cases.make_batch puts label mass on the actions 0, 255, 256 (the
# ends of a thread's first pass and the start of its second), 4015, 4016 (where the last partial pass stops) and 4031.
@pytest.mark.parametrize("R,B,terminal_last", [(0, 1, False), (1, 4, True), (0, 4, True), (1, 1, True)])
def test_gradients_over_shapes_dragonchess(R, B, terminal_last):
    w0 = DCC.weights(R, 16, 5 + R)
    tr = _trainer(w0, max_batch=4)
    assert tr.wide and tr.loss_kind == "per_example"
    batch = DCC.make_batch(B, 60 + B, terminal_last=terminal_last)[:3]
    if not terminal_last or B > 1:
        assert all(batch[2][0, a] > 0 for a in (0, 255, 256, 4015, 4016, 4031))
    grads = PE.check_against_statement(tr, PE.w64(w0), batch, L2, ("dragonchess", R, B))
    assert not tr.last_noise().any()
    if B == 1 and terminal_last:
        for k, g in grads.items():
            if k.startswith("policy/"):
                assert np.array_equal(g, np.zeros_like(w0[k]) if "bias" in k else np.float32(L2) * w0[k]), k
    else:                                                 # the slices a 16-passes-for-every-thread mapping would get wrong
        for a in (0, 255, 256, 4015, 4016, 4031):
            assert grads["policy/policy/bias"][a] != 0.0, a
    tr.close()


# ---- 2. live inputs: no backward factor is zero -------------------------------------------------------------------------------
def _live(w0, batch3):
    want = PE.statement(w0, *batch3, L2, parts=True)
    for k, dg in want[3].items():                         # every variable has a data gradient worth the name
        assert np.abs(dg).max() >= 1e-3, (k, np.abs(dg).max())
    figure = PE.float32_figure(w0, batch3, L2, want)
    return want, figure, live_tol(figure)


@pytest.mark.parametrize("case", [TWO_STEP_CASE, ("connect4", 2, 64, 2, 80, 101, True)], ids=str)
def test_gradients_live(case):
    """The weights and boards of the live cases of tests/trainer_cases.py (every ReLU layer partly on, the tanh unsaturated: that
    depends on weights and boards alone), under this loss: per tensor within tol * max|data gradient| + 2**-23 * max|want| of the
    float64 statement, tol = min(8 f, 1e-5), f the error of the float32 statement on the CPU.
    Measured on the MI355X (f on its host CPU), f / the kernel's error in the same measure / tol:
      tictactoe R2 D16 B6  2.5e-6 / 2.8e-6 / 1e-5      connect4 R2 D64 B2  9.4e-7 / 1.1e-6 / 7.5e-6
      dragonchess R1 D16 B2 (test_gradients_live_dragonchess)  2.0e-6 / 4.2e-6 / 1e-5"""
    ref = live_case(case)
    w0, batch = ref["w"], ref["batch"][:3]
    want, figure, tol = _live(w0, batch)
    tr = _trainer(w0)
    PE.check_against_statement(tr, PE.w64(w0), batch, L2, case, live=(want, tol))
    print(case, "float32 statement %.3g tolerance %.3g" % (figure, tol))
    tr.close()


def test_gradients_live_dragonchess():
    ref = DCC.live_case()
    w0, batch = ref["w"], ref["batch"][:3]
    want, figure, tol = _live(w0, batch)
    tr = _trainer(w0, max_batch=4)
    grads = PE.check_against_statement(tr, PE.w64(w0), batch, L2, "dragonchess live", live=(want, tol))
    for k, s in DCC.LIVE_SLICES.items():
        assert np.abs(want[3][k][s]).max() >= 1e-3 and grads[k][s].any(), k
        PE.close_live(grads[k][s], want[2][k][s], float(np.abs(want[3][k][s]).max()), tol, ("live slice", k))
    print("dragonchess live: float32 statement %.3g tolerance %.3g" % (figure, tol))
    tr.close()


# ---- 3. two optimiser steps, l2 * v in the gradient ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam", "momentum", "sgd"])
@pytest.mark.parametrize("game", ["connect4", "dragonchess"])
def test_two_steps_match_the_statement(game, kind):
    if game == "dragonchess":
        w0, batches = DCC.weights(1, 16, 3), [DCC.make_batch(4, 40 + s)[:3] for s in range(2)]
    else:
        w0, batches = W.init_weights(3, 16, 2, 16, 7, seed=3, perturb=True), [_dense_batch(game, 6, 40 + s) for s in range(2)]
    tr = _trainer(w0, kind, max_batch=6)
    ref_opt = RefOptimizer(kind, 0.9)
    for step, batch in enumerate(batches):                # the second step exercises the optimiser's slots
        here = PE.w64(tr.export())
        grads = PE.check_against_statement(tr, here, batch, L2, (game, kind, step))
        # the update rule is checked on the gradients the step used (tests/test_gpu_hip_trainer.py says why); the step recomputes
        # exactly these: the kernels are bit-repeatable (test_repeatable)
        g64 = {k: v.astype(np.float64) for k, v in grads.items()}
        total, terms = tr.step(batch[0], batch[1], batch[2], LR)
        assert isinstance(total, float) and len(terms) == 3
        want_w = ref_opt.apply(here, g64, LR)
        new = tr.export()
        for k in want_w:
            close(new[k], want_w[k], (game, kind, step, "weights", k))
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
    tr.close()


@pytest.mark.parametrize("kind", ["adam", "momentum", "sgd"])
@pytest.mark.parametrize("game", ["connect4", "dragonchess"])
def test_without_l2_a_weight_without_data_gradient_stays(game, kind):
    """l2 = 0 and a batch of terminal examples: the policy head has no gradient at all, and two steps of every optimiser leave it
    where it was, bit for bit (Adam: 0 / (sqrt(0) + 1e-8)), while everything the value loss reaches moves.  The weights and
    boards are those of a live case (at weights drawn by init_weights alone the tanh saturates and nothing would move)."""
    ref = DCC.live_case() if game == "dragonchess" else live_case(TWO_STEP_CASE)
    w0, (boards, ev, pl) = ref["w"], ref["batch"][:3]
    batch = (boards, ev, np.zeros_like(pl))
    tr = _trainer(w0, kind, l2=0.0, max_batch=6)
    grads = PE.check_against_statement(tr, PE.w64(w0), batch, 0.0, (game, kind, "l2 0"))
    for k, g in grads.items():
        assert g.any() != k.startswith("policy/"), k
    for _step in range(2):
        total, terms = tr.step(batch[0], batch[1], batch[2], LR)
        assert terms[1] == 0.0 and terms[2] == 0.0 and total == terms[0]
    new = tr.export()
    for k in w0:
        still = k.startswith("policy/") or k.endswith("moving_mean") or k.endswith("moving_variance")
        assert np.array_equal(new[k], w0[k]) == still, k
    tr.close()


# ---- 4. the PyTorch trainer on the same two batches -----------------------------------------------------------------------------
@pytest.mark.parametrize("game,kind", [("connect4", "adam"), ("tictactoe", "adam"), ("dragonchess", "momentum")])
def test_same_training_as_the_pytorch_trainer(game, kind):
    """Two batches through both trainers on the GPU, 1e-5 per tensor (the figure the README states for the reference loss, Adam on
    Connect4).  DragonChess takes Momentum, whose update is linear in the gradient: on this case 51 entries of conv_block's
    kernel have |gradient| < 1e-6 (l2 * v against a data gradient of the same size), where Adam's m / (sqrt(v) + 1e-8) turns the
    float32 rounding of a gradient into 1e-3 of lr.  That is the optimiser's conditioning and not either trainer's: with no
    kernel in play, the float32 PyTorch trainer on the CPU and the float64 statement with RefOptimizer('adam') end 1.57e-5 apart
    on that tensor after the same two steps (the HIP trainer and the PyTorch trainer on the GPU: 1.06e-5).  Adam on DragonChess
    is held to the statement on the gradients it used, in test_two_steps_match_the_statement."""
    if game == "dragonchess":
        w0, batches = DCC.weights(1, 16, 7), [DCC.make_batch(4, 50 + s)[:3] for s in range(2)]
    else:
        w0 = W.init_weights(3, 16, 2, 16, GAMES[game][3], seed=7, perturb=True)
        batches = [_dense_batch(game, 6, 50 + s) for s in range(2)]
    a = _trainer(w0, kind, max_batch=6)
    b = Trainer(w0, alpha=ALPHA, epsilon=EPS, optimizer=kind, momentum=0.9, device=DEV, loss="per_example", l2=L2)
    for step, batch in enumerate(batches):
        t = [torch.tensor(np.asarray(x, dtype=np.float32), device=DEV) for x in batch]
        la, lb = a.step_tensors(t[0], t[1], t[2], LR), b.step_tensors(t[0], t[1], t[2], LR)
        close(float(la[0]), float(lb[0]), (game, step, "loss"))
        for x, y, name in zip(la[1], lb[1], ("lossEvaluation", "lossPolicy", "lossParam")):
            close(float(x), float(y), (game, step, name))
    wa, wb = a.export(), b.export()
    moved = 0
    for k in sorted(wb):
        close(wa[k], wb[k], (game, k))
        moved += not np.array_equal(wa[k], w0[k])
    assert moved > len(w0) // 2          # (at these weights the tanh saturates: the value head's biases have no gradient)
    a.close()


# ---- 5. bit-repeatability ---------------------------------------------------------------------------------------------------
def _run(w0, batches, max_batch):
    tr = _trainer(w0, "adam", max_batch=max_batch)
    losses, grads = [], []
    for batch in batches:
        total, terms = tr.step(batch[0], batch[1], batch[2], LR)
        losses.append([total] + terms)
        grads.append(_lib.trainer_read(tr._h, _lib.TRAIN_GRADS))
    out = (tr.export(), tr.slots(), np.array(losses), grads)
    tr.close()
    return out


@pytest.mark.parametrize("game", ["connect4", "dragonchess"])
def test_repeatable(game):
    if game == "dragonchess":
        w0, batches, mb = DCC.weights(1, 16, 3), [DCC.make_batch(4, 70 + s)[:3] for s in range(2)], 4
    else:
        w0, batches, mb = W.init_weights(3, 16, 2, 16, 7, seed=3, perturb=True), [_dense_batch(game, 130, 70 + s) for s in range(2)], 130
    one, two = _run(w0, batches, mb), _run(w0, batches, mb)
    assert np.array_equal(one[2], two[2]) and np.isfinite(one[2]).all() and not np.array_equal(one[2][0], one[2][1])
    for k in one[0]:
        assert np.array_equal(one[0][k], two[0][k]), ("parameters", k)
    for sa, sb in zip(one[1], two[1]):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), ("slots", k)
    for ga, gb in zip(one[3], two[3]):
        assert np.array_equal(ga, gb) and ga.any()


# ---- 6. the epoch straight from records ---------------------------------------------------------------------------------------
_kept = {}


def _selfplay_records(game, tmp_path, monkeypatch):
    """at least 40 records of real self-play, kept on the device, as tests/test_gpu_hip_trainer.py makes them; once per game"""
    if game not in _kept:
        monkeypatch.chdir(tmp_path)
        model = Blackbird.Model(BOARD_CLS[game], "play", {"explorationRate": 0.85, "playLimit": 8}, M.net_config(1, 0.0))
        model.KeepDeviceExamples = True
        np.random.seed(31)
        Blackbird.GenerateTrainingSamples(model, 16, 1.0)
        kept = model.KeptDeviceExamples()
        assert len(kept) >= 40
        _kept[game] = kept.records.clone()
        model._batch_engine.close()
        model.Conn.Close()
    return DeviceExamples(game, _kept[game])


def _loop(tr, ex, order, sym, batch):
    out = []
    for i in range(int(order.numel()) // batch):
        rows = slice(i * batch, (i + 1) * batch)
        total, terms = tr.step_tensors(*ex._batch(order[rows], None if sym is None else sym[rows]), LR)
        out.append(torch.stack([total] + terms))
    return torch.stack(out)


def _state(tr, losses):
    return tr.export(), tr.slots(), losses.cpu().numpy()


def _same_bits(a, b):
    assert a[2].shape == b[2].shape and np.array_equal(a[2], b[2]), ("losses", a[2], b[2])
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), ("parameters", k)
    for sa, sb in zip(a[1], b[1]):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), ("slots", k)


@pytest.mark.parametrize("game,batch,with_sym", [(C4, 17, True), (C4, 6, False), (TTT, 17, True), (TTT, 1, False)])
def test_epoch_is_the_per_batch_loop(game, batch, with_sym, tmp_path, monkeypatch):
    ex = _selfplay_records(game, tmp_path, monkeypatch)
    rng = np.random.RandomState(7 + batch)
    rows = 2 * batch
    order = rng.randint(0, len(ex), rows)
    terminal = np.flatnonzero((ex.batch()[2] == 0).all(dim=1).cpu().numpy())
    assert len(terminal)
    order[0] = terminal[0]                                # a terminal example for certain
    d_order = ex.index_tensor(order)
    d_sym = ex.sym_tensor(rng.randint(0, ex.symmetries, rows)) if with_sym else None
    A = ex.info.A
    w0 = W.init_weights(3, 16, 2, 16, A, seed=3, perturb=True)
    one, two = _trainer(w0, "adam", max_batch=17), _trainer(w0, "adam", max_batch=17)
    losses = one.epoch_records(ex, d_order, batch, LR, sym=d_sym)
    assert tuple(losses.shape) == (2, 4)
    got, want = _state(one, losses), _state(two, _loop(two, ex, d_order, d_sym, batch))
    _same_bits(got, want)
    assert ex.bad() == 0 and np.isfinite(got[2]).all() and (got[2][:, 2] >= 0).all()
    assert any(not np.array_equal(got[0][k], w0[k]) for k in w0)
    with pytest.raises(ValueError, match="noise"):
        one.epoch_records(ex, d_order, batch, LR, sym=d_sym, noise=np.zeros((2, A), np.float32))
    one.close()
    two.close()


@pytest.mark.parametrize("game", [C4, TTT])
def test_epoch_counts_a_malformed_record_and_reads_zeros(game):
    """Record 3 says n_children = S + 1: the row is zeros (no label, outcome 0) and one count in bad(), and the epoch equals the
    loop over what bb_examples_to_batch_sym writes for the same rows.  Nothing can fault: the record's count is checked on the
    device before anything it says becomes an address (examples.hip.h)."""
    rec = MC.copies(game, MC._positions(game, 5, 12), 12, 13, malformed=(3,))
    ex, ex2 = DeviceExamples.from_records(game, rec, DEV), DeviceExamples.from_records(game, rec, DEV)
    order = ex.index_tensor(np.array([0, 3, 5, 7, 1, 2, 9, 10, 11, 4, 3, 6]))
    w0 = W.init_weights(3, 16, 1, 16, ex.info.A, seed=3, perturb=True)
    one, two = _trainer(w0, "adam", max_batch=6), _trainer(w0, "adam", max_batch=6)
    losses = one.epoch_records(ex, order, 6, LR)
    boards, value, policy = ex2._batch(order[:6])
    assert not boards[1].any() and not policy[1].any() and not value[1].any()
    got, want = _state(one, losses), _state(two, _loop(two, ex2, order, None, 6))
    _same_bits(got, want)
    assert ex.bad() == 2 and ex2.bad() == 2 + 1           # (ex2 decoded the first batch twice)
    one.close()
    two.close()


# ---- 7. the step's reported terms are the scorer's ------------------------------------------------------------------------------
@pytest.mark.parametrize("game,B", [("connect4", 6), ("tictactoe", 130)])
def test_reported_terms_are_the_scorers(game, B):
    """lossEvaluation = value_mse and lossPolicy = ce_sum / n of HipTrainer.evaluate_tensors on the same rows at the same weights
    (the sum orders differ -- float32 chains and a double tree there, per-row floats summed in double here --, so not the bits)."""
    w0 = W.init_weights(3, 16, 2, 16, GAMES[game][3], seed=9, perturb=True)
    batch = _dense_batch(game, B, 80)
    tr = _trainer(w0)
    _total, terms, _g = tr.gradients(*batch)
    scored = tr.evaluate_tensors(*batch)
    assert scored["rows"] == B and scored["policy_rows"] == B - 1
    close(terms[0], scored["value_mse"], (game, "lossEvaluation"))
    close(terms[1], scored["ce_sum"] / B, (game, "lossPolicy"))
    tr.close()


# ---- 8. the reference loss is untouched ---------------------------------------------------------------------------------------
def _reference_steps(w0, batches, **kw):
    tr = HipTrainer(w0, alpha=ALPHA, epsilon=EPS, optimizer="adam", momentum=0.9, device=DEV, seed=21, max_batch=6, **kw)
    losses, drawn = [], []
    for batch in batches:
        total, terms = tr.step(batch[0], batch[1], batch[2], LR)        # (the noise is drawn)
        losses.append([total] + terms)
        drawn.append(tr.last_noise())
    out = (tr.export(), tr.slots(), np.array(losses), drawn)
    tr.close()
    return out


@pytest.mark.parametrize("game", ["connect4", "dragonchess"])
def test_reference_is_the_default_bit_for_bit(game):
    if game == "dragonchess":
        w0, batches = DCC.weights(1, 16, 3), [DCC.make_batch(4, 90 + s)[:3] for s in range(2)]
    else:
        w0, batches = W.init_weights(3, 16, 2, 16, 7, seed=3, perturb=True), [_dense_batch(game, 6, 90 + s) for s in range(2)]
    plain, named = _reference_steps(w0, batches), _reference_steps(w0, batches, loss="reference", l2=0.5)
    _same_bits((plain[0], plain[1], plain[2]), (named[0], named[1], named[2]))
    for a, b in zip(plain[3], named[3]):
        assert np.array_equal(a, b) and a.any()
    # ... and it is the loss of the statement of the reference's graph: the drawn noise given back to it
    from tests.trainer_cases import statement
    r_total, r_parts, _g = statement(w0, *batches[0], plain[3][0], EPS)
    close(plain[2][0][0], r_total, (game, "reference loss"))
    close(plain[2][0][2], r_parts[1], (game, "reference lossPolicy"))


@pytest.mark.parametrize("game", ["connect4", "dragonchess"])
def test_set_loss_back_to_reference(game):
    """A per-example step, then bb_trainer_set_loss(BB_LOSS_REFERENCE): the next step is the reference step a fresh trainer makes
    from the same weights with the same noise (sgd: the weights are all the state there is), and a noise pointer is taken again."""
    if game == "dragonchess":
        w0, batches = DCC.weights(1, 16, 3), [DCC.make_batch(4, 95 + s) for s in range(2)]
    else:
        w0 = W.init_weights(3, 16, 2, 16, 7, seed=3, perturb=True)
        batches = [make_batch(6, 7, 7, 6, 95 + s) for s in range(2)]
    a = _trainer(w0, "sgd", max_batch=6)
    with pytest.raises(ValueError, match="noise"):
        a.step(*batches[0][:3], LR, noise=batches[0][3])
    t = [torch.tensor(np.asarray(x, dtype=np.float32), device=DEV) for x in batches[0]]
    with pytest.raises(ValueError, match="noise"):                        # the library's own refusal, below the Python check
        _lib.trainer_step(a._h, len(t[1]), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), noise=t[3].data_ptr(), lr=LR)
    a.step(*batches[0][:3], LR)
    mid = a.export()
    assert any(not np.array_equal(mid[k], w0[k]) for k in w0)
    for bad in ((2, 0.0), (1, -1.0), (1, float("nan"))):
        with pytest.raises(ValueError):
            _lib.trainer_set_loss(a._h, *bad)
    _lib.trainer_set_loss(a._h, _lib.LOSS_REFERENCE, 0.0)
    a.loss_kind = "reference"
    got = a.step(*batches[1][:3], LR, noise=batches[1][3])
    b = _trainer(mid, "sgd", max_batch=6, loss="reference")
    want = b.step(*batches[1][:3], LR, noise=batches[1][3])
    assert got == want
    wa, wb = a.export(), b.export()
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k
    a.close()
    b.close()


# ---- 9. the front end ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def epoch_calls(monkeypatch):
    """how often HipTrainer.epoch_records ran"""
    calls, real = [], HipTrainer.epoch_records

    def counted(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)

    monkeypatch.setattr(HipTrainer, "epoch_records", counted)
    return calls


@pytest.mark.parametrize("backend,fused,handoff", [("hip", False, None), ("hip", True, "device"), ("torch", False, None)])
def test_train_with_device_examples(backend, fused, handoff, tmp_path, monkeypatch, epoch_calls):
    ex = _selfplay_records(C4, tmp_path, monkeypatch)
    ex = DeviceExamples(C4, ex.records[:40].clone())                      # five whole batches of 8
    monkeypatch.chdir(tmp_path)
    cfg = M.net_config(1, 0.3)
    cfg["training"].update({"backend": backend, "loss": "per_example", "l2": 1e-3})
    if handoff:
        cfg["training"]["handoff"] = handoff
    model = Blackbird.Model(Connect4.BoardState, "m_%s%d" % (backend, fused), {"explorationRate": 0.85, "playLimit": 8}, cfg)
    x = _lib.game_encode(C4, _lib.game_initial(C4))
    model.getEvaluation(x)                                                # the engine behind it holds the OLD weights
    before = model._eval_engine.net_eval(planes=x)[1].copy()
    w0 = {k: v.copy() for k, v in model._weights.items()}
    np.random.seed(5)
    Blackbird.TrainWithDeviceExamples(model, 8, LR, examples=ex, augment=True, fused=fused)
    tr = model._trainer
    assert type(tr) is (HipTrainer if backend == "hip" else Trainer) and (tr.loss_kind, tr.l2) == ("per_example", 1e-3)
    assert model.batchCount == 5 and len(epoch_calls) == int(fused)
    assert any(not np.array_equal(model._weights[k], w0[k]) for k in w0)
    after = model._eval_engine.net_eval(planes=x)[1]                      # the engine was reloaded with the trained weights
    assert np.isfinite(after).all() and not np.array_equal(after, before)
    scored = Blackbird.EvaluateDeviceExamples(model, ex)
    assert scored["rows"] == 40 and np.isfinite(scored["policy_ce"])
    model.Conn.Close()


def test_network_train_and_merge(tmp_path, monkeypatch):
    """Network.train (which passes no noise) and the merged rows of TrainWithDeviceExamples under the per-example loss"""
    ex = _selfplay_records(C4, tmp_path, monkeypatch)
    monkeypatch.chdir(tmp_path)
    cfg = M.net_config(1, 0.3)
    cfg["training"].update({"backend": "hip", "loss": "per_example"})
    model = Blackbird.Model(Connect4.BoardState, "m_merge", {"explorationRate": 0.85, "playLimit": 8}, cfg)
    w0 = {k: v.copy() for k, v in model._weights.items()}
    np.random.seed(5)
    Blackbird.TrainWithDeviceExamples(model, 8, LR, examples=ex, merge=True)
    assert model.batchCount >= 1 and model._trainer.loss_kind == "per_example" and model._trainer.l2 == 1e-4
    count = model.batchCount
    boards, value, policy = ex.batch(np.arange(4))
    model.train(boards.cpu().numpy(), value.cpu().numpy(), policy.cpu().numpy(), LR)
    assert model.batchCount == count + 1 and any(not np.array_equal(model._weights[k], w0[k]) for k in w0)
    model.Conn.Close()
