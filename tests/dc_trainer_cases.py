"""What the DragonChess training tests share (not collected): a batch maker for 8x8x17 boards and 4032 actions, and the live
weights built the way tests/trainer_cases.live_weights builds them.  The statement they are held to is trainer_cases.statement,
which takes weights and boards of any shape; tests/test_hip_trainer_dc_cpu.py holds it to training.Trainer on this shape."""
import numpy as np

from blackbird_amd import weights as W
from tests.trainer_cases import ALPHA, EPS, float32_figure, live_tol, statement

H, Wd, C, A = 8, 8, 17, 4032
EDGE_ACTIONS = (0, 255, 256, 4015, 4016, 4031)   # the first and last action of a thread's first pass, and both sides of 4016 =
                                                 # 15 * 256 + 176: where the last 192 threads of the workgroup stop owning a 16th action
R_MAX = 8                                        # training.HIP_TRAINER_DC_BLOCKS (test_hip_trainer_dc_cpu.py holds the two equal)


def make_batch(B, seed, zero_labels=False, terminal_last=True):
    """(boards int8 [B,8,8,17], value [B], policy [B,4032] float64, noise [4032]).  Planes 0..11: at most one piece a square; 12..15:
    four flags, each constant over a row's board; plane 16: the side to move, +1 or -1 everywhere -- never all zero.  A policy row
    is sparse: EDGE_ACTIONS and four more actions carry Dirichlet weights, the rest are zero.  The last row is a terminal example
    (pi = 0) unless terminal_last is False; zero_labels: every row is."""
    rng = np.random.RandomState(seed)
    piece = rng.randint(0, 25, size=(B, H, Wd))              # 1..12: a piece; anything else: empty
    boards = np.zeros((B, H, Wd, C), dtype=np.int8)
    for k in range(12):
        boards[..., k] = piece == k + 1
    boards[..., 12:16] = rng.randint(0, 2, size=(B, 1, 1, 4))
    boards[..., 16] = rng.choice([-1, 1], size=(B, 1, 1))
    ev = rng.choice([-1.0, 0.0, 1.0], size=B).astype(np.float32)
    pl = np.zeros((B, A), dtype=np.float64)
    for j in range(B):
        others = rng.choice(np.setdiff1d(np.arange(A), EDGE_ACTIONS), size=4, replace=False)
        moves = np.concatenate([EDGE_ACTIONS, others])
        pl[j, moves] = rng.dirichlet(np.ones(len(moves)))
    if terminal_last:
        pl[-1] = 0.0
    if zero_labels:
        pl[:] = 0.0
    noise = rng.beta(ALPHA, 1 - ALPHA, size=A)
    return boards, ev, pl, noise


def weights(R, D, seed):
    return W.init_weights(C, 16, R, D, A, seed=seed, perturb=True)


def live_weights(R, D, seed, boards):
    """trainer_cases.live_weights for this shape: value/dense_2/kernel divided by the median |pre-tanh| of these rows, and
    policy/policy/kernel divided so that the widest row of logits spans 4 when it spans more."""
    w = weights(R, D, seed)
    n = len(boards)
    live = statement(w, boards, np.zeros(n), np.zeros((n, A)), None, 0.0, parts=True)[4]
    w["value/dense_2/kernel"] = (w["value/dense_2/kernel"] / np.float32(live["pre_tanh_median"])).astype(np.float32)
    if live["logit_spread"] > 4:
        w["policy/policy/kernel"] = (w["policy/policy/kernel"] / np.float32(live["logit_spread"] / 4)).astype(np.float32)
    return w


LIVE_CASE = (1, 16, 2, 12, 103)    # R, D, B, weight seed, batch seed; no terminal row.  The seed meets trainer_cases.assert_live
_live = {}


def live_case():
    """The live case's inputs and references, computed once and left unchanged (trainer_cases.live_case's dict)."""
    if not _live:
        R, D, B, w_seed, b_seed = LIVE_CASE
        batch = make_batch(B, b_seed, terminal_last=False)
        w = live_weights(R, D, w_seed, batch[0])
        want = statement(w, *batch, EPS, parts=True)
        figure = float32_figure(w, batch, EPS, want)
        _live.update({"w": w, "batch": batch, "want": want, "figure": figure, "tol": live_tol(figure)})
    return _live


LIVE_SLICES = {"resTower/conv_block/conv/kernel": np.s_[:, :, 16, :], "policy/policy/kernel": np.s_[:, 4016:],
               "policy/policy/bias": np.s_[4016:]}
