"""What the training tests share (not collected): the float64 statement of the reference's training graph tied to Connect4 and
two blocks with its numpy optimiser (tests/test_train_parity.py says what it states), and the one for any dense game and
network shape (`statement`, `RefOptimizer`; tests/test_hip_trainer_cpu.py says what it states).  Both stay, written
independently: test_statement_agrees_with_the_connect4_statement holds each to the other, so neither is the only witness of
the trainer it judges."""
import numpy as np
import torch

from blackbird_amd import _lib
from blackbird_amd import weights as W

TOL = 1e-5
H, Wd, C, F, R, D, A, B = 6, 7, 3, 16, 2, 16, 7, 6
ALPHA, EPS = 0.2, 0.3


def _batch(seed):
    rng = np.random.RandomState(seed)
    cells = rng.randint(0, 3, size=(B, H, Wd))
    boards = np.zeros((B, H, Wd, C), dtype=np.int8)
    boards[..., 0] = cells == 1
    boards[..., 1] = cells == 2
    boards[..., 2] = rng.choice([-1, 1], size=(B, 1, 1))
    ev = rng.choice([-1.0, 0.0, 1.0], size=B).astype(np.float32)
    pl = rng.dirichlet(np.ones(A), size=B)
    pl[-1] = 0.0  # a terminal example: pi = zeros (Blackbird.py:256-258)
    noise = rng.beta(ALPHA, 1 - ALPHA, size=A)
    return boards, ev, pl, noise


# ---- the independent statement (float64, NHWC, no conv2d) ---------------------------------------------------------
def _ref_loss(w, boards, ev, pl, noise):
    x = torch.tensor(boards.astype(np.float64))
    ev = torch.tensor(ev.astype(np.float64))
    pl = torch.tensor(pl.astype(np.float64))
    nz = torch.tensor(noise.astype(np.float64))

    def conv(t, scope):  # tf.layers.conv2d, SAME, stride 1, bias
        k, b = w[scope + "/kernel"], w[scope + "/bias"]
        kh = k.shape[0]
        p = kh // 2
        tp = torch.nn.functional.pad(t, (0, 0, p, p, p, p))
        out = 0
        for dy in range(kh):
            for dx in range(kh):
                out = out + torch.einsum("bhwc,cf->bhwf", tp[:, dy:dy + H, dx:dx + Wd, :], k[dy, dx])
        return out + b

    def bn(t, scope):  # batch_normalization, training=False, epsilon 1e-3
        g, be, mu, var = (w[f"{scope}/{f}"] for f in W.BN_FIELDS)
        return g * (t - mu) / torch.sqrt(var + 1e-3) + be

    t = torch.relu(bn(conv(x, "resTower/conv_block/conv"), "resTower/conv_block/batch_norm"))
    for i in range(R):
        h = torch.relu(bn(conv(t, f"resTower/block_{i}/conv_1"), f"resTower/block_{i}/batch_norm_1"))
        h = bn(conv(h, f"resTower/block_{i}/conv_2"), f"resTower/block_{i}/batch_norm_2")
        t = torch.relu(h + t)
    v = torch.relu(bn(conv(t, "value/convolution"), "value/batch_norm"))                       # [B,H,W,1]
    v = torch.einsum("bhwo,od->bhwd", v, w["value/dense_1/kernel"]) + w["value/dense_1/bias"]  # dense on the last axis
    v = torch.relu(v.sum(dim=(1, 2)))                                                           # reduce_sum over H, W
    value = torch.tanh((torch.einsum("bd,do->bo", v, w["value/dense_2/kernel"]) + w["value/dense_2/bias"]).sum(dim=1))
    p = torch.relu(bn(conv(t, "policy/convolution"), "policy/batch_norm"))                     # [B,H,W,2]
    logits = (torch.einsum("bhwo,oa->bhwa", p, w["policy/policy/kernel"]) + w["policy/policy/bias"]).sum(dim=(1, 2))
    z = logits - logits.max(dim=1, keepdim=True).values
    base = torch.exp(z) / torch.exp(z).sum(dim=1, keepdim=True)
    policy = (1 - EPS) * base + EPS * nz[None, :]
    policy = policy / policy.sum()                        # over ALL elements, batch axis included (:182)
    l_eval = ((value - ev) ** 2).mean()
    l_pol = -(torch.log(policy) @ pl.t()).mean()          # the full B x B cross matrix (:190-194)
    l2 = [0.5 * (t_ ** 2).sum() for k_, t_ in w.items() if t_.requires_grad and "bias" not in k_]
    l_par = torch.stack(l2).mean()
    return l_eval + l_pol + l_par, (l_eval, l_pol, l_par)


def _ref_weights(w0):
    w = {}
    for k, v in w0.items():
        t = torch.tensor(np.asarray(v, dtype=np.float64))
        if not (k.endswith("moving_mean") or k.endswith("moving_variance")):
            t.requires_grad_(True)
        w[k] = t
    return w


def _ref_grads(w0, batch):
    w = _ref_weights(w0)
    total, parts = _ref_loss(w, *batch)
    names = [k for k, t in w.items() if t.requires_grad]
    gs = torch.autograd.grad(total, [w[k] for k in names])
    return float(total.detach()), [float(p.detach()) for p in parts], {k: g.numpy() for k, g in zip(names, gs)}


class _RefOptimizer:
    """tf.compat.v1.train.{Adam,Momentum,GradientDescent}Optimizer update rules in numpy float64."""

    def __init__(self, kind, momentum=0.9):
        self.kind, self.mom, self.t, self.m, self.v = kind, momentum, 0, {}, {}

    def apply(self, w, grads, lr):
        out = dict(w)
        self.t += 1
        for k, g in grads.items():
            x = np.asarray(w[k], dtype=np.float64)
            if self.kind == "adam":
                m = 0.9 * self.m.get(k, 0.0) + 0.1 * g
                v = 0.999 * self.v.get(k, 0.0) + 0.001 * g * g
                self.m[k], self.v[k] = m, v
                lr_t = lr * np.sqrt(1 - 0.999 ** self.t) / (1 - 0.9 ** self.t)
                out[k] = x - lr_t * m / (np.sqrt(v) + 1e-8)
            elif self.kind == "momentum":
                acc = self.mom * self.m.get(k, 0.0) + g
                self.m[k] = acc
                out[k] = x - lr * acc
            else:
                out[k] = x - lr * g
        return out


def _close(got, want, what):
    scale = max(1.0, float(np.max(np.abs(want))))
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)))
    assert err <= TOL * scale, (what, err, scale)


# ---- any dense game, any shape --------------------------------------------------------------------------------------------
GAMES = {"connect4": (_lib.GAME_CONNECT4, 6, 7, 7), "tictactoe": (_lib.GAME_TICTACTOE, 3, 3, 9)}  # id, H, W, A


def make_batch(H, Wd, A, B, seed, zero_labels=False, terminal_last=True):
    """A batch as tests/test_train_parity._batch makes it, for any board: labels in {-1, 0, 1}, the last row a terminal
    example (pi = 0) unless terminal_last is False (then every row carries a label; the draws are the same), A
    Beta(alpha, 1-alpha) draws."""
    rng = np.random.RandomState(seed)
    cells = rng.randint(0, 3, size=(B, H, Wd))
    boards = np.zeros((B, H, Wd, 3), dtype=np.int8)
    boards[..., 0] = cells == 1
    boards[..., 1] = cells == 2
    boards[..., 2] = rng.choice([-1, 1], size=(B, 1, 1))
    ev = rng.choice([-1.0, 0.0, 1.0], size=B).astype(np.float32)
    pl = rng.dirichlet(np.ones(A), size=B)
    if terminal_last:
        pl[-1] = 0.0
    if zero_labels:
        pl[:] = 0.0
    noise = rng.beta(ALPHA, 1 - ALPHA, size=A)
    return boards, ev, pl, noise


def statement(w0, boards, ev, pl, noise, eps, parts=False, dtype=torch.float64):
    """(loss, [evaluation, policy, parameter term], {variable: gradient}) in float64.  noise None: zeros (eps == 0).
    parts=True appends {variable: data gradient} -- the gradient of lossEvaluation + lossPolicy alone, what is left of a
    gradient once the L2 part w / N is taken away -- and the liveness report of `_liveness`.  dtype=torch.float32 evaluates the
    same graph in float32: the yardstick for how far float32 arithmetic alone is from this statement."""
    np_dtype = {torch.float64: np.float64, torch.float32: np.float32}[dtype]
    w = {}
    for k, v in w0.items():
        t = torch.tensor(np.asarray(v, dtype=np_dtype))
        if not (k.endswith("moving_mean") or k.endswith("moving_variance")):
            t.requires_grad_(True)
        w[k] = t
    _C, _F, R, _D, A = W.infer_shape(w0)
    x = torch.tensor(np.asarray(boards, dtype=np_dtype))
    H, Wd = x.shape[1], x.shape[2]
    ev = torch.tensor(np.asarray(ev, dtype=np_dtype))
    pl = torch.tensor(np.asarray(pl, dtype=np_dtype))
    nz = torch.zeros(A, dtype=dtype) if noise is None else torch.tensor(np.asarray(noise, dtype=np_dtype))
    pre = {}                                              # what every ReLU is applied to, by layer

    def relu(t, name):
        pre[name] = t.detach().numpy()
        return torch.relu(t)

    def conv(t, scope):  # tf.layers.conv2d, SAME, stride 1, bias
        k, b = w[scope + "/kernel"], w[scope + "/bias"]
        kh = k.shape[0]
        p = kh // 2
        tp = torch.nn.functional.pad(t, (0, 0, p, p, p, p))
        out = 0
        for dy in range(kh):
            for dx in range(kh):
                out = out + torch.einsum("bhwc,cf->bhwf", tp[:, dy:dy + H, dx:dx + Wd, :], k[dy, dx])
        return out + b

    def bn(t, scope):  # batch_normalization, training=False, epsilon 1e-3
        g, be, mu, var = (w[f"{scope}/{f}"] for f in W.BN_FIELDS)
        return g * (t - mu) / torch.sqrt(var + 1e-3) + be

    t = relu(bn(conv(x, "resTower/conv_block/conv"), "resTower/conv_block/batch_norm"), "resTower/conv_block")
    for i in range(R):
        h = relu(bn(conv(t, f"resTower/block_{i}/conv_1"), f"resTower/block_{i}/batch_norm_1"), f"resTower/block_{i}/conv_1")
        h = bn(conv(h, f"resTower/block_{i}/conv_2"), f"resTower/block_{i}/batch_norm_2")
        t = relu(h + t, f"resTower/block_{i}/out")
    v = relu(bn(conv(t, "value/convolution"), "value/batch_norm"), "value/convolution")
    v = torch.einsum("bhwo,od->bhwd", v, w["value/dense_1/kernel"]) + w["value/dense_1/bias"]
    v = relu(v.sum(dim=(1, 2)), "value/dense_1")
    pre_tanh = (torch.einsum("bd,do->bo", v, w["value/dense_2/kernel"]) + w["value/dense_2/bias"]).sum(dim=1)
    value = torch.tanh(pre_tanh)
    p = relu(bn(conv(t, "policy/convolution"), "policy/batch_norm"), "policy/convolution")
    logits = (torch.einsum("bhwo,oa->bhwa", p, w["policy/policy/kernel"]) + w["policy/policy/bias"]).sum(dim=(1, 2))
    z = logits - logits.max(dim=1, keepdim=True).values
    base = torch.exp(z) / torch.exp(z).sum(dim=1, keepdim=True)
    policy = (1 - eps) * base + eps * nz[None, :]
    policy = policy / policy.sum()                        # over ALL elements, batch axis included (:182)
    l_eval = ((value - ev) ** 2).mean()
    l_pol = -(torch.log(policy) @ pl.t()).mean()          # the full B x B cross matrix (:190-194)
    l_par = torch.stack([0.5 * (t_ ** 2).sum() for k_, t_ in w.items() if t_.requires_grad and "bias" not in k_]).mean()
    total = l_eval + l_pol + l_par
    names = [k for k, t_ in w.items() if t_.requires_grad]
    gs = torch.autograd.grad(total, [w[k] for k in names], retain_graph=parts)
    out = (float(total.detach()), [float(l_eval.detach()), float(l_pol.detach()), float(l_par.detach())],
           {k: g.numpy() for k, g in zip(names, gs)})
    if not parts:
        return out
    dgs = torch.autograd.grad(l_eval + l_pol, [w[k] for k in names])
    return out + ({k: g.numpy() for k, g in zip(names, dgs)}, _liveness(pre, pre_tanh.detach().numpy(), logits.detach().numpy()))


def _liveness(pre, pre_tanh, logits):
    """What decides whether a backward pass is multiplied by something: per ReLU the share of positive pre-activations
    ("relu"; "dense_rows": the rows on which any value-dense unit is on, "dense_on": those units themselves), the smallest
    |pre-activation| anywhere ("relu_margin": above float32's error, both precisions take the same masks), the pre-tanh values
    and their min, median and max magnitude, and the largest max - min of a row's logits."""
    a = np.abs(pre_tanh)
    return {"relu": {k: float((v > 0).mean()) for k, v in pre.items()},
            "dense_on": pre["value/dense_1"] > 0,
            "relu_margin": min(float(np.abs(v).min()) for v in pre.values()),
            "pre_tanh": pre_tanh, "pre_tanh_min": float(a.min()), "pre_tanh_median": float(np.median(a)),
            "pre_tanh_max": float(a.max()), "logit_spread": float((logits.max(axis=1) - logits.min(axis=1)).max())}


# ---- live inputs: every backward pass multiplied by something --------------------------------------------------------------
# (game, R, D, B, weight seed, batch seed, terminal_last).  With init_weights(perturb=True) alone the value head saturates
# (|pre-tanh| of 9 to 133: tanh' = 0 in float32) and whole ReLU layers are off, so most of the backward pass is multiplied by
# zero; these seeds, with live_weights' rescales, meet the conditions tests/test_trainer_liveness_cpu.py asserts on the float64
# statement alone.  Shapes: R in {0, 1, 2, 9} (the activation buffers change roles per layer), D in {1, 16, 64} (the loop bounds
# over D), B in {1 with and without a label, 2, 6, 130} (one workgroup, several, the 130 slab sums), both games.  A margin of 1e-4
# around 0 for every pre-activation bounds the element count of a case: the pre-activations of these networks lie about 1.3 per
# unit near 0, so among N of them about 2.6e-4 N fall inside the margin and a draw is clear of it with probability
# exp(-2.6e-4 N).  Connect4 with 130 rows has N = 87 000 in its first layer alone (e^-23); with two blocks and 6 rows N = 21 000
# (0.4 % a draw, and the two-step case needs three such draws at once: none in 250 000); TicTacToe with 130 rows and no block has
# 24 000.  So the 130-row batch is on the small board without blocks, and Connect4 has no live case above 6 rows: there the dead
# cases of test_gradients_over_shapes remain the only witness.
# The first case is the two-step one: its second batch is seed + 1, and its learning rate LIVE_LR keeps the second step live (a
# step of 1e-2 on the rescaled value/dense_2/kernel takes |pre-tanh| to 50).
LIVE_CASES = [("tictactoe", 2, 16, 6, 2686, 101, True),
              ("connect4", 0, 16, 1, 1, 2, True), ("connect4", 0, 16, 1, 1, 2, False), ("tictactoe", 0, 1, 1, 1, 2, True),
              ("connect4", 1, 1, 6, 89, 103, True), ("connect4", 2, 64, 2, 80, 101, True), ("connect4", 9, 16, 1, 11, 101, True),
              ("connect4", 9, 16, 2, 2868, 101, False), ("tictactoe", 9, 64, 2, 45, 100, True),
              ("tictactoe", 0, 16, 130, 306, 100, True)]
TWO_STEP_CASE = LIVE_CASES[0]
LIVE_LR = 1e-3     # test_two_steps_live's bound on the updated weights (2**-22 max|w|) leans on it too: the float32 error of an
                   # update is a few 1e-7 of the step, and the step is LIVE_LR times smaller than the weights
LIVE_FACTOR, LIVE_CAP = 8.0, 1e-5     # the kernel may be 8 float32-statement errors from the statement, never more than TOL


def live_weights(game, R, D, seed, boards):
    """init_weights(perturb=True) with two float32 rescales of head kernels that depend on `boards` alone: value/dense_2/kernel
    divided by the median |pre-tanh| of these rows, and policy/policy/kernel divided so that the widest row of logits spans 4
    when it spans more.  A float32 dict."""
    A = GAMES[game][3]
    w = W.init_weights(3, 16, R, D, A, seed=seed, perturb=True)
    n = len(boards)
    live = statement(w, boards, np.zeros(n), np.zeros((n, A)), None, 0.0, parts=True)[4]
    w["value/dense_2/kernel"] = (w["value/dense_2/kernel"] / np.float32(live["pre_tanh_median"])).astype(np.float32)
    if live["logit_spread"] > 4:
        w["policy/policy/kernel"] = (w["policy/policy/kernel"] / np.float32(live["logit_spread"] / 4)).astype(np.float32)
    return w


def float32_figure(w0, batch, eps, want):
    """How far the statement evaluated in float32 (torch, CPU) is from the float64 one `want` = statement(..., parts=True): the
    largest error of a data gradient over the tensors, each relative to its largest |data gradient|."""
    got = statement(w0, *batch, eps, parts=True, dtype=torch.float32)[3]
    return max(float(np.max(np.abs(got[k] - dg))) / float(np.max(np.abs(dg))) for k, dg in want[3].items() if dg.any())


def live_tol(figure):
    return min(LIVE_FACTOR * figure, LIVE_CAP)


def close_live(got, want, data_scale, tol, what):
    """|got - want| <= tol * data_scale + 2**-23 * max|want|; prints the error relative to data_scale before it asserts, and
    returns it (0 where data_scale is 0: then the bound is the float32 rounding of `want` alone)."""
    want = np.asarray(want, dtype=np.float64)
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)))
    rel = err / data_scale if data_scale else 0.0
    print(what, "err %.3g relative to %.3g: %.3g (tol %.3g)" % (err, data_scale, rel, tol))
    assert err <= tol * data_scale + 2.0 ** -23 * float(np.max(np.abs(want))), (what, err, data_scale, tol)
    return rel


_live = {}


def live_case(case):
    """The inputs and the references of a live case, computed once and left unchanged: weights `w`, `batch`, the float64
    statement with its parts `want`, the float32 figure and the tolerance that follows from it."""
    if case not in _live:
        game, R, D, B, w_seed, b_seed, terminal_last = case
        _g, H, Wd, A = GAMES[game]
        batch = make_batch(H, Wd, A, B, b_seed, terminal_last=terminal_last)
        w = live_weights(game, R, D, w_seed, batch[0])
        want = statement(w, *batch, EPS, parts=True)
        figure = float32_figure(w, batch, EPS, want)
        _live[case] = {"w": w, "batch": batch, "want": want, "figure": figure, "tol": live_tol(figure)}
    return _live[case]


def assert_live(want, B, D, terminal_only, what):
    """The conditions on the float64 statement alone under which a comparison with it sees every backward pass (`want` =
    statement(..., parts=True); terminal_only: the one row has no policy label)."""
    data, live = want[3], want[4]
    print(what, {k: round(v, 3) for k, v in live["relu"].items()}, "pre-tanh min %.3g median %.3g max %.3g" %
          (live["pre_tanh_min"], live["pre_tanh_median"], live["pre_tanh_max"]), "logit spread %.3g margin %.3g" %
          (live["logit_spread"], live["relu_margin"]))
    for k, share in live["relu"].items():
        if k == "value/dense_1" and D == 1:            # one unit: on for at least one row, and not for all of several
            rows = live["dense_on"][:, 0]
            assert rows.any() and not (B >= 2 and rows.all()), (what, k, rows)
        else:
            assert 0.1 <= share <= 0.9, (what, k, share)
    assert live["pre_tanh_max"] <= 2 and live["pre_tanh_min"] >= 0.05, (what, live["pre_tanh"])
    if B >= 2:
        assert (live["pre_tanh"] > 0).any() and (live["pre_tanh"] < 0).any(), (what, live["pre_tanh"])
    for k, g in data.items():
        if terminal_only and k.startswith("policy/"):
            assert not g.any(), (what, k)
        else:
            assert np.abs(g).max() >= 1e-3, (what, k, np.abs(g).max())
    assert live["relu_margin"] >= 1e-4, (what, live["relu_margin"])


class RefOptimizer:
    """tf.compat.v1.train.{Adam,Momentum,GradientDescent}Optimizer in numpy float64 (NetworkFactory.py:234-242)."""

    def __init__(self, kind, momentum=0.9):
        self.kind, self.mom, self.t, self.m, self.v = kind, momentum, 0, {}, {}

    def apply(self, w, grads, lr):
        out = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
        self.t += 1
        for k, g in grads.items():
            g = np.asarray(g, dtype=np.float64)
            if self.kind == "adam":
                self.m[k] = 0.9 * self.m.get(k, 0.0) + 0.1 * g
                self.v[k] = 0.999 * self.v.get(k, 0.0) + 0.001 * g * g
                lr_t = lr * np.sqrt(1 - 0.999 ** self.t) / (1 - 0.9 ** self.t)
                out[k] = out[k] - lr_t * self.m[k] / (np.sqrt(self.v[k]) + 1e-8)
            elif self.kind == "momentum":
                self.m[k] = self.mom * self.m.get(k, 0.0) + g
                out[k] = out[k] - lr * self.m[k]
            else:
                out[k] = out[k] - lr * g
        return out


def close(got, want, what):
    """The `_close` rule of tests/test_train_parity.py; prints the figure before it asserts."""
    want = np.asarray(want, dtype=np.float64)
    scale = max(1.0, float(np.max(np.abs(want))))
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)))
    print(what, "err %.3g scale %.3g" % (err, scale))
    assert err <= TOL * scale, (what, err, scale)
