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


def make_batch(H, Wd, A, B, seed, zero_labels=False):
    """A batch as tests/test_train_parity._batch makes it, for any board: labels in {-1, 0, 1}, the last row a terminal
    example (pi = 0), A Beta(alpha, 1-alpha) draws."""
    rng = np.random.RandomState(seed)
    cells = rng.randint(0, 3, size=(B, H, Wd))
    boards = np.zeros((B, H, Wd, 3), dtype=np.int8)
    boards[..., 0] = cells == 1
    boards[..., 1] = cells == 2
    boards[..., 2] = rng.choice([-1, 1], size=(B, 1, 1))
    ev = rng.choice([-1.0, 0.0, 1.0], size=B).astype(np.float32)
    pl = rng.dirichlet(np.ones(A), size=B)
    pl[-1] = 0.0
    if zero_labels:
        pl[:] = 0.0
    noise = rng.beta(ALPHA, 1 - ALPHA, size=A)
    return boards, ev, pl, noise


def statement(w0, boards, ev, pl, noise, eps):
    """(loss, [evaluation, policy, parameter term], {variable: gradient}) in float64.  noise None: zeros (eps == 0)."""
    w = {}
    for k, v in w0.items():
        t = torch.tensor(np.asarray(v, dtype=np.float64))
        if not (k.endswith("moving_mean") or k.endswith("moving_variance")):
            t.requires_grad_(True)
        w[k] = t
    _C, _F, R, _D, A = W.infer_shape(w0)
    x = torch.tensor(np.asarray(boards, dtype=np.float64))
    H, Wd = x.shape[1], x.shape[2]
    ev = torch.tensor(np.asarray(ev, dtype=np.float64))
    pl = torch.tensor(np.asarray(pl, dtype=np.float64))
    nz = torch.zeros(A, dtype=torch.float64) if noise is None else torch.tensor(np.asarray(noise, dtype=np.float64))

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
    v = torch.relu(bn(conv(t, "value/convolution"), "value/batch_norm"))
    v = torch.einsum("bhwo,od->bhwd", v, w["value/dense_1/kernel"]) + w["value/dense_1/bias"]
    v = torch.relu(v.sum(dim=(1, 2)))
    value = torch.tanh((torch.einsum("bd,do->bo", v, w["value/dense_2/kernel"]) + w["value/dense_2/bias"]).sum(dim=1))
    p = torch.relu(bn(conv(t, "policy/convolution"), "policy/batch_norm"))
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
    gs = torch.autograd.grad(total, [w[k] for k in names])
    return (float(total.detach()), [float(l_eval.detach()), float(l_pol.detach()), float(l_par.detach())],
            {k: g.numpy() for k, g in zip(names, gs)})


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
