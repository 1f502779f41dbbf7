"""The step right after the hot path: Network.train's loss and optimiser
(/root/reference/src/NetworkFactory.py:185-245) on PyTorch-ROCm.  PyTorch is used for this
optimiser step only; self-play never touches it.

Reproduced exactly as written in the reference graph, quirks included:
  * value loss  = mean((evaluation - label)^2)                                         (:187-188)
  * policy      = ((1-eps)*softmax + eps*Beta noise) / sum over ALL elements (batch too) (:176-182)
  * policy loss = -mean(log(policy) @ policyLabel^T)  -- the full BxB cross matrix      (:190-194)
  * L2 term     = mean over non-bias trainable variables of sum(v^2)/2, no coefficient  (:196-201)
  * batch norm runs in inference mode (moving statistics are constants), epsilon 1e-3
  * optimiser: tf.compat.v1.train Adam / Momentum / GradientDescent by config, their update rules written out
    in `Trainer._apply` (TF1's Adam puts epsilon outside the bias correction; torch.optim.Adam does not)  (:234-242)
The teacher term (:205-218) calls the removed `tf.log` in the reference and cannot run there; Network.train refuses it.

An extension, opt-in (loss='per_example'; NetworkConfig['training']['loss']): the ordinary AlphaZero loss.  The cross matrix above
trains every row towards the batch's summed label; this one trains a row towards its own:
  * value loss  = as above
  * policy loss = -(1/n) sum_b sum_a pi_b[a] log_softmax(logits_b)[a]; a row whose label is all zeros (the terminal example) adds 0
  * L2 term     = l2 * sum over the same variables of sum(v^2)/2
  * no noise (alpha and epsilon are not used; a noise= argument is refused)
"""
import numpy as np
import torch
import torch.nn.functional as Fn

from . import _lib
from . import weights as W


LOSSES = ('reference', 'per_example')  # NetworkConfig['training']['loss']


def check_loss(loss, l2):
    """The two loss arguments of both trainers, validated: (loss, float(l2)) or ValueError."""
    if loss not in LOSSES:
        raise ValueError("loss is 'reference' or 'per_example', got %r" % (loss,))
    try:
        value = float(l2)
    except (TypeError, ValueError):
        raise ValueError('l2 must be a finite number >= 0, got %r' % (l2,))
    if not 0.0 <= value <= float(np.finfo(np.float32).max):      # (NaN fails both; the kernels take it as a float32)
        raise ValueError('l2 must be a finite number >= 0, got %r' % (l2,))
    return loss, value


def _no_noise(loss, noise):
    if loss == 'per_example' and noise is not None:
        raise ValueError("the per-example loss has no noise term: noise= must be None with loss='per_example'")


class Trainer:
    def __init__(self, weights, alpha=0.2, epsilon=0.3, optimizer='adam', momentum=0.9, device=None, loss='reference', l2=1e-4):
        self.loss_kind, self.l2 = check_loss(loss, l2)
        self.device = torch.device(device or ('cuda' if torch.cuda.is_available() else 'cpu'))
        self.alpha, self.epsilon = float(alpha), float(epsilon)
        self.C, self.F, self.R, self.D, self.A = W.infer_shape(weights)
        self.params, self.consts = {}, {}
        for k, v in weights.items():
            t = torch.tensor(np.asarray(v, dtype=np.float32), device=self.device)
            if k.endswith('moving_mean') or k.endswith('moving_variance'):
                self.consts[k] = t
            else:
                self.params[k] = t.requires_grad_(True)
        self.kind, self.momentum = optimizer, float(momentum)
        # optimiser slots, one per trainable variable, as the TF1 optimisers keep them (NetworkFactory.py:234-242)
        self.t = 0                                                         # AdamOptimizer's step count (beta powers)
        self.m = {k: torch.zeros_like(v) for k, v in self.params.items()}  # Adam first moment / Momentum accumulator
        self.v = {k: torch.zeros_like(v) for k, v in self.params.items()}  # Adam second moment

    def _apply(self, grads, lr):
        """One optimiser update, written out so that it is the reference's optimiser and not a look-alike:
          tf.compat.v1.train.AdamOptimizer(lr) (beta1 0.9, beta2 0.999, epsilon 1e-8):
              lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t);  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
              var -= lr_t * m / (sqrt(v) + epsilon)        (epsilon OUTSIDE the bias correction, unlike torch.optim.Adam)
          MomentumOptimizer(lr, momentum): accum = momentum * accum + g;  var -= lr * accum
          GradientDescentOptimizer(lr):    var -= lr * g"""
        with torch.no_grad():
            if self.kind == 'adam':
                b1, b2, eps = 0.9, 0.999, 1e-8
                self.t += 1
                lr_t = lr * (1.0 - b2 ** self.t) ** 0.5 / (1.0 - b1 ** self.t)
                for k, p in self.params.items():
                    g = grads[k]
                    self.m[k].mul_(b1).add_(g, alpha=1.0 - b1)
                    self.v[k].mul_(b2).addcmul_(g, g, value=1.0 - b2)
                    p.sub_(lr_t * self.m[k] / (self.v[k].sqrt() + eps))
            elif self.kind == 'momentum':
                for k, p in self.params.items():
                    self.m[k].mul_(self.momentum).add_(grads[k])
                    p.sub_(lr * self.m[k])
            else:
                for k, p in self.params.items():
                    p.sub_(lr * grads[k])

    def _get(self, k):
        return self.params[k] if k in self.params else self.consts[k]

    def _conv(self, x, name):
        k = self._get(f'{name}/kernel').permute(3, 2, 0, 1)
        return Fn.conv2d(x, k, self._get(f'{name}/bias'), padding=k.shape[-1] // 2)

    def _bn(self, x, name):
        g, b, m, v = (self._get(f'{name}/{f}').view(1, -1, 1, 1) for f in W.BN_FIELDS)
        return g * (x - m) / torch.sqrt(v + 1e-3) + b

    def forward(self, boards):
        x = boards.permute(0, 3, 1, 2)
        x = torch.relu(self._bn(self._conv(x, 'resTower/conv_block/conv'), 'resTower/conv_block/batch_norm'))
        for i in range(self.R):
            h = torch.relu(self._bn(self._conv(x, f'resTower/block_{i}/conv_1'), f'resTower/block_{i}/batch_norm_1'))
            h = self._bn(self._conv(h, f'resTower/block_{i}/conv_2'), f'resTower/block_{i}/batch_norm_2')
            x = torch.relu(h + x)
        v = torch.relu(self._bn(self._conv(x, 'value/convolution'), 'value/batch_norm')).permute(0, 2, 3, 1)
        v = torch.relu((v @ self._get('value/dense_1/kernel') + self._get('value/dense_1/bias')).sum(dim=(1, 2)))
        value = torch.tanh((v @ self._get('value/dense_2/kernel') + self._get('value/dense_2/bias')).sum(dim=1))
        p = torch.relu(self._bn(self._conv(x, 'policy/convolution'), 'policy/batch_norm')).permute(0, 2, 3, 1)
        logits = (p @ self._get('policy/policy/kernel') + self._get('policy/policy/bias')).sum(dim=(1, 2))
        return value, logits

    def loss(self, boards, evalLabel, policyLabel, noise=None):
        _no_noise(self.loss_kind, noise)
        value, logits = self.forward(boards)
        if self.loss_kind == 'per_example':
            lossEvaluation = torch.mean((value - evalLabel) ** 2)
            # (a row of zeros contributes 0 * log_softmax = 0 and has no gradient)
            lossPolicy = -(policyLabel * torch.log_softmax(logits, dim=1)).sum() / policyLabel.shape[0]
            lossParam = self.l2 * torch.stack([0.5 * (p ** 2).sum() for k, p in self.params.items() if 'bias' not in k]).sum()
            return lossEvaluation + lossPolicy + lossParam, (lossEvaluation, lossPolicy, lossParam)
        base = torch.softmax(logits, dim=1)
        if noise is None:  # A independent Beta(alpha, 1-alpha) draws shared across the batch
            noise = torch.distributions.Beta(self.alpha, 1.0 - self.alpha).sample((self.A,)).to(self.device)
        policy = (1 - self.epsilon) * base + self.epsilon * noise.view(1, -1)
        policy = policy / policy.sum()
        lossEvaluation = torch.mean((value - evalLabel) ** 2)
        lossPolicy = -torch.mean(torch.log(policy) @ policyLabel.t())
        l2 = [0.5 * (p ** 2).sum() for k, p in self.params.items() if 'bias' not in k]
        lossParam = torch.stack(l2).mean()
        return lossEvaluation + lossPolicy + lossParam, (lossEvaluation, lossPolicy, lossParam)

    def _gradients_tensors(self, boards, evalLabel, policyLabel, noise=None):
        """The tensor-level core of `gradients`, `step` and `step_tensors`: float32 tensors on the trainer's device in,
        (loss, its three terms, {variable: gradient}) out as tensors -- nothing is brought to the host."""
        total, parts = self.loss(boards, evalLabel, policyLabel, noise)
        names = list(self.params)
        gs = torch.autograd.grad(total, [self.params[k] for k in names])
        return total.detach(), [p.detach() for p in parts], dict(zip(names, gs))

    def gradients(self, state, eval, policy, noise=None):
        """Loss, its three terms and d loss / d variable for one batch (what optimizer.minimize(loss) differentiates).
        noise: the A Beta(alpha, 1-alpha) draws of the graph's Dirichlet node, or None to draw them."""
        boards = torch.tensor(np.asarray(state, dtype=np.float32), device=self.device)
        ev = torch.tensor(np.asarray(eval, dtype=np.float32).reshape(-1), device=self.device)
        pl = torch.tensor(np.asarray(policy, dtype=np.float32), device=self.device)
        if noise is not None:
            noise = torch.tensor(np.asarray(noise, dtype=np.float32), device=self.device)
        total, parts, grads = self._gradients_tensors(boards, ev, pl, noise)
        return float(total), [float(p) for p in parts], grads

    def step(self, state, eval, policy, learningRate, noise=None):
        total, parts, grads = self.gradients(state, eval, policy, noise)
        self._apply(grads, float(learningRate))
        return total, parts

    def step_tensors(self, boards, evalLabel, policyLabel, learningRate, noise=None):
        """`step` for a batch that is already on the trainer's device as float32 tensors (boards [B,H,W,C], evalLabel [B],
        policyLabel [B,A], noise [A] or None): no host copy on the way in, and the loss and its terms come back as
        tensors, so the call does not wait for the GPU."""
        total, parts, grads = self._gradients_tensors(boards, evalLabel.reshape(-1), policyLabel, noise)
        self._apply(grads, float(learningRate))
        return total, parts

    def evaluate_tensors(self, boards, evalLabel, policyLabel, rows=False):
        """Score rows with the current weights, forward only (HipTrainer.evaluate_tensors' definitions in float32 torch): per row
        the value, se = (value - z)^2 and ce = -sum_a pi[a] log_softmax(logits)[a] against the row's own label (0 for a row
        whose label is all zeros: the terminal example) -- no noise, no batch coupling, no L2 term.  Returns eval_summary's dict;
        rows=True adds 'per_row' [n, 3] (value, se, ce) and 'flags' [n] (uint8, _lib.ROW_*)."""
        with torch.no_grad():
            z, pi = evalLabel.reshape(-1), policyLabel
            n = int(pi.shape[0])
            if n:
                value, logits = self.forward(boards)
            else:
                value, logits = z.new_zeros(0), pi.new_zeros((0, self.A))
            has = (pi != 0).any(dim=1)
            se = (value - z) ** 2
            ce = torch.where(has, -(pi * torch.log_softmax(logits, dim=1)).sum(dim=1), torch.zeros_like(se))
            top1 = has & (torch.argmax(logits, dim=1) == torch.argmax(pi, dim=1)) if n else has    # (argmax: the first maximum)
            decided = z != 0
            sign_ok = decided & (((value > 0) & (z > 0)) | ((value < 0) & (z < 0)))
            out = eval_summary(n, int(has.sum()), int(top1.sum()), int(decided.sum()), int(sign_ok.sum()),
                               float(se.double().sum()), float(ce.double().sum()))
            if rows:
                out['per_row'] = torch.stack([value, se, ce], dim=1)
                out['flags'] = (has * _lib.ROW_HAS_POLICY + top1 * _lib.ROW_TOP1 + decided * _lib.ROW_DECIDED
                                + sign_ok * _lib.ROW_SIGN_OK + _lib.ROW_COUNTED).to(torch.uint8)
        return out

    def _flat_device(self):
        """The weights as ONE float32 device tensor in weights.flatten's order (weights.flat_fields), constants included, and
        {bb_net_weights field: its offset in floats}: what bb_load_weights_device's descriptor points into."""
        offsets, tensors, at = {}, [], 0
        for field, shape, names, _ in W.blocks(self.C, self.F, self.R, self.D, self.A):
            offsets[field] = at
            tensors += [self._get(name).detach().reshape(-1) for name in names]
            at += int(np.prod(shape))
        flat = torch.cat([t.to(torch.float32) for t in tensors])
        assert int(flat.numel()) == at, (int(flat.numel()), at)
        return flat, offsets

    def load_into(self, engine):
        """Hand the current weights to `engine` (an _lib.Engine that has had load_weights with a network of this shape) on the
        device: one torch.cat into a flat tensor, a descriptor into it, bb_load_weights_device on torch's current stream -- no
        export, no host packing.  16 filters, every game (DragonChess too); the engine refuses anything else (AssertionError
        for a shape that is not what it holds, ValueError for another game)."""
        if self.device.type != 'cuda':
            raise _lib.BlackbirdHipError('load_into hands weights over on the GPU; this trainer is on %s' % self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            flat, offsets = self._flat_device()
            desc = _lib.net_weights_device(engine.info.H, engine.info.W, self.C, self.F, self.R, self.D, self.A, flat.data_ptr(), offsets)
            engine.load_weights_device(desc, stream.cuda_stream)
        flat.record_stream(stream)      # the kernels read it after this returns; `stream` waits for them

    def export(self):
        out = {k: v.detach().cpu().numpy().copy() for k, v in self.params.items()}
        out.update({k: v.cpu().numpy().copy() for k, v in self.consts.items()})
        return out


def eval_summary(rows, policy_rows, top1, decided, sign_ok, se_sum, ce_sum):
    """The dict an evaluation returns, from its counts and its two sums (Python numbers): the counts, the sums, and the means
    value_mse = se_sum / rows, policy_ce = ce_sum / policy_rows, top1_rate = top1 / policy_rows, sign_rate = sign_ok / decided --
    NaN over zero rows.  Counts and sums of several evaluations add; the means are then taken from the added figures."""
    mean = lambda a, b: float(a) / float(b) if b else float('nan')  # noqa: E731
    return {'rows': int(rows), 'policy_rows': int(policy_rows), 'top1': int(top1), 'decided': int(decided), 'sign_ok': int(sign_ok),
            'se_sum': float(se_sum), 'ce_sum': float(ce_sum), 'value_mse': mean(se_sum, rows), 'policy_ce': mean(ce_sum, policy_rows),
            'top1_rate': mean(top1, policy_rows), 'sign_rate': mean(sign_ok, decided)}


EVAL_COUNTS = ('rows', 'policy_rows', 'top1', 'decided', 'sign_ok', 'se_sum', 'ce_sum')     # eval_summary's arguments, in order


def _device_index(dev):
    """The number of the GPU a torch.device names (one without an index: torch's current device)."""
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _records_source(examples, game, index, who, what):
    """What the method `who` of a `what` ('trainer', 'engine') of game `game` on GPU `index` asks of the records it reads: a
    DeviceExamples of that game on that GPU, or ValueError.  Returns the records' device."""
    if not isinstance(examples, DeviceExamples):
        raise ValueError('%s takes a DeviceExamples (merged rows carry sums of their own and are not a records source), got %s'
                         % (who, type(examples).__name__))
    if examples.game != game:
        raise ValueError('the examples are of game %d, the %s of game %d' % (examples.game, what, game))
    dev = examples.records.device
    if dev.type != 'cuda' or _device_index(dev) != index:
        raise ValueError('the examples are on %s, the %s on cuda:%d' % (dev, what, index))
    return dev


def _row_tensors(dev, n, **named):
    """The per-row tensors a records call takes, by name ('sym': uint8, every other one int64), each None or contiguous, of `n`
    entries, on `dev`: ValueError otherwise."""
    for name, t in named.items():
        dtype = torch.uint8 if name == 'sym' else torch.int64
        if t is not None and (t.dtype != dtype or t.device != dev or int(t.numel()) != n or not t.is_contiguous()):
            raise ValueError('%s: a contiguous %s tensor of %d entries on %s is expected' % (name, dtype, n, dev))


def _scored(dev, n, launch, keep, rows, outputs_too=False):
    """The common part of every scorer: the outputs of `n` rows on `dev`, `launch(rows_ptr, flags_ptr, totals_ptr, stream)` on
    torch's current stream, and the one synchronising read of the totals.  `keep`: the tensors the launch reads (None entries
    skipped); outputs_too: the launch runs on a stream torch does not know, so the outputs stay alive past it as well."""
    out_rows = torch.empty((n, 3), dtype=torch.float32, device=dev)
    out_flags = torch.empty((n,), dtype=torch.uint8, device=dev)
    totals = torch.empty(np.dtype(_lib.EVAL_TOTALS_DTYPE).itemsize, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        launch(out_rows.data_ptr(), out_flags.data_ptr(), totals.data_ptr(), stream.cuda_stream)
    for t in tuple(keep) + ((out_rows, out_flags, totals) if outputs_too else ()):   # asynchronous: alive until the stream has used them
        if t is not None:
            t.record_stream(stream)
    tot = totals.cpu().numpy().view(_lib.EVAL_TOTALS_DTYPE)[0]      # (waits for the launches)
    out = eval_summary(*[tot[k].item() for k in EVAL_COUNTS])
    if rows:
        out['per_row'], out['flags'] = out_rows, out_flags
    return out


HIP_TRAINER_LIMITS = 'Connect4 or TicTacToe, 16 filters, 0 to 9 blocks, a dense width of 1 to 64'
HIP_TRAINER_DC_BLOCKS = 8     # train_max_blocks<DragonChess>() of csrc/train.hip.h: the blocks whose workgroup fits a CU's 160 KB of LDS
HIP_TRAINER_LIMITS_ALL = ('Connect4 or TicTacToe (0 to 9 blocks) or DragonChess (0 to %d blocks: the LDS of a CU; batch tensors only, no '
                          'records source, no scorer), 16 filters, a dense width of 1 to 64' % HIP_TRAINER_DC_BLOCKS)
HIP_GAMES = ('dense', 'all')  # NetworkConfig['training']['hip_games']: what backend 'hip' may be asked for
_GAME_BY_PLANES = {(7, 3): (_lib.GAME_CONNECT4, 6, 7), (9, 3): (_lib.GAME_TICTACTOE, 3, 3),
                   (4032, 17): (_lib.GAME_DRAGONCHESS, 8, 8)}   # (A, C) -> game, H, W
_OPTIMIZERS = {'adam': _lib.OPT_ADAM, 'momentum': _lib.OPT_MOMENTUM, 'sgd': _lib.OPT_SGD}


def hip_trainer_supports(weights, games='dense'):
    """Whether `weights` (TF-named dict) is a network the HIP training kernels cover: games='dense', Connect4 and TicTacToe
    (HIP_TRAINER_LIMITS); games='all', DragonChess too (HIP_TRAINER_LIMITS_ALL)."""
    if games not in HIP_GAMES:
        raise ValueError("hip_games is 'dense' or 'all', got %r" % (games,))
    C, F, R, D, A = W.infer_shape(weights)
    if (A, C) not in _GAME_BY_PLANES or F != 16 or not 1 <= D <= 64:
        return False
    if _GAME_BY_PLANES[(A, C)][0] == _lib.GAME_DRAGONCHESS:
        return games == 'all' and 0 <= R <= HIP_TRAINER_DC_BLOCKS
    return 0 <= R <= 9


class HipTrainer:
    """`Trainer` with the step as HIP kernels of libblackbird_hip.so (bb_trainer_*, csrc/train.hip.h): the same loss, the
    same optimiser rules, the same interface -- chosen with NetworkConfig['training']['backend'] = 'hip'.  Parameters,
    optimiser slots and gradients live in the library's own device buffers; `export` reads the parameters back.  Covers
    HIP_TRAINER_LIMITS_ALL; anything else raises ValueError.  A DragonChess trainer (`wide`) steps from batch tensors only:
    epoch_records, evaluate_records and evaluate_tensors raise ValueError for it.  `seed` keys the Beta noise a step draws when none is given
    (None: from numpy's generator, as the engines do); `max_batch` bounds the examples of one step.  loss='per_example' (with its
    coefficient `l2`) makes every step the per-example loss of the module's docstring (bb_trainer_set_loss), from either source."""

    def __init__(self, weights, alpha=0.2, epsilon=0.3, optimizer='adam', momentum=0.9, device=None, seed=None, max_batch=1024,
                 loss='reference', l2=1e-4):
        self.loss_kind, self.l2 = check_loss(loss, l2)
        self.device = torch.device(device or 'cuda')
        if self.device.type != 'cuda':
            raise _lib.BlackbirdHipError('HipTrainer runs on the GPU only (device %s)' % self.device)
        self.alpha, self.epsilon = float(alpha), float(epsilon)
        self.C, self.F, self.R, self.D, self.A = W.infer_shape(weights)
        if not hip_trainer_supports(weights, 'all'):
            raise ValueError('the hip training backend covers %s; got %d input planes, %d actions, %d filters, %d blocks, '
                             'dense %d' % (HIP_TRAINER_LIMITS_ALL, self.C, self.A, self.F, self.R, self.D))
        if optimizer not in _OPTIMIZERS:   # (Trainer treats any other name as sgd; the kernels are asked by number)
            optimizer = 'sgd'
        self.kind, self.momentum = optimizer, float(momentum)
        self.game, self.H, self.Wd = _GAME_BY_PLANES[(self.A, self.C)]
        self.wide = self.game == _lib.GAME_DRAGONCHESS
        self.max_batch = int(max_batch)
        if seed is None:
            from .MCTS import _seed_from_numpy
            seed = _seed_from_numpy()
        self._index = _device_index(self.device)
        self._h = _lib.trainer_create(self.game, W.flatten(weights), self.H, self.Wd, _OPTIMIZERS[optimizer], self.max_batch,
                                      device=self._index, momentum=self.momentum, alpha=self.alpha, epsilon=self.epsilon,
                                      seed=seed)
        self.count = _lib.trainer_param_count(self._h)
        if self.loss_kind != 'reference':      # (a trainer is created with the reference loss)
            _lib.trainer_set_loss(self._h, _lib.LOSS_PER_EXAMPLE, self.l2)

    def close(self):
        h, self._h = getattr(self, '_h', None), None
        _lib.trainer_destroy(h)

    __del__ = close

    def _f32(self, x, shape):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        t = t.to(device=self.device, dtype=torch.float32).reshape(shape).contiguous()
        return t

    def _batch_tensors(self, boards, evalLabel, policyLabel):
        """(n, boards [n,H,W,C], evalLabel [n], policyLabel [n,A]): a batch as float32 tensors on the trainer's device."""
        n = int(policyLabel.shape[0]) if hasattr(policyLabel, 'shape') else len(policyLabel)
        return n, self._f32(boards, (n, self.H, self.Wd, self.C)), self._f32(evalLabel, (n,)), self._f32(policyLabel, (n, self.A))

    def _launch(self, boards, evalLabel, policyLabel, noise, lr, apply):
        """One bb_trainer_step on torch's current stream; returns the device tensor [4] of the loss and its terms."""
        _no_noise(self.loss_kind, noise)
        n, boards, ev, pl = self._batch_tensors(boards, evalLabel, policyLabel)
        nz = None if noise is None else self._f32(noise, (self.A,))
        loss = torch.empty(4, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.trainer_step(self._h, n, boards.data_ptr(), ev.data_ptr(), pl.data_ptr(), None if nz is None else nz.data_ptr(),
                              lr, apply, loss.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        for t in (boards, ev, pl, nz):     # the launch is asynchronous: the inputs stay alive until the stream has used them
            if t is not None:
                t.record_stream(torch.cuda.current_stream(self.device))
        return loss

    def _not_wide(self, who):
        if self.wide:
            raise ValueError('%s: the records source and the scorer of the hip training backend cover Connect4 and TicTacToe; a '
                             'DragonChess trainer steps from batch tensors (step, step_tensors, gradients)' % who)

    def _named(self, what):
        return W.unflatten(_lib.trainer_read(self._h, what), self.C, self.F, self.R, self.D, self.A)

    def gradients(self, state, eval, policy, noise=None):
        """Loss, its three terms (floats) and {TF variable name: d loss / d variable} of one batch; no update."""
        loss = self._launch(np.asarray(state), np.asarray(eval).reshape(-1), np.asarray(policy), noise, 0.0, False).cpu().numpy()
        grads = {k: torch.from_numpy(v).to(self.device) for k, v in self._named(_lib.TRAIN_GRADS).items()
                 if not (k.endswith('moving_mean') or k.endswith('moving_variance'))}
        return float(loss[0]), [float(x) for x in loss[1:]], grads

    def step(self, state, eval, policy, learningRate, noise=None):
        loss = self._launch(np.asarray(state), np.asarray(eval).reshape(-1), np.asarray(policy), noise, float(learningRate),
                            True).cpu().numpy()
        return float(loss[0]), [float(x) for x in loss[1:]]

    def step_tensors(self, boards, evalLabel, policyLabel, learningRate, noise=None):
        """`step` for float32 tensors already on the trainer's device: launched on torch's current stream, not waited for;
        the loss and its terms come back as device tensors."""
        loss = self._launch(boards, evalLabel, policyLabel, noise, float(learningRate), True)
        return loss[0], [loss[1], loss[2], loss[3]]

    def epoch_records(self, examples, order, batchSize, learningRate, sym=None, noise=None):
        """A whole epoch of steps straight from example records (bb_trainer_epoch): batch i is the records
        order[i * batchSize:(i + 1) * batchSize] -- each under its entry of `sym`, when given --, and the steps are, bit for
        bit, those of `step_tensors(*examples._batch(order[rows], sym[rows]), learningRate)` batch after batch, without the batch
        tensors and without a trip through Python per batch.  Enqueued on torch's current stream in one call and not waited
        for; returns the device tensor [n_batches, 4] of every batch's loss and its three terms.

        examples: a DeviceExamples of the trainer's game on the trainer's device (merged rows are not a records source:
        ValueError).  order, sym: tensors as examples.index_tensor and examples.sym_tensor return them (order None: the records
        in order), whole batches.  noise: [n_batches, A] or None to draw it.  Malformed rows count in examples.bad()."""
        self._not_wide('epoch_records')
        _no_noise(self.loss_kind, noise)
        dev = _records_source(examples, self.game, self._index, 'epoch_records', 'trainer')
        batch = int(batchSize)
        if batch < 1 or batch > self.max_batch:
            raise ValueError('batches of %d examples; the trainer takes 1..%d (max_batch)' % (batch, self.max_batch))
        rows = len(examples) if order is None else int(order.numel())
        if rows % batch:
            raise ValueError('%d rows are no whole number of batches of %d' % (rows, batch))
        n_batches = rows // batch
        _row_tensors(dev, rows, order=order, sym=sym)
        nz = None if noise is None else self._f32(noise, (n_batches, self.A))
        loss = torch.empty((n_batches, 4), dtype=torch.float32, device=self.device)
        if n_batches == 0:
            return loss
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            _lib.trainer_epoch(self._h, len(examples), examples.records.data_ptr(), n_batches, batch,
                               None if order is None else order.data_ptr(), None if sym is None else sym.data_ptr(),
                               None if nz is None else nz.data_ptr(), float(learningRate), loss.data_ptr(),
                               examples._bad.data_ptr(), stream.cuda_stream)
        for t in (examples.records, examples._bad, order, sym, nz):   # asynchronous: alive until the stream has used them
            if t is not None:
                t.record_stream(stream)
        return loss

    def evaluate_records(self, examples, index=None, sym=None, rows=False):
        """Score example records with the trainer's current device parameters (bb_trainer_eval: forward only -- no step, no noise,
        no export; parameters, slots, gradients and the noise stream of later steps are untouched).  Row k is record index[k]
        (None: every record, in order) under symmetry sym[k] (None: as played), decoded as `examples._batch(index, sym)` decodes
        it.  Any number of rows: max_batch does not bound it.  Returns eval_summary's dict of Python numbers -- the counts rows,
        policy_rows, top1, decided, sign_ok, the sums se_sum, ce_sum and the means value_mse, policy_ce, top1_rate, sign_rate (NaN
        over zero rows) -- after one synchronising read; rows=True adds the device tensors 'per_row' [n, 3] (value, se, ce) and
        'flags' [n] (uint8, _lib.ROW_*).

        examples: a DeviceExamples of the trainer's game on the trainer's device (merged rows are not a records source:
        ValueError).  index, sym: tensors as examples.index_tensor and examples.sym_tensor return them, or anything those take.
        Malformed rows are zeros with flags 0, outside every total, and count in examples.bad()."""
        self._not_wide('evaluate_records')
        dev = _records_source(examples, self.game, self._index, 'evaluate_records', 'trainer')
        if index is not None and not torch.is_tensor(index):
            index = examples.index_tensor(index)
        if sym is not None and not torch.is_tensor(sym):
            sym = examples.sym_tensor(sym)
        n = len(examples) if index is None else int(index.numel())
        _row_tensors(dev, n, index=index, sym=sym)
        return _scored(
            self.device, n, lambda r, f, tot, st: _lib.trainer_eval(self._h, len(examples), examples.records.data_ptr() if len(examples) else None, n,
                                                       None if index is None else index.data_ptr(),
                                                       None if sym is None else sym.data_ptr(), r, f, tot, examples._bad.data_ptr(), st),
            (examples.records, examples._bad, index, sym), rows)

    def evaluate_tensors(self, boards, evalLabel, policyLabel, rows=False):
        """`evaluate_records` for rows given as the three tensors of a batch (bb_trainer_eval_tensors): boards [n,H,W,C], evalLabel
        [n], policyLabel [n,A].  The same kernel reads either source: evaluate_records(ex, index, sym) and
        evaluate_tensors(*ex._batch(index, sym)) give the same bits."""
        self._not_wide('evaluate_tensors')
        n, boards, ev, pl = self._batch_tensors(boards, evalLabel, policyLabel)
        return _scored(
            self.device, n, lambda r, f, tot, st: _lib.trainer_eval_tensors(self._h, n, boards.data_ptr() if n else None, ev.data_ptr() if n else None,
                                                               pl.data_ptr() if n else None, r, f, tot, st),
            (boards, ev, pl), rows)

    def last_noise(self):
        """The noise of the last step (given or drawn), read back from the device."""
        return _lib.trainer_read(self._h, _lib.TRAIN_NOISE, self.A)

    def slots(self):
        """(m, v) as TF-named dicts: Adam's moments, or Momentum's accumulator and zeros."""
        drop = lambda d: {k: v for k, v in d.items() if not (k.endswith('moving_mean') or k.endswith('moving_variance'))}  # noqa: E731
        return drop(self._named(_lib.TRAIN_SLOT_M)), drop(self._named(_lib.TRAIN_SLOT_V))

    def export(self):
        return self._named(_lib.TRAIN_PARAMS)

    def load_into(self, engine):
        """Hand the current parameters to `engine` (an _lib.Engine of the trainer's game that has had load_weights with a
        network of this shape) on the device (bb_trainer_load_engine on torch's current stream): the operand images are packed
        by kernels straight from the parameter buffer, behind the steps already queued -- no export, no host packing.  The
        engine refuses what it cannot take: AssertionError for a shape that is not what it holds or an engine without
        weights, ValueError for another game or device."""
        with torch.cuda.device(self.device):
            _lib.trainer_load_engine(self._h, engine, torch.cuda.current_stream(self.device).cuda_stream)


def epoch_order(n, batchSize):
    """The order in which an epoch visits `n` examples in whole batches: TrainWithExamples' draw (Blackbird.py:292-293),
    consuming numpy's global generator exactly as it does -- the same numpy seed gives the same batches on the host
    path and on the device path."""
    return np.random.choice(n, n - n % batchSize, replace=False)


class _ExampleRows:
    """What DeviceExamples and MergedExamples share: `records` on a device, len(self) rows over them (records, or groups of
    them), and `batch`, which turns any selection of the rows into the three float32 tensors the loss takes -- one HIP launch
    on torch's current stream, the class's own (`_to_batch`), nothing staged through the host."""

    def index_tensor(self, index):
        """`index` (int64 tensor or anything numpy takes) as an int64 tensor on the records' device, range-checked:
        every entry must name one of the len(self) rows (records; of merged rows, groups)."""
        if torch.is_tensor(index):
            idx = index.to(device=self.records.device, dtype=torch.int64).reshape(-1)
            wrong = bool(((idx < 0) | (idx >= len(self))).any()) if idx.numel() else False
        else:
            host = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
            wrong = bool(((host < 0) | (host >= len(self))).any())
            idx = torch.from_numpy(host).to(self.records.device)
        if wrong:
            raise IndexError('example index out of range [0, %d)' % len(self))
        return idx.contiguous()

    @property
    def symmetries(self):
        """How many board symmetries the game has (bb_game_symmetries): the values `sym` may take are 0 .. symmetries - 1."""
        return _lib.game_symmetries(self.game)

    def sym_tensor(self, sym):
        """`sym` (uint8 tensor on the records' device, or anything numpy takes) as a uint8 tensor on the records' device.  What
        arrives from the host is range-checked here against `symmetries` (ValueError); a tensor that is on the device already
        is left to the kernel, which writes a row of zeros for a symmetry the game does not have and counts it in bad()."""
        if torch.is_tensor(sym) and sym.device == self.records.device and sym.device.type != 'cpu':
            if sym.dtype != torch.uint8:
                raise ValueError('sym: a uint8 tensor is expected on the device, got %s' % sym.dtype)
            return sym.reshape(-1).contiguous()
        host = np.asarray(sym.cpu() if torch.is_tensor(sym) else sym).reshape(-1)
        if host.size and (host.dtype.kind not in 'iub' or int(host.min()) < 0 or int(host.max()) >= self.symmetries):
            raise ValueError('sym: integers in [0, %d) are expected (the symmetries of game %d)' % (self.symmetries, self.game))
        return torch.from_numpy(host.astype(np.uint8)).to(self.records.device)

    def batch(self, index=None, sym=None):
        """(boards [n,H,W,C], value [n], policy [n,A]) of the rows `index` names (None: all, in order), fresh float32
        tensors on the records' device: what TrainWithExamples stacks per batch, in Network.train's argument order.
        sym (None: as played): one symmetry of the game per output row, < `symmetries` -- the row is that of the position
        mirrored or turned so, planes and policy alike (bb_examples_to_batch_sym; an extension, the reference does not
        augment)."""
        return self._batch(None if index is None else self.index_tensor(index), None if sym is None else self.sym_tensor(sym))

    def _batch(self, idx, sym=None):
        """`batch` for an index tensor that index_tensor returned (or a slice of one), and a symmetry tensor that sym_tensor
        returned (or a slice of one)."""
        gi, dev = self.info, self.records.device
        n = len(self) if idx is None else int(idx.numel())
        if sym is not None and int(sym.numel()) != n:
            raise ValueError('sym: one entry per output row is expected (%d rows, %d entries)' % (n, int(sym.numel())))
        boards = torch.empty((n, gi.H, gi.W, gi.C), dtype=torch.float32, device=dev)
        value = torch.empty((n,), dtype=torch.float32, device=dev)
        policy = torch.empty((n, gi.A), dtype=torch.float32, device=dev)
        if n == 0:
            return boards, value, policy
        if dev.type != 'cuda':
            raise _lib.BlackbirdHipError('%s.batch runs on the GPU only (records on %s)' % (type(self).__name__, dev))
        with torch.cuda.device(dev):
            self._to_batch(n, None if idx is None else idx.data_ptr(), None if sym is None else sym.data_ptr(), boards.data_ptr(),
                           policy.data_ptr(), value.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return boards, value, policy


class DeviceExamples(_ExampleRows):
    """Self-play example records that stay on the GPU: a game id and a uint8 tensor [N, example_bytes] in the layout of
    bb_examples_fetch.  `batch` turns any selection of them into the three float32 tensors the loss takes
    (bb_examples_to_batch: one HIP launch on torch's current stream, nothing staged through the host).

    The records may come from one engine (`from_engine`), from the host (`from_records`) or from every rank:
    DeviceExamples(game, dist.allgather_engine_examples(eng, device)[0]) takes the all-gathered tensor as it is."""

    def __init__(self, game, records):
        gi = _lib.game_info(game)
        if records.dtype != torch.uint8 or records.dim() != 2 or records.shape[1] != gi.example_bytes:
            raise ValueError('records: a uint8 tensor [N, %d] is expected, got %s %r'
                             % (gi.example_bytes, records.dtype, tuple(records.shape)))
        self.game, self.info = game, gi
        self.records = records.contiguous()
        self._bad = torch.zeros(1, dtype=torch.int32, device=records.device)

    @classmethod
    def from_engine(cls, eng, device):
        """A snapshot of the finished games' records of `eng`, in (game, ply) order.  dist.engine_records_device compacts
        the engine's store into a tensor of its own; the clone makes the snapshot independent of how it does so -- the
        store is written again by the next bb_selfplay_begin."""
        from . import dist
        return cls(eng.game, dist.engine_records_device(eng, device).clone())

    @classmethod
    def from_records(cls, game, records, device):
        """From a host structured array (Engine.fetch_examples / fetch_games, _lib.example_dtype)."""
        raw = np.ascontiguousarray(records).view(np.uint8).reshape(len(records), -1)
        return cls(game, torch.from_numpy(raw.copy()).to(torch.device(device)))

    @classmethod
    def cat(cls, parts):
        """The records of several sets of one game, in list order; the count of rejected rows carries over."""
        parts = list(parts)
        if not parts or any(p.game != parts[0].game for p in parts):
            raise ValueError('cat needs at least one DeviceExamples, all of one game')
        out = cls(parts[0].game, torch.cat([p.records for p in parts]))
        for p in parts:
            out._bad += p._bad.to(out._bad.device)
        return out

    def __len__(self):
        return int(self.records.shape[0])

    def split_games(self, fraction, seed):
        """(train, held): these records split by whole games, for a held-out score (HipTrainer.evaluate_records).  Games are told
        apart by the header's game_id (bytes 0..3 of a record).  k = round(fraction * n_games) games are held out, clipped to
        [1, n_games - 1]: the first k entries of np.random.RandomState(seed).permutation(sorted unique ids) -- numpy's global
        generator is not touched.  Both parts keep the record order, so no game straddles the split.  ValueError with fewer than
        two games.  Plain torch indexing on the records' own device (CPU records too), for every game: only the header is read.
        The count of rejected rows does not carry over."""
        ids = self.records[:, :4].contiguous().view(torch.int32).reshape(-1)
        uniq = torch.unique(ids).cpu().numpy()                        # (sorted)
        if len(uniq) < 2:
            raise ValueError('split_games needs at least two games, the records hold %d' % len(uniq))
        k = min(max(int(round(float(fraction) * len(uniq))), 1), len(uniq) - 1)
        held_ids = np.random.RandomState(seed).permutation(uniq)[:k]
        held = torch.isin(ids, torch.from_numpy(held_ids).to(ids.device))
        return type(self)(self.game, self.records[~held]), type(self)(self.game, self.records[held])

    def _to_batch(self, n, idx, sym, boards, policy, value, stream):
        _lib.examples_to_batch_sym(self.game, len(self), self.records.data_ptr(), n, idx, sym, boards, policy, value,
                                   self._bad.data_ptr(), stream)

    def score_with(self, engine, index=None, rows=False, chunk_rows=4096):
        """Score these records with the network `engine` (an _lib.Engine of this game, on the records' device, with weights
        loaded) holds -- bb_examples_score: the engine's own network launch, whatever its game, width and net form, so the
        figures are those of the arithmetic that evaluates positions in self-play.  Row k is record index[k] (None: every
        record, in order).  Returns eval_summary's dict of Python numbers, HipTrainer.evaluate_records' keys with the same
        meaning, after one synchronising read; rows=True adds the device tensors 'per_row' [n, 3] (value, se, ce) and 'flags' [n]
        (uint8, _lib.ROW_*).  chunk_rows: the rows per network launch; the workspace (states, values and logits of one chunk:
        bb_examples_score_workspace) is a torch tensor kept with the records and reused while it is large enough.  The chunk
        size does not change a bit of the result.  The engine's trees, counters, evaluation cache and weights are untouched; the
        call waits for the engine's own streams first.  Malformed rows are zeros with flags 0, outside every total, and count in
        bad()."""
        if not isinstance(engine, _lib.Engine):
            raise ValueError('score_with takes an _lib.Engine, got %s' % type(engine).__name__)
        dev = _records_source(self, engine.game, int(engine.cfg.device), 'score_with', 'engine')
        if index is not None and not torch.is_tensor(index):
            index = self.index_tensor(index)
        n = len(self) if index is None else int(index.numel())
        if index is not None and (index.dtype != torch.int64 or index.device != dev or not index.is_contiguous()):
            raise ValueError('index: a contiguous %s tensor on %s is expected' % (torch.int64, dev))
        chunk = min(max(int(chunk_rows), 1), max(n, 1))
        nbytes = engine.score_workspace(chunk)
        work = getattr(self, '_score_work', None)
        if work is None or int(work.numel()) < nbytes:
            work = self._score_work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return _scored(     # (the engine's stream uses the outputs and the workspace: alive until torch's stream is past its wait)
            dev, n, lambda r, f, tot, st: engine.score_examples(len(self), self.records.data_ptr() if len(self) else None, n,
                                                                None if index is None else index.data_ptr(), r if n else None,
                                                                f if n else None, tot, self._bad.data_ptr(), work.data_ptr(), nbytes, st),
            (self.records, self._bad, index, work), rows, outputs_too=True)

    def bad(self):
        """Rows that bb_examples_to_batch rejected (and wrote as zeros) since this object was made: malformed records.
        Waits for the GPU -- look at it once per epoch, not once per batch."""
        return int(self._bad.item())

    def merged(self):
        """These records with the copies of a position merged into one row each (MergedExamples; an extension, Connect4 and
        TicTacToe): bb_examples_merge on torch's current stream and one look at the group count."""
        return MergedExamples(self)


def _merge_scope(game):
    if game not in _lib.GRID:
        raise ValueError('merging duplicate positions covers Connect4 and TicTacToe: DragonChess (game %d) has a 64-byte board key '
                         'plus castle flags, compact child lists and few transpositions, and is not covered' % game)


def merge_records_host(game, records):
    """The definition of merging, in numpy, on a host structured array (_lib.example_dtype) -- the statement the tests hold
    bb_examples_merge against; the product uses it for records that are on the CPU and never for device records.

    The key of a record is what the network sees of its state: the cells of both players and the side to move (not the previous
    player, not the header).  A record with n_children > S is malformed: group -1.  Groups are numbered by the index of their
    first member.  Returns (group [n] int32, rep [G] int32, count [G] int32, zsum [G] int32, total [G] uint64, visits [G, A]
    uint64): per group the first member, the member count and the integer sums of z, total and visits[:A]."""
    _merge_scope(game)
    gi = _lib.game_info(game)
    records = np.asarray(records)
    n = len(records)
    group = np.full(n, -1, dtype=np.int32)
    good = np.flatnonzero(records['n_children'] <= gi.S) if n else np.zeros(0, dtype=np.int64)
    if good.size == 0:
        return (group, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint64),
                np.zeros((0, gi.A), np.uint64))
    st = np.ascontiguousarray(records['state']).view('<u8').reshape(n, 2)[good]
    cells = np.uint64(0x00FFFFFFFFFFFFFF)
    key = np.stack([st[:, 0] & cells, st[:, 1] & cells, (st[:, 0] >> np.uint64(56)) & np.uint64(3)], axis=1)
    _uniq, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    by_first = np.argsort(first, kind='stable')          # unique keys in the order of their first member
    number = np.empty(len(first), dtype=np.int64)
    number[by_first] = np.arange(len(first))
    g = number[inverse.reshape(-1)]
    group[good] = g
    G = len(first)
    rep = good[first[by_first]].astype(np.int32)
    count = np.bincount(g, minlength=G).astype(np.int32)
    zsum = np.zeros(G, dtype=np.int64)
    np.add.at(zsum, g, records['z'][good].astype(np.int64))
    total = np.zeros(G, dtype=np.uint64)
    np.add.at(total, g, records['total'][good].astype(np.uint64))
    visits = np.zeros((G, gi.A), dtype=np.uint64)
    np.add.at(visits, g, records['visits'][good][:, :gi.A].astype(np.uint64))
    return group, rep, count, zsum.astype(np.int32), total, visits


class MergedExamples(_ExampleRows):
    """A DeviceExamples with the copies of every position merged into one training row (DeviceExamples.merged): the source
    records plus, per group, its first member `rep`, its size `count` and the integer sums `zsum`, `total`, `visits` -- tensors
    on the records' device, trimmed to the number of groups --, and `group` [records], the group of every record (-1: malformed).
    A row's planes are those of its first member, its policy visits / total over the whole group (a copy searched longer weighs
    more), its value the mean outcome; a group of one is exactly DeviceExamples.batch's row.  `batch` is DeviceExamples.batch
    over groups (bb_examples_merged_to_batch).  Made with one look at the device (the group count); sums are integers, so the
    same records give the same bits every time.  Records on the CPU are merged by merge_records_host (batch needs the GPU)."""

    def __init__(self, examples):
        _merge_scope(examples.game)
        self.game, self.info, self.records = examples.game, examples.info, examples.records
        dev, n, A = self.records.device, len(examples), examples.info.A
        self._bad = torch.zeros(1, dtype=torch.int32, device=dev)
        if dev.type != 'cuda':
            raw = self.records.numpy().reshape(-1).view(_lib.example_dtype(self.game))
            group, rep, count, zsum, total, visits = merge_records_host(self.game, raw)
            self._merge_bad = int((group < 0).sum())
            parts = [torch.from_numpy(group), torch.from_numpy(rep), torch.from_numpy(count), torch.from_numpy(zsum),
                     torch.from_numpy(total.astype(np.int64)), torch.from_numpy(visits.astype(np.int64))]
        else:
            i32 = dict(dtype=torch.int32, device=dev)
            parts = [torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, **i32),
                     torch.empty(n, dtype=torch.int64, device=dev), torch.empty((n, A), dtype=torch.int64, device=dev)]
            look = torch.zeros(2, **i32)      # [n_groups, malformed records]
            if n:
                nbytes = _lib.examples_merge_workspace(self.game, n)
                work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                with torch.cuda.device(dev):
                    _lib.examples_merge(self.game, n, self.records.data_ptr(), *[t.data_ptr() for t in parts],
                                        n_groups=look.data_ptr(), bad=look.data_ptr() + 4, workspace=work.data_ptr(),
                                        workspace_bytes=nbytes, stream=torch.cuda.current_stream(dev).cuda_stream)
            n_groups, self._merge_bad = (int(x) for x in look.cpu())   # the one host look (waits for the launches above)
            _lib_check_merge(n_groups)
            parts = [parts[0]] + [t[:n_groups] for t in parts[1:]]
        self.group, self.rep, self.count, self.zsum, self.total, self.visits = parts

    def __len__(self):
        return int(self.rep.shape[0])

    def counts(self):
        """The number of records in every group (int32 tensor on the records' device)."""
        return self.count

    def _to_batch(self, n, idx, sym, boards, policy, value, stream):
        _lib.examples_merged_to_batch(self.game, int(self.records.shape[0]), self.records.data_ptr(), len(self), self.rep.data_ptr(),
                                      self.count.data_ptr(), self.zsum.data_ptr(), self.total.data_ptr(), self.visits.data_ptr(), n, idx,
                                      sym, boards, policy, value, self._bad.data_ptr(), stream)

    def score_with(self, engine, index=None, rows=False, chunk_rows=4096):
        """Merged rows carry sums of their own and are not a records source: ValueError, as HipTrainer.evaluate_records answers."""
        _records_source(self, None, None, 'score_with', 'engine')

    def bad(self):
        """Malformed records that the merge left out, plus rows that `batch` rejected (and wrote as zeros) since.  Waits for
        the GPU -- look at it once per epoch, not once per batch."""
        return self._merge_bad + int(self._bad.item())


def _lib_check_merge(n_groups):
    """bb_examples_merge reports a probe that ran out through its group count: an error code where a count belongs."""
    if n_groups < 0:
        raise _lib.BlackbirdHipError('libblackbird_hip error %d: bb_examples_merge found no place for a record in its position '
                                     'table' % n_groups)
