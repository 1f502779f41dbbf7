"""Mirror of /root/reference/src/Network.py:9-112.  getEvaluation/getPolicy run the fused HIP
tower (bb_net_eval) on the int8 planes AsInputArray returns; weights live in an .npz with the
reference's TensorFlow variable names instead of a TF checkpoint.  train() is the step right after
the hot path: PyTorch-ROCm optimiser over the same parameters (or, with
NetworkConfig['training']['backend'] = 'hip', the HIP training kernels -- Connect4 and TicTacToe; DragonChess too with
NetworkConfig['training']['hip_games'] = 'all'), then the new weights are
pushed back into the engine."""
import os

import numpy as np

from . import _lib
from . import weights as W
from .MCTS import _seed_from_numpy

_GAME_BY_SHAPE = {(6, 7, 3): _lib.GAME_CONNECT4, (3, 3, 3): _lib.GAME_TICTACTOE, (8, 8, 17): _lib.GAME_DRAGONCHESS}


class Network:
    HANDOFF_LIMITS = '16 filters (the fused tower; Connect4, TicTacToe, DragonChess)'

    def __init__(self, name, networkConstructor=None, tensorflowConfig={}):
        self.batchCount = 0
        self._handoff = 'host'            # NetworkConfig['training']['handoff'], read when the trainer is made
        self._weights_stale = False       # 'device' hand-off: the trainer's device parameters are ahead of the host copy
        self._netName = name
        self._constructor = networkConstructor
        self._weights = None
        self._eval_engine = None
        self._trainer = None
        alpha = getattr(networkConstructor, 'alpha', None)
        epsilon = getattr(networkConstructor, 'epsilon', None)
        self.alpha = 0.2 if alpha is None else alpha          # (an explicit epsilon of 0 switches the noise off)
        self.epsilon = 0.3 if epsilon is None else epsilon
        if not self.loadModel(name):
            if networkConstructor is not None and getattr(networkConstructor, 'inputShape', None):
                self._weights = networkConstructor()
                self.saveModel(name)

    # ---- weights -------------------------------------------------------------------------------------
    @property
    def _weights(self):
        """The host copy of the weights (TF-named dict).  With the 'device' hand-off training leaves it stale; whoever reads it
        -- saveModel, _ensure_weights, a new engine's first load -- gets the trainer's current values, exported once."""
        if self._weights_stale and getattr(self, '_trainer', None) is not None:
            self._weights_host = self._trainer.export()
        self._weights_stale = False
        return self._weights_host

    @_weights.setter
    def _weights(self, value):
        self._weights_host, self._weights_stale = value, False

    def _ensure_weights(self, in_planes):
        if self._weights is None:
            if self._constructor is None:
                raise _lib.BlackbirdHipError('no saved model %r and no NetworkFactory to build one' % self._netName)
            self._weights = self._constructor(in_planes)
            self.saveModel(self._netName)
        return self._weights

    def _engine_for(self, shape):
        game = _GAME_BY_SHAPE.get(tuple(int(x) for x in shape))
        if game is None:
            raise ValueError('no game with input planes of shape %r' % (shape,))
        if self._eval_engine is None or self._eval_engine.game != game:
            self._eval_engine = _lib.Engine(game, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET,
                                            alpha=float(self.alpha), epsilon=float(self.epsilon),
                                            seed=_seed_from_numpy())
            self._eval_engine.load_weights(W.flatten(self._ensure_weights(shape[2])))
        return self._eval_engine

    def _engine_loader(self):
        """What hands the current weights to an engine that has had its first load: the trainer's load_into while its device
        parameters are ahead of the host copy ('device' hand-off), else load_weights of the host copy, flattened once."""
        if self._weights_stale and self._trainer is not None:
            return self._trainer.load_into
        flat = W.flatten(self._weights)
        return lambda eng: eng.load_weights(flat)

    def _weights_changed(self):
        if self._eval_engine is not None:
            self._engine_loader()(self._eval_engine)

    def _trained(self):
        """After optimiser steps: 'host' exports the trainer's parameters and reloads every engine through the host; 'device'
        marks the host copy stale and hands the parameters to the engines on the device."""
        if self._handoff == 'device':
            self._weights_stale = True
        else:
            self._weights = self._trainer.export()
        self._weights_changed()

    # ---- reference API ---------------------------------------------------------------------------------
    def getEvaluation(self, state):
        """Network.py:48-54: value of `state` (int8 [n,H,W,C]) for the side to move; returns element 0."""
        state = np.asarray(state)
        v, _l, _p = self._engine_for(state.shape[1:]).net_eval(planes=state.astype(np.int8))
        return v[0]

    def getPolicy(self, state):
        """Network.py:56-64: softmax policy mixed with Beta(alpha,1-alpha) noise (always on, as in the
        reference graph, NetworkFactory.py:176-182); returns row 0."""
        state = np.asarray(state)
        eng = self._engine_for(state.shape[1:])
        eng._noise_calls = getattr(eng, '_noise_calls', 0) + 1
        _v, _l, p = eng.net_eval(planes=state.astype(np.int8), noise=eng._noise_calls)  # fresh draw per call
        return p[0]

    def _trainer_for(self, in_planes):
        """The optimiser over this network's weights, created on first use (optimiser kind from NetworkConfig, the graph's
        alpha and epsilon) and kept, with its slots, until other weights are loaded."""
        from . import training
        if self._trainer is None:
            self._ensure_weights(in_planes)     # (a trainer that exists has them; reading them would export a stale copy)
            cfg = (getattr(self._constructor, 'NetworkConfig', None) or {}).get('training') or {}
            backend = cfg.get('backend', 'torch')
            if backend not in ('torch', 'hip'):
                raise ValueError("NetworkConfig['training']['backend'] is 'torch' or 'hip', got %r" % (backend,))
            handoff = cfg.get('handoff', 'host')
            if handoff not in ('host', 'device'):
                raise ValueError("NetworkConfig['training']['handoff'] is 'host' or 'device', got %r" % (handoff,))
            if handoff == 'device' and W.infer_shape(self._weights)[1] != 16:
                raise ValueError("NetworkConfig['training']['handoff'] = 'device' covers %s; this network has %d filters.  Use "
                                 "the 'host' hand-off for it." % (self.HANDOFF_LIMITS, W.infer_shape(self._weights)[1]))
            hip_games = cfg.get('hip_games', 'dense')
            if hip_games not in training.HIP_GAMES:
                raise ValueError("NetworkConfig['training']['hip_games'] is 'dense' or 'all', got %r" % (hip_games,))
            loss, l2 = training.check_loss(cfg.get('loss', 'reference'), cfg.get('l2', 1e-4))   # (ValueError, as for the keys above)
            self._handoff = handoff
            if backend == 'hip' and not training.hip_trainer_supports(self._weights, hip_games):
                raise ValueError("NetworkConfig['training']['backend'] = 'hip' covers %s; this network has shape "
                                 "(planes, filters, blocks, dense, actions) = %r.  Use the 'torch' backend for it."
                                 % (training.HIP_TRAINER_LIMITS if hip_games == 'dense' else training.HIP_TRAINER_LIMITS_ALL,
                                    W.infer_shape(self._weights)))
            make = training.HipTrainer if backend == 'hip' else training.Trainer
            self._trainer = make(self._weights, alpha=self.alpha, epsilon=self.epsilon,
                                 optimizer=cfg.get('optimizer', 'adam'), momentum=cfg.get('momentum', 0.9), loss=loss, l2=l2)
        return self._trainer

    def train(self, state, eval, policy, learningRate=0.01, teacher=None):
        """Network.py:66-84 (see blackbird_amd/training.py for the loss)."""
        if teacher is not None:
            # the reference's teacher branch (NetworkFactory.py:205-218) calls the removed tf.log and cannot run; refusing
            # is better than silently training without the term
            raise NotImplementedError('policy distillation from a teacher (hasTeacher) is not supported')
        state = np.asarray(state)
        self._trainer_for(state.shape[-1]).step(state, eval, policy, learningRate)
        self._trained()
        self.batchCount += 1

    def saveModel(self, name=None):
        """Network.py:86-98"""
        if name is None:
            name = self.Name
        saveDir = os.path.join('blackbird_models', name)
        os.makedirs(saveDir, exist_ok=True)
        W.save_npz(os.path.join(saveDir, 'best.npz'), self._weights)

    def loadModel(self, name):
        """Network.py:100-112"""
        path = os.path.join('blackbird_models', name, 'best.npz')
        if not os.path.isfile(path):
            return False
        self._weights = W.load_npz(path)
        self._trainer = None  # parameters and optimiser state of the old weights do not carry over
        self._weights_changed()
        return True
