"""Support shared by test modules (not collected): Blackbird.Model factories and the fixture that records what the front end passes to _lib.Engine."""
import numpy as np
import pytest

from blackbird_amd import Blackbird, _lib


def net_config(blocks, eps):
    return {"blocks": blocks, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
            "policy": {"dirichlet": {"alpha": 0.2, "epsilon": eps}}, "training": {"optimizer": "adam"}}


def model(game, name, *, seed, play_limit, eps, blocks):
    """seed: numpy's, set before the weights are drawn (weight initialisation draws from numpy's stream); None: left alone."""
    if seed is not None:
        np.random.seed(seed)
    return Blackbird.Model(game, name, {"explorationRate": 0.85, "playLimit": play_limit}, net_config(blocks, eps))


class Recorded(Exception):
    pass


@pytest.fixture
def engine_args(monkeypatch):
    """The arguments of the next _lib.Engine(...) call (nothing is created: no GPU here); the call raises Recorded."""
    seen = {}

    def fake(game, **kw):
        seen.update(kw, game=game)
        raise Recorded()

    monkeypatch.setattr(_lib, "Engine", fake)
    return seen
