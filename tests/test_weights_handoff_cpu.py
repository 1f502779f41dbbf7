"""Without a GPU: the argument checks of the device hand-off's entry points (bb_load_weights_device, bb_trainer_load_engine,
bb_weights_read) come before any device call, and NetworkConfig['training']['handoff'] is read and refused as documented."""
import ctypes as C

import numpy as np
import pytest

from blackbird_amd import Network as N
from blackbird_amd import _lib, training
from blackbird_amd import weights as W


def test_null_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    w = _lib.NetWeights()
    something = C.c_void_p(16)          # never dereferenced: the other argument is null
    n = C.c_int64(-1)
    buf = np.zeros(8, dtype=np.uint8)
    for rc in (L.bb_load_weights_device(None, C.byref(w), None), L.bb_load_weights_device(something, None, None),
               L.bb_trainer_load_engine(None, something, None), L.bb_trainer_load_engine(something, None, None),
               L.bb_weights_read(None, 0, _lib.ptr(buf), 8, C.byref(n))):
        assert rc == _lib.ERR_ARG and _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(L.bb_load_weights_device(None, None, None))
    assert n.value == -1 and not buf.any()


class _Factory:
    """what Network asks of a NetworkFactory here: the configuration, and no input shape (no weights are drawn, none saved)"""

    def __init__(self, training_cfg):
        self.NetworkConfig = {"training": training_cfg} if training_cfg is not None else {}


def _network(tmp_path, monkeypatch, training_cfg, filters=16):
    monkeypatch.chdir(tmp_path)
    net = N.Network("handoff_cpu", _Factory(training_cfg))
    assert net._weights is None
    net._weights = W.init_weights(3, filters, 1, 16, 7, seed=1)
    return net


@pytest.mark.parametrize("value", ["gpu", "Device", "", None, 1])
def test_other_handoff_values_raise(tmp_path, monkeypatch, value):
    net = _network(tmp_path, monkeypatch, {"handoff": value})
    with pytest.raises(ValueError, match="'host' or 'device'"):
        net._trainer_for(3)
    assert net._trainer is None and net._handoff == "host"


def test_device_handoff_names_its_limit(tmp_path, monkeypatch):
    net = _network(tmp_path, monkeypatch, {"handoff": "device"}, filters=32)
    with pytest.raises(ValueError, match="16 filters"):
        net._trainer_for(3)
    assert net._trainer is None and net._handoff == "host"
    ok = _network(tmp_path, monkeypatch, {"handoff": "device"})          # 16 filters: taken, and nothing is handed over yet
    assert isinstance(ok._trainer_for(3), training.Trainer) and ok._handoff == "device" and not ok._weights_stale


@pytest.mark.parametrize("cfg", [None, {}, {"optimizer": "adam"}, {"handoff": "host"}])
def test_the_defaults_are_what_they_were(tmp_path, monkeypatch, cfg):
    net = _network(tmp_path, monkeypatch, cfg)
    tr = net._trainer_for(3)
    assert type(tr) is training.Trainer and net._handoff == "host" and not net._weights_stale
    w = net._weights
    assert w is net._weights and sorted(w) == sorted(W.init_weights(3, 16, 1, 16, 7, seed=1))


def test_a_stale_host_copy_is_exported_once_when_read(tmp_path, monkeypatch):
    net = _network(tmp_path, monkeypatch, {"handoff": "device"})
    tr = net._trainer_for(3)
    calls = []
    fresh = {k: v + 1 for k, v in tr.export().items()}
    monkeypatch.setattr(tr, "export", lambda: calls.append(1) or fresh)
    net._weights_stale = True           # what training leaves behind under the 'device' hand-off
    assert net._weights is fresh and net._weights is fresh and calls == [1] and not net._weights_stale
    net._weights = {"x": 1}             # other weights loaded: nothing stale any more
    assert net._weights == {"x": 1} and calls == [1]
