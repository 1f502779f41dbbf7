"""-m gpu: a trainer's weights handed to an engine on the device (bb_load_weights_device, bb_trainer_load_engine,
csrc/net_pack.hip.h; HipTrainer.load_into, Trainer.load_into, NetworkConfig['training']['handoff'] = 'device').

The yardstick is the host route -- export(), weights.flatten, Engine.load_weights, whose images tests/test_net_pack_cpu.py holds
to golden digests -- and the comparison is exact: every operand buffer of the engine (Engine.weights_image) must hold the same
BYTES, and the network must then give the same bits.  The engine under test is first loaded with OTHER weights of the same
shape, so an image the kernels did not write shows.  Shapes are the smallest at which a loop bound or a padding rule bites: no
tower block (empty tower images), one, two, nine (the HIP trainer's limit) and ten (the PyTorch trainer's route); dense widths 1,
3 and 64 (the head's padding to four floats); TicTacToe (9 actions), Connect4 (7), DragonChess (17 input planes: the wide first
convolution; 4032 actions); both net forms.  The weights carry +0, -0, 1e-30, 3e38 and a value whose second bf16 residue rounds up,
in convolution kernels and in head kernels."""
import numpy as np
import pytest
import torch

from blackbird_amd import Blackbird, Connect4, _lib
from blackbird_amd import weights as W
from blackbird_amd.training import DeviceExamples, HipTrainer, Trainer
from tests import merge_cases as MC
from tests import model_cases as M
from tests import selfplay_cases as SP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C4, TTT, DC = _lib.GAME_CONNECT4, _lib.GAME_TICTACTOE, _lib.GAME_DRAGONCHESS
AUTO, F32 = _lib.NET_FORM_AUTO, _lib.NET_FORM_F32
ROUNDS_UP = np.array([0x3F8040E0], dtype=np.uint32).view(np.float32)[0]   # 1 + 0x40E0 ulp: see test_the_planted_value
PLANTED = np.array([0.0, -0.0, 1e-30, 3e38, ROUNDS_UP], dtype=np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bf16(x):
    u = _bits(x).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32) << 16).view(np.float32)


def test_the_planted_value():
    """its second bf16 residue lies above the half-way point, so the second plane rounds UP and the third is negative"""
    v = np.array([ROUNDS_UP], dtype=np.float32)
    r1 = v - _bf16(v)
    r2 = r1 - _bf16(r1)
    assert (_bits(r1) & 0xFFFF)[0] > 0x8000 and _bf16(r1)[0] > r1[0] and r2[0] < 0


def _engine(game, net_form=AUTO, **kw):
    gi = _lib.game_info(game)
    kw.setdefault("max_plies", 4 if game == DC else None)
    return _lib.Engine(game, n_slots=1, sims_per_move=2, evaluator=_lib.EVAL_NET, net_form=net_form, **kw), gi


def _weights(game, R, D, seed, plant):
    gi = _lib.game_info(game)
    w = W.init_weights(gi.C, 16, R, D, gi.A, seed=seed, perturb=True)
    if plant:
        names = ["resTower/conv_block/conv/kernel", "value/convolution/kernel", "policy/convolution/kernel", "policy/policy/kernel",
                 "value/dense_1/kernel"] + (["resTower/block_0/conv_2/kernel"] if R else [])
        for k, name in enumerate(names):
            flat = w[name].reshape(-1)                       # (a view: the arrays are contiguous)
            at = (7 * k + np.arange(len(PLANTED)) * 3) % flat.size
            flat[at[:min(len(PLANTED), flat.size)]] = PLANTED[:min(len(PLANTED), flat.size)]
    return w


def _images(eng):
    return {k: eng.weights_image(k) for k in _lib.WEIGHTS_IMAGES}


def _same_images(a, b, what=""):
    for k in _lib.WEIGHTS_IMAGES:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else -1)


def _planes(gi, n, seed):
    return (np.random.RandomState(seed).randint(0, 3, size=(n, gi.H, gi.W, gi.C)) == 1).astype(np.int8)


def _same_eval(a, b, gi, what=""):
    planes = _planes(gi, 5, 4)
    for x, y, name in zip(a.net_eval(planes=planes), b.net_eval(planes=planes), ("value", "logits", "policy")):
        assert np.array_equal(_bits(x), _bits(y)), (what, name)


def _make_trainer(kind, w):
    if kind == "hip":
        return HipTrainer(w, device=DEV, seed=3, max_batch=2)
    return Trainer(w, device=DEV)


# ---- 1, 2. the images byte for byte, the evaluations bit for bit -----------------------------------------------------------------
CASES = [(g, "hip", R, D, f) for g in (C4, TTT) for f in (AUTO, F32) for R, D in ((0, 1), (1, 3), (2, 64), (9, 3))]
CASES += [(DC, "torch", R, D, f) for f in (AUTO, F32) for R, D in ((0, 3), (2, 64))]
CASES += [(C4, "torch", 10, 1, AUTO), (TTT, "torch", 1, 64, F32)]


@pytest.mark.parametrize("game,kind,R,D,net_form", CASES)
def test_images_are_the_host_routes(game, kind, R, D, net_form):
    w = _weights(game, R, D, 11, plant=True)
    other = _weights(game, R, D, 12, plant=False)
    tr = _make_trainer(kind, w)
    a, gi = _engine(game, net_form)
    b, _ = _engine(game, net_form)
    try:
        a.load_weights(W.flatten(tr.export()))               # the host route
        b.load_weights(W.flatten(other))                      # ... and B holds something else first
        want = _images(a)
        assert (want["x3"].size == 0) == (net_form == F32)
        before = _images(b)
        assert all(R == 0 and k == "wt" or not np.array_equal(before[k], want[k]) for k in ("w0", "wt", "epi", "head"))
        tr.load_into(b)
        _same_images(_images(b), want, (game, kind, R, D, net_form))
        _same_eval(a, b, gi)
        for k, v in tr.export().items():                      # the hand-off reads the parameters and leaves them alone
            assert np.array_equal(_bits(v), _bits(w[k])), k
    finally:
        a.close()
        b.close()
        if kind == "hip":
            tr.close()


# ---- 3. ordered behind the steps queued on the caller's stream -------------------------------------------------------------------
def test_handoff_waits_for_the_steps_queued_before_it():
    B = 256
    w = _weights(C4, 2, 16, 21, plant=False)
    tr = HipTrainer(w, device=DEV, seed=5, max_batch=B)
    a, gi = _engine(C4)
    b, _ = _engine(C4)
    rng = np.random.RandomState(2)
    boards = torch.from_numpy(_planes(gi, B, 6).astype(np.float32)).to(DEV)
    value = torch.from_numpy(rng.choice([-1.0, 0.0, 1.0], size=B).astype(np.float32)).to(DEV)
    policy = torch.from_numpy(rng.dirichlet(np.ones(gi.A), size=B).astype(np.float32)).to(DEV)
    try:
        b.load_weights(W.flatten(w))
        torch.cuda.synchronize()
        for _ in range(3):
            tr.step_tensors(boards, value, policy, 1e-2)
        tr.load_into(b)                                       # nothing waited for in between
        after = tr.export()                                   # (waits) -- the host route after the same three steps
        assert any(not np.array_equal(after[k], w[k]) for k in w)
        a.load_weights(W.flatten(after))
        _same_images(_images(b), _images(a), "after three steps")
        tr.step_tensors(boards, value, policy, 1e-2)          # a later step waits for the packing: B keeps the three-step images
        torch.cuda.synchronize()
        _same_images(_images(b), _images(a), "after a fourth step")
    finally:
        a.close()
        b.close()
        tr.close()


# ---- 4. the evaluation cache is cleared --------------------------------------------------------------------------------------------
def test_no_evaluation_outlives_the_weights(monkeypatch):
    wa, wb = W.init_weights(3, 16, 4, 16, 7, seed=0), W.init_weights(3, 16, 4, 16, 7, seed=1)
    tr = HipTrainer(wb, device=DEV, seed=5, max_batch=2)
    eng = SP.c4_engine_under_cache(monkeypatch, True, 8, 16, 8, log2=16)
    try:
        first = SP.play_loaded(eng, W.flatten(wa), 8, 8, mode=None)
        assert first["cnt"]["eval_cache_probes"] > 0          # this engine plays with the cache
        tr.load_into(eng)
        after = SP.play_loaded(eng, None, 8, 8, mode=None)
    finally:
        eng.close()
    fresh = SP.c4_engine_under_cache(monkeypatch, True, 8, 16, 8, log2=16)
    try:
        ref = SP.play_loaded(fresh, W.flatten(tr.export()), 8, 8, mode=None)
    finally:
        fresh.close()
        tr.close()
    SP.assert_same_records(after, ref, "after a hand-off")


# ---- 5. reuse and lifetime -----------------------------------------------------------------------------------------------------------
def test_two_handoffs_and_a_closed_trainer():
    w1, w2 = _weights(TTT, 1, 3, 31, plant=True), _weights(TTT, 1, 3, 32, plant=False)
    t1, t2 = HipTrainer(w1, device=DEV, seed=1, max_batch=2), HipTrainer(w2, device=DEV, seed=1, max_batch=2)
    a, gi = _engine(TTT)
    b, _ = _engine(TTT)
    try:
        b.load_weights(W.flatten(_weights(TTT, 1, 3, 33, plant=False)))
        for tr, w in ((t1, w1), (t2, w2), (t1, w1)):
            tr.load_into(b)
            a.load_weights(W.flatten(w))
            _same_images(_images(b), _images(a))
        t1.close()                                            # the engine keeps its own images
        t2.close()
        _same_images(_images(b), _images(a), "trainers closed")
        _same_eval(a, b, gi, "trainers closed")
        tt = Trainer(w2, device=DEV)                          # the torch route: its flat tensor is gone when load_into returns
        tt.load_into(b)
        del tt
        torch.cuda.empty_cache()
        a.load_weights(W.flatten(w2))
        _same_images(_images(b), _images(a), "torch route")
    finally:
        a.close()
        b.close()


# ---- 6. the front end ------------------------------------------------------------------------------------------------------------------
def _model(name, handoff, backend="hip"):
    cfg = M.net_config(1, 0.3)
    cfg["training"]["backend"] = backend
    if handoff is not None:
        cfg["training"]["handoff"] = handoff
    return Blackbird.Model(Connect4.BoardState, name, {"explorationRate": 0.85, "playLimit": 8}, cfg)


def _train_batch(gi, B=6):
    rng = np.random.RandomState(8)
    return (_planes(gi, B, 9), rng.choice([-1.0, 0.0, 1.0], size=B).astype(np.float32), rng.dirichlet(np.ones(gi.A), size=B))


@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_network_train_hands_over_on_the_device(tmp_path, monkeypatch, backend):
    monkeypatch.chdir(tmp_path)
    np.random.seed(3)
    gi = _lib.game_info(C4)
    net = _model("dev_" + backend, "device", backend)
    planes = _planes(gi, 3, 1)
    net.getEvaluation(planes[:1])                             # the evaluation engine exists and has had its first load
    w0 = {k: v.copy() for k, v in net._weights.items()}
    exports = []
    real = type(net._trainer_for(gi.C)).export
    monkeypatch.setattr(type(net._trainer), "export", lambda self: exports.append(1) or real(self))
    for _ in range(2):
        net.train(*_train_batch(gi), 1e-2)
    assert not exports and net._weights_stale and net.batchCount == 2      # two steps, two hand-offs, no export
    _v, logits, _p = net._eval_engine.net_eval(planes=planes)
    trained = net._weights                                    # (the one export)
    assert len(exports) == 1 and not net._weights_stale
    assert any(not np.array_equal(trained[k], w0[k]) for k in w0)
    ref, _ = _engine(C4)
    try:
        ref.load_weights(W.flatten(trained))
        assert np.array_equal(_bits(logits), _bits(ref.net_eval(planes=planes)[1]))
        _same_images(_images(net._eval_engine), _images(ref))
    finally:
        ref.close()
    net.train(*_train_batch(gi), 1e-2)
    net.saveModel("kept")                                     # reads the stale copy: saves what the trainer holds
    want = net._trainer.export()
    back = _model("other", None)
    assert back.loadModel("kept")
    assert sorted(back._weights) == sorted(want) and all(np.array_equal(_bits(back._weights[k]), _bits(want[k])) for k in want)
    for m in (net, back):
        m.Conn.Close()


def test_train_with_device_examples_ends_with_the_host_settings_weights(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rec = MC.playout_records(C4, 40, 21)
    w0 = W.init_weights(3, 16, 1, 16, 7, seed=4, perturb=True)
    got = {}
    for handoff in ("host", "device"):
        m = _model("twde_" + handoff, handoff)
        m._weights = {k: v.copy() for k, v in w0.items()}
        m.getEvaluation(_planes(_lib.game_info(C4), 1, 1))    # an engine to reload
        np.random.seed(5)
        Blackbird.TrainWithDeviceExamples(m, 8, 1e-2, examples=DeviceExamples.from_records(C4, rec, DEV))
        assert m._weights_stale == (handoff == "device") and m.batchCount == 5
        imgs = _images(m._eval_engine)
        got[handoff] = ({k: v.copy() for k, v in m._weights.items()}, imgs)
        m.Conn.Close()
    for k in w0:
        assert np.array_equal(_bits(got["host"][0][k]), _bits(got["device"][0][k])), k
    assert any(not np.array_equal(got["host"][0][k], w0[k]) for k in w0)
    _same_images(got["host"][1], got["device"][1], "the engines of both settings")


# ---- 7. refusals: the documented error, and the engine's images untouched ---------------------------------------------------------------
def test_refusals_leave_the_engine_alone():
    w = _weights(C4, 1, 3, 41, plant=False)
    tr = HipTrainer(w, device=DEV, seed=1, max_batch=2)
    held = W.flatten(_weights(C4, 1, 3, 42, plant=False))
    try:
        bare, _ = _engine(C4)                                 # never had load_weights: no buffers
        with pytest.raises(AssertionError, match="no weight buffers"):
            tr.load_into(bare)
        with pytest.raises(_lib.BlackbirdHipError):
            bare.weights_image("w0")
        bare.close()
        for what, eng, flat, err in (
                ("blocks", _engine(C4)[0], W.flatten(_weights(C4, 2, 3, 42, plant=False)), AssertionError),
                ("dense", _engine(C4)[0], W.flatten(_weights(C4, 1, 4, 42, plant=False)), AssertionError),
                ("general_net", _engine(C4, general_net=True)[0], held, AssertionError),
                ("game", _engine(TTT)[0], W.flatten(_weights(TTT, 1, 3, 42, plant=False)), ValueError)):
            try:
                eng.load_weights(flat)
                before = _images(eng)
                with pytest.raises(err):
                    tr.load_into(eng)
                _same_images(_images(eng), before, what)
            finally:
                eng.close()
        form, _ = _engine(C4, F32)                            # a descriptor with a null block
        try:
            form.load_weights(held)
            before = _images(form)
            tt = Trainer(w, device=DEV)
            flat, offsets = tt._flat_device()
            desc = _lib.net_weights_device(6, 7, 3, 16, 1, 3, 7, flat.data_ptr(), offsets)
            desc.blk_k = None
            with pytest.raises(ValueError, match="missing"):
                form.load_weights_device(desc, 0)
            _same_images(_images(form), before, "null block")
        finally:
            form.close()
    finally:
        tr.close()
