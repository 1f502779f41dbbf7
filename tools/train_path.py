"""From finished self-play games to a trained network, both ways, timed: python tools/train_path.py [--games N]
[--play-limit P] [--batch B] [--lr LR] [--augment] [--merge] [--holdout FRACTION] [--skip-host] [--skip-device] [--skip-hip]
[--handoff host|device] [--game connect4|dragonchess] [--warmup-games W] [--score-engine] [--loss reference|per_example]
[--temp-schedule PLIES,TEMP]

--game dragonchess: the same on DragonChess (17 planes, 4032 actions), the hip model with NetworkConfig['training']['hip_games'] =
'all'.  The records source and the scorer do not cover that game, so hip_epoch_s is null and --holdout and --merge are refused;
--warmup-games (default 64) bounds the untimed warm-up runs, whose games are long there.

N Connect4 games at PlayLimit P are played once (Model.KeepDeviceExamples on, so that sqlite and the GPU hold the same
examples); then one epoch over them is trained twice with the same batch size:

  host path    what Blackbird.TrainWithExamples does: Conn.GetGames + ExampleState.FromSerialized per example (decode),
               then np.vstack per batch + Model.train, which exports the weights and reloads the engines after every batch
  device path  Blackbird.TrainWithDeviceExamples on the kept records: bb_examples_to_batch + Trainer.step_tensors per
               batch, one export and one reload at the end
  hip path     the same epoch through TrainWithDeviceExamples with NetworkConfig['training']['backend'] = 'hip' (the
               training step as HIP kernels), on a second model built from the same saved weights, both ways: the per-batch
               loop (fused=False: bb_examples_to_batch + bb_trainer_step per batch; hip_path_s) and then the epoch call
               (bb_trainer_epoch: the step's kernels read the records themselves, one call enqueues the epoch; hip_epoch_s)

and the bare DeviceExamples.batch calls of that epoch alone.  Every timed region ends in a device synchronise; one training
step is run before any of them, per trainer (the first step pays for the library's kernel selection).  --augment: the
device and hip paths and the bare batches present every example mirrored or not (TrainWithDeviceExamples' augment=True,
bb_examples_to_batch_sym); the host path has no such thing and stays as it is.  --merge: the copies of a position among the
kept records are merged first (DeviceExamples.merged, bb_examples_merge): the records, the groups, the five largest groups and
the time of merged() (its kernels and its one host look, after one untimed call on 256 records that loads the kernels) are
printed, and one more epoch is timed on the first model through TrainWithDeviceExamples(merge=True), next to the bare merged
batches of that epoch; every other figure is measured as without it.  --skip-host / --skip-hip leave the host path / the hip
path out (their figures are null).

--handoff host|device: NetworkConfig['training']['handoff'] of the hip model (default host: export and reload through the host).
Either way the hip model is given the engines a playing, training model owns -- its evaluation engine and, after a warm-up run
of 64 games, its self-play engine -- and two more legs are timed on it: train_loop_s, the reference API's shape, Model.train
once per batch of the epoch on host arrays staged beforehand (a step, then every engine reloaded: where the hand-off matters),
and handoff_s against export_load_s, the median of five calls of one HipTrainer.load_into of the evaluation engine against one
export() + flatten + load_weights of it (handoff_s is null on a build without load_into).  --skip-device leaves the PyTorch
trainer's device path out.

--holdout FRACTION: a held-out score of one epoch.  The run's records are split by whole games (DeviceExamples.split_games, seed
--seed); a third model with the hip backend, given the first model's initial weights, scores both parts (Blackbird.EvaluateDeviceExamples:
HipTrainer.evaluate_records, bb_trainer_eval), trains one epoch on the training part alone (TrainWithDeviceExamples with --augment
and --merge as given) and scores both parts again: value_mse, policy_ce, top1_rate and sign_rate of each are printed under
"holdout".  Two times are taken on the held-out part, each the median of five calls after an untimed one: evaluate_records, and
the route to the same figures without it -- trainer.export(), a fresh engine with those weights, examples._batch to the host,
Engine.net_eval, numpy.  Every other figure is measured as without it, on all records.

--score-engine (with --holdout): the held-out part is also scored by the model's evaluation engine
(Blackbird.EvaluateDeviceExamples(scorer='engine'): DeviceExamples.score_with, bb_examples_score -- the network in the arithmetic
self-play uses), timed the same way next to the other routes (score_engine_s; score_with_s is the score_with call alone), with
its figures and their distance from evaluate_records'.  With --game dragonchess --holdout is accepted together with
--score-engine only: a model with the PyTorch trainer scores the held-out part both ways -- Trainer.evaluate_tensors over
examples._batch chunks (torch_route_s), which was the only route for that game, and scorer='engine' -- and nothing is trained.

--loss reference|per_example (default reference): NetworkConfig['training']['loss'] of every model of the run -- the PyTorch
trainer, the hip model and the --holdout model alike; per_example is the ordinary AlphaZero loss (each row's own label, l2 1e-4,
no noise).  Every figure is measured as without it.

--temp-schedule PLIES,TEMP: every self-play run of the tool (the warm-up runs too) plays the first PLIES plies of a game at
temperature 1 and the rest at TEMP (Model.SelfPlayTempSchedule; 0: the PUCT arg-max move).  Without it every move is
drawn at temperature 1, as before.  Connect4 runs also print duplicate_share: the share of the kept records that are a further
copy of a position already among them (1 - groups / records of DeviceExamples.merged), counted after everything that is timed.
Prints one JSON line."""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from blackbird_amd import Blackbird, Connect4, DragonChess, _lib  # noqa: E402
from blackbird_amd import weights as W  # noqa: E402
from blackbird_amd.training import epoch_order, eval_summary  # noqa: E402

CFG = {"blocks": 4, "filters": 16, "eval": {"dense": 16}, "hasTeacher": False,
       "policy": {"dirichlet": {"alpha": 0.2, "epsilon": 0.3}}, "training": {"optimizer": "adam"}}


MEANS = ("value_mse", "policy_ce", "top1_rate", "sign_rate")


def host_route(trainer, examples):
    """The held-out figures without bb_trainer_eval: the weights exported, a fresh engine loaded with them, the rows brought to
    the host, one Engine.net_eval, and the definitions of HipTrainer.evaluate_records in numpy."""
    eng = _lib.Engine(examples.game, n_slots=16, sims_per_move=2, evaluator=_lib.EVAL_NET)
    try:
        eng.load_weights(W.flatten(trainer.export()))
        boards, z, pi = (t.cpu().numpy() for t in examples._batch(None))
        value, logits, _policy = eng.net_eval(planes=boards.astype(np.int8))
    finally:
        eng.close()
    has = (pi != 0).any(axis=1)
    shifted = logits.astype(np.float64) - logits.max(axis=1, keepdims=True)
    logp = shifted - np.log(np.exp(shifted).sum(axis=1, keepdims=True))
    ce = np.where(has, -(pi * logp).sum(axis=1), 0.0)
    top1 = has & (logits.argmax(axis=1) == pi.argmax(axis=1))
    decided = z != 0
    return eval_summary(len(z), has.sum(), top1.sum(), decided.sum(), (decided & (value * z > 0)).sum(),
                        ((value.astype(np.float64) - z) ** 2).sum(), ce.sum())


def median_time(fn, reps=5):
    fn()                                   # untimed: kernels loaded, allocations made
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t = time.time()
        fn()
        torch.cuda.synchronize()
        times.append(time.time() - t)
    return float(np.median(times))


def holdout_run(a, kept, cfg, weights):
    """--holdout: see the module's docstring"""
    train, held = kept.split_games(a.holdout, a.seed)
    m = Blackbird.Model(Connect4.BoardState, "train_path", {"explorationRate": 0.85, "playLimit": a.play_limit}, cfg)
    m._weights, m._trainer = {k: v.copy() for k, v in weights.items()}, None
    means = lambda d: {k: round(d[k], 5) for k in MEANS}  # noqa: E731
    score = lambda: {"train": means(Blackbird.EvaluateDeviceExamples(m, examples=train)),  # noqa: E731
                     "held": means(Blackbird.EvaluateDeviceExamples(m, examples=held))}
    before = score()
    np.random.seed(a.seed + 1)
    Blackbird.TrainWithDeviceExamples(m, a.batch, a.lr, examples=train, augment=a.augment, merge=a.merge)
    after = score()
    mine, theirs = m._trainer.evaluate_records(held), host_route(m._trainer, held)
    eval_s = median_time(lambda: m._trainer.evaluate_records(held))
    host_s = median_time(lambda: host_route(m._trainer, held))
    out = {"fraction": a.holdout, "train_records": len(train), "held_records": len(held), "merge": bool(a.merge),
           "before": before, "after": after, "evaluate_records_s": round(eval_s, 5), "host_route_s": round(host_s, 5),
           "host_route_agrees": {k: round(abs(mine[k] - theirs[k]), 7) for k in MEANS}}
    if a.score_engine:
        out.update(engine_scores(m, held, mine))
    return out


def engine_scores(m, held, other):
    """--score-engine: the held-out part scored by the model's evaluation engine, timed, against the figures `other`"""
    got = Blackbird.EvaluateDeviceExamples(m, examples=held, scorer="engine")
    front_s = median_time(lambda: Blackbird.EvaluateDeviceExamples(m, examples=held, scorer="engine"))
    eng = m._eval_engine
    call_s = median_time(lambda: held.score_with(eng))
    return {"score_engine": {k: round(got[k], 5) for k in MEANS}, "score_engine_s": round(front_s, 5), "score_with_s": round(call_s, 5),
            "score_engine_net_form": eng.net_form(), "score_engine_agrees": {k: round(abs(got[k] - other[k]), 7) for k in MEANS}}


def holdout_run_dc(a, kept, board):
    """--game dragonchess --holdout --score-engine: see the module's docstring"""
    _train, held = kept.split_games(a.holdout, a.seed)
    m = Blackbird.Model(board, "train_path", {"explorationRate": 0.85, "playLimit": a.play_limit}, CFG)
    theirs = Blackbird.EvaluateDeviceExamples(m, examples=held)
    torch_s = median_time(lambda: Blackbird.EvaluateDeviceExamples(m, examples=held))
    return {"fraction": a.holdout, "held_records": len(held), "torch_route": {k: round(theirs[k], 5) for k in MEANS},
            "torch_route_s": round(torch_s, 5), **engine_scores(m, held, theirs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--play-limit", type=int, default=32)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--augment", action="store_true")
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--holdout", type=float, default=None)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-hip", action="store_true")
    ap.add_argument("--skip-device", action="store_true")
    ap.add_argument("--handoff", choices=("host", "device"), default="host")
    ap.add_argument("--game", choices=("connect4", "dragonchess"), default="connect4")
    ap.add_argument("--warmup-games", type=int, default=64)
    ap.add_argument("--score-engine", action="store_true")
    ap.add_argument("--loss", choices=("reference", "per_example"), default="reference")
    ap.add_argument("--temp-schedule", default=None, metavar="PLIES,TEMP")
    a = ap.parse_args()
    schedule = None
    if a.temp_schedule is not None:
        try:
            plies, late = a.temp_schedule.split(",")
            schedule = _lib.temp_schedule((int(plies), float(late)))
        except ValueError as err:
            ap.error("--temp-schedule PLIES,TEMP: %s" % err)
    if a.loss != "reference":
        CFG["training"]["loss"] = a.loss  # (every model of the run is made from CFG or a copy of it)
    dc = a.game == "dragonchess"
    if a.score_engine and a.holdout is None:
        ap.error("--score-engine goes with --holdout")
    if dc and (a.merge or a.augment or (a.holdout is not None and not a.score_engine)):
        ap.error("--merge and --augment cover Connect4 only, --holdout on DragonChess needs --score-engine")
    board = DragonChess.BoardState if dc else Connect4.BoardState
    planes = _lib.game_info(board.GAME_ID).C
    os.chdir(tempfile.mkdtemp())  # the sqlite file and the saved networks of this run
    np.random.seed(a.seed)
    model = Blackbird.Model(board, "train_path", {"explorationRate": 0.85, "playLimit": a.play_limit}, CFG)
    model.KeepDeviceExamples = True
    initial = {k: v.copy() for k, v in model._ensure_weights(planes).items()}
    model.SelfPlayTempSchedule = schedule
    Blackbird.GenerateTrainingSamples(model, a.warmup_games, 1.0)  # warm-up run (its examples are trained on too)
    t = time.time()
    Blackbird.GenerateTrainingSamples(model, a.games, 1.0)
    selfplay_s = time.time() - t
    kept = model.KeptDeviceExamples()
    n, B = len(kept), a.batch
    boards, value, policy = (x.cpu().numpy() for x in kept.batch(np.arange(min(B, n))))
    # the second model: the weights the first one saved when it was made, the hip backend
    hip_cfg = copy.deepcopy(CFG)
    hip_cfg["training"]["backend"] = "hip"
    if dc:
        hip_cfg["training"]["hip_games"] = "all"
    if a.handoff != "host":
        hip_cfg["training"]["handoff"] = a.handoff
    hip_model = Blackbird.Model(board, "train_path", {"explorationRate": 0.85, "playLimit": a.play_limit}, hip_cfg)
    assert all(np.array_equal(hip_model._weights[k], model._weights[k]) for k in model._weights)
    model.train(boards, value, policy, a.lr)  # warm-up step
    if not a.skip_hip:
        hip_model.getEvaluation(boards[:1].astype(np.int8))     # the engines a playing, training model owns: evaluation ...
        state = np.random.get_state()
        hip_model.SelfPlayTempSchedule = schedule
        Blackbird.GenerateTrainingSamples(hip_model, a.warmup_games, 1.0)    # ... and self-play (numpy's generator left where it was)
        np.random.set_state(state)
        hip_model.train(boards, value, policy, a.lr)
    torch.cuda.synchronize()

    # bare batches of one epoch
    order = kept.index_tensor(epoch_order(n, B))
    syms = kept.sym_tensor(np.random.randint(kept.symmetries, size=len(order))) if a.augment else None
    torch.cuda.synchronize()
    t = time.time()
    for i in range(len(order) // B):
        kept._batch(order[i * B:(i + 1) * B], None if syms is None else syms[i * B:(i + 1) * B])
    torch.cuda.synchronize()
    batch_s = time.time() - t

    # host path: TrainWithExamples, statement by statement, with a clock after the decode
    host_s = decode_s = None
    if not a.skip_host:
        t = time.time()
        states = model.Conn.GetGames(model.Name, model.Version)
        examples = [Blackbird.ExampleState.FromSerialized(s) for s in states]
        decode_s = time.time() - t
        assert len(examples) == n, (len(examples), n)
        horder = np.random.choice(len(examples), len(examples) - (len(examples) % B), replace=False)
        examples = [examples[i] for i in horder]
        for i in range(len(examples) // B):
            b = examples[i * B:(i + 1) * B]
            model.train(np.vstack([e.Board for e in b]), np.hstack([e.MctsEval for e in b]),
                        np.vstack([e.MctsPolicy for e in b]), a.lr)
        torch.cuda.synchronize()
        host_s = time.time() - t

    # device path
    device_s = None
    if not a.skip_device:
        t = time.time()
        Blackbird.TrainWithDeviceExamples(model, B, a.lr, examples=kept, augment=a.augment)
        torch.cuda.synchronize()
        device_s = time.time() - t

    # hip path: the same epoch (the same examples, an order drawn the same way) with the step as HIP kernels
    # -- both ways: the per-batch loop (fused=False: bb_examples_to_batch + bb_trainer_step per batch), then the epoch call
    # (bb_trainer_epoch: the step's kernels read the records, one call enqueues the epoch), after one untimed batch of it
    hip_s = hip_epoch_s = None
    if not a.skip_hip:
        t = time.time()
        Blackbird.TrainWithDeviceExamples(hip_model, B, a.lr, examples=kept, augment=a.augment, fused=False)
        torch.cuda.synchronize()
        hip_s = time.time() - t
        if not dc:
            hip_model._trainer.epoch_records(kept, order[:B], B, a.lr)
            torch.cuda.synchronize()
            t = time.time()
            Blackbird.TrainWithDeviceExamples(hip_model, B, a.lr, examples=kept, augment=a.augment, fused=True)
            torch.cuda.synchronize()
            hip_epoch_s = time.time() - t

    # the reference API's shape on the hip model: Model.train per batch (a step, then every engine the model owns reloaded), on
    # host arrays staged beforehand; then one hand-off alone against one export + load_weights, on the evaluation engine
    loop_s = handoff_s = export_load_s = None
    if not a.skip_hip:
        staged = [tuple(x.cpu().numpy() for x in kept._batch(order[i * B:(i + 1) * B])) for i in range(len(order) // B)]
        torch.cuda.synchronize()
        t = time.time()
        for b, v, p in staged:
            hip_model.train(b, v, p, a.lr)
        torch.cuda.synchronize()
        loop_s = time.time() - t
        tr, eng = hip_model._trainer, hip_model._eval_engine
        export_load_s = median_time(lambda: eng.load_weights(W.flatten(tr.export())))
        if hasattr(tr, "load_into"):
            handoff_s = median_time(lambda: (tr.load_into(eng), eng.synchronize()))

    # merged: the merge itself, the bare merged batches of an epoch, and the epoch through TrainWithDeviceExamples(merge=True)
    merge = {}
    if a.merge:
        type(kept)(kept.game, kept.records[:256]).merged()  # (untimed: the first call loads the kernels)
        torch.cuda.synchronize()
        t = time.time()
        merged = kept.merged()
        merge_s = time.time() - t   # (merged() ends in its host look: nothing is in flight)
        sizes = merged.counts().cpu().numpy()
        morder = merged.index_tensor(epoch_order(len(merged), B))
        msyms = merged.sym_tensor(np.random.randint(merged.symmetries, size=len(morder))) if a.augment else None
        torch.cuda.synchronize()
        t = time.time()
        for i in range(len(morder) // B):
            merged._batch(morder[i * B:(i + 1) * B], None if msyms is None else msyms[i * B:(i + 1) * B])
        torch.cuda.synchronize()
        mbatch_s = time.time() - t
        t = time.time()
        Blackbird.TrainWithDeviceExamples(model, B, a.lr, examples=kept, augment=a.augment, merge=True)
        torch.cuda.synchronize()
        merge = {"merge_records": n, "merge_groups": len(merged), "merge_bad": merged.bad(),
                 "merge_largest_groups": np.sort(sizes)[::-1][:5].tolist(), "merge_singletons": int((sizes == 1).sum()),
                 "merge_s": round(merge_s, 5), "merged_batches": len(merged) // B, "merged_batches_only_s": round(mbatch_s, 4),
                 "device_path_merge_s": round(time.time() - t, 3)}

    holdout = {} if a.holdout is None else {"holdout": holdout_run_dc(a, kept, board) if dc else holdout_run(a, kept, hip_cfg, initial)}

    duplicate_share = None if dc else round(1.0 - len(kept.merged()) / float(n), 5)
    r3 = lambda x: None if x is None else round(x, 3)  # noqa: E731
    print(json.dumps({"tool": "train_path", "game": a.game, "loss": a.loss, "games": a.games, "warmup_games": a.warmup_games, "play_limit": a.play_limit,
                      "temp_schedule": None if schedule is None else list(schedule), "duplicate_share": duplicate_share,
                      "examples": n, "augment": bool(a.augment), "batch_size": B, "batches": n // B, "selfplay_s": round(selfplay_s, 3),
                      "host_path_s": r3(host_s), "host_decode_s": r3(decode_s),
                      "device_path_s": r3(device_s), "device_batches_only_s": round(batch_s, 4),
                      "host_over_device": None if host_s is None or device_s is None else round(host_s / device_s, 2),
                      "hip_path_s": r3(hip_s),
                      "device_over_hip": None if hip_s is None or device_s is None else round(device_s / hip_s, 2),
                      "hip_epoch_s": r3(hip_epoch_s), "hip_over_hip_epoch": None if hip_s is None or hip_epoch_s is None else round(hip_s / hip_epoch_s, 2),
                      "handoff": a.handoff, "train_loop_s": r3(loop_s),
                      "handoff_s": None if handoff_s is None else round(handoff_s, 6),
                      "export_load_s": None if export_load_s is None else round(export_load_s, 6), **merge, **holdout}))


if __name__ == "__main__":
    main()
