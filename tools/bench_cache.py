"""bench.py plus the evaluation cache's share of the timed region: after bench's own JSON line, one more line with
eval_cache_hits / eval_cache_probes / hit_share / evals (tower runs) of the timed steps, read through Engine.counters(),
and the table in use: table_log2 (2^k entries) and table_bytes.

usage: [BB_EVAL_CACHE=0|1] [BB_LIB=<lib.so>] python tools/bench_cache.py [--launch-rounds] [bench.py arguments]

--launch-rounds creates the engine with launch=LAUNCH_ROUNDS: the c2 workload's 16-filter network then plays as asynchronous
rounds (k_net_x3 per round) instead of in the persistent kernel -- the shape that decides whether the round probe pays for
a small network.  bench.py itself is not changed: its Engine is wrapped here."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blackbird_amd import _lib  # noqa: E402

if os.environ.get("BB_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["BB_LIB"])
rounds = "--launch-rounds" in sys.argv
if rounds:
    sys.argv.remove("--launch-rounds")

last = {}


class Engine(_lib.Engine):
    def __init__(self, *a, **kw):
        if rounds:
            kw["launch"] = _lib.LAUNCH_ROUNDS
        super().__init__(*a, **kw)
        # the table this engine owns, as eval_cache_log2_of (csrc/host_engine.hip.h) sizes it (the defaults are those of the in-tree build)
        dc = self.game == _lib.GAME_DRAGONCHESS
        k = min(max(int(os.environ.get("BB_EVAL_CACHE_LOG2") or (24 if dc else 27)), 10), 32)
        if os.environ.get("BB_EVAL_CACHE", "1").strip() in ("0", ""):
            k = 0
        last.update(table_log2=k, table_bytes=((128 if dc else 64) << k) if k else 0)

    def counters(self):
        c = super().counters()
        last.update(c, selfplay_mode=self.selfplay_mode())
        return c


_lib.Engine = Engine
import bench  # noqa: E402

rc = 0
try:
    bench.main()
except SystemExit as ex:  # (bench.main ends in sys.exit)
    rc = ex.code or 0
h, p = last.get("eval_cache_hits", 0), last.get("eval_cache_probes", 0)
print(json.dumps({"eval_cache_hits": h, "eval_cache_probes": p, "hit_share": (h / p if p else 0.0), "evals": last.get("evals"),
                  "sims": last.get("sims"), "table_log2": last.get("table_log2"), "table_bytes": last.get("table_bytes"), "selfplay_mode": last.get("selfplay_mode"),
                  "BB_EVAL_CACHE": os.environ.get("BB_EVAL_CACHE", "")}))
sys.exit(rc)
