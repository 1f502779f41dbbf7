#!/usr/bin/env python3
"""Generate tests/golden/resetroot_dc.npz: MCTS.ResetRoot and the Node graph below the root for DragonChess, from the
reference's own run (make_golden.gen_resetroot).  Three moves from the start position -- White, White, then Black -- so the
ancestor chain crosses an edge where the player to move does not change.

Runs ONLY where the reference's sources are available (see make_golden.py); the tests read the .npz file only.

usage: PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION=python python tests/make_golden_dc_tree.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden  # noqa: E402

if __name__ == "__main__":
    os.makedirs(make_golden.OUT, exist_ok=True)
    make_golden.gen_resetroot("dc", sims=24, moves=3, sims_after=16, salt=4300)
