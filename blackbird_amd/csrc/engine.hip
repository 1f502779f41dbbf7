// engine.hip -- host side of libblackbird_hip.so: the C ABI of include/blackbird_hip.h, one translation unit.
// The kernels come first, then the host code by object, in the order it is compiled (the order of the includes below fixes the order
// in which kernel templates are instantiated, and with it the layout of the code object: keep it):
//   host_common.hip.h    the thread's last error (fail, HIPCHK), nblk, GAME_SWITCH, the HIP side of dev_mem.h, Staged<T>
//   host_launch.hip.h    Launch<G>: which kernel a game family launches for a step, and on what grid
//   host_games.hip.h     bb_game_info_get and the stateless batched game ops
//   host_engine.hip.h    bb_engine, its allocation, views and pool sizing, bb_create / bb_destroy
//   host_weights.hip.h   bb_load_weights*, launch_gnet / launch_net, bb_net_eval*, bb_hash_eval
//   host_search.hip.h    the simulation loop, roots, bb_run_sims*, sampling, node views
//   host_selfplay.hip.h  start positions, bb_selfplay_begin / step in every launch structure, counters
//   host_examples.hip.h  bb_examples_*: fetch, batches, merged duplicates
//   host_arena.hip.h     bb_arena
//   host_trainer.hip.h   bb_trainer
//   host_timing.hip.h    bb_timing_*, the stamp entry points of diagnostic builds
//   host_score.hip.h     bb_examples_score: records scored with the engine's network (last: nothing before it moves)
// Device memory, streams and events have one owner per object (dev_mem.h: DevOwner); a call's scratch is a Staged<T>.
//   simulation  = k_tree_step (apply previous leaf: expand+backup; select next leaf)  ->  evaluator kernel
//   move        = k_selfplay_move (apply last leaf; sample; record example; re-root; game over -> next game)
#include "../../include/blackbird_hip.h"
#include "eval.hip.h"
#include "net.hip.h"
#include "net_x3.hip.h"
#include "gnet.hip.h"
#include "gnet_x3.hip.h"
#include "eval_probe.hip.h"
#include "tree.hip.h"
#include "tree_dc.hip.h"
#include "mega2.hip.h"
#include "mega_dc.hip.h"
#include "search_wave.hip.h"
#include "search_wave_dc.hip.h"
#include "selfplay_wave.hip.h"
#include "examples.hip.h"
#include "examples_merge.hip.h"
#include "arena.hip.h"
#include "train.hip.h"
#include "train_eval.hip.h"
#include "net_blocks.h"
#include "net_pack.h"
#include "net_pack.hip.h"
#include "examples_score.hip.h"

#include "host_common.hip.h"
#include "host_launch.hip.h"
#include "host_games.hip.h"
#include "host_engine.hip.h"
#include "host_weights.hip.h"
#include "host_search.hip.h"
#include "host_selfplay.hip.h"
#include "host_examples.hip.h"
#include "host_arena.hip.h"
#include "host_trainer.hip.h"
#include "host_timing.hip.h"
#include "host_score.hip.h"
