// engine.hip -- host side of libblackbird_hip.so: the C ABI of include/blackbird_hip.h.
// Owns all device memory (hipMalloc), one HIP stream per engine, and the launch sequences:
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

#include <cassert>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static thread_local std::string g_err;
static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(x)                                                                                      \
    do {                                                                                               \
        hipError_t _e = (x);                                                                           \
        if (_e != hipSuccess) return fail(BB_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), \
                                          __FILE__, __LINE__);                                         \
    } while (0)

extern "C" const char *bb_last_error(void) { return g_err.c_str(); }

extern "C" int bb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

template <class G>
static void fill_info(bb_game_info *o) {
    o->H = G::H;
    o->W = G::W;
    o->C = G::C;
    o->A = G::A;
    o->S = G::S;
    o->state_bytes = (int)sizeof(typename G::State);
    o->dense = 1;
    o->example_bytes = (int)(sizeof(ExampleHdr) + sizeof(typename G::State) + 4 * G::S);
}

extern "C" int bb_game_info_get(int game, bb_game_info *out) {
    if (!out) return fail(BB_ERR_ARG, "null out");
    switch (game) {
    case BB_GAME_CONNECT4: fill_info<Connect4>(out); return BB_OK;
    case BB_GAME_TICTACTOE: fill_info<TicTacToe>(out); return BB_OK;
    case BB_GAME_DRAGONCHESS:
        fill_info<DragonChess>(out);
        out->dense = 0;
        out->example_bytes = (int)(sizeof(ExampleHdr) + sizeof(DCState) + 4 * DragonChess::S + 2 * DragonChess::S);
        return BB_OK;
    default: return fail(BB_ERR_ARG, "unknown or unsupported game %d", game);
    }
}

extern "C" int bb_game_symmetries(int game) {
    const int n = game_symmetries(game); // (symmetry.h)
    return n > 0 ? n : fail(BB_ERR_ARG, "unknown or unsupported game %d", game);
}

// ---- device scratch with automatic release ---------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t bytes) {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        return e == hipSuccess ? 0 : fail(BB_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
};

static inline int nblk(size_t n, int per = 256) { return (int)((n + per - 1) / per); }
// grid and block of every one-wave-per-slot kernel (search_wave*.hip.h, selfplay_wave.hip.h): <<<SW_GRID(d), 0, stream>>>
#define SW_GRID(d) nblk((d).n_slots, SW_WAVES), 64 * SW_WAVES

// ---- launch tables ---------------------------------------------------------------------------------------------
// THE place that knows which kernel a game family launches for a step of the lock-step engine, and on what grid: the primary template
// for the dense-action games (G::S lanes per slot; gpw games per wave in the tree step), the specialisation for DragonChess (one
// wave per slot, and the edge pool E that the dense family ignores).  Every member is exactly one launch, of 256-thread blocks (the
// node view: one wave).  The entry points below check, stage, call one member and copy back: none names a k_dc_* lock-step kernel or
// sizes a grid for one, and a new lock-step kernel's launch goes here, in both halves -- never into an entry point.
// (measurement switch of tools/search_latency.py: the dense games' one-launch rollout with lane 0 alone doing the playout)
static bool rollout_plain() {
    static const bool plain = [] { const char *v = getenv("BB_SW_ROLLOUT_PLAIN"); return v && v[0] == '1'; }();
    return plain;
}
template <class G>
struct Launch {
    using State = typename G::State;
    static void legal(int n, const State *s, uint8_t *out) { k_game_legal<G><<<nblk(n), 256>>>(n, s, out); }
    static void encode(int n, const State *s, int8_t *out) { k_game_encode<G><<<nblk((size_t)n * G::H * G::W), 256>>>(n, s, out); }
    static void tree_step(const TreeDev &d, const DCEdges &, hipStream_t st) { k_tree_step<G><<<nblk((size_t)((d.n_slots + d.gpw - 1) / d.gpw) * 64), 256, 0, st>>>(d); }
    static void tree_apply(const TreeDev &d, const DCEdges &, hipStream_t st) { k_tree_apply<G><<<nblk((size_t)d.n_slots * G::S), 256, 0, st>>>(d); }
    // BB_LAUNCH_WAVE: `sims` steps of tree_step + the evaluator, and tree_apply, as one launch with a wave per slot (search_wave.hip.h);
    // x3 with operands: the 16-filter network, else the hash evaluator.  cache (run_sims_api: bb_config.search_cache on an engine that
    // owns a table): the network's instantiation that probes and fills d.eval_cache, for a game with a one-word key.
    // false: this family has no such kernel.
    static bool search_wave(const TreeDev &d, const DCEdges &, hipStream_t st, int sims, const NetDev &nd, const NetX3 &x3, int noise, bool cache) {
        if (d.evaluator == BB_EVAL_ROLLOUT) { // (bb_search_rollouts)
            if (rollout_plain()) k_search_wave_rollout<G, false><<<SW_GRID(d), 0, st>>>(d, sims);
            else k_search_wave_rollout<G, true><<<SW_GRID(d), 0, st>>>(d, sims);
            return true;
        }
        if constexpr (G::CACHE_KEY) {
            if (x3.w0 && cache && d.eval_cache) {
                k_search_wave<G, true, true><<<SW_GRID(d), 0, st>>>(d, nd, x3, sims, noise);
                return true;
            }
        }
        if (x3.w0) k_search_wave<G, true><<<SW_GRID(d), 0, st>>>(d, nd, x3, sims, noise);
        else k_search_wave<G, false><<<SW_GRID(d), 0, st>>>(d, nd, x3, sims, 0);
        return true;
    }
    static void hash(hipStream_t st, int n, const State *s, const uint32_t *game_id, uint64_t salt, int salt_per_game, uint32_t first_game_id, float *value, float *policy, int pstride) {
        k_hash_eval<G><<<nblk(n), 256, 0, st>>>(n, s, game_id, salt, salt_per_game, first_game_id, value, policy, pstride);
    }
    static void rollout(const TreeDev &d, const DCEdges &, hipStream_t st) {
        k_rollout<G><<<nblk(d.n_slots), 256, 0, st>>>(d.n_slots, (const State *)d.leaf_state, d.leaf_game_id, d.sim_serial, d.pend_leaf, d.seed, d.eval_value);
    }
    static void sample(const TreeDev &d, const DCEdges &, hipStream_t st, double temp, int32_t *) { k_sample<G><<<nblk((size_t)d.n_slots * G::S), 256, 0, st>>>(d, temp); }
    static void move_roots(const TreeDev &d, const DCEdges &, hipStream_t st, const int32_t *actions) { k_move_roots<G><<<nblk((size_t)d.n_slots * G::S), 256, 0, st>>>(d, actions); }
    static void set_roots(const TreeDev &d, const DCEdges &, hipStream_t st, int n, const int32_t *slots, const State *s, const uint32_t *game_ids) {
        k_set_roots<G><<<nblk(n), 256, 0, st>>>(d, n, slots, s, game_ids);
    }
    static void reset_roots(const TreeDev &d, const DCEdges &, hipStream_t st) { k_reset_roots<G><<<nblk(d.n_slots), 256, 0, st>>>(d); }
    static void get_roots(const TreeDev &d, const DCEdges &, hipStream_t st, State *out) { k_get_roots<G><<<nblk(d.n_slots), 256, 0, st>>>(d, out); }
    static void node_edges(const TreeDev &d, const DCEdges &, hipStream_t st, int slot, int node, int32_t *, int32_t *child, int32_t *plays, float *value,
                           State *state, int32_t *info) { // (slot i is action i: no action list; info word 1 is the legal mask)
        k_node_view<G><<<1, 64, 0, st>>>(d, slot, node, child, plays, value, state, info);
    }
    static void check_starts(hipStream_t st, int n, const State *s, uint8_t *verdict) { k_check_starts<G><<<nblk(n), 256, 0, st>>>(n, s, verdict); }
    static void selfplay_begin(const TreeDev &d, const DCEdges &, hipStream_t st) { k_selfplay_begin<G><<<nblk(d.n_slots), 256, 0, st>>>(d); }
    static void selfplay_move(const TreeDev &d, const DCEdges &, hipStream_t st) { k_selfplay_move<G><<<nblk((size_t)d.n_slots * G::S), 256, 0, st>>>(d); }
    // PLAY_WAVE_ROLLOUT: `plies` times (`sims` steps of tree_step + rollout, then selfplay_move) as one launch with a wave per slot
    // (selfplay_wave.hip.h); move = 0: `sims` steps of one ply and no move
    static void selfplay_wave_rollout(const TreeDev &d, const DCEdges &, hipStream_t st, int plies, int sims, int move) {
        k_selfplay_wave_rollout<G><<<SW_GRID(d), 0, st>>>(d, plies, sims, move);
    }
    static void examples_to_batch(hipStream_t st, int n_records, const uint8_t *rec, int n, const int64_t *index, const uint8_t *sym, float *boards, float *policy, float *value, int32_t *bad) {
        k_examples_to_batch<G><<<nblk((size_t)n * (G::H * G::W * G::C + G::A + 1)), 256, 0, st>>>(n_records, rec, n, index, sym, boards, policy, value, bad);
    }
};
template <>
struct Launch<DragonChess> {
    using State = DCState;
    static void legal(int n, const State *s, uint8_t *out) { k_dc_legal<<<nblk((size_t)n * 64), 256>>>(n, s, out); }
    static void encode(int n, const State *s, int8_t *out) { k_dc_encode<<<nblk((size_t)n * 64), 256>>>(n, s, out); }
    static void tree_step(const TreeDev &d, const DCEdges &E, hipStream_t st) { k_dc_tree_step<<<nblk((size_t)d.n_slots * 64), 256, 0, st>>>(d, E); }
    static void tree_apply(const TreeDev &d, const DCEdges &E, hipStream_t st) { k_dc_tree_apply<<<nblk((size_t)d.n_slots * 64), 256, 0, st>>>(d, E); }
    // (search_structure sends the wide game here with a 16-filter split-operand network that fits the kernel's LDS, and nothing else;
    // its prior noise is mixed in at expansion: E.noise_on)
    static bool search_wave(const TreeDev &d, const DCEdges &E, hipStream_t st, int sims, const NetDev &nd, const NetX3 &x3, int, bool cache) {
        if (d.evaluator == BB_EVAL_ROLLOUT) { // (bb_search_rollouts)
            k_dc_search_wave_rollout<<<SW_GRID(d), 0, st>>>(d, E, sims);
            return true;
        }
        if (!x3.w0 || nd.R > DC_RMAX || nd.head_floats > DC_HEAD_FLOATS) return false;
        if (cache && d.eval_cache) k_dc_search_wave_cached<<<SW_GRID(d), 0, st>>>(d, E, nd, x3, sims);
        else k_dc_search_wave<<<SW_GRID(d), 0, st>>>(d, E, nd, x3, sims);
        return true;
    }
    static void hash(hipStream_t st, int n, const State *s, const uint32_t *game_id, uint64_t salt, int salt_per_game, uint32_t first_game_id, float *value, float *policy, int pstride) {
        k_dc_hash_eval<<<nblk((size_t)n * 64), 256, 0, st>>>(n, s, game_id, salt, salt_per_game, first_game_id, value, policy, pstride);
    }
    static void rollout(const TreeDev &d, const DCEdges &, hipStream_t st) {
        k_dc_rollout<<<nblk((size_t)d.n_slots * 64), 256, 0, st>>>(d.n_slots, (const State *)d.leaf_state, d.leaf_game_id, d.sim_serial, d.pend_leaf, d.seed, d.eval_value);
    }
    static void sample(const TreeDev &d, const DCEdges &E, hipStream_t st, double temp, int32_t *child_action) { k_dc_sample<<<nblk((size_t)d.n_slots * 64), 256, 0, st>>>(d, E, temp, child_action); }
    static void move_roots(const TreeDev &d, const DCEdges &E, hipStream_t st, const int32_t *actions) { k_dc_move_roots<<<nblk((size_t)d.n_slots * 64), 256, 0, st>>>(d, E, actions); }
    static void set_roots(const TreeDev &d, const DCEdges &E, hipStream_t st, int n, const int32_t *slots, const State *s, const uint32_t *game_ids) {
        k_dc_set_roots<<<nblk(n), 256, 0, st>>>(d, E, n, slots, s, game_ids);
    }
    static void reset_roots(const TreeDev &d, const DCEdges &, hipStream_t st) { k_dc_reset_roots<<<nblk(d.n_slots), 256, 0, st>>>(d); }
    static void get_roots(const TreeDev &d, const DCEdges &, hipStream_t st, State *out) { k_dc_get_roots<<<nblk(d.n_slots), 256, 0, st>>>(d, out); }
    static void node_edges(const TreeDev &d, const DCEdges &E, hipStream_t st, int slot, int node, int32_t *action, int32_t *child, int32_t *plays, float *value,
                           State *state, int32_t *info) {
        k_dc_node_edges<<<1, 64, 0, st>>>(d, E, slot, node, action, child, plays, value, state, info);
    }
    static void check_starts(hipStream_t st, int n, const State *s, uint8_t *verdict) { k_check_starts<DragonChess><<<nblk((size_t)n * 64), 256, 0, st>>>(n, s, verdict); }
    static void selfplay_begin(const TreeDev &d, const DCEdges &E, hipStream_t st) { k_dc_selfplay_begin<<<nblk(d.n_slots), 256, 0, st>>>(d, E); }
    static void selfplay_move(const TreeDev &d, const DCEdges &E, hipStream_t st) { k_dc_selfplay_move<<<nblk((size_t)d.n_slots * 64), 256, 0, st>>>(d, E); }
    static void selfplay_wave_rollout(const TreeDev &d, const DCEdges &E, hipStream_t st, int plies, int sims, int move) {
        k_dc_selfplay_wave_rollout<<<SW_GRID(d), 0, st>>>(d, E, plies, sims, move);
    }
    static void examples_to_batch(hipStream_t st, int n_records, const uint8_t *rec, int n, const int64_t *index, const uint8_t *sym, float *boards, float *policy, float *value, int32_t *bad) {
        k_dc_examples_to_batch<<<n, 256, 0, st>>>(n_records, rec, index, sym, boards, policy, value, bad);
    }
};

// ---- stateless batched game ops ------------------------------------------------------------------
template <class G>
static int game_legal(int n, const void *states, uint8_t *out) {
    DevBuf ds, dout;
    if (ds.alloc((size_t)n * sizeof(typename G::State)) || dout.alloc((size_t)n * G::A)) return BB_ERR_HIP;
    HIPCHK(hipMemcpy(ds.p, states, (size_t)n * sizeof(typename G::State), hipMemcpyDefault));
    Launch<G>::legal(n, (const typename G::State *)ds.p, (uint8_t *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dout.p, (size_t)n * G::A, hipMemcpyDefault));
    return BB_OK;
}
template <class G>
static int game_apply(int n, void *states, const int32_t *actions, int32_t *status) {
    DevBuf ds, da, dst;
    if (ds.alloc((size_t)n * sizeof(typename G::State)) || da.alloc((size_t)n * 4) || dst.alloc((size_t)n * 4))
        return BB_ERR_HIP;
    HIPCHK(hipMemcpy(ds.p, states, (size_t)n * sizeof(typename G::State), hipMemcpyDefault));
    HIPCHK(hipMemcpy(da.p, actions, (size_t)n * 4, hipMemcpyDefault));
    k_game_apply<G><<<nblk(n), 256>>>(n, (typename G::State *)ds.p, (const int32_t *)da.p, (int32_t *)dst.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(states, ds.p, (size_t)n * sizeof(typename G::State), hipMemcpyDefault));
    if (status) HIPCHK(hipMemcpy(status, dst.p, (size_t)n * 4, hipMemcpyDefault));
    return BB_OK;
}
template <class G>
static int game_winner(int n, const void *states, const int32_t *prev, int8_t *out) {
    DevBuf ds, dp, dout;
    if (ds.alloc((size_t)n * sizeof(typename G::State)) || dp.alloc((size_t)n * 4) || dout.alloc((size_t)n))
        return BB_ERR_HIP;
    HIPCHK(hipMemcpy(ds.p, states, (size_t)n * sizeof(typename G::State), hipMemcpyDefault));
    if (prev) HIPCHK(hipMemcpy(dp.p, prev, (size_t)n * 4, hipMemcpyDefault));
    k_game_winner<G><<<nblk(n), 256>>>(n, (const typename G::State *)ds.p, prev ? (const int32_t *)dp.p : nullptr,
                                       (int8_t *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dout.p, (size_t)n, hipMemcpyDefault));
    return BB_OK;
}
template <class G>
static int game_encode(int n, const void *states, int8_t *out) {
    size_t ob = (size_t)n * G::H * G::W * G::C;
    DevBuf ds, dout;
    if (ds.alloc((size_t)n * sizeof(typename G::State)) || dout.alloc(ob)) return BB_ERR_HIP;
    HIPCHK(hipMemcpy(ds.p, states, (size_t)n * sizeof(typename G::State), hipMemcpyDefault));
    Launch<G>::encode(n, (const typename G::State *)ds.p, (int8_t *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dout.p, ob, hipMemcpyDefault));
    return BB_OK;
}

#define GAME_SWITCH(game, ...)                                                   \
    switch (game) {                                                              \
    case BB_GAME_CONNECT4: { using G = Connect4; __VA_ARGS__; }                  \
    case BB_GAME_TICTACTOE: { using G = TicTacToe; __VA_ARGS__; }                \
    case BB_GAME_DRAGONCHESS: { using G = DragonChess; __VA_ARGS__; }            \
    default: return fail(BB_ERR_ARG, "unknown game %d", game);                   \
    }

extern "C" int bb_game_legal(int game, int n, const void *states, uint8_t *legal_out) {
    if (n == 0) return BB_OK; // an empty batch is a no-op
    if (n < 0 || !states || !legal_out) return fail(BB_ERR_ARG, "bad arguments");
    GAME_SWITCH(game, return game_legal<G>(n, states, legal_out));
}
extern "C" int bb_game_apply(int game, int n, void *states, const int32_t *actions, int32_t *status_out) {
    if (n == 0) return BB_OK;
    if (n < 0 || !states || !actions) return fail(BB_ERR_ARG, "bad arguments");
    GAME_SWITCH(game, return game_apply<G>(n, states, actions, status_out));
}
extern "C" int bb_game_winner(int game, int n, const void *states, const int32_t *prev, int8_t *winner_out) {
    if (n == 0) return BB_OK;
    if (n < 0 || !states || !winner_out) return fail(BB_ERR_ARG, "bad arguments");
    GAME_SWITCH(game, return game_winner<G>(n, states, prev, winner_out));
}
extern "C" int bb_game_encode(int game, int n, const void *states, int8_t *planes_out) {
    if (n == 0) return BB_OK;
    if (n < 0 || !states || !planes_out) return fail(BB_ERR_ARG, "bad arguments");
    GAME_SWITCH(game, return game_encode<G>(n, states, planes_out));
}
extern "C" int bb_game_initial(int game, void *state_out) {
    if (!state_out) return fail(BB_ERR_ARG, "null out");
    GAME_SWITCH(game, {
        typename G::State s = G::initial();
        memcpy(state_out, &s, sizeof s);
        return BB_OK;
    });
}

// ---- engine ----------------------------------------------------------------------------------------
// The launch structures of self-play (bb_selfplay_mode's values): lock-step launches per simulation (run_sims); dense games:
// k_tree_async rounds + evaluator; persistent per-CU kernel with an LDS work queue (mega2.hip.h); DragonChess: mega_dc.hip.h; the
// rollout evaluator of every game after bb_selfplay_rollouts(e, 1): one launch per step, a wave per slot (selfplay_wave.hip.h)
enum { PLAY_LOCKSTEP = 0, PLAY_ROUNDS = 1, PLAY_QUEUE = 3, PLAY_DC_FUSED = 5, PLAY_WAVE_ROLLOUT = 6 };
// What a configuration asks for -- the ONE place that reads mcts_kind / evaluator / launch / game for this.  (Whether the
// network fits a persistent kernel's LDS is known only at bb_load_weights: selfplay_structure.)
static int selfplay_plan(const bb_config *cfg) {
    const bool net_auto = cfg->evaluator == BB_EVAL_NET && cfg->launch == BB_LAUNCH_AUTO;
    if (cfg->mcts_kind != BB_MCTS_DYNAMIC) return PLAY_LOCKSTEP;
    if (cfg->game == BB_GAME_DRAGONCHESS) return net_auto ? PLAY_DC_FUSED : PLAY_LOCKSTEP;
    if (net_auto) return PLAY_QUEUE; // (else rounds, for the deterministic evaluators)
    return cfg->evaluator != BB_EVAL_ROLLOUT && (cfg->launch == BB_LAUNCH_AUTO || cfg->launch == BB_LAUNCH_ROUNDS) ? PLAY_ROUNDS : PLAY_LOCKSTEP;
}

struct bb_engine {
    bb_config cfg;
    bb_game_info info;
    TreeDev dev;
    DCEdges edges; // DragonChess only
    int32_t *d_child_action = nullptr;
    NetDev net;
    NetX3 x3 = {nullptr, nullptr, nullptr, nullptr, nullptr}; // 16-filter network of a dense game on the bf16 matrix pipe (net_x3.hip.h); null: float32 MFMA path
    size_t x3_bytes = 0;
    bool has_weights = false;
    bool search_rollouts = false; // bb_search_rollouts: a BB_EVAL_ROLLOUT engine with launch = BB_LAUNCH_WAVE searches in one launch
    bool selfplay_rollouts = false; // bb_selfplay_rollouts: a BB_EVAL_ROLLOUT engine plays bb_selfplay_step in one launch per call
    int net_F = 0, net_C = 0;
    bool general_net = false; // F != 16 (or BB_GNET=1): one implicit-GEMM launch per conv layer (gnet.hip.h)
    GNetDev gnet = {};
    GNetX3 gx3 = {nullptr, {nullptr, nullptr}}; // tower layers of the general-filter network on the bf16 matrix pipe (gnet_x3.hip.h)
    size_t gx3_bytes = 0;
    int gnet_C = 0;
    size_t net_sizes[4] = {0, 0, 0, 0};
    hipStream_t stream = nullptr;
    hipEvent_t w_event[2] = {nullptr, nullptr}; // bb_load_weights_device: the caller's stream -> the engine's, and back (no timing)
    std::vector<void *> allocs;
    int n_games_target = 0;
    StartsTable starts; // bb_selfplay_set_starts: the device copy dev.starts / view[].starts point at (starts.h); not in `allocs`
    int sims_now = 0;
    size_t node_bytes = 0;
    double *d_u = nullptr;
    int32_t *d_actions = nullptr;
    // optional HIP-event timing of the evaluator launches
    // pipelined asynchronous self-play: slot-range views of `dev`, one HIP stream each, so that one
    // group's (latency-bound) tree kernel runs underneath the other group's (MFMA-bound) network kernel
    int n_views = 1;
    TreeDev view[2];
    hipStream_t vstream[2] = {nullptr, nullptr};
    int vround[2] = {0, 0};
    // kernel-tuning knobs, read from the environment ONCE in bb_create (never on the step path); not part of the API
    struct {
        int launch_steps = 64, queue_limit_s = 30;
        int wave_rollout_sims = 0; // PLAY_WAVE_ROLLOUT: simulations per slot and launch; 0 = the game's figure (selfplay_wave_rollout)
        bool level_budget_set = false;
    } tune;
    size_t eval_cache_bytes = 0; // evaluation cache of self-play (dev.eval_cache: the persistent kernels and the asynchronous rounds), zeroed with every weight load
    // asynchronous rounds with the cache: the posted leaves the probe kernel did not answer (eval_probe.hip.h), what the
    // network launches of a round take.  Per view like post_count / post_slot: counters [4 v .. 4 v + 3], slots from slot_offset.
    // They are probed for the launch-per-layer networks (general_net) only: for a 16-filter network that plays as rounds the
    // probe launch costs more than the shorter k_net_x3 launch saves (75.8 against 60.5 ms per 800-visit step of 4096 games
    // with 36 % hits) -- such an engine owns the table, because it cannot know its network at bb_create, and
    // leaves it alone.
    int *miss_count = nullptr; // [8]
    int *miss_slot = nullptr;  // [n_slots]
    unsigned char *miss_way = nullptr; // [n_slots] the way of its bucket a missed slot's entry goes to
    int miss_next[2] = {0, 0}; // per view: the round whose counter the last probe launch cleared ahead (the rotation holds only across consecutive probed rounds)
    int plan = PLAY_LOCKSTEP; // selfplay_plan(cfg); what it plays through once its network is known: selfplay_structure
    int round = 0;
    int time_every = 0;
    uint64_t eval_launches = 0;
    std::vector<hipEvent_t> ev_pool; // pairs (start, stop)
    size_t ev_used = 0;
};

static hipError_t sync_all(bb_engine *e) {
    if (e->vstream[1]) {
        hipError_t r = hipStreamSynchronize(e->vstream[1]);
        if (r != hipSuccess) return r;
    }
    return hipStreamSynchronize(e->stream);
}

template <class T>
static int dalloc(bb_engine *e, T *&p, size_t count, bool zero = true) {
    void *q = nullptr;
    size_t bytes = count * sizeof(T);
    hipError_t err = hipMalloc(&q, bytes ? bytes : 16);
    if (err != hipSuccess) return fail(BB_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
    e->allocs.push_back(q);
    if (zero && bytes) {
        err = hipMemsetAsync(q, 0, bytes, e->stream);
        if (err != hipSuccess) return fail(BB_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(err));
    }
    p = (T *)q;
    return 0;
}

template <class G> struct NodeOf { using type = DenseNode<G>; }; // a node of the family's pool
template <> struct NodeOf<DragonChess> { using type = DCNode; };
#define SLOT_EXTENTS(G, max_plies) /* what the rows of BB_SLOT_ARRAYS (tree.hip.h) are written in */ \
    constexpr size_t S = G::S, MP = G::MAXPATH, PS = G::GID == BB_GAME_DRAGONCHESS ? G::A : G::S; \
    const size_t ANC = (size_t)((max_plies) + 2) * (G::GID == BB_GAME_DRAGONCHESS ? 2 : 1)

template <class G>
static int engine_alloc(bb_engine *e) {
    TreeDev &d = e->dev;
    const bb_config &c = e->cfg;
    size_t n = (size_t)c.n_slots;
    constexpr bool DC = G::GID == BB_GAME_DRAGONCHESS;
    constexpr size_t NODE_BYTES = sizeof(typename NodeOf<G>::type);
    e->node_bytes = NODE_BYTES;
    SLOT_EXTENTS(G, c.max_plies);
    bool bad = false;
#define X(T, f, per) bad = bad || dalloc(e, d.f, n * (per));
    BB_SLOT_ARRAYS(X)
#undef X
    if (bad || dalloc(e, e->d_u, n) || dalloc(e, e->d_actions, n) || dalloc(e, e->d_child_action, n * S) ||
        dalloc(e, d.stamps, STAMP_BUFFER_WORDS) || dalloc(e, d.visit_pool, 16) || dalloc(e, d.post_count, 8))
        return BB_ERR_HIP;
    typename G::State *ls;
    if (dalloc(e, ls, n)) return BB_ERR_HIP;
    d.leaf_state = ls;
    uint8_t *nodes;
    if (dalloc(e, nodes, n * (size_t)d.node_cap * NODE_BYTES, false)) return BB_ERR_HIP;
    d.nodes = nodes;
    if constexpr (DC) {
        DCEdges &E = e->edges;
        E.edge_cap = d.node_cap * 24; // ~15-25 legal moves per position; overflow is counted, never silent
        size_t ne = n * (size_t)E.edge_cap;
        bad = dalloc(e, E.e, ne, false);
#define X(T, f, per) bad = bad || dalloc(e, E.f, n * (per));
        BB_DC_SLOT_ARRAYS(X)
#undef X
        if (bad) return BB_ERR_HIP;
        E.noise_on = c.noise_on;
        E.alpha = c.alpha;
        E.eps = c.epsilon;
    }
    size_t ng = (size_t)c.max_games;
    if (dalloc(e, d.examples, ng * (size_t)(c.max_plies + 1) * (size_t)e->info.example_bytes, false) ||
        dalloc(e, d.game_hdr, ng * 4))
        return BB_ERR_HIP;
    // every slot idle until roots are set / self-play begins
    HIPCHK(hipMemsetAsync(d.game_lid, 0xFF, n * 4, e->stream));
    HIPCHK(hipMemsetAsync(d.pend_leaf, 0xFF, n * 4, e->stream));
    HIPCHK(hipMemsetAsync(d.resume_cur, 0xFF, n * 4, e->stream));
    HIPCHK(sync_all(e));
    return BB_OK;
}

// Slot-range views for pipelined self-play: every per-slot pointer is advanced by the view's first slot.
template <class G>
static void make_views(bb_engine *e) {
    const TreeDev &d = e->dev;
    int n = d.n_slots;
    SLOT_EXTENTS(G, d.max_plies);
    for (int v = 0; v < e->n_views; v++) {
        TreeDev w = d;
        int off = v == 0 ? 0 : n / 2;
        int cnt = e->n_views == 1 ? n : (v == 0 ? n / 2 : n - n / 2);
        w.n_slots = cnt;
        w.slot_offset = off;
#define X(T, f, per) w.f += (size_t)off * (per);
        BB_SLOT_ARRAYS(X) // (the dense games' anc by the stride it is allocated with; DragonChess, whose anc is two planes, gets one view)
#undef X
        w.leaf_state = (char *)d.leaf_state + (size_t)off * sizeof(typename G::State);
        w.nodes = (char *)d.nodes + (size_t)off * d.node_cap * e->node_bytes;
        w.post_count += 4 * v; // per view, not per slot
        e->view[v] = w;
    }
}

// ---- pool sizing ------------------------------------------------------------------------------------------------
// log2 of the entries of the evaluation cache (net.hip.h EvalCache) an engine of this configuration owns, 0 = none.
// Connect4 self-play (64-byte entries in two-way buckets; default 2^27: 8 GiB -- the smallest table whose games/s is within
// the run-to-run spread of the best, and the largest that bb_create still allocates in milliseconds: DESIGN.md section 11)
// probes it in the persistent kernel (mega2.hip.h) and in the
// asynchronous rounds that any other network or BB_LAUNCH_ROUNDS runs as (eval_probe.hip.h); DragonChess in its
// one-wave-per-game kernel (mega_dc.hip.h, 128-byte entries; default 2^24: 2 GiB, ~16 M positions against the ~0.4 M a ply
// of 1024 games evaluates, next to pools of ~190 GB).  The search API (bb_run_sims / bb_run_sims_masked) probes it in its one-launch
// structure when the engine asks for both (bb_config.launch = BB_LAUNCH_WAVE with search_cache = 1, a network evaluator, Connect4 or
// DragonChess: search_wave.hip.h, search_wave_dc.hip.h) -- such an engine plays self-play in lock-step, so without search_cache it owns
// no table, as before; the lock-step search never probes.  BB_EVAL_CACHE=0 turns it off,
// BB_EVAL_CACHE_LOG2 sizes it -- tuning knobs, read from the environment at bb_create / bb_fit_slots.
static size_t eval_cache_entry_bytes(const bb_config *cfg) { return cfg->game == BB_GAME_DRAGONCHESS ? 128 : 64; }
static int eval_cache_log2_of(const bb_config *cfg) {
    // THE rule of who owns a table: a configuration whose structure probes one.  (TicTacToe has no key: games.hip.h CACHE_KEY.)
    const bool c4 = cfg->game == BB_GAME_CONNECT4;
    const bool search_probes = cfg->search_cache == 1 && cfg->launch == BB_LAUNCH_WAVE && cfg->evaluator == BB_EVAL_NET &&
                               (c4 || cfg->game == BB_GAME_DRAGONCHESS); // (whether the loaded network has a one-launch search: search_structure)
    if (!search_probes) switch (selfplay_plan(cfg)) {
    case PLAY_DC_FUSED: break;                                                // mega_dc.hip.h
    case PLAY_QUEUE: if (!c4) return 0; break;                                // mega2.hip.h, and the rounds of a network that does not fit it
    case PLAY_ROUNDS: if (!c4 || cfg->evaluator != BB_EVAL_NET) return 0; break; // eval_probe.hip.h (the hash evaluator's rounds probe nothing)
    default: return 0;                                                        // lock-step self-play does not
    }
    const char *on = getenv("BB_EVAL_CACHE"), *lg = getenv("BB_EVAL_CACHE_LOG2");
    if (on && atoi(on) == 0) return 0;
    const int k = lg ? atoi(lg) : cfg->game == BB_GAME_DRAGONCHESS ? 24 : 27;
    return k < 10 ? 10 : k > 32 ? 32 : k;
}

static long node_capacity_of(const bb_config *cfg) {
    long cap = cfg->node_capacity > 0 ? cfg->node_capacity : (long)cfg->sims_per_move * cfg->max_plies + 2;
    if (cfg->mcts_kind == BB_MCTS_FIXED && cfg->node_capacity <= 0) cap = cap * cfg->max_depth;
    return cap;
}

// device bytes engine_alloc<G> asks for: per slot (node pool, DragonChess edge pool, mailboxes, paths) and per engine
// (example store of max_games games).  bb_fit_slots reports the per-slot figure, and it UNDER-COUNTS against the table
// (tree.hip.h BB_SLOT_ARRAYS): of the MAXPATH-long rows it has `path` (and path_edge) but not path_N, path_all and path_W, and
// it has no `anc` at all -- noise next to a node pool; a change of what bb_fit_slots returns should sum the rows instead.
template <class G>
static void pool_bytes(const bb_config *cfg, size_t *per_slot, size_t *fixed) {
    constexpr bool DC = G::GID == BB_GAME_DRAGONCHESS;
    constexpr size_t NODE_BYTES = sizeof(typename NodeOf<G>::type);
    const size_t cap = (size_t)node_capacity_of(cfg);
    size_t ps = cap * NODE_BYTES;
    if (DC) ps += cap * 24 * sizeof(DCEdge) + (size_t)G::MAXPATH * 4;
    ps += (size_t)G::MAXPATH * 4 + (DC ? (size_t)G::A : (size_t)G::S) * 4 + (size_t)G::S * 16 + sizeof(typename G::State) + 256;
    bb_game_info gi;
    bb_game_info_get(cfg->game, &gi);
    const size_t ng = (size_t)(cfg->max_games > 0 ? cfg->max_games : cfg->n_slots);
    *per_slot = ps;
    *fixed = ng * ((size_t)(cfg->max_plies + 1) * (size_t)gi.example_bytes + 16) + (64u << 20); // + weights, scratch, runtime slack
    if (const int k = eval_cache_log2_of(cfg)) *fixed += eval_cache_entry_bytes(cfg) << k;
}

static int check_config(const bb_config *cfg) {
    if (!cfg) return fail(BB_ERR_ARG, "null argument");
    if (cfg->n_slots <= 0) return fail(BB_ERR_ARG, "n_slots must be positive");
    if (cfg->mcts_kind == BB_MCTS_FIXED && cfg->max_depth <= 0)
        return fail(BB_ERR_ARG, "MaxDepth for MCTS must be > 0."); // FixedMCTS.py:15-16
    if (cfg->sims_per_move < 0 || cfg->max_plies <= 0) return fail(BB_ERR_ARG, "bad sims_per_move/max_plies");
    if (cfg->search_cache != 0 && cfg->search_cache != 1) return fail(BB_ERR_ARG, "bb_config.search_cache must be 0 or 1");
    int ndev = bb_device_count();
    if (ndev <= 0) return fail(BB_ERR_HIP, "no HIP device available (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(BB_ERR_ARG, "device %d out of range", cfg->device);
    if (node_capacity_of(cfg) >= (1 << 26)) return fail(BB_ERR_ARG, "node capacity too large");
    return BB_OK;
}

extern "C" int bb_fit_slots(const bb_config *cfg, int *n_slots_out, uint64_t *bytes_per_slot_out) {
    int rc = check_config(cfg);
    if (rc) return rc;
    size_t per_slot = 0, fixed = 0;
    GAME_SWITCH(cfg->game, pool_bytes<G>(cfg, &per_slot, &fixed); break);
    HIPCHK(hipSetDevice(cfg->device));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t usable = free_b - free_b / 16; // leave 1/16 of what is free to the runtime and to other engines' scratch
    long fit = usable > fixed ? (long)((usable - fixed) / per_slot) : 0;
    if (fit > cfg->n_slots) fit = cfg->n_slots;
    if (n_slots_out) *n_slots_out = (int)fit;
    if (bytes_per_slot_out) *bytes_per_slot_out = (uint64_t)per_slot;
    if (fit <= 0)
        return fail(BB_ERR_CAPACITY, "not even one game slot (%zu bytes) + the example store (%zu bytes) fits the %zu free bytes of device %d",
                    per_slot, fixed, free_b, cfg->device);
    return BB_OK;
}

extern "C" int bb_create(const bb_config *cfg, bb_engine **out) {
    if (!cfg || !out) return fail(BB_ERR_ARG, "null argument");
    {
        int rc = check_config(cfg);
        if (rc) return rc;
        int fit = 0;
        uint64_t per_slot = 0;
        rc = bb_fit_slots(cfg, &fit, &per_slot);
        if (rc) return rc;
        if (fit < cfg->n_slots)
            return fail(BB_ERR_CAPACITY, "%d game slots of %llu bytes each do not fit the free memory of device %d (%d would; "
                        "fewer slots play the same games one after another)", cfg->n_slots, (unsigned long long)per_slot, cfg->device, fit);
    }
    bb_engine *e = new bb_engine();
    e->cfg = *cfg;
    e->sims_now = cfg->sims_per_move;
    int rc = bb_game_info_get(cfg->game, &e->info);
    if (rc) {
        delete e;
        return rc;
    }
    HIPCHK(hipSetDevice(cfg->device));
    HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    for (hipEvent_t &ev : e->w_event) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    TreeDev &d = e->dev;
    memset(&d, 0, sizeof d);
    d.n_slots = cfg->n_slots;
    d.sims_per_move = cfg->sims_per_move;
    d.max_plies = cfg->max_plies;
    d.kind = cfg->mcts_kind;
    d.max_depth = cfg->max_depth;
    d.evaluator = cfg->evaluator;
    d.priors_ones = (cfg->mcts_kind == BB_MCTS_FIXED || cfg->evaluator == BB_EVAL_ROLLOUT) ? 1 : 0;
    d.salt_per_game = cfg->salt_per_game;
    d.track_anc = cfg->track_ancestors != 0 ? 1 : 0;
    d.max_games = cfg->max_games > 0 ? cfg->max_games : cfg->n_slots;
    e->cfg.max_games = d.max_games;
    d.c_puct = cfg->c_puct;
    d.seed = cfg->seed;
    d.salt = cfg->hash_salt;
    d.first_game_id = cfg->first_game_id;
    d.node_cap = (int)node_capacity_of(cfg);
    d.example_bytes = e->info.example_bytes;
    d.gpw = 64 / e->info.S;
    d.level_budget = 16; // tree levels per call of the launch-per-round structures (20 x 256 in-search: 12 / 16 / 24 -> 93 / 105 / 106 k evaluations/s); the persistent kernel uses 12, below
    d.slot_offset = 0;
    d.pool_g0 = 0;
    d.noise_alpha = cfg->alpha;
    d.lid_stride = cfg->n_slots;
    auto env_int = [](const char *name, int dflt) {
        const char *v = getenv(name);
        return v ? atoi(v) : dflt;
    };
    if (int v = env_int("BB_LEVEL_BUDGET", 0); v >= 1) {
        d.level_budget = v;
        e->tune.level_budget_set = true;
    }
    e->tune.launch_steps = env_int("BB_LAUNCH_STEPS", 64);
    e->tune.queue_limit_s = env_int("BB_QUEUE_LIMIT_S", 30);
    if (int v = env_int("BB_SELFPLAY_WAVE_SIMS", 0); v >= 1) e->tune.wave_rollout_sims = v; // (the tests of the launch split)
    if (cfg->launch < 0 || cfg->launch > BB_LAUNCH_WAVE || cfg->net_form < 0 || cfg->net_form > BB_NET_FORM_SPLIT) {
        delete e;
        return fail(BB_ERR_ARG, "bad bb_config.launch / net_form");
    }
    e->plan = selfplay_plan(cfg);
    const bool rounds_kernels = e->plan == PLAY_ROUNDS || e->plan == PLAY_QUEUE; // (a queue engine plays rounds when its network does not fit)
    if (int v = env_int("BB_TREE_GPW", 0); v >= 1 && v <= 64 / e->info.S) d.gpw = v;
    d.temp = 1.0;
    GAME_SWITCH(cfg->game, rc = engine_alloc<G>(e); break);
    if (!rc) { // (a configuration that owns a table plays through a structure that probes it: eval_cache_log2_of asks selfplay_plan)
        if (const int k = eval_cache_log2_of(cfg)) {
            uint8_t *tab = nullptr;
            e->eval_cache_bytes = eval_cache_entry_bytes(cfg) << k;
            rc = dalloc(e, tab, e->eval_cache_bytes); // (zeroed: empty)
            d.eval_cache = tab;
            d.eval_cache_log2 = k;
        }
    }
    if (!rc) rc = dalloc(e, d.eval_cache_ctr, 2);
    if (!rc && d.eval_cache && rounds_kernels)
        rc = dalloc(e, e->miss_count, 8) || dalloc(e, e->miss_slot, (size_t)cfg->n_slots) || dalloc(e, e->miss_way, (size_t)cfg->n_slots);
    if (rc) {
        bb_destroy(e);
        return rc;
    }
    e->n_views = 1;
    if (e->plan == PLAY_ROUNDS && cfg->evaluator == BB_EVAL_NET && cfg->n_slots >= 512) e->n_views = 2;
    if (const char *env = getenv("BB_GROUPS")) e->n_views = (atoi(env) == 2 && rounds_kernels && cfg->n_slots >= 2) ? 2 : 1; // (tuning)
    e->vstream[0] = e->stream;
    if (e->n_views == 2) HIPCHK(hipStreamCreateWithFlags(&e->vstream[1], hipStreamNonBlocking));
    GAME_SWITCH(cfg->game, make_views<G>(e); break);
    *out = e;
    return BB_OK;
}

extern "C" int bb_destroy(bb_engine *e) {
    if (!e) return BB_OK;
    (void)hipSetDevice(e->cfg.device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (void *p : e->allocs) (void)hipFree(p);
    if (e->starts.dev) (void)hipFree(e->starts.dev);
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->w_event)
        if (ev) (void)hipEventDestroy(ev);
    if (e->vstream[1]) {
        (void)hipStreamSynchronize(e->vstream[1]);
        (void)hipStreamDestroy(e->vstream[1]);
    }
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return BB_OK;
}

extern "C" int bb_timing_enable(bb_engine *e, int every_n) {
    if (!e || every_n < 0) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    if (every_n > 0 && e->ev_pool.empty()) {
        e->ev_pool.resize(2 * 512);
        for (auto &ev : e->ev_pool) HIPCHK(hipEventCreate(&ev));
    }
    e->time_every = every_n;
    e->eval_launches = 0;
    e->ev_used = 0;
    return BB_OK;
}

extern "C" int bb_timing_read(bb_engine *e, double *mean_ms_out, double *min_ms_out, int *count_out) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    double sum = 0.0, mn = 1e30;
    int cnt = 0;
    for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->ev_pool[i], e->ev_pool[i + 1]));
        sum += ms;
        if (ms < mn) mn = ms;
        cnt++;
    }
    if (mean_ms_out) *mean_ms_out = cnt ? sum / cnt : 0.0;
    if (min_ms_out) *min_ms_out = cnt ? mn : 0.0;
    if (count_out) *count_out = cnt;
    e->ev_used = 0;
    e->eval_launches = 0;
    return BB_OK;
}

extern "C" int bb_net_form(bb_engine *e) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    if (e->general_net) return e->gx3.wt ? 3 : 1;
    return e->x3.w0 ? 2 : 0;
}

// The structure the engine plays through at this moment: its plan, unless that is a persistent kernel whose LDS the loaded network
// does not fit (16 filters, at most rmax blocks and head_max packed head parameters).  Without weights the plan is the answer, which
// only bb_selfplay_mode sees: a step needs bb_selfplay_begin, and that refuses a network evaluator without weights (check_eval).
static int selfplay_structure(const bb_engine *e) {
    auto fits = [&](int rmax, int head_max) { return !e->has_weights || (!e->general_net && e->net.R <= rmax && e->net.head_floats <= head_max); };
    if (e->plan == PLAY_QUEUE && !fits(MEGA_RMAX, MEGA_HEAD_FLOATS)) return PLAY_ROUNDS;
    if (e->plan == PLAY_DC_FUSED && !fits(DC_RMAX, DC_HEAD_FLOATS)) return PLAY_LOCKSTEP;
    // (selfplay_plan sends every rollout engine to lock-step, whatever its game, mcts_kind and launch: the opt-in replaces that)
    if (e->cfg.evaluator == BB_EVAL_ROLLOUT && e->selfplay_rollouts) return PLAY_WAVE_ROLLOUT;
    return e->plan;
}

extern "C" int bb_selfplay_rollouts(bb_engine *e, int on) {
    if (!e || (on != 0 && on != 1)) return fail(BB_ERR_ARG, "bb_selfplay_rollouts: an engine and 0 or 1");
    e->selfplay_rollouts = on != 0; // (read by selfplay_structure, for BB_EVAL_ROLLOUT engines only)
    return BB_OK;
}

extern "C" int bb_selfplay_mode(bb_engine *e) { return e ? selfplay_structure(e) : fail(BB_ERR_ARG, "null engine"); }

extern "C" int bb_synchronize(bb_engine *e) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    if (e->vstream[1]) HIPCHK(hipStreamSynchronize(e->vstream[1]));
    HIPCHK(sync_all(e));
    return BB_OK;
}

// ---- weights: pack on the host (net_pack.h), keep or reallocate the operand buffers, upload ---------------------------
static_assert(GNET_X3_BLOCK * 2 == GX3_PAIR_B, "net_pack.h and gnet_x3.hip.h must agree on the tower's weight block");
template <class T>
static int upload(void *dst, const std::vector<T> &v) {
    if (!v.empty()) HIPCHK(hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return BB_OK;
}

// ---- general-F network (gnet.hip.h): buffers, weights, launch sequence -------------------------------------------------
template <class G>
static int gnet_reserve(bb_engine *e, int n) {
    using GG = GNetGeom<G>;
    GNetDev &g = e->gnet;
    int cap = (n + GG::PPB - 1) / GG::PPB * GG::PPB;
    if (cap <= g.cap) return BB_OK;
    HIPCHK(sync_all(e));
    size_t pos_floats = (size_t)g.NCB * 4 * GG::PLANE;
    if (dalloc(e, g.inp, (size_t)cap * GG::SLOTS * GG::CP) || dalloc(e, g.act[0], (size_t)cap * pos_floats))
        return BB_ERR_HIP; // zero-filled: the halo ring of every position stays zero for the buffers' lifetime
    if (e->gx3.wt) { // bf16-pipe tower: two buffers of three bf16 planes; the float32 buffer above only carries the last layer
        const size_t pos_bytes = (size_t)g.NCB * GG::SLOTS * 96;
        if (dalloc(e, e->gx3.act3[0], (size_t)cap * pos_bytes) || dalloc(e, e->gx3.act3[1], (size_t)cap * pos_bytes)) return BB_ERR_HIP;
    } else if (dalloc(e, g.act[1], (size_t)cap * pos_floats)) {
        return BB_ERR_HIP;
    }
    HIPCHK(sync_all(e)); // the fills ran on the engine stream; the caller may launch on another one
    g.cap = cap;
    return BB_OK;
}

// img: pack_f32 at F / 16 filter blocks
static int load_general_weights(bb_engine *e, const bb_net_weights *w, const NetF32 &img) {
    const int F = w->F, C = w->C, R = w->R, NCB = F / 16;
    // the tower layers' operands as three bf16 planes (gnet_x3.hip.h); BB_NET_FORM_F32 keeps the float32-MFMA layers
    const bool want3 = R > 0 && e->cfg.net_form != BB_NET_FORM_F32;
    const std::vector<uint16_t> x = want3 ? pack_gnet_x3(w, NCB) : std::vector<uint16_t>();
    GNetDev &g = e->gnet;
    // weights are reloaded after every training step: keep the device buffers (operands and activation scratch) when
    // the network shape is unchanged instead of allocating new ones each time
    const bool same = g.F == F && g.R == R && g.NCB == NCB && g.w0 && e->gnet_C == C;
    float *d_w0 = (float *)g.w0, *d_wt = (float *)g.wt, *d_epi = (float *)g.epi;
    if (!same) {
        g = GNetDev{};
        g.F = F;
        g.NCB = NCB;
        g.R = R;
        e->gnet_C = C;
        if (dalloc(e, d_w0, img.w0.size(), false) || dalloc(e, d_wt, img.wt.size(), false) || dalloc(e, d_epi, img.epi.size(), false))
            return BB_ERR_HIP;
    }
    HIPCHK(sync_all(e));
    if (upload(d_w0, img.w0) || upload(d_wt, img.wt) || upload(d_epi, img.epi)) return BB_ERR_HIP;
    g.w0 = d_w0;
    g.wt = (const f32x4 *)d_wt;
    g.epi = d_epi;
    if (want3) {
        unsigned char *d_x = (unsigned char *)e->gx3.wt;
        if (!d_x || x.size() * 2 != e->gx3_bytes) {
            if (dalloc(e, d_x, x.size() * 2 + 16, false)) return BB_ERR_HIP;
            e->gx3_bytes = x.size() * 2;
            g.cap = 0; // (the activation buffers of the other form are re-reserved on the next launch)
        }
        if (upload(d_x, x)) return BB_ERR_HIP;
        e->gx3.wt = d_x;
    } else {
        if (e->gx3.wt) g.cap = 0;
        e->gx3.wt = nullptr;
    }
    return BB_OK;
}

// How launch_gnet cuts a call of up to n_max positions at NCB filter blocks -- the ONE place that decides it.  Small batch: one
// position x one filter block per wave (latency of a lone evaluation: 40 layers x ~25 us instead of x ~170 us at 256 filters);
// every larger call, and every call whose size lives on the device (n_ptr), takes PPB positions x FBW filter blocks per wave.
// bb_net_eval_structure reports it for a host-sized call.
static bool gnet_small_launch(int n_max, int NCB, const int *n_ptr) { return (long)n_max * NCB <= 2048 && !n_ptr; }

// n_ptr != nullptr: the batch size lives in device memory (<= n_max); slot_list maps batch entries to mailbox slots
template <class G>
static int launch_gnet(bb_engine *e, int n_max, const int *n_ptr, const int *slot_list, const typename G::State *states,
                       const int8_t *planes, const uint32_t *game_id, const int32_t *serial, int noise, float *value,
                       float *logits, float *policy, int pstride, hipStream_t st, int buf_offset = 0,
                       EvalCache store = {nullptr, 0}) {
    // store: the evaluation cache the heads fill (the batch is a round's miss list: eval_probe.hip.h)
    // buf_offset: first position of the activation buffers this call may use (the two slot-range views of pipelined
    // rounds run on two streams at once and must not share scratch)
    using GG = GNetGeom<G>;
    buf_offset = (buf_offset + GG::PPB - 1) / GG::PPB * GG::PPB;
    int rc = gnet_reserve<G>(e, buf_offset + n_max);
    if (rc) return rc;
    GNetDev g = e->gnet;
    {
        const size_t pos_floats = (size_t)g.NCB * 4 * GG::PLANE;
        g.inp += (size_t)buf_offset * GG::SLOTS * GG::CP;
        g.act[0] += (size_t)buf_offset * pos_floats;
        if (g.act[1]) g.act[1] += (size_t)buf_offset * pos_floats; // (not allocated when the tower layers run in the split-operand form)
    }
    k_gnet_input<G><<<nblk((size_t)n_max * GG::HW), 256, 0, st>>>(g, n_max, n_ptr, slot_list, states, planes);
    GNetX3 gx = e->gx3; // wt != nullptr: tower layers on the bf16 matrix pipe (gnet_x3.hip.h); first conv in float32 MFMA, writing the split form
    if (gx.wt) {
        const size_t pos_bytes = (size_t)g.NCB * GG::SLOTS * 96;
        gx.act3[0] += (size_t)buf_offset * pos_bytes;
        gx.act3[1] += (size_t)buf_offset * pos_bytes;
    }
    const bool small = gnet_small_launch(n_max, g.NCB, n_ptr);
    constexpr int FBW3 = 4;
    // a workgroup's four waves take `per` neighbours along y (filter blocks, or groups of FBW of them) and 4 / per along x
    // (positions, or groups of PPB of them)
    const int nx = small ? n_max : (n_max + GG::PPB - 1) / GG::PPB;
    auto cut = [&](int fbw, int &per) {
        const int ny = small ? g.NCB : (g.NCB + fbw - 1) / fbw;
        per = ny >= 4 ? 4 : (ny >= 2 ? 2 : 1);
        return dim3((nx + 4 / per - 1) / (4 / per), (ny + per - 1) / per);
    };
    int per0, per;
    const dim3 grid0 = cut(GN_FBW, per0), grid = cut(gx.wt ? FBW3 : GN_FBW, per); // first convolution, tower
    auto *conv0 = small ? k_gnet_conv<G, true, 1, 1> : k_gnet_conv<G, true>;
    conv0<<<grid0, 256, 0, st>>>(g, 0, n_max, n_ptr, nullptr, g.act[0], 0, per0, gx.wt ? gx.act3[0] : nullptr);
    const int L = 2 * g.R;
    if (gx.wt) {
        auto *mid = small ? k_gnet_conv_x3<G, 1, 1, false> : k_gnet_conv_x3<G, GG::PPB, FBW3, false>;
        auto *last = small ? k_gnet_conv_x3<G, 1, 1, true> : k_gnet_conv_x3<G, GG::PPB, FBW3, true>; // writes float32, for the heads
        for (int l = 0; l < L; l++)
            (l + 1 < L ? mid : last)<<<grid, 256, 0, st>>>(g, gx, 1 + l, n_max, n_ptr, gx.act3[l & 1], gx.act3[(l & 1) ^ 1],
                                                           l + 1 < L ? nullptr : g.act[0], l & 1, per);
    } else {
        auto *conv = small ? k_gnet_conv<G, false, 1, 1> : k_gnet_conv<G, false>;
        for (int l = 0; l < L; l++)
            conv<<<grid, 256, 0, st>>>(g, 1 + l, n_max, n_ptr, g.act[l & 1], g.act[(l & 1) ^ 1], l & 1, per, nullptr);
    }
    k_gnet_heads<G><<<(n_max + 3) / 4, 256, 0, st>>>(g, e->net, n_max, n_ptr, slot_list, g.act[0], game_id, serial, noise, value,
                                                     logits, policy, pstride, store, planes ? nullptr : states);
    HIPCHK(hipGetLastError());
    return BB_OK;
}

// What every entry point asks of a bb_net_weights before anything else: the game's planes and actions, and every block the
// shape needs (net_blocks.h).  `who`, where given, goes in front of the message.
static int check_weights(const bb_net_weights *w, const bb_game_info &gi, const char *who = nullptr) {
    const std::string pre = who ? std::string(who) + ": " : "";
    if (w->H != gi.H || w->W != gi.W || w->C != gi.C || w->A != gi.A)
        return fail(BB_ERR_ARG, "%sweights are for a %dx%dx%d/%d network, game needs %dx%dx%d/%d", pre.c_str(), w->H, w->W, w->C, w->A,
                    gi.H, gi.W, gi.C, gi.A);
    if (net_block_missing(*w)) return fail(BB_ERR_ARG, "%sa weight block is missing", pre.c_str());
    return BB_OK;
}

extern "C" int bb_load_weights(bb_engine *e, const bb_net_weights *w) {
    if (!e || !w) return fail(BB_ERR_ARG, "null argument");
    if (int rc = check_weights(w, e->info)) return rc;
    if (w->F <= 0 || w->F % 16 != 0 || w->F > 1024)
        return fail(BB_ERR_ARG, "filters must be a multiple of 16 (MFMA tile), got %d", w->F);
    if (w->D <= 0 || w->D > 64 || w->R < 0) return fail(BB_ERR_ARG, "unsupported dense/blocks");
    HIPCHK(hipSetDevice(e->cfg.device));
    // no evaluation outlives the weights (or the network form) it was made with
    if (e->eval_cache_bytes) HIPCHK(hipMemsetAsync(e->dev.eval_cache, 0, e->eval_cache_bytes, e->stream));
    const int F = w->F, C = w->C, R = w->R;
    e->general_net = F != 16 || e->cfg.general_net != 0;
    // operands of the fused single-wave tower (net.hip.h): the one-block image; a wider network leaves them zero
    const NetF32 img = F == 16 ? pack_f32(w, 1) : NetF32(C, R, 1);
    if (e->general_net) {
        int rc = load_general_weights(e, w, F == 16 ? img : pack_f32(w, F / 16));
        if (rc) return rc;
    }
    const NetHead head = pack_head(w);
    // the bf16-pipe form of the same network (every game, 16 filters); BB_NET_FORM_F32 keeps the float32 MFMA path
    const bool want3 = F == 16 && C <= 32 && !e->general_net && e->cfg.net_form != BB_NET_FORM_F32;
    const NetX3Image x = want3 ? pack_x3(w) : NetX3Image();
    NetDev &nd = e->net;
    // (weights are reloaded after every training step: the operand buffers are reused while their sizes stay the same)
    float *d_w0 = (float *)nd.w0, *d_wt = (float *)nd.wt, *d_epi = (float *)nd.epi, *d_head = (float *)nd.head;
    const size_t sizes[4] = {img.w0.size(), img.wt.size(), img.epi.size(), head.v.size()};
    if (!d_w0 || memcmp(sizes, e->net_sizes, sizeof(sizes)) != 0) {
        if (dalloc(e, d_w0, sizes[0], false) || dalloc(e, d_wt, sizes[1], false) || dalloc(e, d_epi, sizes[2], false) ||
            dalloc(e, d_head, sizes[3], false))
            return BB_ERR_HIP;
        memcpy(e->net_sizes, sizes, sizeof(sizes));
    }
    HIPCHK(sync_all(e));
    if (upload(d_w0, img.w0) || upload(d_wt, img.wt) || upload(d_epi, img.epi) || upload(d_head, head.v)) return BB_ERR_HIP;
    if (want3) { // one buffer, the five images back to back
        const std::vector<uint16_t> *part[5] = {&x.w0, &x.wt12, &x.wt3, &x.wt8, &x.wh};
        size_t at[6] = {0};
        for (int i = 0; i < 5; i++) at[i + 1] = at[i] + part[i]->size() * 2;
        unsigned char *d_x = (unsigned char *)e->x3.w0;
        if (!d_x || at[5] != e->x3_bytes) {
            if (dalloc(e, d_x, at[5] + 16, false)) return BB_ERR_HIP;
            e->x3_bytes = at[5];
        }
        for (int i = 0; i < 5; i++)
            if (upload(d_x + at[i], *part[i])) return BB_ERR_HIP;
        e->x3 = NetX3{d_x + at[0], d_x + at[1], d_x + at[2], d_x + at[3], d_x + at[4]};
    } else {
        e->x3 = NetX3{nullptr, nullptr, nullptr, nullptr, nullptr};
    }
    nd.R = R;
    nd.D = w->D;
    nd.A = w->A;
    nd.w0 = d_w0;
    nd.wt = (const f32x4 *)d_wt;
    nd.epi = d_epi;
    nd.head = d_head;
    nd.head_floats = (int)head.v.size();
    nd.off_vk = head.off_vk; nd.off_v3 = head.off_v3; nd.off_d1k = head.off_d1k; nd.off_d1b = head.off_d1b; nd.off_d2k = head.off_d2k;
    nd.off_d2b = head.off_d2b; nd.off_pk = head.off_pk; nd.off_p6 = head.off_p6; nd.off_pdk = head.off_pdk; nd.off_pdb = head.off_pdb;
    nd.seed = e->cfg.seed;
    nd.alpha = e->cfg.alpha;
    nd.eps = e->cfg.epsilon;
    nd.inv_alpha = 1.0f / nd.alpha;
    nd.inv_beta = 1.0f / (1.0f - nd.alpha);
    nd.dbg = 0; // (ablation switches exist in diagnostic builds only: bb_timing_net, stamps.hip.h)
    e->has_weights = true;
    e->net_F = F;
    e->net_C = C;
    return BB_OK;
}

// ---- weights that are in device memory already: pack on the device (net_pack.hip.h) into the buffers bb_load_weights made ----
static int load_weights_device(bb_engine *e, const bb_net_weights *w, hipStream_t stream, const char *who) {
    if (int rc = check_weights(w, e->info, who)) return rc;
    if (!e->has_weights || !e->net.w0 || !e->net.head)
        return fail(BB_ERR_STATE, "%s: the engine has no weight buffers yet -- its first load is bb_load_weights, which allocates them", who);
    if (e->general_net)
        return fail(BB_ERR_STATE, "%s covers the fused 16-filter tower; this engine runs its %d-filter network through the "
                    "launch-per-layer kernels", who, e->net_F);
    const bool want3 = w->C <= 32 && e->cfg.net_form != BB_NET_FORM_F32;
    if (w->F != 16 || e->net_F != 16 || w->C != e->net_C || w->R != e->net.R || w->D != e->net.D || w->A != e->net.A ||
        want3 != (e->x3.w0 != nullptr))
        return fail(BB_ERR_STATE, "%s: the engine's buffers hold a network of %d planes, %d filters, %d blocks, dense %d, %d actions "
                    "(%s); the weights given have %d, %d, %d, %d, %d", who, e->net_C, e->net_F, e->net.R, e->net.D, e->net.A,
                    e->x3.w0 ? "split form" : "float32 form", w->C, w->F, w->R, w->D, w->A);
    NetDev &nd = e->net;
    const NetHeadOff off = head_offsets(16, w->D, w->A);
    if (off.floats != nd.head_floats || (size_t)off.floats != e->net_sizes[3])
        return fail(BB_ERR_STATE, "%s: the head array holds %d floats, these weights need %d", who, nd.head_floats, off.floats);
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (dev != e->cfg.device)
        return fail(BB_ERR_ARG, "%s: the engine lives on device %d, the current device (the stream's and the weights') is %d", who,
                    e->cfg.device, dev);
    HIPCHK(sync_all(e)); // weights must not change under a running search: the engine's own streams only, never `stream`
    // behind whatever `stream` has queued (the steps that made these weights) ...
    HIPCHK(hipEventRecord(e->w_event[0], stream));
    HIPCHK(hipStreamWaitEvent(e->stream, e->w_event[0], 0));
    // ... no evaluation outlives the weights it was made with ...
    if (e->eval_cache_bytes) HIPCHK(hipMemsetAsync(e->dev.eval_cache, 0, e->eval_cache_bytes, e->stream));
    auto blocks = [](int threads) { return (unsigned)((threads + NET_PACK_THREADS - 1) / NET_PACK_THREADS); };
    k_pack_f32<<<blocks(pack_f32_threads(w->C, w->R)), NET_PACK_THREADS, 0, e->stream>>>(*w, (float *)nd.w0, (float *)nd.wt, (float *)nd.epi);
    k_pack_head<<<blocks(off.floats), NET_PACK_THREADS, 0, e->stream>>>(*w, off, (float *)nd.head);
    if (e->x3.w0)
        k_pack_x3<<<blocks(pack_x3_threads(w->C, w->R)), NET_PACK_THREADS, 0, e->stream>>>(
            *w, (uint16_t *)e->x3.w0, (uint16_t *)e->x3.wt12, (uint16_t *)e->x3.wt3, (uint16_t *)e->x3.wt8, (uint16_t *)e->x3.wh);
    HIPCHK(hipGetLastError());
    // ... and everything else waits for the images: the engine's second stream, and `stream` itself, so that the weights may be
    // freed or stepped on as soon as `stream` has come this far
    HIPCHK(hipEventRecord(e->w_event[1], e->stream));
    if (e->vstream[1]) HIPCHK(hipStreamWaitEvent(e->vstream[1], e->w_event[1], 0));
    HIPCHK(hipStreamWaitEvent(stream, e->w_event[1], 0));
    return BB_OK;
}

extern "C" int bb_load_weights_device(bb_engine *e, const bb_net_weights *w_dev, void *stream) {
    if (!e || !w_dev) return fail(BB_ERR_ARG, "null argument");
    return load_weights_device(e, w_dev, (hipStream_t)stream, "bb_load_weights_device");
}

extern "C" int bb_weights_read(bb_engine *e, int which, void *host_out, int64_t capacity, int64_t *bytes_out) {
    if (!e || (!host_out && !bytes_out)) return fail(BB_ERR_ARG, "null argument");
    if (which < BB_WEIGHTS_W0 || which > BB_WEIGHTS_X3) return fail(BB_ERR_ARG, "unknown image %d", which);
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    const void *src[5] = {e->net.w0, e->net.wt, e->net.epi, e->net.head, e->x3.w0};
    const int64_t bytes = which == BB_WEIGHTS_X3 ? (e->x3.w0 ? (int64_t)e->x3_bytes : 0) : (int64_t)(e->net_sizes[which] * sizeof(float));
    if (bytes_out) *bytes_out = bytes;
    if (!host_out) return BB_OK;
    if (capacity < bytes) return fail(BB_ERR_ARG, "image %d has %lld bytes, the buffer %lld", which, (long long)bytes, (long long)capacity);
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    if (bytes) HIPCHK(hipMemcpy(host_out, src[which], (size_t)bytes, hipMemcpyDeviceToHost));
    return BB_OK;
}

// positions per wave of the fused tower, chosen so that 4 waves' activations fill the 160 KiB LDS
template <class G> struct NetPW;
template <> struct NetPW<Connect4> { static constexpr int v = 4; };
template <> struct NetPW<TicTacToe> { static constexpr int v = 12; };
template <> struct NetPW<DragonChess> { static constexpr int v = 1; }; // 64 pixels = 4 full tiles; 1024 games fill 256 CUs

template <class G>
static int launch_net(bb_engine *e, int n, const typename G::State *states, const int8_t *planes,
                      const uint32_t *game_id, const int32_t *serial, int noise, float *value, float *logits,
                      float *policy, int pstride, hipStream_t st) {
    if (e->general_net)
        return launch_gnet<G>(e, n, nullptr, nullptr, states, planes, game_id, serial, noise, value, logits, policy, pstride, st);
    // positions per wave: the fewest that still put a wave on every SIMD (1024 waves) -- a single FindMove position
    // must not pay for the 11 MFMA tiles of a 4-position wave
    constexpr int PW = NetPW<G>::v;
    {
        if (e->x3.w0) { // one position per wave on the bf16 pipe: the same arithmetic everywhere (bb_net_eval, search, self-play)
            k_net_x3<G><<<(n + 3) / 4, 256, 0, st>>>(e->net, e->x3, n, nullptr, nullptr, states, planes, game_id, serial, noise, value,
                                                     logits, policy, pstride, EvalCache{nullptr, 0});
            HIPCHK(hipGetLastError());
            return BB_OK;
        }
    }
    if (PW > 1 && n <= 1024) {
        k_net_fused16<G, 1><<<(n + 3) / 4, 256, 0, st>>>(e->net, n, states, planes, game_id, serial, noise, value, logits, policy,
                                                         pstride);
    } else if (PW > 2 && n <= 2048) {
        k_net_fused16<G, 2><<<(n + 7) / 8, 256, 0, st>>>(e->net, n, states, planes, game_id, serial, noise, value, logits, policy,
                                                         pstride);
    } else {
        int blocks = (n + 4 * PW - 1) / (4 * PW);
        k_net_fused16<G, PW><<<blocks, 256, 0, st>>>(e->net, n, states, planes, game_id, serial, noise, value, logits,
                                                      policy, pstride);
    }
    HIPCHK(hipGetLastError());
    return BB_OK;
}

template <class G>
static int net_eval(bb_engine *e, int n, const void *states, const int8_t *planes, float *value, float *logits,
                    float *policy, int noise, const uint32_t *game_ids = nullptr, const int32_t *serials = nullptr) {
    const int A = G::A;
    size_t pb = (size_t)n * G::H * G::W * G::C;
    DevBuf din, dv, dl, dp, dg, dser;
    if (din.alloc(states ? (size_t)n * sizeof(typename G::State) : pb) || dv.alloc((size_t)n * 4) ||
        dl.alloc((size_t)n * A * 4) || dp.alloc((size_t)n * A * 4) || dg.alloc((size_t)n * 4) || dser.alloc((size_t)n * 4))
        return BB_ERR_HIP;
    HIPCHK(hipMemcpy(din.p, states ? states : (const void *)planes, states ? (size_t)n * sizeof(typename G::State) : pb,
                     hipMemcpyDefault));
    if (game_ids) HIPCHK(hipMemcpy(dg.p, game_ids, (size_t)n * 4, hipMemcpyDefault));
    if (serials) HIPCHK(hipMemcpy(dser.p, serials, (size_t)n * 4, hipMemcpyDefault));
    int rc = launch_net<G>(e, n, states ? (const typename G::State *)din.p : nullptr,
                           states ? nullptr : (const int8_t *)din.p, game_ids ? (const uint32_t *)dg.p : nullptr,
                           serials ? (const int32_t *)dser.p : nullptr, noise, (float *)dv.p,
                           (float *)dl.p, (float *)dp.p, A, e->stream);
    if (rc) return rc;
    HIPCHK(sync_all(e));
    if (value) HIPCHK(hipMemcpy(value, dv.p, (size_t)n * 4, hipMemcpyDefault));
    if (logits) HIPCHK(hipMemcpy(logits, dl.p, (size_t)n * A * 4, hipMemcpyDefault));
    if (policy) HIPCHK(hipMemcpy(policy, dp.p, (size_t)n * A * 4, hipMemcpyDefault));
    return BB_OK;
}

extern "C" int bb_net_eval(bb_engine *e, int n, const void *states, const int8_t *planes, float *value_out,
                           float *logits_out, float *policy_out, int noise) {
    if (e && n == 0) return BB_OK; // an empty batch is a no-op
    if (!e || n < 0 || (!states == !planes)) return fail(BB_ERR_ARG, "bad arguments (exactly one of states/planes)");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    HIPCHK(hipSetDevice(e->cfg.device));
    GAME_SWITCH(e->cfg.game, return net_eval<G>(e, n, states, planes, value_out, logits_out, policy_out, noise));
}

extern "C" int bb_net_eval_structure(bb_engine *e, int n, int32_t *out) {
    if (!e || !out || n < 0) return fail(BB_ERR_ARG, "bb_net_eval_structure: an engine, n >= 0 and a place for the answer");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    *out = !e->general_net ? BB_NET_EVAL_FUSED : gnet_small_launch(n, e->gnet.NCB, nullptr) ? BB_NET_EVAL_SMALL : BB_NET_EVAL_BATCH;
    return BB_OK;
}

extern "C" int bb_net_eval_keyed(bb_engine *e, int n, const void *states, const int8_t *planes, const uint32_t *game_ids,
                                 const int32_t *node_serials, float *value_out, float *logits_out, float *policy_out) {
    if (e && n == 0) return BB_OK;
    if (!e || n < 0 || (!states == !planes) || !game_ids || !node_serials)
        return fail(BB_ERR_ARG, "bad arguments (exactly one of states/planes; game_ids and node_serials are required)");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    HIPCHK(hipSetDevice(e->cfg.device));
    GAME_SWITCH(e->cfg.game, return net_eval<G>(e, n, states, planes, value_out, logits_out, policy_out, 1, game_ids, node_serials));
}

template <class G>
static int hash_eval(bb_engine *e, int n, const void *states, float *value, float *policy) {
    DevBuf ds, dv, dp;
    if (ds.alloc((size_t)n * sizeof(typename G::State)) || dv.alloc((size_t)n * 4) || dp.alloc((size_t)n * G::A * 4))
        return BB_ERR_HIP;
    HIPCHK(hipMemcpy(ds.p, states, (size_t)n * sizeof(typename G::State), hipMemcpyDefault));
    Launch<G>::hash(e->stream, n, (const typename G::State *)ds.p, nullptr, e->cfg.hash_salt, 0, 0, (float *)dv.p, (float *)dp.p, G::A);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_all(e));
    if (value) HIPCHK(hipMemcpy(value, dv.p, (size_t)n * 4, hipMemcpyDefault));
    if (policy) HIPCHK(hipMemcpy(policy, dp.p, (size_t)n * G::A * 4, hipMemcpyDefault));
    return BB_OK;
}

extern "C" int bb_hash_eval(bb_engine *e, int n, const void *states, float *value_out, float *policy_out) {
    if (e && n == 0) return BB_OK;
    if (!e || n < 0 || !states) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    GAME_SWITCH(e->cfg.game, return hash_eval<G>(e, n, states, value_out, policy_out));
}

// ---- simulation loop ---------------------------------------------------------------------------------
// bb_timing_enable: `launch` between a pair of HIP events on `st` while the pool has one left: every time_every-th of the evaluator
// launches (the rounds count their first view's only and never time the second's), each of the persistent launches.
enum { TIME_NEVER, TIME_SAMPLED, TIME_EACH };
template <class F>
static int timed_launch(bb_engine *e, hipStream_t st, int which, F launch) {
    const bool timed = which != TIME_NEVER && e->time_every > 0 &&
                       (which == TIME_EACH || (e->eval_launches++ % (uint64_t)e->time_every) == 0) && e->ev_used + 2 <= e->ev_pool.size();
    if (timed) HIPCHK(hipEventRecord(e->ev_pool[e->ev_used], st));
    if (int rc = launch()) return rc;
    if (timed) {
        HIPCHK(hipEventRecord(e->ev_pool[e->ev_used + 1], st));
        e->ev_used += 2;
    }
    return BB_OK;
}

template <class G>
static int launch_eval_inner(bb_engine *e) {
    TreeDev &d = e->dev;
    int n = d.n_slots;
    const typename G::State *ls = (const typename G::State *)d.leaf_state;
    constexpr bool DC = G::GID == BB_GAME_DRAGONCHESS;
    constexpr int PS = DC ? G::A : G::S; // floats of a slot's eval_policy row (SLOT_EXTENTS)
    switch (d.evaluator) {
    case BB_EVAL_HASH:
        Launch<G>::hash(e->stream, n, ls, d.leaf_game_id, d.salt, d.salt_per_game, d.first_game_id, d.eval_value, d.eval_policy, PS);
        break;
    case BB_EVAL_NET:
        // (a wide game's prior noise is mixed in at expansion, over the legal moves only: tree_dc.hip.h)
        return launch_net<G>(e, n, ls, nullptr, d.leaf_game_id, d.leaf_serial, DC ? 0 : e->cfg.noise_on, d.eval_value, nullptr, d.eval_policy,
                             PS, e->stream);
    case BB_EVAL_ROLLOUT: Launch<G>::rollout(d, e->edges, e->stream); break;
    default: return fail(BB_ERR_ARG, "unknown evaluator %d", d.evaluator);
    }
    HIPCHK(hipGetLastError());
    return BB_OK;
}

template <class G>
static int launch_eval(bb_engine *e) { return timed_launch(e, e->stream, TIME_SAMPLED, [&] { return launch_eval_inner<G>(e); }); }

template <class G>
static int run_sims(bb_engine *e, int sims) {
    for (int s = 0; s < sims; s++) {
        Launch<G>::tree_step(e->dev, e->edges, e->stream);
        HIPCHK(hipGetLastError());
        if (int rc = launch_eval<G>(e)) return rc;
    }
    return BB_OK;
}

static int check_eval(bb_engine *e) {
    if (e->cfg.evaluator == BB_EVAL_NET && !e->has_weights)
        return fail(BB_ERR_WEIGHTS, "network evaluator needs bb_load_weights first");
    return BB_OK;
}

template <class G>
static int set_roots(bb_engine *e, int n, const int32_t *slots, const void *states, const uint32_t *gids) {
    DevBuf ds, dsl, dg;
    if (ds.alloc((size_t)n * sizeof(typename G::State)) || dsl.alloc((size_t)n * 4) || dg.alloc((size_t)n * 4))
        return BB_ERR_HIP;
    HIPCHK(hipMemcpy(ds.p, states, (size_t)n * sizeof(typename G::State), hipMemcpyDefault));
    if (slots) HIPCHK(hipMemcpy(dsl.p, slots, (size_t)n * 4, hipMemcpyDefault));
    if (gids) HIPCHK(hipMemcpy(dg.p, gids, (size_t)n * 4, hipMemcpyDefault));
    Launch<G>::set_roots(e->dev, e->edges, e->stream, n, slots ? (const int32_t *)dsl.p : nullptr, (const typename G::State *)ds.p,
                         gids ? (const uint32_t *)dg.p : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_all(e));
    return BB_OK;
}

extern "C" int bb_set_roots(bb_engine *e, int n, const int32_t *slots, const void *states, const uint32_t *game_ids) {
    if (!e || n <= 0 || n > e->cfg.n_slots || !states) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    GAME_SWITCH(e->cfg.game, return set_roots<G>(e, n, slots, states, game_ids));
}

// The structure bb_run_sims / bb_run_sims_masked search through at this moment -- the ONE place that reads launch / game / evaluator /
// the loaded network for this: BB_LAUNCH_WAVE where the engine asked for it and a one-launch kernel exists for what it is (a dense
// game with the hash evaluator, or any game with a 16-filter network in the split-operand form -- for DragonChess one that also fits
// k_dc_search_wave's LDS, the test selfplay_structure applies to the self-play kernel), else the lock-step loop.
// The rollout evaluator has a one-launch kernel for every game and is sent there only after bb_search_rollouts(e, 1).
// bb_run_sims_structure reports it, so an engine that asked and was refused is visible.
static int search_structure(const bb_engine *e) {
    if (e->cfg.launch != BB_LAUNCH_WAVE) return BB_LAUNCH_LOCKSTEP;
    const bool dc = e->cfg.game == BB_GAME_DRAGONCHESS;
    if (e->cfg.evaluator == BB_EVAL_HASH && !dc) return BB_LAUNCH_WAVE;
    if (e->cfg.evaluator == BB_EVAL_ROLLOUT && e->search_rollouts) return BB_LAUNCH_WAVE; // (every game, both mcts_kinds)
    if (e->cfg.evaluator == BB_EVAL_NET && e->has_weights && !e->general_net && e->x3.w0 &&
        (!dc || (e->net.R <= DC_RMAX && e->net.head_floats <= DC_HEAD_FLOATS)))
        return BB_LAUNCH_WAVE;
    return BB_LAUNCH_LOCKSTEP;
}

extern "C" int bb_search_rollouts(bb_engine *e, int on) {
    if (!e || (on != 0 && on != 1)) return fail(BB_ERR_ARG, "bb_search_rollouts: an engine and 0 or 1");
    e->search_rollouts = on != 0; // (read by search_structure, for BB_EVAL_ROLLOUT engines only)
    return BB_OK;
}

extern "C" int bb_run_sims_structure(bb_engine *e, int32_t *out) {
    if (!e || !out) return fail(BB_ERR_ARG, "null argument");
    if (int rc = check_eval(e)) return rc;
    *out = search_structure(e);
    return BB_OK;
}

// `sims` more simulations on the slots of `dev_mask` (DEVICE memory, [n_slots]; null: every active slot), through the structure
// search_structure names: launches on the engine's stream only -- no allocation, no synchronisation.  (The caller has checked the
// evaluator and set the device.)
static int enqueue_sims(bb_engine *e, int sims, const uint8_t *dev_mask) {
    int rc = BB_OK;
    k_add_sims<<<nblk(e->dev.n_slots), 256, 0, e->stream>>>(e->dev, sims, dev_mask);
    const bool wave = search_structure(e) == BB_LAUNCH_WAVE;
    GAME_SWITCH(e->cfg.game, {
        if (wave) { // every simulation of every slot, and the last leaf's apply, in one launch
            const bool net = e->cfg.evaluator == BB_EVAL_NET;
            rc = timed_launch(e, e->stream, TIME_EACH, [&]() -> int {
                if (!Launch<G>::search_wave(e->dev, e->edges, e->stream, sims, e->net, net ? e->x3 : NetX3{nullptr, nullptr, nullptr, nullptr, nullptr}, e->cfg.noise_on,
                                            e->cfg.search_cache != 0))
                    return fail(BB_ERR_STATE, "no one-launch search for this game");
                return BB_OK;
            });
            if (rc) return rc;
        } else {
            rc = run_sims<G>(e, sims);
            if (rc) return rc;
            Launch<G>::tree_apply(e->dev, e->edges, e->stream);
        }
        HIPCHK(hipGetLastError());
        return BB_OK;
    });
}

static int run_sims_api(bb_engine *e, int sims, const uint8_t *mask) {
    if (!e || sims <= 0) return fail(BB_ERR_ARG, "Not enough information to decide a stop time."); // MCTS.py:181-182
    int rc = check_eval(e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->cfg.device));
    DevBuf dm;
    if (mask) {
        if (dm.alloc((size_t)e->dev.n_slots)) return BB_ERR_HIP;
        HIPCHK(hipMemcpyAsync(dm.p, mask, (size_t)e->dev.n_slots, hipMemcpyDefault, e->stream));
    }
    rc = enqueue_sims(e, sims, mask ? (const uint8_t *)dm.p : nullptr);
    if (rc) return rc;
    if (mask) HIPCHK(sync_all(e)); // the mask buffer is freed on return
    return BB_OK;
}

extern "C" int bb_run_sims(bb_engine *e, int sims) { return run_sims_api(e, sims, nullptr); }

extern "C" int bb_run_sims_masked(bb_engine *e, int sims, const uint8_t *mask) {
    if (!mask) return fail(BB_ERR_ARG, "null mask");
    return run_sims_api(e, sims, mask);
}

template <class G>
static int sample_moves(bb_engine *e, double temp, const double *u, int32_t *action, float *wr, int32_t *rp,
                        int32_t *cact, int32_t *cplays, float *cval) {
    TreeDev d = e->dev;
    size_t n = (size_t)d.n_slots;
    if (u) HIPCHK(hipMemcpyAsync(e->d_u, u, n * 8, hipMemcpyDefault, e->stream));
    d.in_u = u ? e->d_u : nullptr;
    Launch<G>::sample(d, e->edges, e->stream, temp, e->d_child_action);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_all(e));
    if (action) HIPCHK(hipMemcpy(action, d.out_action, n * 4, hipMemcpyDefault));
    if (wr) HIPCHK(hipMemcpy(wr, d.out_root_winrate, n * 4, hipMemcpyDefault));
    if (rp) HIPCHK(hipMemcpy(rp, d.out_root_plays, n * 4, hipMemcpyDefault));
    if (cplays) HIPCHK(hipMemcpy(cplays, d.out_child_plays, n * G::S * 4, hipMemcpyDefault));
    if (cval) HIPCHK(hipMemcpy(cval, d.out_child_value, n * G::S * 4, hipMemcpyDefault));
    if constexpr (G::GID == BB_GAME_DRAGONCHESS) { // its kernel lists the actions of the root's edges
        if (cact) HIPCHK(hipMemcpy(cact, e->d_child_action, n * G::S * 4, hipMemcpyDefault));
    } else if (cact) { // dense games: slot i is action i
        std::vector<int32_t> ca(n * G::S);
        for (size_t g = 0; g < n; g++)
            for (int i = 0; i < G::S; i++) ca[g * G::S + i] = i < G::A ? i : -1;
        HIPCHK(hipMemcpy(cact, ca.data(), ca.size() * 4, hipMemcpyDefault));
    }
    return BB_OK;
}

extern "C" int bb_sample_moves(bb_engine *e, double temp, const double *u, int32_t *action_out,
                               float *root_winrate_out, int32_t *root_plays_out, int32_t *child_action_out,
                               int32_t *child_plays_out, float *child_value_out) {
    if (!e || temp < 0) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    GAME_SWITCH(e->cfg.game, return sample_moves<G>(e, temp, u, action_out, root_winrate_out, root_plays_out,
                                                    child_action_out, child_plays_out, child_value_out));
}

extern "C" int bb_move_roots(bb_engine *e, const int32_t *actions) {
    if (!e || !actions) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipMemcpyAsync(e->d_actions, actions, (size_t)e->dev.n_slots * 4, hipMemcpyDefault, e->stream));
    GAME_SWITCH(e->cfg.game, {
        Launch<G>::move_roots(e->dev, e->edges, e->stream, e->d_actions);
        HIPCHK(hipGetLastError());
        HIPCHK(sync_all(e));
        return BB_OK;
    });
}

extern "C" int bb_reset_roots(bb_engine *e) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    if (!e->dev.track_anc) return fail(BB_ERR_STATE, "this engine does not keep the ancestors of its roots (bb_config.track_ancestors)");
    HIPCHK(hipSetDevice(e->cfg.device));
    if (e->cfg.game == BB_GAME_DRAGONCHESS) {
        // a slot whose chain outgrew its max_plies + 2 entries cannot find its top-most ancestor (tree_dc.hip.h DC_ANC_BROKEN)
        std::vector<int32_t> na((size_t)e->dev.n_slots);
        HIPCHK(sync_all(e));
        HIPCHK(hipMemcpy(na.data(), e->dev.anc_len, na.size() * 4, hipMemcpyDeviceToHost));
        for (size_t g = 0; g < na.size(); g++)
            if (na[g] < 0)
                return fail(BB_ERR_CAPACITY, "slot %zu moved its root more than max_plies + 2 times (max_plies %d) since the tree "
                                             "was primed: its ancestors were not all kept", g, e->cfg.max_plies);
    }
    GAME_SWITCH(e->cfg.game, {
        Launch<G>::reset_roots(e->dev, e->edges, e->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(sync_all(e));
        return BB_OK;
    });
}

// One node of a slot's tree, staged on the device and copied out; action_out only where the family's kernel lists actions
template <class G>
static int node_fetch(bb_engine *e, int slot, int node, int32_t *action_out, int32_t *child_node_out, int32_t *child_plays_out,
                      float *child_value_out, void *state_out, int32_t *info_out) {
    constexpr int S = G::S;
    DevBuf da, dc, dp, dv, ds, di;
    if ((action_out && da.alloc(S * 4)) || dc.alloc(S * 4) || dp.alloc(S * 4) || dv.alloc(S * 4) || ds.alloc(sizeof(typename G::State)) || di.alloc(16))
        return BB_ERR_HIP;
    Launch<G>::node_edges(e->dev, e->edges, e->stream, slot, node, (int32_t *)da.p, (int32_t *)dc.p, (int32_t *)dp.p, (float *)dv.p,
                          (typename G::State *)ds.p, (int32_t *)di.p);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_all(e));
    HIPCHK(hipMemcpy(child_node_out, dc.p, S * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(child_plays_out, dp.p, S * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(child_value_out, dv.p, S * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(state_out, ds.p, sizeof(typename G::State), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(info_out, di.p, 12, hipMemcpyDeviceToHost));
    if (action_out) HIPCHK(hipMemcpy(action_out, da.p, S * 4, hipMemcpyDeviceToHost));
    return BB_OK;
}

extern "C" int bb_node_view(bb_engine *e, int slot, int node, int32_t *child_node_out, int32_t *child_plays_out, float *child_value_out,
                            void *state_out, int32_t *info_out) {
    if (!e || slot < 0 || slot >= e->cfg.n_slots || !child_node_out || !child_plays_out || !child_value_out || !state_out || !info_out)
        return fail(BB_ERR_ARG, "bad arguments");
    if (node >= e->dev.node_cap) return fail(BB_ERR_ARG, "node %d out of range", node);
    HIPCHK(hipSetDevice(e->cfg.device));
    if (e->cfg.game == BB_GAME_DRAGONCHESS) return fail(BB_ERR_ARG, "node views exist for the dense-action games");
    HIPCHK(sync_all(e));
    GAME_SWITCH(e->cfg.game, return node_fetch<G>(e, slot, node, nullptr, child_node_out, child_plays_out, child_value_out, state_out, info_out));
}

extern "C" int bb_node_edges(bb_engine *e, int slot, int node, int32_t *child_action_out, int32_t *child_node_out,
                             int32_t *child_plays_out, float *child_value_out, void *state_out, int32_t *info_out) {
    if (!e || slot < 0 || slot >= e->cfg.n_slots || !child_action_out || !child_node_out || !child_plays_out || !child_value_out ||
        !state_out || !info_out)
        return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    int32_t nn = 0;
    HIPCHK(hipMemcpy(&nn, e->dev.n_nodes + slot, 4, hipMemcpyDeviceToHost));
    if (node >= nn) return fail(BB_ERR_ARG, "node %d is not in slot %d's tree (%d nodes)", node, slot, nn);
    GAME_SWITCH(e->cfg.game, {
        constexpr bool DC = G::GID == BB_GAME_DRAGONCHESS;
        if (int rc = node_fetch<G>(e, slot, node, DC ? child_action_out : nullptr, child_node_out, child_plays_out, child_value_out, state_out, info_out))
            return rc;
        if constexpr (!DC) { // slot i is action i; the node view's info word 1 is the legal mask
            const uint32_t legal = (uint32_t)info_out[1];
            int cnt = 0;
            for (int i = 0; i < G::S; i++) {
                const bool on = i < G::A && ((legal >> i) & 1u);
                child_action_out[i] = on ? i : -1;
                if (!on) {
                    child_node_out[i] = CHILD_NONE;
                    child_plays_out[i] = 0;
                    child_value_out[i] = 0.f;
                }
                cnt += on;
            }
            info_out[1] = cnt;
        }
        return BB_OK;
    });
}

extern "C" int bb_get_root_states(bb_engine *e, void *states_out) {
    if (!e || !states_out) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    GAME_SWITCH(e->cfg.game, {
        DevBuf ds;
        size_t bytes = (size_t)e->dev.n_slots * sizeof(typename G::State);
        if (ds.alloc(bytes)) return BB_ERR_HIP;
        Launch<G>::get_roots(e->dev, e->edges, e->stream, (typename G::State *)ds.p);
        HIPCHK(hipGetLastError());
        HIPCHK(sync_all(e));
        HIPCHK(hipMemcpy(states_out, ds.p, bytes, hipMemcpyDefault));
        return BB_OK;
    });
}

extern "C" int bb_set_sims_per_move(bb_engine *e, int sims) {
    if (!e || sims <= 0) return fail(BB_ERR_ARG, "bad arguments");
    long need = (long)sims * e->cfg.max_plies + 2;
    if (e->cfg.node_capacity <= 0 && sims > e->cfg.sims_per_move && need > e->dev.node_cap)
        return fail(BB_ERR_CAPACITY, "node pool was sized for %d simulations per move", e->cfg.sims_per_move);
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    e->sims_now = sims;
    e->dev.sims_per_move = sims;
    for (int v = 0; v < e->n_views; v++) e->view[v].sims_per_move = sims;
    k_add_sims<<<nblk(e->dev.n_slots), 256, 0, e->stream>>>(e->dev, sims); // slots waiting for their next move
    HIPCHK(hipGetLastError());
    HIPCHK(sync_all(e));
    return BB_OK;
}

extern "C" int bb_set_rng_stream(bb_engine *e, uint64_t seed, uint32_t first_game_id) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    e->cfg.seed = seed;
    e->cfg.first_game_id = first_game_id;
    e->dev.seed = seed;
    e->dev.first_game_id = first_game_id;
    for (int v = 0; v < 2; v++) {
        e->view[v].seed = seed;
        e->view[v].first_game_id = first_game_id;
    }
    e->net.seed = seed;
    return BB_OK;
}

// ---- self-play ----------------------------------------------------------------------------------------
// The device side of starts_replace (starts.h) for one engine; the checks run on the engine's stream
template <class G>
static StartsOps starts_ops(bb_engine *e) {
    StartsOps ops;
    ops.ctx = e;
    ops.alloc = [](void *, size_t bytes, void **out) -> int {
        const hipError_t r = hipMalloc(out, bytes);
        if (r != hipSuccess) (void)hipGetLastError();
        return r == hipSuccess ? 0 : r == hipErrorOutOfMemory ? 1 : 2;
    };
    ops.upload = [](void *, void *dst, const void *src, size_t bytes) -> int { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess; };
    ops.check = [](void *ctx, const void *dev_states, int n, uint8_t *verdict_out) -> int {
        bb_engine *en = (bb_engine *)ctx;
        DevBuf dv;
        if (dv.alloc((size_t)n)) return 1;
        Launch<G>::check_starts(en->stream, n, (const typename G::State *)dev_states, (uint8_t *)dv.p);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(en->stream) != hipSuccess) return 1;
        return hipMemcpy(verdict_out, dv.p, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess;
    };
    ops.release = [](void *, void *p) { (void)hipFree(p); };
    return ops;
}

extern "C" int bb_selfplay_set_starts(bb_engine *e, int n, const void *states) {
    char msg[384];
    if (starts_check_args(e != nullptr, n, states, msg, sizeof msg)) return fail(BB_ERR_ARG, "%s", msg);
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e)); // between runs only: nothing of the engine is in flight when the table changes
    int rc = STARTS_DONE;
    GAME_SWITCH(e->cfg.game, rc = starts_replace(e->starts, n, states, sizeof(typename G::State), starts_ops<G>(e), msg, sizeof msg); break);
    switch (rc) {
    case STARTS_DONE: break;
    case STARTS_REFUSED: return fail(BB_ERR_ARG, "%s", msg);
    case STARTS_NO_FIT: return fail(BB_ERR_CAPACITY, "%s", msg);
    default: return fail(BB_ERR_HIP, "%s", msg);
    }
    e->dev.starts = e->starts.dev;
    e->dev.n_starts = e->starts.n;
    for (int v = 0; v < 2; v++) {
        e->view[v].starts = e->starts.dev;
        e->view[v].n_starts = e->starts.n;
    }
    return BB_OK;
}

extern "C" int bb_selfplay_begin(bb_engine *e, int n_games, double temp) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    if (n_games <= 0) return fail(BB_ERR_ARG, "Use a positive integer for number of games."); // Blackbird.py:235-236
    if (e->dev.track_anc && e->cfg.game == BB_GAME_DRAGONCHESS) // (its self-play kernels do not keep the chain)
        return fail(BB_ERR_STATE, "DragonChess self-play does not keep ancestor chains: create the engine without track_ancestors");
    if (n_games > e->cfg.max_games)
        return fail(BB_ERR_CAPACITY, "n_games %d exceeds the engine's max_games %d", n_games, e->cfg.max_games);
    if (e->sims_now < 2 && temp != 0.0)
        return fail(BB_ERR_NAN, "probabilities contain NaN (a fresh root needs >= 2 simulations, MCTS.py:336-338)");
    int rc = check_eval(e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->cfg.device));
    e->n_games_target = n_games;
    e->dev.n_games_target = n_games;
    e->dev.temp = temp;
    HIPCHK(sync_all(e));
    HIPCHK(hipMemsetAsync(e->dev.game_hdr, 0, (size_t)e->cfg.max_games * 16, e->stream));
    HIPCHK(hipMemsetAsync(e->dev.resume_cur, 0xFF, (size_t)e->dev.n_slots * 4, e->stream));
    HIPCHK(hipMemsetAsync(e->dev.post_count, 0, 8 * sizeof(int), e->stream));
    if (e->miss_count) HIPCHK(hipMemsetAsync(e->miss_count, 0, 8 * sizeof(int), e->stream));
    HIPCHK(sync_all(e));
    e->vround[0] = e->vround[1] = 0;
    e->miss_next[0] = e->miss_next[1] = 0;
    GAME_SWITCH(e->cfg.game, {
        if constexpr (G::GID == BB_GAME_DRAGONCHESS) { // one view (make_views), never played through the rounds
            Launch<G>::selfplay_begin(e->dev, e->edges, e->stream);
        } else {
            for (int v = 0; v < e->n_views; v++) {
                e->view[v].n_games_target = n_games;
                e->view[v].temp = temp;
                e->view[v].sims_per_move = e->sims_now;
                Launch<G>::selfplay_begin(e->view[v], e->edges, e->vstream[v]);
            }
        }
        HIPCHK(hipGetLastError());
        return BB_OK;
    });
}

__global__ void k_set_i32(int *p, int v) { *p = v; }

// A persistent launch's visits, per_slot each: 7/8 dealt to the slots (returned), the rest pooled (mega2.hip.h, mega_dc.hip.h)
static int deal_visits(bb_engine *e, int per_slot) {
    const int own = per_slot - (per_slot + 7) / 8;
    k_set_i32<<<1, 1, 0, e->stream>>>(e->dev.visit_pool, e->dev.n_slots * (per_slot - own));
    return own;
}

// PLAY_QUEUE: persistent launches of at most 64 steps' worth of visits (3 s at 4096 Connect4 games x 800 visits): every spin
// loop inside is bounded by BB_QUEUE_LIMIT_S of wall clock (30 s), so a launch must stay far below it whatever the caller asks
// for.  Not shorter either: a launch ends when its SLOWEST workgroup is done, ~35 ms after the fastest: 4 % of 16 steps.
template <class G>
static int selfplay_queue(bb_engine *e, int visits) {
    const TreeDev &d = e->dev;
    const int nb = (d.n_slots + 15) / 16;
    int per_launch = e->tune.launch_steps * (e->sims_now > 0 ? e->sims_now : 1);
    if (per_launch > (1 << 30) / d.n_slots) per_launch = (1 << 30) / d.n_slots; // the launch's visit pool is an int
    for (int done = 0; done < visits; done += per_launch) {
        const int now = visits - done < per_launch ? visits - done : per_launch;
        if (int rc = timed_launch(e, e->stream, TIME_EACH, [&]() -> int {
            TreeDev dm = d;
            // tree levels per call: 10 / 12 / 16 / 20 / 24 -> 155.6 / 155.8 / 153.6 / 151.6 / 151.2 M sims/s (Connect4 @800, bf16-pipe network)
            if (!e->tune.level_budget_set) dm.level_budget = 12;
            const int own = deal_visits(e, now), lim = e->tune.queue_limit_s;
            if (e->x3.w0) { // bf16-pipe network: Connect4 8 network + 4 tree waves (168 VGPRs), TicTacToe 4 + 4 waves
                if constexpr (G::S <= 8) k_selfplay_queue<G, 8, true, 12><<<nb, 768, 0, e->stream>>>(dm, e->net, e->x3, e->cfg.noise_on, lim, own);
                else k_selfplay_queue<G, 4, true, 8><<<nb, 512, 0, e->stream>>>(dm, e->net, e->x3, e->cfg.noise_on, lim, own);
            } else { // float32-MFMA network: 8 network + 4 tree waves
                k_selfplay_queue<G, 8><<<nb, 768, 0, e->stream>>>(dm, e->net, e->x3, e->cfg.noise_on, lim, own);
            }
            HIPCHK(hipGetLastError());
            return BB_OK;
        })) return rc;
    }
    return BB_OK;
}

// PLAY_DC_FUSED: at most 64 plies' worth of simulations per launch (a launch is plies x sims x ~45 us long; nothing inside can
// spin); the waves draw them from one pool (mega_dc.hip.h)
static int selfplay_dc_fused(bb_engine *e, int plies) {
    int cap = 64;
    if ((long)cap * e->sims_now * e->dev.n_slots > (1l << 30)) cap = (int)((1l << 30) / ((long)e->sims_now * e->dev.n_slots));
    if (cap < 1) cap = 1;
    for (int done = 0; done < plies; done += cap) {
        const int now = plies - done < cap ? plies - done : cap;
        if (int rc = timed_launch(e, e->stream, TIME_EACH, [&]() -> int {
            const int own = deal_visits(e, now * e->sims_now);
            k_dc_selfplay_fused<<<nblk((size_t)e->dev.n_slots * 64), 256, 0, e->stream>>>(e->dev, e->edges, e->net, e->x3, e->cfg.noise_on, own);
            HIPCHK(hipGetLastError());
            return BB_OK;
        })) return rc;
    }
    return BB_OK;
}

// PLAY_WAVE_ROLLOUT: nothing inside the kernel waits, so a launch is as long as its slowest slot's simulations, and the host bounds
// those: at most `cap` simulations per slot and launch.  The figures are the measured costs of one simulation of a slot whose wave
// runs alone on its SIMD (README): about 19 us for Connect4 Fixed-10 (15.8 ms per 800, TicTacToe is cheaper)
// and about 4.3 ms for a DragonChess Dynamic simulation, nearly all of it the playout (1735 ms per 400).  65536 dense simulations
// are then about 1.2 s, 512 DragonChess simulations about 2.2 s: launches in the low seconds -- up to twice that where two waves share a SIMD, and
// the figure shrinks with the slot count beyond what the device holds at once (below) --, far below any watchdog and long enough that the launch cost (~10 us) is nothing.  Whole plies per launch
// where a ply fits (cap / sims_now of them); a ply of more simulations than the cap is cut into launches of `cap` steps without
// the move (move = 0: the leaf stays pending between them as it does between lock-step launches) and a last one with it.  Per
// slot the sequence of operations is the same wherever the cuts fall, so the split cannot change a result.
template <class G>
static int selfplay_wave_rollout(bb_engine *e, int plies) {
    const int sims = e->sims_now;
    // (a full device holds 2 waves per SIMD of either kernel -- 186 / 214 VGPRs -- that is 2048 slots on 256 CUs; more slots run one
    // after another inside the launch, so the figure is divided by the number of such rounds)
    const int rounds = (e->dev.n_slots + 2047) / 2048;
    const int dflt = (G::GID == BB_GAME_DRAGONCHESS ? 512 : 65536) / rounds;
    const int cap = e->tune.wave_rollout_sims > 0 ? e->tune.wave_rollout_sims : dflt > 0 ? dflt : 1;
    auto launch = [&](int n_plies, int n_sims, int move) {
        return timed_launch(e, e->stream, TIME_EACH, [&]() -> int {
            Launch<G>::selfplay_wave_rollout(e->dev, e->edges, e->stream, n_plies, n_sims, move);
            HIPCHK(hipGetLastError());
            return BB_OK;
        });
    };
    if (sims > cap) { // a ply is longer than a launch
        for (int p = 0; p < plies; p++)
            for (int done = 0; done < sims; done += cap) {
                const int now = sims - done < cap ? sims - done : cap;
                if (int rc = launch(1, now, done + now == sims)) return rc;
            }
        return BB_OK;
    }
    const int per_launch = cap / (sims > 0 ? sims : 1);
    for (int done = 0; done < plies; done += per_launch)
        if (int rc = launch(plies - done < per_launch ? plies - done : per_launch, sims, 1)) return rc;
    return BB_OK;
}

// PLAY_ROUNDS: per view, k_tree_async and then the evaluator over the leaves it posted
template <class G>
static int selfplay_rounds_async(bb_engine *e, int rounds) {
    constexpr int PWMAX = NetPW<G>::v;
    for (int r = 0; r < rounds; r++) {
        for (int v = 0; v < e->n_views; v++) {
            TreeDev &d = e->view[v];
            hipStream_t st = e->vstream[v];
            int tb = nblk((size_t)((d.n_slots + d.gpw - 1) / d.gpw) * 64);
            int nb = (d.n_slots + 4 * PWMAX - 1) / (4 * PWMAX);
            if (e->n_views == 2) nb = 256 > nb ? 256 : nb; // spread a half batch over every CU (pw <= 2)
            int round = e->vround[v]++;
            k_tree_async<G><<<tb, 256, 0, st>>>(d, round);
            HIPCHK(hipGetLastError());
            const typename G::State *ls = (const typename G::State *)d.leaf_state;
            if (d.evaluator != BB_EVAL_NET) { // validation evaluator over every slot's mailbox of the view
                k_hash_eval<G><<<nblk(d.n_slots), 256, 0, st>>>(d.n_slots, ls, d.leaf_game_id, d.salt, d.salt_per_game,
                                                                d.first_game_id, d.eval_value, d.eval_policy, G::S);
                HIPCHK(hipGetLastError());
                continue;
            }
            if (int rc = timed_launch(e, st, v == 0 ? TIME_SAMPLED : TIME_NEVER, [&]() -> int { // (the first view's launches only, as ever)
                // the round's batch: the posted leaves -- or, with the evaluation cache, those of them that the probe kernel
                // did not answer from the table (eval_probe.hip.h); the heads of these store their entries
                const int *n_ptr = d.post_count + (round & 3), *slot_list = d.post_slot;
                EvalCache store = {nullptr, 0};
                if constexpr (G::CACHE_KEY) {
                    if (d.eval_cache && e->miss_count && e->general_net) {
                        store = {(u32x4 *)d.eval_cache, d.eval_cache_log2, e->miss_way + d.slot_offset};
                        int *mc = e->miss_count + 4 * v, *ms = e->miss_slot + d.slot_offset;
                        if (e->miss_next[v] != round) // (weights of the other kind were loaded in between: unprobed rounds)
                            HIPCHK(hipMemsetAsync(mc, 0, 4 * sizeof(int), st));
                        e->miss_next[v] = round + 1;
                        k_eval_cache_probe<G><<<(d.n_slots + 3) / 4, 256, 0, st>>>(e->net, store, n_ptr, slot_list, mc, round, ms,
                                                                                   e->miss_way + d.slot_offset, ls, d.leaf_game_id,
                                                                                   d.leaf_serial, e->cfg.noise_on, d.eval_value,
                                                                                   d.eval_policy, G::S, d.evals, d.eval_cache_ctr);
                        n_ptr = mc + (round & 3);
                        slot_list = ms;
                    }
                }
                if (e->general_net) {
                    if (int rc = launch_gnet<G>(e, d.n_slots, n_ptr, slot_list, ls, nullptr, d.leaf_game_id, d.leaf_serial, e->cfg.noise_on,
                                                d.eval_value, nullptr, d.eval_policy, G::S, st, d.slot_offset, store)) return rc;
                } else if (e->x3.w0) {
                    if constexpr (G::C <= 4)
                        k_net_x3<G><<<(d.n_slots + 3) / 4, 256, 0, st>>>(e->net, e->x3, 0, n_ptr, slot_list, ls, nullptr, d.leaf_game_id,
                                                                          d.leaf_serial, e->cfg.noise_on, d.eval_value, nullptr,
                                                                          d.eval_policy, G::S, store);
                } else {
                    k_net_compact<G, PWMAX><<<nb, 256, 0, st>>>(e->net, n_ptr, slot_list, ls, d.leaf_game_id, d.leaf_serial,
                                                                 e->cfg.noise_on, d.eval_value, d.eval_policy, G::S, store);
                }
                HIPCHK(hipGetLastError());
                return BB_OK;
            })) return rc;
        }
    }
    return BB_OK;
}

extern "C" int bb_selfplay_step(bb_engine *e, int plies) {
    if (!e || plies <= 0) return fail(BB_ERR_ARG, "bad arguments");
    if (e->n_games_target <= 0) return fail(BB_ERR_ARG, "bb_selfplay_begin has not been called");
    HIPCHK(hipSetDevice(e->cfg.device));
    GAME_SWITCH(e->cfg.game, {
        constexpr bool DC = G::GID == BB_GAME_DRAGONCHESS; // (selfplay_plan gives each game its own structures only)
        const int mode = selfplay_structure(e);
        if (mode == PLAY_WAVE_ROLLOUT) return selfplay_wave_rollout<G>(e, plies);
        if constexpr (DC) {
            if (mode == PLAY_DC_FUSED) return selfplay_dc_fused(e, plies);
        } else if (mode == PLAY_QUEUE || mode == PLAY_ROUNDS) {
            return mode == PLAY_QUEUE ? selfplay_queue<G>(e, plies * e->sims_now) : selfplay_rounds_async<G>(e, plies * e->sims_now);
        }
        for (int p = 0; p < plies; p++) { // PLAY_LOCKSTEP
            if (int rc = run_sims<G>(e, e->sims_now)) return rc;
            Launch<G>::selfplay_move(e->dev, e->edges, e->stream);
            HIPCHK(hipGetLastError());
        }
        return BB_OK;
    });
}

static int sum_counters(bb_engine *e, bb_counters *out) {
    size_t n = (size_t)e->dev.n_slots * 8;
    std::vector<uint64_t> h(n);
    HIPCHK(sync_all(e));
    HIPCHK(hipMemcpy(h.data(), e->dev.ctr, n * 8, hipMemcpyDeviceToHost));
    uint64_t t[8] = {0};
    for (size_t i = 0; i < n; i++) t[i & 7] += h[i];
    std::vector<uint64_t> ev((size_t)e->dev.n_slots);
    HIPCHK(hipMemcpy(ev.data(), e->dev.evals, ev.size() * 8, hipMemcpyDeviceToHost));
    out->evals = 0;
    for (uint64_t v : ev) out->evals += v;
    out->sims = t[0];
    out->sum_depth = t[1];
    out->nodes = t[2];
    out->terminal_leaves = t[3];
    out->games_finished = t[4];
    out->plies = t[5];
    out->overflow = t[6];
    out->examples = t[7];
    uint64_t ec[2];
    HIPCHK(hipMemcpy(ec, e->dev.eval_cache_ctr, sizeof ec, hipMemcpyDeviceToHost));
    out->eval_cache_hits = ec[0];
    out->eval_cache_probes = ec[1];
    return BB_OK;
}

extern "C" int bb_get_counters(bb_engine *e, bb_counters *out) {
    if (!e || !out) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    return sum_counters(e, out);
}

extern "C" int bb_reset_counters(bb_engine *e) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipMemsetAsync(e->dev.ctr, 0, (size_t)e->dev.n_slots * 64, e->stream));
    HIPCHK(hipMemsetAsync(e->dev.evals, 0, (size_t)e->dev.n_slots * 8, e->stream));
    HIPCHK(hipMemsetAsync(e->dev.eval_cache_ctr, 0, 16, e->stream));
    return BB_OK;
}

extern "C" int bb_selfplay_done(bb_engine *e, int *done_out, int *games_finished_out) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    int ng = e->n_games_target;
    std::vector<int32_t> h((size_t)ng * 4);
    if (ng) HIPCHK(hipMemcpy(h.data(), e->dev.game_hdr, h.size() * 4, hipMemcpyDeviceToHost));
    int fin = 0;
    for (int g = 0; g < ng; g++) fin += h[(size_t)g * 4 + 3] != 0;
    if (done_out) *done_out = (ng > 0 && fin == ng) ? 1 : 0;
    if (games_finished_out) *games_finished_out = fin;
    return BB_OK;
}

extern "C" int bb_examples_fetch(bb_engine *e, int first_game, int n_games, void *records_out, int max_records,
                                 int32_t *game_offsets_out, int8_t *winner_out) {
    if (!e || first_game < 0 || n_games <= 0 || first_game + n_games > e->cfg.max_games || !records_out)
        return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    const size_t eb = (size_t)e->info.example_bytes, per = (size_t)(e->cfg.max_plies + 1) * eb;
    std::vector<int32_t> hdr((size_t)n_games * 4);
    HIPCHK(hipMemcpy(hdr.data(), e->dev.game_hdr + (size_t)first_game * 4, hdr.size() * 4, hipMemcpyDeviceToHost));
    std::vector<uint8_t> stage((size_t)n_games * per);
    HIPCHK(hipMemcpy(stage.data(), e->dev.examples + (size_t)first_game * per, stage.size(), hipMemcpyDeviceToHost));
    int total = 0;
    uint8_t *out = (uint8_t *)records_out;
    for (int g = 0; g < n_games; g++) {
        if (game_offsets_out) game_offsets_out[g] = total;
        int done = hdr[(size_t)g * 4 + 3], nex = hdr[(size_t)g * 4 + 0];
        if (winner_out) winner_out[g] = done ? (int8_t)hdr[(size_t)g * 4 + 1] : (int8_t)-2;
        if (!done) continue;
        if (total + nex > max_records) return fail(BB_ERR_CAPACITY, "records_out too small");
        memcpy(out + (size_t)total * eb, stage.data() + (size_t)g * per, (size_t)nex * eb);
        total += nex;
    }
    if (game_offsets_out) game_offsets_out[n_games] = total;
    return total;
}

extern "C" int bb_selfplay_headers(bb_engine *e, int first_game, int n_games, int32_t *hdr_out) {
    if (!e || first_game < 0 || n_games <= 0 || first_game + n_games > e->cfg.max_games || !hdr_out) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    HIPCHK(hipMemcpy(hdr_out, e->dev.game_hdr + (size_t)first_game * 4, (size_t)n_games * 16, hipMemcpyDeviceToHost));
    return BB_OK;
}

// record r of the compacted output <- record (r - off[g]) of game ids[g]: one thread per 16 bytes
__global__ void __launch_bounds__(256) k_gather_examples(const uint8_t *store, size_t game_stride, int eb16, int n, const int32_t *ids,
                                                         const int32_t *off, uint4 *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)off[n] * eb16;
    if (i >= total) return;
    const int rec = (int)(i / eb16), part = (int)(i % eb16);
    int lo = 0, hi = n - 1; // the game this record belongs to: last g with off[g] <= rec
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= rec) lo = mid;
        else hi = mid - 1;
    }
    out[i] = ((const uint4 *)(store + (size_t)ids[lo] * game_stride))[(size_t)(rec - off[lo]) * eb16 + part];
}

extern "C" int bb_examples_fetch_games(bb_engine *e, int n, const int32_t *game_ids, void *records_out, int max_records,
                                       int32_t *game_offsets_out, int8_t *winner_out) {
    if (!e || n <= 0 || !game_ids || !records_out) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    const size_t eb = (size_t)e->info.example_bytes, per = (size_t)(e->cfg.max_plies + 1) * eb;
    if (eb % 16) return fail(BB_ERR_ARG, "example records are copied in 16-byte units");
    std::vector<int32_t> hdr((size_t)e->cfg.max_games * 4);
    HIPCHK(hipMemcpy(hdr.data(), e->dev.game_hdr, hdr.size() * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> off((size_t)n + 1, 0);
    for (int g = 0; g < n; g++) {
        const int id = game_ids[g];
        if (id < 0 || id >= e->cfg.max_games) return fail(BB_ERR_ARG, "game id %d out of range", id);
        const int done = hdr[(size_t)id * 4 + 3];
        if (winner_out) winner_out[g] = done ? (int8_t)hdr[(size_t)id * 4 + 1] : (int8_t)-2;
        off[g + 1] = off[g] + (done ? hdr[(size_t)id * 4 + 0] : 0);
    }
    if (game_offsets_out) memcpy(game_offsets_out, off.data(), off.size() * 4);
    const int total = off[n];
    if (total > max_records) return fail(BB_ERR_CAPACITY, "records_out too small");
    if (total == 0) return 0;
    DevBuf d_ids, d_off, d_out;
    if (d_ids.alloc((size_t)n * 4) || d_off.alloc(((size_t)n + 1) * 4) || d_out.alloc((size_t)total * eb)) return BB_ERR_HIP;
    HIPCHK(hipMemcpy(d_ids.p, game_ids, (size_t)n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    k_gather_examples<<<nblk((size_t)total * (eb / 16)), 256, 0, e->stream>>>(e->dev.examples, per, (int)(eb / 16), n, (const int32_t *)d_ids.p,
                                                                            (const int32_t *)d_off.p, (uint4 *)d_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_all(e));
    HIPCHK(hipMemcpy(records_out, d_out.p, (size_t)total * eb, hipMemcpyDeviceToHost));
    return total;
}

extern "C" int bb_examples_device(bb_engine *e, void **ptr_out, uint64_t *bytes_out, uint64_t *record_bytes_out,
                                  int32_t **game_hdr_out) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    if (ptr_out) *ptr_out = e->dev.examples;
    if (bytes_out) *bytes_out = (uint64_t)e->cfg.max_games * (uint64_t)(e->cfg.max_plies + 1) * (uint64_t)e->info.example_bytes;
    if (record_bytes_out) *record_bytes_out = (uint64_t)e->info.example_bytes;
    if (game_hdr_out) *game_hdr_out = e->dev.game_hdr;
    return BB_OK;
}

extern "C" int bb_examples_to_batch_sym(int game, int n_records, const void *records, int n, const int64_t *index, const uint8_t *sym,
                                        float *boards_out, float *policy_out, float *value_out, int32_t *bad_out, void *stream) {
    if (n == 0) return BB_OK; // an empty batch is a no-op
    if (n < 0 || n_records < 0 || !records || (!boards_out && !policy_out && !value_out)) return fail(BB_ERR_ARG, "bad arguments");
    if (((uintptr_t)records | (uintptr_t)boards_out | (uintptr_t)policy_out) % 16)
        return fail(BB_ERR_ARG, "records, boards_out and policy_out are accessed in 16-byte units");
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *rec = (const uint8_t *)records;
    GAME_SWITCH(game, Launch<G>::examples_to_batch(st, n_records, rec, n, index, sym, boards_out, policy_out, value_out, bad_out); break);
    HIPCHK(hipGetLastError());
    return BB_OK;
}

extern "C" int bb_examples_to_batch(int game, int n_records, const void *records, int n, const int64_t *index, float *boards_out,
                                    float *policy_out, float *value_out, int32_t *bad_out, void *stream) {
    return bb_examples_to_batch_sym(game, n_records, records, n, index, nullptr, boards_out, policy_out, value_out, bad_out, stream);
}

// ---- duplicate positions merged (examples_merge.hip.h): the dense games only -------------------------------------------------
static int merge_game_check(int game) {
    if (game == BB_GAME_DRAGONCHESS)
        return fail(BB_ERR_ARG, "merging example records covers Connect4 and TicTacToe; DragonChess (a 64-byte key, compact child "
                                "lists, few transpositions) is not covered");
    if (game != BB_GAME_CONNECT4 && game != BB_GAME_TICTACTOE) return fail(BB_ERR_ARG, "unknown game %d", game);
    return BB_OK;
}

extern "C" int bb_examples_merge_workspace(int game, int n_records, uint64_t *bytes_out) {
    if (int rc = merge_game_check(game)) return rc;
    if (n_records < 0 || n_records > MERGE_MAX_RECORDS || !bytes_out)
        return fail(BB_ERR_ARG, "n_records in [0, %d] and a place for the size are expected", MERGE_MAX_RECORDS);
    *bytes_out = n_records ? (uint64_t)merge_workspace(n_records).bytes : 0;
    return BB_OK;
}

template <class G>
static void merge_launch(hipStream_t st, int n, const uint8_t *rec, const MergeWorkspace &w, uint8_t *ws, int32_t *group, int32_t *rep,
                         int32_t *count, int32_t *zsum, uint64_t *total, uint64_t *visits, int32_t *n_groups, int32_t *bad) {
    int32_t *owner = (int32_t *)(ws + w.owner), *first = (int32_t *)(ws + w.first), *slot_of = (int32_t *)(ws + w.slot_of);
    int32_t *sums = (int32_t *)(ws + w.sums), *err = (int32_t *)(ws + w.err);
    k_merge_insert<G><<<w.blocks, 256, 0, st>>>(n, rec, w.cap, owner, first, slot_of, bad, err);
    k_merge_count<<<w.blocks, 256, 0, st>>>(n, slot_of, first, sums);
    k_merge_offsets<<<1, 256, 0, st>>>(w.blocks, sums, err, n_groups);
    k_merge_number<G><<<w.blocks, 256, 0, st>>>(n, rec, slot_of, first, sums, owner, rep, count, zsum, total, visits);
    k_merge_sum<G><<<nblk((size_t)n * (G::A + 1)), 256, 0, st>>>(n, rec, slot_of, first, owner, group, count, zsum, total, visits);
}

extern "C" int bb_examples_merge(int game, int n_records, const void *records, int32_t *group_out, int32_t *rep_out, int32_t *count_out,
                                 int32_t *zsum_out, uint64_t *total_out, uint64_t *visits_out, int32_t *n_groups_out, int32_t *bad_out,
                                 void *workspace, uint64_t workspace_bytes, void *stream) {
    if (int rc = merge_game_check(game)) return rc;
    if (n_records < 0 || n_records > MERGE_MAX_RECORDS) return fail(BB_ERR_ARG, "n_records must be in [0, %d]", MERGE_MAX_RECORDS);
    if (n_records == 0) return BB_OK; // nothing to merge: a no-op
    if (!records || !group_out || !rep_out || !count_out || !zsum_out || !total_out || !visits_out || !n_groups_out || !bad_out || !workspace)
        return fail(BB_ERR_ARG, "bb_examples_merge: every pointer is required");
    if (((uintptr_t)records | (uintptr_t)workspace) % 16 || ((uintptr_t)total_out | (uintptr_t)visits_out) % 8 ||
        ((uintptr_t)group_out | (uintptr_t)rep_out | (uintptr_t)count_out | (uintptr_t)zsum_out | (uintptr_t)n_groups_out | (uintptr_t)bad_out) % 4)
        return fail(BB_ERR_ARG, "bb_examples_merge: records and workspace are accessed in 16-byte units, the outputs in their own");
    const MergeWorkspace w = merge_workspace(n_records);
    if (workspace_bytes < w.bytes)
        return fail(BB_ERR_ARG, "workspace of %llu bytes, %zu are needed (bb_examples_merge_workspace)", (unsigned long long)workspace_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    HIPCHK(hipMemsetAsync(ws + w.owner, 0xFF, (size_t)w.cap * 4, st)); // MERGE_EMPTY
    HIPCHK(hipMemsetAsync(ws + w.first, 0x7F, (size_t)w.cap * 4, st)); // MERGE_NO_FIRST
    HIPCHK(hipMemsetAsync(ws + w.err, 0, 16, st));
    const uint8_t *rec = (const uint8_t *)records;
    if (game == BB_GAME_CONNECT4)
        merge_launch<Connect4>(st, n_records, rec, w, ws, group_out, rep_out, count_out, zsum_out, total_out, visits_out, n_groups_out, bad_out);
    else
        merge_launch<TicTacToe>(st, n_records, rec, w, ws, group_out, rep_out, count_out, zsum_out, total_out, visits_out, n_groups_out, bad_out);
    HIPCHK(hipGetLastError());
    return BB_OK;
}

extern "C" int bb_examples_merged_to_batch(int game, int n_records, const void *records, int n_groups, const int32_t *rep, const int32_t *count,
                                           const int32_t *zsum, const uint64_t *total, const uint64_t *visits, int n, const int64_t *index,
                                           const uint8_t *sym, float *boards_out, float *policy_out, float *value_out, int32_t *bad_out,
                                           void *stream) {
    if (int rc = merge_game_check(game)) return rc;
    if (n == 0) return BB_OK; // an empty batch is a no-op
    if (n < 0 || n_records < 0 || n_groups < 0 || !records || !rep || !count || !zsum || !total || !visits ||
        (!boards_out && !policy_out && !value_out))
        return fail(BB_ERR_ARG, "bad arguments");
    if (((uintptr_t)records | (uintptr_t)boards_out | (uintptr_t)policy_out) % 16 || ((uintptr_t)total | (uintptr_t)visits) % 8)
        return fail(BB_ERR_ARG, "records, boards_out and policy_out are accessed in 16-byte units, total and visits in 8-byte units");
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *rec = (const uint8_t *)records;
    if (game == BB_GAME_CONNECT4)
        k_merged_to_batch<Connect4><<<nblk((size_t)n * (Connect4::H * Connect4::W * Connect4::C + Connect4::A + 1)), 256, 0, st>>>(
            n_records, rec, n_groups, rep, count, zsum, total, visits, n, index, sym, boards_out, policy_out, value_out, bad_out);
    else
        k_merged_to_batch<TicTacToe><<<nblk((size_t)n * (TicTacToe::H * TicTacToe::W * TicTacToe::C + TicTacToe::A + 1)), 256, 0, st>>>(
            n_records, rec, n_groups, rep, count, zsum, total, visits, n, index, sym, boards_out, policy_out, value_out, bad_out);
    HIPCHK(hipGetLastError());
    return BB_OK;
}

// ---- the arena on the device (arena.hip.h): Blackbird.TestModels' match loop without the host in it -----------------------
struct bb_arena {
    bb_engine *a = nullptr, *b = nullptr; // borrowed
    ArenaDev dev = {};
    std::vector<void *> allocs;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // prep done (a), b sampled, moved (a), b's roots moved
    double temp = 0.0;
    int enqueued = 0; // plies enqueued since bb_arena_begin
    bool begun = false;
};

template <class T>
static int arena_alloc(bb_arena *ar, T *&p, size_t count) {
    void *q = nullptr;
    const size_t bytes = count * sizeof(T);
    hipError_t err = hipMalloc(&q, bytes ? bytes : 16);
    if (err != hipSuccess) return fail(BB_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
    ar->allocs.push_back(q);
    p = (T *)q;
    return 0;
}

extern "C" int bb_arena_destroy(bb_arena *ar) {
    if (!ar) return BB_OK;
    (void)hipSetDevice(ar->a->cfg.device);
    (void)sync_all(ar->a);
    (void)sync_all(ar->b);
    for (void *p : ar->allocs) (void)hipFree(p);
    for (hipEvent_t ev : ar->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete ar;
    return BB_OK;
}

extern "C" int bb_arena_create(bb_engine *a, bb_engine *b, int log_plies, bb_arena **out) {
    if (!a || !b || !out) return fail(BB_ERR_ARG, "bb_arena_create: null argument");
    if (a == b) return fail(BB_ERR_ARG, "bb_arena_create: the two sides must be two engines");
    if (log_plies < 0) return fail(BB_ERR_ARG, "bb_arena_create: log_plies = %d is negative", log_plies);
    if (a->cfg.game != b->cfg.game || a->cfg.n_slots != b->cfg.n_slots || a->cfg.device != b->cfg.device)
        return fail(BB_ERR_ARG, "bb_arena_create: the engines differ in game (%d, %d), n_slots (%d, %d) or device (%d, %d)", a->cfg.game,
                    b->cfg.game, a->cfg.n_slots, b->cfg.n_slots, a->cfg.device, b->cfg.device);
    HIPCHK(hipSetDevice(a->cfg.device));
    bb_arena *ar = new bb_arena();
    ar->a = a;
    ar->b = b;
    ArenaDev &d = ar->dev;
    const size_t n = (size_t)a->cfg.n_slots;
    d.n_slots = (int)n;
    d.log_plies = log_plies;
    uint8_t *st = nullptr;
    bool bad = arena_alloc(ar, st, n * (size_t)a->info.state_bytes) || arena_alloc(ar, d.a_to_move, n) || arena_alloc(ar, d.a_player, n) ||
               arena_alloc(ar, d.alive, n) || arena_alloc(ar, d.primed_a, n) || arena_alloc(ar, d.primed_b, n) || arena_alloc(ar, d.result, n) ||
               arena_alloc(ar, d.plies, n) || arena_alloc(ar, d.err, n) || arena_alloc(ar, d.log, n * (size_t)log_plies) ||
               arena_alloc(ar, d.mask_a, n) || arena_alloc(ar, d.mask_b, n) || arena_alloc(ar, d.prime_a, n) || arena_alloc(ar, d.prime_b, n) ||
               arena_alloc(ar, d.mv_a, n) || arena_alloc(ar, d.mv_b, n) || arena_alloc(ar, d.gids, n);
    d.states = st;
    for (hipEvent_t &ev : ar->ev)
        if (!bad && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) bad = fail(BB_ERR_HIP, "hipEventCreate failed") != 0;
    if (bad) {
        const std::string why = g_err;
        bb_arena_destroy(ar);
        g_err = why;
        return BB_ERR_HIP;
    }
    *out = ar;
    return BB_OK;
}

template <class G>
static int arena_begin(bb_arena *ar, int n_games, const uint8_t *a_first, const void *start_states) {
    using State = typename G::State;
    ArenaDev &d = ar->dev;
    const size_t n = (size_t)d.n_slots;
    std::vector<State> st(n, G::initial());
    if (start_states) memcpy((void *)st.data(), start_states, (size_t)n_games * sizeof(State));
    HIPCHK(hipMemcpy(d.states, st.data(), n * sizeof(State), hipMemcpyHostToDevice));
    if (start_states) { // bb_selfplay_set_starts' checks, by its kernel
        DevBuf dv;
        if (dv.alloc((size_t)n_games)) return BB_ERR_HIP;
        Launch<G>::check_starts(ar->a->stream, n_games, (const State *)d.states, (uint8_t *)dv.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ar->a->stream));
        std::vector<uint8_t> verdict((size_t)n_games);
        HIPCHK(hipMemcpy(verdict.data(), dv.p, (size_t)n_games, hipMemcpyDeviceToHost));
        int reason = BB_START_OK;
        const int refused = starts_first_refused(verdict.data(), n_games, &reason);
        if (refused >= 0)
            return fail(BB_ERR_ARG, "bb_arena_begin: start state %d refused: %s (reason %d)", refused, starts_reason_text(reason), reason);
    }
    std::vector<uint8_t> first(n, 0), player(n, 0), alive(n, 0);
    std::vector<uint32_t> gids(n);
    for (size_t i = 0; i < n; i++) {
        gids[i] = (uint32_t)i;
        if (i >= (size_t)n_games) continue;
        first[i] = a_first[i] != 0;
        player[i] = first[i] ? 1 : 2; // model1Player (Blackbird.py:187-193)
        alive[i] = 1;
    }
    HIPCHK(hipMemcpy(d.a_to_move, first.data(), n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.a_player, player.data(), n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.alive, alive.data(), n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.gids, gids.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d.primed_a, 0, n)); // DropRoot at the top of every game (Blackbird.py:189-190): the first turn primes
    HIPCHK(hipMemset(d.primed_b, 0, n));
    HIPCHK(hipMemset(d.result, 0, n));
    HIPCHK(hipMemset(d.plies, 0, n * 4));
    HIPCHK(hipMemset(d.err, 0, n * 4));
    HIPCHK(hipMemset(d.log, 0xFF, n * (size_t)d.log_plies * 4));
    HIPCHK(hipDeviceSynchronize());
    return BB_OK;
}

extern "C" int bb_arena_begin(bb_arena *ar, int n_games, const uint8_t *a_first, const void *start_states, double temp) {
    if (!ar || !a_first) return fail(BB_ERR_ARG, "bb_arena_begin: null argument");
    if (n_games < 1 || n_games > ar->dev.n_slots)
        return fail(BB_ERR_ARG, "bb_arena_begin: n_games = %d outside 1 .. n_slots = %d", n_games, ar->dev.n_slots);
    if (!(temp >= 0)) return fail(BB_ERR_ARG, "bb_arena_begin: temp must be >= 0");
    for (bb_engine *e : {ar->a, ar->b}) {
        if (int rc = check_eval(e)) return rc;
        if (e->sims_now < 2 && temp != 0.0) // (bb_selfplay_begin's rule)
            return fail(BB_ERR_ARG, "probabilities contain NaN (a fresh root needs >= 2 simulations, MCTS.py:336-338)");
    }
    HIPCHK(hipSetDevice(ar->a->cfg.device));
    HIPCHK(sync_all(ar->a));
    HIPCHK(sync_all(ar->b));
    ar->begun = false;
    GAME_SWITCH(ar->a->cfg.game, {
        if (int rc = arena_begin<G>(ar, n_games, a_first, start_states)) return rc;
        break;
    });
    ar->dev.n_games = n_games;
    ar->temp = temp;
    ar->enqueued = 0;
    ar->begun = true;
    return BB_OK;
}

// One ply.  Stream a: prep | prime a, search a, sample a | wait for b's sample | move | a's MoveRoot.
//           Stream b:  wait for prep | prime b, search b, sample b |   wait for move   | b's MoveRoot.
// Between prep and move the two streams share nothing they write: each side's launches touch its own engine, and the arena's
// arrays are only read there -- so the two searches may run at the same time.  The next ply's prep rewrites what b's MoveRoot
// reads, so stream a waits for that first.
template <class G>
static int arena_ply(bb_arena *ar) {
    using State = typename G::State;
    bb_engine *a = ar->a, *b = ar->b;
    const ArenaDev &d = ar->dev;
    hipStream_t sa = a->stream, sb = b->stream;
    const int blocks = nblk(d.n_slots);
    if (ar->enqueued > 0) HIPCHK(hipStreamWaitEvent(sa, ar->ev[3], 0));
    k_arena_prep<<<blocks, 256, 0, sa>>>(d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ar->ev[0], sa));
    HIPCHK(hipStreamWaitEvent(sb, ar->ev[0], 0));
    struct Side { bb_engine *e; const int32_t *prime; const uint8_t *mask; };
    for (const Side &s : {Side{a, d.prime_a, d.mask_a}, Side{b, d.prime_b, d.mask_b}}) {
        bb_engine *e = s.e;
        // the callers alternate every ply, so after two plies every live game is primed on both sides: nothing left to prime
        if (ar->enqueued < 2) {
            Launch<G>::set_roots(e->dev, e->edges, e->stream, d.n_games, s.prime, (const State *)d.states, d.gids);
            HIPCHK(hipGetLastError());
        }
        if (int rc = enqueue_sims(e, e->sims_now, s.mask)) return rc;
        TreeDev t = e->dev;
        t.in_u = nullptr; // the Philox draw of (seed, game id, ply), as bb_sample_moves with u == NULL
        Launch<G>::sample(t, e->edges, e->stream, ar->temp, e->d_child_action);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ar->ev[1], sb));
    HIPCHK(hipStreamWaitEvent(sa, ar->ev[1], 0));
    k_arena_move<G><<<blocks, 256, 0, sa>>>(d, a->dev.out_action, b->dev.out_action);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ar->ev[2], sa));
    HIPCHK(hipStreamWaitEvent(sb, ar->ev[2], 0));
    Launch<G>::move_roots(a->dev, a->edges, sa, d.mv_a);
    Launch<G>::move_roots(b->dev, b->edges, sb, d.mv_b);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ar->ev[3], sb));
    ar->enqueued += 1;
    return BB_OK;
}

extern "C" int bb_arena_step(bb_arena *ar, int plies) {
    if (!ar || plies <= 0) return fail(BB_ERR_ARG, "bb_arena_step: an arena and a positive number of plies");
    if (!ar->begun) return fail(BB_ERR_ARG, "bb_arena_begin has not been called");
    HIPCHK(hipSetDevice(ar->a->cfg.device));
    GAME_SWITCH(ar->a->cfg.game, {
        for (int p = 0; p < plies; p++)
            if (int rc = arena_ply<G>(ar)) return rc;
        return BB_OK;
    });
}

extern "C" int bb_arena_status(bb_arena *ar, int *alive_out) {
    if (!ar || !alive_out) return fail(BB_ERR_ARG, "bb_arena_status: null argument");
    if (!ar->begun) return fail(BB_ERR_ARG, "bb_arena_begin has not been called");
    HIPCHK(hipSetDevice(ar->a->cfg.device));
    HIPCHK(sync_all(ar->a));
    HIPCHK(sync_all(ar->b));
    const size_t n = (size_t)ar->dev.n_games;
    std::vector<uint8_t> alive(n);
    std::vector<int32_t> err(n);
    HIPCHK(hipMemcpy(alive.data(), ar->dev.alive, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(err.data(), ar->dev.err, n * 4, hipMemcpyDeviceToHost));
    int live = 0;
    for (uint8_t v : alive) live += v != 0;
    *alive_out = live;
    for (bb_engine *e : {ar->a, ar->b}) {
        bb_counters c;
        if (int rc = sum_counters(e, &c)) return rc;
        if (c.overflow) return fail(BB_ERR_CAPACITY, "search tree outgrew the node pool (side %s)", e == ar->a ? "a" : "b");
    }
    for (size_t i = 0; i < n; i++)
        if (err[i]) {
            if (err[i] == BB_ARENA_ERR_ILLEGAL) return fail(BB_ERR_NAN, "game %zu: Tried to make an illegal move.", i);
            return fail(BB_ERR_NAN, "game %zu: probabilities contain NaN (action %d)", i, err[i]);
        }
    return BB_OK;
}

extern "C" int bb_arena_fetch(bb_arena *ar, int8_t *result_out, int32_t *plies_out, int32_t *moves_out, void *states_out) {
    if (!ar) return fail(BB_ERR_ARG, "bb_arena_fetch: null arena");
    if (!ar->begun) return fail(BB_ERR_ARG, "bb_arena_begin has not been called");
    HIPCHK(hipSetDevice(ar->a->cfg.device));
    HIPCHK(sync_all(ar->a));
    HIPCHK(sync_all(ar->b));
    const ArenaDev &d = ar->dev;
    const size_t n = (size_t)d.n_games;
    if (result_out) HIPCHK(hipMemcpy(result_out, d.result, n, hipMemcpyDeviceToHost));
    if (plies_out) HIPCHK(hipMemcpy(plies_out, d.plies, n * 4, hipMemcpyDeviceToHost));
    if (moves_out && d.log_plies) HIPCHK(hipMemcpy(moves_out, d.log, n * (size_t)d.log_plies * 4, hipMemcpyDeviceToHost));
    if (states_out) HIPCHK(hipMemcpy(states_out, d.states, n * (size_t)ar->a->info.state_bytes, hipMemcpyDeviceToHost));
    return BB_OK;
}

// ---- the training step (train.hip.h) ----------------------------------------------------------------------------------
struct bb_trainer {
    bb_train_config cfg;
    TrainLayout lay;
    int A, P, C;
    size_t lds_bytes;
    float *prm, *slot_m, *slot_v, *grads, *slabs, *le, *lp, *loss;
    uint8_t *kind;
    TrainAux *aux;
    float *eval_rows; // scratch of bb_trainer_eval for callers that pass no rows_out / flags_out: grows, never shrinks
    uint8_t *eval_flags;
    size_t eval_cap;  // rows the scratch holds
    uint64_t calls; // steps made so far, gradient-only ones included: the counter of the noise stream
    int64_t t;      // updates applied so far: AdamOptimizer's beta powers
};

static TrainLayout train_layout(int C, int R, int D, int A) {
    const NetBlocks t = net_blocks(C, BB_TRAIN_F, R, D, A);
    TrainLayout l = {};
    l.R = R; l.D = D;
#define X(name, kind, units, per) l.name = t.b[NET_BLOCK_##name].at;
    BB_NET_BLOCKS(X)
#undef X
    l.count = t.count;
    l.n_l2 = net_blocks_l2(t);
    assert(l.n_l2 == 12 + 6 * R); // kernel, gamma, beta of 1 + 2R tower convs and of the two head convs; dense_1, dense_2, policy kernels
    return l;
}

static void trainer_free(bb_trainer *t) {
    void *ps[] = {t->prm, t->slot_m, t->slot_v, t->grads, t->slabs, t->le, t->lp, t->loss, t->kind, t->aux, t->eval_rows, t->eval_flags};
    for (void *p : ps)
        if (p) (void)hipFree(p);
    delete t;
}

// `using G = ` the trainer's game (bb_trainer_create admits these two only) around the statements given, GAME_SWITCH's way
#define TRAINER_SWITCH(t, ...)                                                   \
    switch ((t)->cfg.game) {                                                     \
    case BB_GAME_CONNECT4: { using G = Connect4; __VA_ARGS__; }                  \
    default: { using G = TicTacToe; __VA_ARGS__; }                               \
    }

// the entry points that launch do not switch devices: the caller's current device must be the trainer's
static int trainer_on_device(const bb_trainer *t) {
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (dev != t->cfg.device) return fail(BB_ERR_ARG, "the trainer lives on device %d, the current device is %d", t->cfg.device, dev);
    return BB_OK;
}

template <class G>
static int trainer_lds(bb_trainer *t) { // (the same dynamic LDS whichever source feeds the workgroup)
    t->lds_bytes = (size_t)train_lds_floats<G>(t->lay.R) * sizeof(float);
    HIPCHK(hipFuncSetAttribute((const void *)k_train_grad<G, TrainTensors<G>>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t->lds_bytes));
    HIPCHK(hipFuncSetAttribute((const void *)k_train_grad<G, TrainRecords<G>>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t->lds_bytes));
    return BB_OK;
}

static int trainer_alloc(bb_trainer *t, const bb_net_weights *w) {
    const TrainLayout &l = t->lay;
    const size_t cb = (size_t)l.count * sizeof(float), slab_b = cb * (size_t)t->cfg.max_batch;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (slab_b + 8 * cb > free_b - free_b / 16)
        return fail(BB_ERR_CAPACITY, "%d gradient slabs of %zu bytes do not fit the %zu free bytes of device %d", t->cfg.max_batch, cb,
                    free_b, t->cfg.device);
    HIPCHK(hipMalloc(&t->prm, cb));
    HIPCHK(hipMalloc(&t->slot_m, cb));
    HIPCHK(hipMalloc(&t->slot_v, cb));
    HIPCHK(hipMalloc(&t->grads, cb));
    HIPCHK(hipMalloc(&t->slabs, slab_b));
    HIPCHK(hipMalloc(&t->le, (size_t)t->cfg.max_batch * sizeof(float)));
    HIPCHK(hipMalloc(&t->lp, (size_t)t->cfg.max_batch * sizeof(float)));
    HIPCHK(hipMalloc(&t->loss, 4 * sizeof(float)));
    HIPCHK(hipMalloc(&t->kind, (size_t)l.count));
    HIPCHK(hipMalloc(&t->aux, sizeof(TrainAux)));
    HIPCHK(hipMemset(t->slot_m, 0, cb));
    HIPCHK(hipMemset(t->slot_v, 0, cb));
    HIPCHK(hipMemset(t->grads, 0, cb));
    HIPCHK(hipMemset(t->loss, 0, 4 * sizeof(float)));
    HIPCHK(hipMemset(t->aux, 0, sizeof(TrainAux)));
    const NetBlocks tb = net_blocks(t->C, BB_TRAIN_F, l.R, l.D, t->A); // (what train_layout took l from)
    const std::vector<uint8_t> kind = net_block_kinds(tb);
    HIPCHK(hipMemcpy(t->kind, kind.data(), kind.size(), hipMemcpyHostToDevice));
    for (int i = 0; i < NET_BLOCKS; i++)
        if (const int n = tb.b[i].count())
            HIPCHK(hipMemcpy(t->prm + tb.b[i].at, net_block(*w, i), (size_t)n * sizeof(float), hipMemcpyDefault));
    TRAINER_SWITCH(t, return trainer_lds<G>(t));
}

extern "C" int bb_trainer_create(const bb_train_config *cfg, const bb_net_weights *w, bb_trainer **out) {
    if (!cfg || !w || !out) return fail(BB_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->game != BB_GAME_CONNECT4 && cfg->game != BB_GAME_TICTACTOE)
        return fail(BB_ERR_ARG, "the HIP trainer covers Connect4 and TicTacToe, not game %d", cfg->game);
    bb_game_info gi;
    bb_game_info_get(cfg->game, &gi);
    if (int rc = check_weights(w, gi)) return rc;
    if (w->F != BB_TRAIN_F || w->R < 0 || w->R > 9 || w->D < 1 || w->D > 64)
        return fail(BB_ERR_ARG, "the HIP trainer covers 16 filters, 0..9 blocks and a dense width of 1..64; got %d filters, %d blocks, "
                    "dense %d", w->F, w->R, w->D);
    if (cfg->optimizer != BB_OPT_ADAM && cfg->optimizer != BB_OPT_MOMENTUM && cfg->optimizer != BB_OPT_SGD)
        return fail(BB_ERR_ARG, "unknown optimizer %d", cfg->optimizer);
    if (cfg->max_batch <= 0 || cfg->max_batch > (1 << 20)) return fail(BB_ERR_ARG, "max_batch %d out of range", cfg->max_batch);
    if (!(cfg->epsilon >= 0.f && cfg->epsilon <= 1.f) || (cfg->epsilon != 0.f && !(cfg->alpha > 0.f && cfg->alpha < 1.f)))
        return fail(BB_ERR_ARG, "epsilon must lie in [0, 1] and alpha in (0, 1)");
    const int ndev = bb_device_count();
    if (ndev <= 0) return fail(BB_ERR_HIP, "no HIP device available (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(BB_ERR_ARG, "device %d out of range", cfg->device);
    int prev = 0;
    HIPCHK(hipGetDevice(&prev));
    HIPCHK(hipSetDevice(cfg->device));
    bb_trainer *t = new bb_trainer();
    t->cfg = *cfg;
    t->A = gi.A; t->P = gi.H * gi.W; t->C = gi.C;
    t->lay = train_layout(gi.C, w->R, w->D, gi.A);
    const int rc = trainer_alloc(t, w);
    (void)hipSetDevice(prev);
    if (rc) {
        const std::string keep = g_err;
        trainer_free(t);
        g_err = keep;
        return rc;
    }
    *out = t;
    return BB_OK;
}

extern "C" int bb_trainer_destroy(bb_trainer *t) {
    if (!t) return BB_OK;
    int prev = 0;
    const bool ok = hipGetDevice(&prev) == hipSuccess && hipSetDevice(t->cfg.device) == hipSuccess;
    if (ok) (void)hipDeviceSynchronize();
    trainer_free(t);
    if (ok) (void)hipSetDevice(prev);
    return BB_OK;
}

// One step's three launches on `st`, the batch read through `src` (train.hip.h): what bb_trainer_step and every batch of
// bb_trainer_epoch enqueue.  Host state moves as the launches are made: the noise counter, Adam's step count and lr_t.
template <class G, class Src>
static void trainer_launch(bb_trainer *t, int n, const Src &src, const float *noise, double lr, int apply, float *loss_out, hipStream_t st) {
    const TrainLayout &l = t->lay;
    const float eps = t->cfg.epsilon;
    k_train_prep<G, Src><<<1, BB_TRAIN_THREADS, 0, st>>>(n, l.count, l.n_l2, t->prm, t->kind, src, noise, eps, t->cfg.alpha, t->cfg.seed, t->calls,
                                                         t->aux);
    t->calls++;
    k_train_grad<G, Src><<<n, BB_TRAIN_THREADS, t->lds_bytes, st>>>(l, t->prm, t->aux, src, n, eps, t->slabs, t->le, t->lp);
    float rate = (float)lr;
    if (apply) {
        t->t++;
        if (t->cfg.optimizer == BB_OPT_ADAM) // AdamOptimizer's lr_t (beta1 0.9, beta2 0.999)
            rate = (float)(lr * std::sqrt(1.0 - std::pow(0.999, (double)t->t)) / (1.0 - std::pow(0.9, (double)t->t)));
    }
    k_train_apply<<<nblk((size_t)l.count, BB_TRAIN_THREADS) + 1, BB_TRAIN_THREADS, 0, st>>>(
        l.count, n, l.n_l2, t->slabs, t->kind, t->prm, t->slot_m, t->slot_v, t->grads, t->cfg.optimizer, rate, t->cfg.momentum,
        apply != 0, t->le, t->lp, t->aux, t->loss, loss_out);
}

extern "C" int bb_trainer_step(bb_trainer *t, int n, const float *boards, const float *value, const float *policy, const float *noise,
                               double lr, int apply, float *loss_out, void *stream) {
    if (!t) return fail(BB_ERR_ARG, "null trainer");
    if (n <= 0 || n > t->cfg.max_batch) return fail(BB_ERR_ARG, "a batch of %d examples; the trainer takes 1..%d (max_batch)", n, t->cfg.max_batch);
    if (!boards || !value || !policy) return fail(BB_ERR_ARG, "boards, value and policy are required");
    if (((uintptr_t)boards | (uintptr_t)value | (uintptr_t)policy | (uintptr_t)noise | (uintptr_t)loss_out) % sizeof(float))
        return fail(BB_ERR_ARG, "float32 pointers must be 4-byte aligned");
    if (!std::isfinite(lr)) return fail(BB_ERR_ARG, "the learning rate is not finite");
    if (int rc = trainer_on_device(t)) return rc;
    TRAINER_SWITCH(t, trainer_launch<G>(t, n, TrainTensors<G>{boards, value, policy}, noise, lr, apply, loss_out, (hipStream_t)stream); break);
    HIPCHK(hipGetLastError());
    return BB_OK;
}

template <class G>
static void trainer_epoch(bb_trainer *t, int n_records, const uint8_t *records, int n_batches, int batch, const int64_t *order,
                          const uint8_t *sym, const float *noise, double lr, float *loss_out, int32_t *bad_out, hipStream_t st) {
    for (int i = 0; i < n_batches; i++)
        trainer_launch<G>(t, batch, TrainRecords<G>{n_records, records, order, sym, (size_t)i * (size_t)batch, bad_out},
                          noise ? noise + (size_t)i * t->A : nullptr, lr, 1, loss_out ? loss_out + (size_t)i * 4 : nullptr, st);
}

extern "C" int bb_trainer_epoch(bb_trainer *t, int n_records, const void *records, int n_batches, int batch, const int64_t *order,
                                const uint8_t *sym, const float *noise, double lr, float *loss_out, int32_t *bad_out, void *stream) {
    if (!t) return fail(BB_ERR_ARG, "null trainer");
    if (n_batches < 0 || n_records < 0) return fail(BB_ERR_ARG, "negative count (%d batches, %d records)", n_batches, n_records);
    if (batch <= 0 || batch > t->cfg.max_batch)
        return fail(BB_ERR_ARG, "batches of %d examples; the trainer takes 1..%d (max_batch)", batch, t->cfg.max_batch);
    if (!std::isfinite(lr)) return fail(BB_ERR_ARG, "the learning rate is not finite");
    if ((uintptr_t)order % sizeof(int64_t) || ((uintptr_t)noise | (uintptr_t)loss_out | (uintptr_t)bad_out) % 4)
        return fail(BB_ERR_ARG, "order must be 8-byte aligned, noise, loss_out and bad_out 4-byte aligned");
    if (n_batches == 0) return BB_OK;
    if (!records || (uintptr_t)records % 16) return fail(BB_ERR_ARG, "records must be a 16-byte aligned device pointer");
    if (int rc = trainer_on_device(t)) return rc;
    TRAINER_SWITCH(t, trainer_epoch<G>(t, n_records, (const uint8_t *)records, n_batches, batch, order, sym, noise, lr, loss_out, bad_out, (hipStream_t)stream);
                   break);
    HIPCHK(hipGetLastError());
    return BB_OK;
}

// ---- scoring rows with the trainer's parameters (train_eval.hip.h) ----
static_assert(sizeof(bb_eval_totals) == sizeof(EvalTotals) && sizeof(bb_eval_totals) == 56, "bb_eval_totals is the kernels' EvalTotals");

// The checks both entry points share, and the per-row outputs: the caller's, or the trainer's scratch grown to n rows.
static int trainer_eval_prepare(bb_trainer *t, int n, float **rows, uint8_t **flags, const bb_eval_totals *totals) {
    if (!t) return fail(BB_ERR_ARG, "null trainer");
    if (n < 0) return fail(BB_ERR_ARG, "negative count (%d rows)", n);
    if (!totals || (uintptr_t)totals % 8) return fail(BB_ERR_ARG, "totals_out must be an 8-byte aligned device pointer");
    if ((uintptr_t)*rows % sizeof(float)) return fail(BB_ERR_ARG, "float32 pointers must be 4-byte aligned");
    if (int rc = trainer_on_device(t)) return rc;
    if ((!*rows || !*flags) && (size_t)n > t->eval_cap) {
        if (t->eval_rows) (void)hipFree(t->eval_rows); // (hipFree waits for the device: no launch still reads the old scratch)
        if (t->eval_flags) (void)hipFree(t->eval_flags);
        t->eval_rows = nullptr;
        t->eval_flags = nullptr;
        t->eval_cap = 0;
        if (hipMalloc(&t->eval_rows, (size_t)n * 3 * sizeof(float)) != hipSuccess || hipMalloc(&t->eval_flags, (size_t)n) != hipSuccess) {
            (void)hipGetLastError();
            if (t->eval_rows) (void)hipFree(t->eval_rows);
            t->eval_rows = nullptr;
            t->eval_flags = nullptr;
            return fail(BB_ERR_CAPACITY, "no device memory for the per-row figures of %d rows", n);
        }
        t->eval_cap = (size_t)n;
    }
    if (!*rows) *rows = t->eval_rows;
    if (!*flags) *flags = t->eval_flags;
    return BB_OK;
}

template <class G, class Src>
static void trainer_eval_launch(bb_trainer *t, int n, const Src &src, float *rows, uint8_t *flags, bb_eval_totals *totals, hipStream_t st) {
    if (n > 0) k_train_eval<G, Src><<<n, BB_TRAIN_THREADS, 0, st>>>(t->lay, t->prm, src, n, rows, flags);
    k_train_eval_totals<<<1, BB_TRAIN_THREADS, 0, st>>>(n, rows, flags, (EvalTotals *)totals);
}

extern "C" int bb_trainer_eval(bb_trainer *t, int n_records, const void *records, int n, const int64_t *index, const uint8_t *sym,
                               float *rows_out, uint8_t *flags_out, bb_eval_totals *totals_out, int32_t *bad, void *stream) {
    if (n_records < 0) return fail(BB_ERR_ARG, "negative count (%d records)", n_records);
    if ((uintptr_t)index % sizeof(int64_t) || (uintptr_t)bad % 4) return fail(BB_ERR_ARG, "index must be 8-byte aligned, bad 4-byte aligned");
    if (n > 0 && (!records || (uintptr_t)records % 16)) return fail(BB_ERR_ARG, "records must be a 16-byte aligned device pointer");
    if (int rc = trainer_eval_prepare(t, n, &rows_out, &flags_out, totals_out)) return rc;
    TRAINER_SWITCH(t, trainer_eval_launch<G>(t, n, TrainRecords<G>{n_records, (const uint8_t *)records, index, sym, 0, bad}, rows_out, flags_out,
                                             totals_out, (hipStream_t)stream);
                   break);
    HIPCHK(hipGetLastError());
    return BB_OK;
}

extern "C" int bb_trainer_eval_tensors(bb_trainer *t, int n, const float *boards, const float *value, const float *policy, float *rows_out,
                                       uint8_t *flags_out, bb_eval_totals *totals_out, void *stream) {
    if (n > 0 && (!boards || !value || !policy)) return fail(BB_ERR_ARG, "boards, value and policy are required");
    if (((uintptr_t)boards | (uintptr_t)value | (uintptr_t)policy) % sizeof(float)) return fail(BB_ERR_ARG, "float32 pointers must be 4-byte aligned");
    if (int rc = trainer_eval_prepare(t, n, &rows_out, &flags_out, totals_out)) return rc;
    TRAINER_SWITCH(t, trainer_eval_launch<G>(t, n, TrainTensors<G>{boards, value, policy}, rows_out, flags_out, totals_out, (hipStream_t)stream); break);
    HIPCHK(hipGetLastError());
    return BB_OK;
}

extern "C" int bb_trainer_param_count(bb_trainer *t, int64_t *count_out) {
    if (!t || !count_out) return fail(BB_ERR_ARG, "null argument");
    *count_out = t->lay.count;
    return BB_OK;
}

extern "C" int bb_trainer_read(bb_trainer *t, int what, float *host_out, int64_t count) {
    if (!t || !host_out) return fail(BB_ERR_ARG, "null argument");
    const float *src = nullptr;
    int64_t want = t->lay.count;
    switch (what) {
    case BB_TRAIN_PARAMS: src = t->prm; break;
    case BB_TRAIN_GRADS: src = t->grads; break;
    case BB_TRAIN_SLOT_M: src = t->slot_m; break;
    case BB_TRAIN_SLOT_V: src = t->slot_v; break;
    case BB_TRAIN_NOISE: src = t->aux->noise; want = t->A; break;
    default: return fail(BB_ERR_ARG, "unknown selector %d", what);
    }
    if (count != want) return fail(BB_ERR_ARG, "count %lld, expected %lld", (long long)count, (long long)want);
    int prev = 0;
    HIPCHK(hipGetDevice(&prev));
    HIPCHK(hipSetDevice(t->cfg.device));
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host_out, src, (size_t)want * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) return fail(BB_ERR_HIP, "reading the trainer failed: %s", hipGetErrorString(e));
    return BB_OK;
}

// The trainer's parameters are bb_net_weights' fields back to back (TrainLayout): a descriptor into them, packed on the device.
extern "C" int bb_trainer_load_engine(bb_trainer *t, bb_engine *e, void *stream) {
    if (!t || !e) return fail(BB_ERR_ARG, "null argument");
    if (t->cfg.game != e->cfg.game) return fail(BB_ERR_ARG, "the trainer is of game %d, the engine of game %d", t->cfg.game, e->cfg.game);
    if (t->cfg.device != e->cfg.device)
        return fail(BB_ERR_ARG, "the trainer lives on device %d, the engine on device %d", t->cfg.device, e->cfg.device);
    const TrainLayout &l = t->lay;
    const float *p = t->prm;
    bb_net_weights w = {};
    w.H = e->info.H; w.W = e->info.W; w.C = t->C; w.F = BB_TRAIN_F; w.R = l.R; w.D = l.D; w.A = t->A;
#define X(name, kind, units, per) w.name = p + l.name;
    BB_NET_BLOCKS(X)
#undef X
    return load_weights_device(e, &w, (hipStream_t)stream, "bb_trainer_load_engine");
}

extern "C" int bb_timing_net(bb_engine *e, int iters, int noise, int ablate, double *ms_per_launch_out) {
    if (!e || iters <= 0) return fail(BB_ERR_ARG, "bad arguments");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
#ifndef BB_DIAG
    if (ablate) return fail(BB_ERR_ARG, "the ablation switches exist in diagnostic builds only (-DBB_DIAG)");
#endif
    HIPCHK(hipSetDevice(e->cfg.device));
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    TreeDev &d = e->dev;
    int saved = e->net.dbg;
    e->net.dbg = ablate;
    int rc = BB_OK;
    GAME_SWITCH(e->cfg.game, {
        const typename G::State *ls = (const typename G::State *)d.leaf_state;
        for (int i = 0; i < 3 && !rc; i++)
            rc = launch_net<G>(e, d.n_slots, ls, nullptr, d.leaf_game_id, d.leaf_serial, noise, d.eval_value, nullptr,
                               d.eval_policy, G::S, e->stream);
        HIPCHK(hipEventRecord(a, e->stream));
        for (int i = 0; i < iters && !rc; i++)
            rc = launch_net<G>(e, d.n_slots, ls, nullptr, d.leaf_game_id, d.leaf_serial, noise, d.eval_value, nullptr,
                               d.eval_policy, G::S, e->stream);
        HIPCHK(hipEventRecord(b, e->stream));
        break;
    });
    e->net.dbg = saved;
    if (rc) return rc;
    HIPCHK(hipEventSynchronize(b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (ms_per_launch_out) *ms_per_launch_out = (double)ms / iters;
    return BB_OK;
}


#ifdef BB_STAMPS // (host API of the diagnostic builds; the switches and the stamp-word map: stamps.hip.h)
// diagnostic builds only: point the stamp buffer at host-coherent memory so that it can be read while a kernel runs
extern "C" int bb_debug_host_stamps(bb_engine *e, unsigned long long **host_out) {
    unsigned long long *p = nullptr;
    HIPCHK(hipHostMalloc((void **)&p, STAMP_BUFFER_BYTES, hipHostMallocCoherent | hipHostMallocMapped));
    memset(p, 0, STAMP_BUFFER_BYTES);
    e->dev.stamps = p;
    for (int v = 0; v < 2; v++) e->view[v].stamps = p;
    *host_out = p;
    return BB_OK;
}
extern "C" int bb_debug_net_stamps(bb_engine *e, unsigned long long *out8) {
    HIPCHK(sync_all(e));
    HIPCHK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_net_stamps), NET_STAMP_WORDS * 8));
    unsigned long long z[NET_STAMP_WORDS] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_net_stamps), z, sizeof(z)));
    return BB_OK;
}
extern "C" int bb_stream_done(bb_engine *e) { return hipStreamQuery(e->stream) == hipSuccess ? 1 : 0; }
// diagnostic builds only (tools/): in-kernel cycle stamps accumulated by the tree / persistent kernels
extern "C" int bb_debug_stamps(bb_engine *e, unsigned long long *out8) {
    HIPCHK(sync_all(e));
    unsigned long long all[STAMP_BUFFER_WORDS]; // STAMP_COPIES copies (the DragonChess kernels spread their flushes), summed here
    HIPCHK(hipMemcpy(all, e->dev.stamps, sizeof(all), hipMemcpyDeviceToHost));
    for (int i = 0; i < STAMP_WORDS; i++) {
        out8[i] = 0;
        for (int c = 0; c < STAMP_COPIES; c++) out8[i] += all[c * STAMP_WORDS + i];
    }
    HIPCHK(hipMemset(e->dev.stamps, 0, sizeof(all)));
    return BB_OK;
}
#endif
