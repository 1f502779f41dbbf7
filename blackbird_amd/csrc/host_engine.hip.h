// host_engine.hip.h -- bb_engine: what it holds, its allocation, slot-range views, pool sizing, bb_create and bb_destroy.
#pragma once
// ---- engine ----------------------------------------------------------------------------------------
// The launch structures of self-play (bb_selfplay_mode's values): lock-step launches per simulation (run_sims); dense games:
// k_tree_async rounds + evaluator; persistent per-CU kernel with an LDS work queue (mega2.hip.h); DragonChess: mega_dc.hip.h; the
// rollout evaluator of every game after bb_selfplay_rollouts(e, 1): one launch per step, a wave per slot (selfplay_wave.hip.h)
enum { PLAY_LOCKSTEP = 0, PLAY_ROUNDS = 1, PLAY_QUEUE = 3, PLAY_DC_FUSED = 5, PLAY_WAVE_ROLLOUT = 6 };
// What a configuration asks for -- the ONE place that reads mcts_kind / evaluator / launch / game / track_ancestors for this.
// (Whether the network fits a persistent kernel's LDS is known only at bb_load_weights: selfplay_structure.)
// track_ancestors: the persistent queue kernel backs a recorded leaf up with stores only (backup_path<G, true>, tree.hip.h), which
// never walks the ancestor chain, and in either form that kernel indexes per-slot arrays with the workgroup-local slot number, which
// is right only for the rows it shadows in LDS -- anc / anc_len / top_N are not among them (mega2.hip.h BB_QUEUE_SHADOWED).  So a
// dense engine that keeps the chain never plans for that kernel: it plays the rounds, whose plain async_game<G> walks the chain,
// with the same network kernels and the same records byte for byte.  (DragonChess self-play refuses such an engine: bb_selfplay_begin.)
static int selfplay_plan(const bb_config *cfg) {
    const bool net_auto = cfg->evaluator == BB_EVAL_NET && cfg->launch == BB_LAUNCH_AUTO;
    if (cfg->mcts_kind != BB_MCTS_DYNAMIC) return PLAY_LOCKSTEP;
    if (cfg->game == BB_GAME_DRAGONCHESS) return net_auto ? PLAY_DC_FUSED : PLAY_LOCKSTEP;
    if (net_auto) return cfg->track_ancestors ? PLAY_ROUNDS : PLAY_QUEUE; // (else rounds, for the deterministic evaluators)
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
    DevOwner own{HIP_OPS}; // every allocation, stream and event below, starts.dev apart; zero fills run on `stream`, its first
    hipStream_t stream = nullptr;
    hipEvent_t w_event[2] = {nullptr, nullptr}; // engine_stream_after / _release: the caller's stream -> the engine's, and back (no timing)
    int n_games_target = 0;
    StartsTable starts; // bb_selfplay_set_starts: the device copy dev.starts / view[].starts point at (starts.h); not in `own`
    int sched_plies = -1;    // bb_selfplay_set_temp_schedule: plies at the run's own temperature (< 0: no schedule) and the
    double sched_late = 0.0; // temperature from there on; host state, copied into dev / view[] by bb_selfplay_begin
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

// The entry points that take a caller's stream do not switch devices: the current device must be the engine's.  `what`: what
// else of the caller's lives there.
static int engine_on_current_device(const bb_engine *e, const char *who, const char *what) {
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (dev != e->cfg.device)
        return fail(BB_ERR_ARG, "%s: the engine lives on device %d, the current device (the stream's and the %s') is %d", who,
                    e->cfg.device, what, dev);
    return BB_OK;
}

// The engine's stream borrowed for a caller that works on `caller`.  After: nothing of the engine is in flight (its own streams
// only are waited for, never `caller`), and e->stream stands behind whatever `caller` has queued.  Release: `caller` goes on
// once e->stream has come this far -- and, with_second, the engine's second stream too.
static int engine_stream_after(bb_engine *e, hipStream_t caller) {
    HIPCHK(sync_all(e));
    HIPCHK(hipEventRecord(e->w_event[0], caller));
    HIPCHK(hipStreamWaitEvent(e->stream, e->w_event[0], 0));
    return BB_OK;
}
static int engine_stream_release(bb_engine *e, hipStream_t caller, bool with_second = false) {
    HIPCHK(hipEventRecord(e->w_event[1], e->stream));
    if (with_second && e->vstream[1]) HIPCHK(hipStreamWaitEvent(e->vstream[1], e->w_event[1], 0));
    HIPCHK(hipStreamWaitEvent(caller, e->w_event[1], 0));
    return BB_OK;
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
#define X(T, f, per) bad = bad || e->own.alloc(d.f, n * (per));
    BB_SLOT_ARRAYS(X)
#undef X
    if (bad || e->own.alloc(e->d_u, n) || e->own.alloc(e->d_actions, n) || e->own.alloc(e->d_child_action, n * S) ||
        e->own.alloc(d.stamps, STAMP_BUFFER_WORDS) || e->own.alloc(d.visit_pool, 16) || e->own.alloc(d.post_count, 8))
        return BB_ERR_HIP;
    typename G::State *ls;
    if (e->own.alloc(ls, n)) return BB_ERR_HIP;
    d.leaf_state = ls;
    uint8_t *nodes;
    if (e->own.alloc(nodes, n * (size_t)d.node_cap * NODE_BYTES, false)) return BB_ERR_HIP;
    d.nodes = nodes;
    if constexpr (DC) {
        DCEdges &E = e->edges;
        E.edge_cap = d.node_cap * 24; // ~15-25 legal moves per position; overflow is counted, never silent
        size_t ne = n * (size_t)E.edge_cap;
        bad = e->own.alloc(E.e, ne, false);
#define X(T, f, per) bad = bad || e->own.alloc(E.f, n * (per));
        BB_DC_SLOT_ARRAYS(X)
#undef X
        if (bad) return BB_ERR_HIP;
        E.noise_on = c.noise_on;
        E.alpha = c.alpha;
        E.eps = c.epsilon;
    }
    size_t ng = (size_t)c.max_games;
    if (e->own.alloc(d.examples, ng * (size_t)(c.max_plies + 1) * (size_t)e->info.example_bytes, false) ||
        e->own.alloc(d.game_hdr, ng * 4))
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
    Building<bb_engine, bb_destroy> built(new bb_engine());
    bb_engine *e = built.get();
    e->cfg = *cfg;
    e->sims_now = cfg->sims_per_move;
    int rc = bb_game_info_get(cfg->game, &e->info);
    if (rc) return rc;
    HIPCHK(hipSetDevice(cfg->device));
    if (e->own.stream(e->stream) || e->own.event(e->w_event[0], false) || e->own.event(e->w_event[1], false)) return BB_ERR_HIP;
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
    if (cfg->launch < 0 || cfg->launch > BB_LAUNCH_WAVE || cfg->net_form < 0 || cfg->net_form > BB_NET_FORM_SPLIT)
        return fail(BB_ERR_ARG, "bad bb_config.launch / net_form");
    e->plan = selfplay_plan(cfg);
    const bool rounds_kernels = e->plan == PLAY_ROUNDS || e->plan == PLAY_QUEUE; // (a queue engine plays rounds when its network does not fit)
    if (int v = env_int("BB_TREE_GPW", 0); v >= 1 && v <= 64 / e->info.S) d.gpw = v;
    d.temp = 1.0;
    d.temp_late = 1.0;
    d.temp_plies = INT_MAX; // no schedule
    GAME_SWITCH(cfg->game, rc = engine_alloc<G>(e); break);
    if (!rc) { // (a configuration that owns a table plays through a structure that probes it: eval_cache_log2_of asks selfplay_plan)
        if (const int k = eval_cache_log2_of(cfg)) {
            uint8_t *tab = nullptr;
            e->eval_cache_bytes = eval_cache_entry_bytes(cfg) << k;
            rc = e->own.alloc(tab, e->eval_cache_bytes); // (zeroed: empty)
            d.eval_cache = tab;
            d.eval_cache_log2 = k;
        }
    }
    if (!rc) rc = e->own.alloc(d.eval_cache_ctr, 2);
    if (!rc && d.eval_cache && rounds_kernels)
        rc = e->own.alloc(e->miss_count, 8) || e->own.alloc(e->miss_slot, (size_t)cfg->n_slots) || e->own.alloc(e->miss_way, (size_t)cfg->n_slots);
    if (rc) return rc;
    e->n_views = 1;
    if (e->plan == PLAY_ROUNDS && cfg->evaluator == BB_EVAL_NET && cfg->n_slots >= 512) e->n_views = 2;
    if (const char *env = getenv("BB_GROUPS")) e->n_views = (atoi(env) == 2 && rounds_kernels && cfg->n_slots >= 2) ? 2 : 1; // (tuning)
    e->vstream[0] = e->stream;
    if (e->n_views == 2 && e->own.stream(e->vstream[1])) return BB_ERR_HIP;
    GAME_SWITCH(cfg->game, make_views<G>(e); break);
    *out = built.release();
    return BB_OK;
}

extern "C" int bb_destroy(bb_engine *e) {
    if (!e) return BB_OK;
    (void)hipSetDevice(e->cfg.device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->vstream[1]) (void)hipStreamSynchronize(e->vstream[1]);
    if (e->starts.dev) HIP_OPS.free(nullptr, e->starts.dev);
    delete e; // (`own`: the events, then the memory, then the streams)
    return BB_OK;
}

extern "C" int bb_synchronize(bb_engine *e) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    if (e->vstream[1]) HIPCHK(hipStreamSynchronize(e->vstream[1]));
    HIPCHK(sync_all(e));
    return BB_OK;
}
