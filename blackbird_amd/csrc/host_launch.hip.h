// host_launch.hip.h -- the launch tables: which kernel a game family launches for a step, and on what grid.
#pragma once
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
