// host_search.hip.h -- the search API: the simulation loop and its timed launches, roots, bb_run_sims*, sampling, node views.
#pragma once
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
    Staged<typename G::State> ds;
    Staged<int32_t> dsl;
    Staged<uint32_t> dg;
    if (ds.alloc((size_t)n) || dsl.alloc((size_t)n) || dg.alloc((size_t)n)) return BB_ERR_HIP;
    if (int rc = ds.from_host(states)) return rc;
    if (slots)
        if (int rc = dsl.from_host(slots)) return rc;
    if (gids)
        if (int rc = dg.from_host(gids)) return rc;
    Launch<G>::set_roots(e->dev, e->edges, e->stream, n, slots ? dsl.get() : nullptr, ds.get(), gids ? dg.get() : nullptr);
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
    Staged<uint8_t> dm; // (null without a mask)
    if (mask) {
        const size_t n = (size_t)e->dev.n_slots;
        if (dm.alloc(n)) return BB_ERR_HIP;
        HIPCHK(hipMemcpyAsync(dm.get(), mask, n, hipMemcpyDefault, e->stream)); // on the engine's stream, in front of the search
    }
    rc = enqueue_sims(e, sims, dm.get());
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
    { // every game: a slot whose chain outgrew its max_plies + 2 entries cannot find its top-most ancestor (tree.hip.h ANC_BROKEN)
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
    Staged<int32_t> da, dc, dp, di; // (da: null where no actions are asked for; di: four words, of which three go out)
    Staged<float> dv;
    Staged<typename G::State> ds;
    if ((action_out && da.alloc(S)) || dc.alloc(S) || dp.alloc(S) || dv.alloc(S) || ds.alloc(1) || di.alloc(4)) return BB_ERR_HIP;
    Launch<G>::node_edges(e->dev, e->edges, e->stream, slot, node, da.get(), dc.get(), dp.get(), dv.get(), ds.get(), di.get());
    HIPCHK(hipGetLastError());
    HIPCHK(sync_all(e));
    if (int rc = dc.to_host(child_node_out)) return rc;
    if (int rc = dp.to_host(child_plays_out)) return rc;
    if (int rc = dv.to_host(child_value_out)) return rc;
    if (int rc = ds.to_host(state_out)) return rc;
    if (int rc = di.to_host(info_out, 3)) return rc;
    return action_out ? da.to_host(action_out) : BB_OK;
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
        Staged<typename G::State> ds;
        if (ds.alloc((size_t)e->dev.n_slots)) return BB_ERR_HIP;
        Launch<G>::get_roots(e->dev, e->edges, e->stream, ds.get());
        HIPCHK(hipGetLastError());
        HIPCHK(sync_all(e));
        return ds.to_host(states_out);
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
