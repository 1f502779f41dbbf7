// host_selfplay.hip.h -- self-play: the structure an engine plays through, start positions, begin / step in every launch
// structure, counters and bb_selfplay_done.
#pragma once
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

// ---- self-play ----------------------------------------------------------------------------------------
// The device side of starts_replace (starts.h) for one engine; the checks run on the engine's stream
template <class G>
static StartsOps starts_ops(bb_engine *e) {
    StartsOps ops;
    ops.ctx = e;
    ops.alloc = [](void *, size_t bytes, void **out) -> int {
        const int r = HIP_OPS.alloc(nullptr, bytes, out);
        if (r != hipSuccess) (void)hipGetLastError();
        return r == hipSuccess ? 0 : r == hipErrorOutOfMemory ? 1 : 2;
    };
    ops.upload = [](void *, void *dst, const void *src, size_t bytes) -> int { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess; };
    ops.check = [](void *ctx, const void *dev_states, int n, uint8_t *verdict_out) -> int {
        bb_engine *en = (bb_engine *)ctx;
        Staged<uint8_t> dv;
        if (dv.alloc((size_t)n)) return 1;
        Launch<G>::check_starts(en->stream, n, (const typename G::State *)dev_states, dv.get());
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(en->stream) != hipSuccess) return 1;
        return dv.to_host(verdict_out) != 0;
    };
    ops.release = HIP_OPS.free;
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

// The temperature of the move out of ply `ply` under the schedule (plies, late); plies < 0: no schedule.  The host's copy of the
// select in selfplay_move_body / dc_selfplay_move_body (the arena picks per enqueued ply with it).
static double scheduled_temp(double temp, int plies, double late, int ply) { return plies < 0 || ply < plies ? temp : late; }

extern "C" int bb_selfplay_set_temp_schedule(bb_engine *e, int plies, double temp_late) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    if (!(temp_late >= 0.0 && temp_late < INFINITY))
        return fail(BB_ERR_ARG, "bb_selfplay_set_temp_schedule: temp_late must be finite and >= 0");
    e->sched_plies = plies < 0 ? -1 : plies; // (host state: the next bb_selfplay_begin copies it next to temp)
    e->sched_late = temp_late;
    return BB_OK;
}

extern "C" int bb_selfplay_begin(bb_engine *e, int n_games, double temp) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    if (n_games <= 0) return fail(BB_ERR_ARG, "Use a positive integer for number of games."); // Blackbird.py:235-236
    if (e->dev.track_anc && e->cfg.game == BB_GAME_DRAGONCHESS) // (its self-play kernels do not keep the chain)
        return fail(BB_ERR_STATE, "DragonChess self-play does not keep ancestor chains: create the engine without track_ancestors");
    if (n_games > e->cfg.max_games)
        return fail(BB_ERR_CAPACITY, "n_games %d exceeds the engine's max_games %d", n_games, e->cfg.max_games);
    const bool sched = e->sched_plies >= 0;
    if (e->sims_now < 2 && (temp != 0.0 || (sched && e->sched_late != 0.0))) // (either temperature of a schedule)
        return fail(BB_ERR_NAN, "probabilities contain NaN (a fresh root needs >= 2 simulations, MCTS.py:336-338)");
    int rc = check_eval(e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->cfg.device));
    e->n_games_target = n_games;
    e->dev.n_games_target = n_games;
    e->dev.temp = temp;
    e->dev.temp_late = sched ? e->sched_late : temp;
    e->dev.temp_plies = sched ? e->sched_plies : INT_MAX;
    for (int v = 0; v < 2; v++) {
        e->view[v].temp_late = e->dev.temp_late;
        e->view[v].temp_plies = e->dev.temp_plies;
    }
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
