// host_arena.hip.h -- bb_arena: head-to-head games of two engines without the host in the loop.
#pragma once
// ---- the arena on the device (arena.hip.h): Blackbird.TestModels' match loop without the host in it -----------------------
struct bb_arena {
    bb_engine *a = nullptr, *b = nullptr; // borrowed
    ArenaDev dev = {};
    DevOwner own{HIP_OPS}; // dev's arrays and the events
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // prep done (a), b sampled, moved (a), b's roots moved
    double temp = 0.0;
    int sched_plies = -1;    // bb_arena_set_temp_schedule (host state; < 0: no schedule): what the next bb_arena_begin takes ...
    double sched_late = 0.0;
    int run_plies = -1;      // ... and what the run begun last plays under: ply p of the match samples at scheduled_temp(.., p)
    double run_late = 0.0;
    int enqueued = 0; // plies enqueued since bb_arena_begin
    bool begun = false;
};

extern "C" int bb_arena_destroy(bb_arena *ar) {
    if (!ar) return BB_OK;
    (void)hipSetDevice(ar->a->cfg.device);
    (void)sync_all(ar->a);
    (void)sync_all(ar->b);
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
    Building<bb_arena, bb_arena_destroy> built(new bb_arena());
    bb_arena *ar = built.get();
    ar->a = a;
    ar->b = b;
    ArenaDev &d = ar->dev;
    const size_t n = (size_t)a->cfg.n_slots;
    d.n_slots = (int)n;
    d.log_plies = log_plies;
    uint8_t *st = nullptr;
    auto take = [&](auto *&p, size_t count) { return ar->own.alloc(p, count, false); }; // (bb_arena_begin fills them)
    if (take(st, n * (size_t)a->info.state_bytes) || take(d.a_to_move, n) || take(d.a_player, n) || take(d.alive, n) || take(d.primed_a, n) ||
        take(d.primed_b, n) || take(d.result, n) || take(d.plies, n) || take(d.err, n) || take(d.log, n * (size_t)log_plies) || take(d.mask_a, n) ||
        take(d.mask_b, n) || take(d.prime_a, n) || take(d.prime_b, n) || take(d.mv_a, n) || take(d.mv_b, n) || take(d.gids, n))
        return BB_ERR_HIP;
    d.states = st;
    for (hipEvent_t &ev : ar->ev)
        if (ar->own.event(ev, false)) return BB_ERR_HIP;
    *out = built.release();
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
        Staged<uint8_t> dv;
        if (dv.alloc((size_t)n_games)) return BB_ERR_HIP;
        Launch<G>::check_starts(ar->a->stream, n_games, (const State *)d.states, dv.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ar->a->stream));
        std::vector<uint8_t> verdict((size_t)n_games);
        if (int rc = dv.to_host(verdict.data())) return rc;
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

extern "C" int bb_arena_set_temp_schedule(bb_arena *ar, int plies, double temp_late) {
    if (!ar) return fail(BB_ERR_ARG, "bb_arena_set_temp_schedule: null arena");
    if (!(temp_late >= 0.0 && temp_late < INFINITY))
        return fail(BB_ERR_ARG, "bb_arena_set_temp_schedule: temp_late must be finite and >= 0");
    ar->sched_plies = plies < 0 ? -1 : plies;
    ar->sched_late = temp_late;
    return BB_OK;
}

extern "C" int bb_arena_begin(bb_arena *ar, int n_games, const uint8_t *a_first, const void *start_states, double temp) {
    if (!ar || !a_first) return fail(BB_ERR_ARG, "bb_arena_begin: null argument");
    if (n_games < 1 || n_games > ar->dev.n_slots)
        return fail(BB_ERR_ARG, "bb_arena_begin: n_games = %d outside 1 .. n_slots = %d", n_games, ar->dev.n_slots);
    if (!(temp >= 0)) return fail(BB_ERR_ARG, "bb_arena_begin: temp must be >= 0");
    for (bb_engine *e : {ar->a, ar->b}) {
        if (int rc = check_eval(e)) return rc;
        if (e->sims_now < 2 && (temp != 0.0 || (ar->sched_plies >= 0 && ar->sched_late != 0.0))) // (bb_selfplay_begin's rule)
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
    ar->run_plies = ar->sched_plies;
    ar->run_late = ar->sched_late;
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
    // every live game is on ply `enqueued` of the match (they all began at bb_arena_begin): the schedule is chosen here, per ply
    const double temp = scheduled_temp(ar->temp, ar->run_plies, ar->run_late, ar->enqueued);
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
        Launch<G>::sample(t, e->edges, e->stream, temp, e->d_child_action);
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
