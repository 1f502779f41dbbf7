// host_timing.hip.h -- timing and diagnostics: bb_timing_enable / read / net, and the stamp entry points of diagnostic builds.
#pragma once
extern "C" int bb_timing_enable(bb_engine *e, int every_n) {
    if (!e || every_n < 0) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    while (every_n > 0 && e->ev_pool.size() < 2 * 512) { // (a call that fails here leaves a shorter pool of good events; the next goes on)
        hipEvent_t ev = nullptr;
        if (int rc = e->own.event(ev, true)) return rc;
        e->ev_pool.push_back(ev);
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

extern "C" int bb_timing_net(bb_engine *e, int iters, int noise, int ablate, double *ms_per_launch_out) {
    if (!e || iters <= 0) return fail(BB_ERR_ARG, "bad arguments");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
#ifndef BB_DIAG
    if (ablate) return fail(BB_ERR_ARG, "the ablation switches exist in diagnostic builds only (-DBB_DIAG)");
#endif
    HIPCHK(hipSetDevice(e->cfg.device));
    DevOwner timing(HIP_OPS); // destroys the two events on every way out
    hipEvent_t a = nullptr, b = nullptr;
    if (timing.event(a, true) || timing.event(b, true)) return BB_ERR_HIP;
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
