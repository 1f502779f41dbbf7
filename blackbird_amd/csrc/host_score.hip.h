// host_score.hip.h -- bb_examples_score: example records scored with the network an engine holds (examples_score.hip.h).
#pragma once

// The caller's workspace for chunks of c rows: the gathered states, value[c], ok[c] and logits[c][A], each part starting on a
// 16-byte boundary.  bytes grows with c and is a multiple of 16.
struct ScoreWorkspace {
    size_t states, value, ok, logits, bytes;
};
static ScoreWorkspace score_workspace(const bb_game_info &gi, size_t c) {
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    ScoreWorkspace w;
    w.states = 0;
    w.value = w.states + up(c * (size_t)gi.state_bytes);
    w.ok = w.value + up(c * sizeof(float));
    w.logits = w.ok + up(c);
    w.bytes = w.logits + up(c * (size_t)gi.A * sizeof(float));
    return w;
}

extern "C" int bb_examples_score_workspace(bb_engine *e, int rows_per_chunk, uint64_t *bytes_out) {
    if (!e || !bytes_out || rows_per_chunk < 0) return fail(BB_ERR_ARG, "bb_examples_score_workspace: an engine, rows_per_chunk >= 0 and a place for the size");
    *bytes_out = (uint64_t)score_workspace(e->info, (size_t)rows_per_chunk).bytes;
    return BB_OK;
}

template <class G>
static int examples_score(bb_engine *e, int n_records, const uint8_t *rec, int n, const int64_t *index, float *rows, uint8_t *flags,
                          int32_t *bad, uint8_t *ws, int chunk) {
    const ScoreWorkspace w = score_workspace(e->info, (size_t)chunk);
    auto *states = (typename G::State *)(ws + w.states);
    float *value = (float *)(ws + w.value), *logits = (float *)(ws + w.logits);
    uint8_t *ok = ws + w.ok;
    hipStream_t st = e->stream;
    for (int first = 0; first < n; first += chunk) {
        const int c = n - first < chunk ? n - first : chunk;
        k_score_gather<G><<<nblk((size_t)c), 256, 0, st>>>(n_records, rec, c, first, index, states, ok, bad);
        if (int rc = launch_net<G>(e, c, states, nullptr, nullptr, nullptr, 0, value, logits, nullptr, G::A, st)) return rc;
        k_score_rows<G><<<nblk((size_t)c, 4), 256, 0, st>>>(n_records, rec, c, first, index, ok, value, logits, rows, flags);
    }
    return BB_OK;
}

extern "C" int bb_examples_score(bb_engine *e, int n_records, const void *records, int n, const int64_t *index, float *rows_out,
                                 uint8_t *flags_out, bb_eval_totals *totals_out, int32_t *bad, void *workspace, uint64_t workspace_bytes,
                                 void *stream) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    if (n < 0 || n_records < 0) return fail(BB_ERR_ARG, "negative count (%d rows of %d records)", n, n_records);
    if (int rc = score_outputs_ok(totals_out)) return rc;
    if ((uintptr_t)records % 16 || (uintptr_t)workspace % 16 || (uintptr_t)index % sizeof(int64_t) || ((uintptr_t)rows_out | (uintptr_t)bad) % 4)
        return fail(BB_ERR_ARG, "records and workspace must be 16-byte aligned, index 8-byte, rows_out and bad 4-byte");
    if (n > 0 && (!records || !rows_out || !flags_out || !workspace))
        return fail(BB_ERR_ARG, "records, rows_out, flags_out and workspace are required when there are rows");
    int chunk = 0;
    if (n > 0) { // the rows the given workspace holds: the largest c whose layout fits (score_workspace grows with c)
        const size_t per_row = (size_t)e->info.state_bytes + sizeof(float) + 1 + (size_t)e->info.A * sizeof(float);
        size_t c = (size_t)(workspace_bytes / per_row);
        if (c > (size_t)n) c = (size_t)n;
        while (c > 0 && score_workspace(e->info, c).bytes > workspace_bytes) c--;
        if (c == 0)
            return fail(BB_ERR_ARG, "a workspace of %llu bytes does not hold one row (%zu bytes: bb_examples_score_workspace)",
                        (unsigned long long)workspace_bytes, score_workspace(e->info, 1).bytes);
        chunk = (int)c;
    }
    if (e->cfg.evaluator != BB_EVAL_NET) return fail(BB_ERR_WEIGHTS, "bb_examples_score scores with the engine's network; this engine's evaluator is not the network");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    if (int rc = engine_on_current_device(e, "bb_examples_score", "records")) return rc;
    // a score never runs beside a search; behind whatever `stream` has queued (the records, the index) ...
    if (int rc = engine_stream_after(e, (hipStream_t)stream)) return rc;
    if (n > 0) {
        const uint8_t *rec = (const uint8_t *)records;
        GAME_SWITCH(e->cfg.game, if (int rc = examples_score<G>(e, n_records, rec, n, index, rows_out, flags_out, bad, (uint8_t *)workspace, chunk)) return rc;
                    break);
    }
    k_train_eval_totals<<<1, BB_TRAIN_THREADS, 0, e->stream>>>(n, rows_out, flags_out, (EvalTotals *)totals_out);
    HIPCHK(hipGetLastError());
    // ... and `stream` goes on once the figures are there
    return engine_stream_release(e, (hipStream_t)stream);
}
