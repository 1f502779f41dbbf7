// host_examples.hip.h -- example records: fetching them, turning them into batches, merging duplicate positions.
#pragma once
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
    Staged<int32_t> d_ids, d_off;
    Staged<uint4> d_out; // (records in the 16-byte units the kernel copies them in)
    if (d_ids.alloc((size_t)n) || d_off.alloc(off.size()) || d_out.alloc((size_t)total * (eb / 16))) return BB_ERR_HIP;
    if (int rc = d_ids.from_host(game_ids)) return rc;
    if (int rc = d_off.from_host(off.data())) return rc;
    k_gather_examples<<<nblk((size_t)total * (eb / 16)), 256, 0, e->stream>>>(e->dev.examples, per, (int)(eb / 16), n, d_ids.get(), d_off.get(),
                                                                            d_out.get());
    HIPCHK(hipGetLastError());
    HIPCHK(sync_all(e));
    if (int rc = d_out.to_host(records_out)) return rc;
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
