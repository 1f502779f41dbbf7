// host_trainer.hip.h -- bb_trainer: the fused training step, whole epochs, scoring rows, and the hand-off to an engine.
#pragma once
// ---- the training step (train.hip.h) ----------------------------------------------------------------------------------
struct bb_trainer {
    bb_train_config cfg;
    TrainLayout lay;
    int A, P, C;
    size_t lds_bytes;
    DevOwner own{HIP_OPS}; // the arrays below
    float *prm, *slot_m, *slot_v, *grads, *slabs, *le, *lp, *loss;
    uint8_t *kind;
    TrainAux *aux;
    float *noise, *L; // A floats each: the dense games' lie in *aux, DragonChess's in one allocation of 2 A floats (k_train_prep_wide)
    float *eval_rows; // scratch of bb_trainer_eval for callers that pass no rows_out / flags_out: grows, never shrinks
    uint8_t *eval_flags;
    size_t eval_cap;  // rows the scratch holds
    uint64_t calls; // steps made so far, gradient-only ones included: the counter of the noise stream
    int64_t t;      // updates applied so far: AdamOptimizer's beta powers
    int loss_kind = BB_LOSS_REFERENCE; // BB_LOSS_*: which loss the next step takes (bb_trainer_set_loss)
    float l2 = 0.f;               // BB_LOSS_PER_EXAMPLE: the coefficient of the L2 term
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

// `using G = ` the trainer's dense game around the statements given, GAME_SWITCH's way: the dispatch of the records source and the
// scorer, which DragonChess (trainer_is_wide) never reaches (trainer_not_wide), so that neither TrainRecords<DragonChess> nor
// k_train_eval<DragonChess, ...> is made.  TRAINER_SWITCH_TENSORS: every game -- what is fed by batch tensors alone (the step).
#define TRAINER_SWITCH(t, ...)                                                   \
    switch ((t)->cfg.game) {                                                     \
    case BB_GAME_CONNECT4: { using G = Connect4; __VA_ARGS__; }                  \
    default: { using G = TicTacToe; __VA_ARGS__; }                               \
    }
#define TRAINER_SWITCH_TENSORS(t, ...)                                           \
    switch ((t)->cfg.game) {                                                     \
    case BB_GAME_DRAGONCHESS: { using G = DragonChess; __VA_ARGS__; }            \
    case BB_GAME_CONNECT4: { using G = Connect4; __VA_ARGS__; }                  \
    default: { using G = TicTacToe; __VA_ARGS__; }                               \
    }

static bool trainer_is_wide(const bb_trainer *t) { return t->cfg.game == BB_GAME_DRAGONCHESS; }
static int trainer_not_wide(const bb_trainer *t, const char *who) {
    if (trainer_is_wide(t))
        return fail(BB_ERR_ARG, "%s: the records source and the scorer do not cover DragonChess (compact child lists: a row's share of "
                    "an action is a search); step it from batch tensors with bb_trainer_step", who);
    return BB_OK;
}

// the entry points that launch do not switch devices: the caller's current device must be the trainer's
static int trainer_on_device(const bb_trainer *t) {
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (dev != t->cfg.device) return fail(BB_ERR_ARG, "the trainer lives on device %d, the current device is %d", t->cfg.device, dev);
    return BB_OK;
}

template <class G>
static int trainer_lds(bb_trainer *t) { // (the same dynamic LDS whichever source feeds the workgroup and whichever loss it takes)
    t->lds_bytes = (size_t)train_lds_floats<G>(t->lay.R) * sizeof(float);
    const int bytes = (int)t->lds_bytes;
    HIPCHK(hipFuncSetAttribute((const void *)k_train_grad<G, TrainTensors<G>, BB_LOSS_REFERENCE>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    HIPCHK(hipFuncSetAttribute((const void *)k_train_grad<G, TrainTensors<G>, BB_LOSS_PER_EXAMPLE>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if constexpr (TrainScratch<G>::dense) { // the records source: the dense games alone (TRAINER_SWITCH)
        HIPCHK(hipFuncSetAttribute((const void *)k_train_grad<G, TrainRecords<G>, BB_LOSS_REFERENCE>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        HIPCHK(hipFuncSetAttribute((const void *)k_train_grad<G, TrainRecords<G>, BB_LOSS_PER_EXAMPLE>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    }
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
    const size_t params = (size_t)l.count, batch = (size_t)t->cfg.max_batch;
    auto take = [&](auto *&p, size_t count) { return t->own.alloc(p, count, false); }; // (filled below where the kernels read before they write)
    if (take(t->prm, params) || take(t->slot_m, params) || take(t->slot_v, params) || take(t->grads, params) || take(t->slabs, params * batch) ||
        take(t->le, batch) || take(t->lp, batch) || take(t->loss, 4) || take(t->kind, params) || take(t->aux, 1))
        return BB_ERR_HIP;
    HIPCHK(hipMemset(t->slot_m, 0, cb));
    HIPCHK(hipMemset(t->slot_v, 0, cb));
    HIPCHK(hipMemset(t->grads, 0, cb));
    HIPCHK(hipMemset(t->loss, 0, 4 * sizeof(float)));
    HIPCHK(hipMemset(t->aux, 0, sizeof(TrainAux)));
    if (trainer_is_wide(t)) {
        if (take(t->noise, 2 * (size_t)t->A)) return BB_ERR_HIP;
        HIPCHK(hipMemset(t->noise, 0, 2 * (size_t)t->A * sizeof(float)));
        t->L = t->noise + t->A;
    } else {
        t->noise = (float *)t->aux + offsetof(TrainAux, noise) / sizeof(float); // (addresses inside the device's TrainAux)
        t->L = (float *)t->aux + offsetof(TrainAux, L) / sizeof(float);
    }
    const NetBlocks tb = net_blocks(t->C, BB_TRAIN_F, l.R, l.D, t->A); // (what train_layout took l from)
    const std::vector<uint8_t> kind = net_block_kinds(tb);
    HIPCHK(hipMemcpy(t->kind, kind.data(), kind.size(), hipMemcpyHostToDevice));
    for (int i = 0; i < NET_BLOCKS; i++)
        if (const int n = tb.b[i].count())
            HIPCHK(hipMemcpy(t->prm + tb.b[i].at, net_block(*w, i), (size_t)n * sizeof(float), hipMemcpyDefault));
    TRAINER_SWITCH_TENSORS(t, return trainer_lds<G>(t));
}

extern "C" int bb_trainer_create(const bb_train_config *cfg, const bb_net_weights *w, bb_trainer **out) {
    if (!cfg || !w || !out) return fail(BB_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->game != BB_GAME_CONNECT4 && cfg->game != BB_GAME_TICTACTOE && cfg->game != BB_GAME_DRAGONCHESS)
        return fail(BB_ERR_ARG, "the HIP trainer covers Connect4, TicTacToe and DragonChess, not game %d", cfg->game);
    bb_game_info gi;
    bb_game_info_get(cfg->game, &gi);
    if (int rc = check_weights(w, gi)) return rc;
    // DragonChess: the blocks whose k_train_grad workgroup fits a CU's LDS (train_max_blocks, train.hip.h)
    const int max_blocks = cfg->game == BB_GAME_DRAGONCHESS ? train_max_blocks<DragonChess>() : 9;
    if (w->F != BB_TRAIN_F || w->R < 0 || w->R > max_blocks || w->D < 1 || w->D > 64)
        return fail(BB_ERR_ARG, "the HIP trainer covers 16 filters, 0..%d blocks%s and a dense width of 1..64; got %d filters, %d blocks, "
                    "dense %d", max_blocks, cfg->game == BB_GAME_DRAGONCHESS ? " (DragonChess: the 160 KB of LDS of a CU)" : "", w->F,
                    w->R, w->D);
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
    Building<bb_trainer, bb_trainer_destroy> built(new bb_trainer());
    bb_trainer *t = built.get();
    t->cfg = *cfg;
    t->A = gi.A; t->P = gi.H * gi.W; t->C = gi.C;
    t->lay = train_layout(gi.C, w->R, w->D, gi.A);
    const int rc = trainer_alloc(t, w);
    (void)hipSetDevice(prev);
    if (rc) return rc;
    *out = built.release();
    return BB_OK;
}

// Which loss the steps after this call take: host state only -- no launch, no allocation, nothing of the device touched.
extern "C" int bb_trainer_set_loss(bb_trainer *t, int loss, double l2) {
    if (loss != BB_LOSS_REFERENCE && loss != BB_LOSS_PER_EXAMPLE)
        return fail(BB_ERR_ARG, "unknown loss %d (BB_LOSS_REFERENCE = 0, BB_LOSS_PER_EXAMPLE = 1)", loss);
    if (!(l2 >= 0.0) || !std::isfinite(l2) || !std::isfinite((float)l2)) return fail(BB_ERR_ARG, "l2 must be a finite number >= 0, got %g", l2);
    if (!t) return fail(BB_ERR_ARG, "null trainer");
    t->loss_kind = loss;
    t->l2 = (float)l2;
    return BB_OK;
}

// the per-example loss has no noise term: a caller that passes one has mistaken the mode
static int trainer_noise_ok(const bb_trainer *t, const float *noise, const char *who) {
    if (noise && t->loss_kind == BB_LOSS_PER_EXAMPLE)
        return fail(BB_ERR_ARG, "%s: the per-example loss (BB_LOSS_PER_EXAMPLE) takes no noise; pass NULL", who);
    return BB_OK;
}

extern "C" int bb_trainer_destroy(bb_trainer *t) {
    if (!t) return BB_OK;
    int prev = 0;
    const bool ok = hipGetDevice(&prev) == hipSuccess && hipSetDevice(t->cfg.device) == hipSuccess;
    if (ok) (void)hipDeviceSynchronize();
    delete t;
    if (ok) (void)hipSetDevice(prev);
    return BB_OK;
}

// The last of a step's three launches: Adam's step count and lr_t move here, as the launch is made.
static void trainer_launch_apply(bb_trainer *t, int n, double lr, int apply, float *loss_out, hipStream_t st) {
    const TrainLayout &l = t->lay;
    float rate = (float)lr;
    if (apply) {
        t->t++;
        if (t->cfg.optimizer == BB_OPT_ADAM) // AdamOptimizer's lr_t (beta1 0.9, beta2 0.999)
            rate = (float)(lr * std::sqrt(1.0 - std::pow(0.999, (double)t->t)) / (1.0 - std::pow(0.9, (double)t->t)));
    }
    k_train_apply<<<nblk((size_t)l.count, BB_TRAIN_THREADS) + 1, BB_TRAIN_THREADS, 0, st>>>(
        l.count, n, l.n_l2, t->loss_kind, t->l2, t->slabs, t->kind, t->prm, t->slot_m, t->slot_v, t->grads, t->cfg.optimizer, rate, t->cfg.momentum,
        apply != 0, t->le, t->lp, t->aux, t->loss, loss_out);
}

// One step's three launches on `st`, the batch read through `src` (train.hip.h): what bb_trainer_step and every batch of
// bb_trainer_epoch enqueue.  Host state moves as the launches are made: the noise counter, Adam's step count and lr_t.
// The loss is a template argument of prep and grad (train.hip.h): the per-example step takes the same launches with other kernels.
// The prep kernel is the game family's: one workgroup for the dense games, 1 + ceil(A / 256) for DragonChess (per example: one --
// there is no label sweep).
template <class G, class Src, int LOSS>
static void trainer_launch_as(bb_trainer *t, int n, const Src &src, const float *noise, double lr, int apply, float *loss_out, hipStream_t st) {
    const TrainLayout &l = t->lay;
    const float eps = t->cfg.epsilon;
    if constexpr (TrainScratch<G>::dense) {
        k_train_prep<G, Src, LOSS><<<1, BB_TRAIN_THREADS, 0, st>>>(n, l.count, l.n_l2, t->prm, t->kind, src, noise, eps, t->cfg.alpha, t->cfg.seed,
                                                                   t->calls, t->l2, t->aux);
    } else {
        const unsigned groups = LOSS == BB_LOSS_PER_EXAMPLE ? 1u : 1u + (unsigned)nblk((size_t)G::A, BB_TRAIN_THREADS);
        k_train_prep_wide<G, Src, LOSS><<<groups, BB_TRAIN_THREADS, 0, st>>>(n, l.count, l.n_l2, t->prm, t->kind, src, noise, eps, t->cfg.alpha,
                                                                             t->cfg.seed, t->calls, t->l2, t->aux, t->noise, t->L);
    }
    t->calls++;
    k_train_grad<G, Src, LOSS><<<n, BB_TRAIN_THREADS, t->lds_bytes, st>>>(l, t->prm, t->aux, t->noise, t->L, src, n, eps, t->slabs, t->le, t->lp);
    trainer_launch_apply(t, n, lr, apply, loss_out, st);
}

template <class G, class Src>
static void trainer_launch(bb_trainer *t, int n, const Src &src, const float *noise, double lr, int apply, float *loss_out, hipStream_t st) {
    if (t->loss_kind == BB_LOSS_PER_EXAMPLE)
        trainer_launch_as<G, Src, BB_LOSS_PER_EXAMPLE>(t, n, src, noise, lr, apply, loss_out, st);
    else
        trainer_launch_as<G, Src, BB_LOSS_REFERENCE>(t, n, src, noise, lr, apply, loss_out, st);
}

extern "C" int bb_trainer_step(bb_trainer *t, int n, const float *boards, const float *value, const float *policy, const float *noise,
                               double lr, int apply, float *loss_out, void *stream) {
    if (!t) return fail(BB_ERR_ARG, "null trainer");
    if (n <= 0 || n > t->cfg.max_batch) return fail(BB_ERR_ARG, "a batch of %d examples; the trainer takes 1..%d (max_batch)", n, t->cfg.max_batch);
    if (!boards || !value || !policy) return fail(BB_ERR_ARG, "boards, value and policy are required");
    if (((uintptr_t)boards | (uintptr_t)value | (uintptr_t)policy | (uintptr_t)noise | (uintptr_t)loss_out) % sizeof(float))
        return fail(BB_ERR_ARG, "float32 pointers must be 4-byte aligned");
    if (!std::isfinite(lr)) return fail(BB_ERR_ARG, "the learning rate is not finite");
    if (int rc = trainer_noise_ok(t, noise, "bb_trainer_step")) return rc;
    if (int rc = trainer_on_device(t)) return rc;
    TRAINER_SWITCH_TENSORS(t, trainer_launch<G>(t, n, TrainTensors<G>{boards, value, policy}, noise, lr, apply, loss_out, (hipStream_t)stream); break);
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
    if (int rc = trainer_not_wide(t, "bb_trainer_epoch")) return rc;
    if (n_batches < 0 || n_records < 0) return fail(BB_ERR_ARG, "negative count (%d batches, %d records)", n_batches, n_records);
    if (batch <= 0 || batch > t->cfg.max_batch)
        return fail(BB_ERR_ARG, "batches of %d examples; the trainer takes 1..%d (max_batch)", batch, t->cfg.max_batch);
    if (!std::isfinite(lr)) return fail(BB_ERR_ARG, "the learning rate is not finite");
    if ((uintptr_t)order % sizeof(int64_t) || ((uintptr_t)noise | (uintptr_t)loss_out | (uintptr_t)bad_out) % 4)
        return fail(BB_ERR_ARG, "order must be 8-byte aligned, noise, loss_out and bad_out 4-byte aligned");
    if (int rc = trainer_noise_ok(t, noise, "bb_trainer_epoch")) return rc;
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
    if (int rc = trainer_not_wide(t, "bb_trainer_eval")) return rc;
    if (n < 0) return fail(BB_ERR_ARG, "negative count (%d rows)", n);
    if (int rc = score_outputs_ok(totals)) return rc;
    if ((uintptr_t)*rows % sizeof(float)) return fail(BB_ERR_ARG, "float32 pointers must be 4-byte aligned");
    if (int rc = trainer_on_device(t)) return rc;
    if ((!*rows || !*flags) && (size_t)n > t->eval_cap) {
        t->own.release(t->eval_rows); // (hipFree waits for the device: no launch still reads the old scratch)
        t->own.release(t->eval_flags);
        t->eval_rows = nullptr;
        t->eval_flags = nullptr;
        t->eval_cap = 0;
        if (t->own.alloc(t->eval_rows, (size_t)n * 3, false) || t->own.alloc(t->eval_flags, (size_t)n, false)) {
            (void)hipGetLastError();
            t->own.release(t->eval_rows);
            t->eval_rows = nullptr;
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
    case BB_TRAIN_NOISE: src = t->noise; want = t->A; break;
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
