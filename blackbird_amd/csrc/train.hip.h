// train.hip.h -- one optimiser step of Network.train (NetworkFactory.py:185-245) for the 16-filter networks, as three launches
// (bb_trainer_step; bb_trainer_epoch: the same three per batch, for every batch of an epoch):
//   k_train_prep   the step's Beta noise (caller's, or A Philox draws keyed by seed and step count), the batch-wide label sum
//                  L[a] = sum_j label_j[a], log S of the policy normalisation, and the L2 loss term
//   k_train_grad   one workgroup per example: forward with every layer's post-activation and normalised conv output in
//                  LDS, the example's loss pieces, backward, and the gradient of every trainable variable into the
//                  workgroup's own slab in HBM
//   k_train_apply  per parameter element: the slabs summed in example order, + v / N for the non-bias variables, the
//                  TF1 optimiser update in place; its last workgroup reduces the loss terms
// The batch couples the examples in two places only, and neither reaches a gradient across examples: policy / policy.sum()
// divides by S = B (1 - eps) + B eps sum(noise), which holds no weight (softmax rows sum to 1), and
// -mean(log(policy) @ label^T) = -(1 / B^2) sum_i sum_a log policy_i[a] L[a].
// No float atomics: every sum has its order written down here, so the same steps give the same bits.
// The flat parameter vector is bb_net_weights' fields back to back (TrainLayout); a batch-norm block is [4][n] = gamma,
// beta, moving_mean, moving_variance, and the moving statistics are constants (kind 0: no gradient, no update).
// float32 throughout, every fused multiply-add explicit (-ffp-contract=off); the loss sums are taken in double.
//
// One step, a policy head per game family.  k_train_grad is one kernel for every game: the forward tower, the head convolutions,
// value/dense_1, the value loss piece, the heads' backward pass from d logit on, the backward tower and the conv0 weight gradient
// are each written once (tr_tower_fwd, tr_heads_conv, tr_heads_dense, tr_value_loss, tr_heads_bwd, tr_tower_bwd) and called by
// every game.  What differs is the policy head between the head convolutions and d logit -- logits, max, softmax, the two losses,
// d logit, policy/policy's gradients and g_j, the gradient at a square's policy/convolution activation j before its ReLU mask --
// and where a workgroup's head scratch lies (TrainScratch<G>); both are chosen at compile time on G::A <= 16:
//   dense games (Connect4, TicTacToe; A <= 16)   tr_policy_dense: one lane, serially over the A actions
//   wide game (DragonChess: 17 planes, 4032 actions; 0 .. train_max_blocks<DragonChess>() = 8 blocks)   the else branch in
//                  k_train_grad's body: 16 actions a thread, workgroup tree reductions (why it is no function: at its comment)
// The sum orders of each head are written at it.  The noise and L reach k_train_grad as two pointers to A floats each: into
// TrainAux for the dense games, into an allocation of their own for the wide one (TrainAux keeps logS and l2 either way).
// The prep kernels stay two, because their grids and label sweeps differ (k_train_prep: one workgroup; k_train_prep_wide:
// 1 + ceil(A / 256)); they share the L2 sum (tr_l2_partial) and thread 0's epilogue (tr_prep_finish).
//
// The batch reaches the kernels through a source type (Src, below): the caller's three tensors (bb_trainer_step), or the
// example records themselves (bb_trainer_epoch: prep, grad and apply enqueued for every batch of an epoch in one call, no batch
// tensors in between).  k_train_grad never reads the policy rows -- the policy loss reaches it through L alone --, its planes
// are a function of one 16-byte packed state and its value label is the record's z, so a step needs nothing a batch holds
// that the records do not.  Both sources give the kernels the same floats in the same order: batch i of an epoch is, bit for
// bit, the bb_trainer_step the per-batch loop would have made.  DragonChess is fed by the tensors source only -- the records
// source and the scorer (train_eval.hip.h) are not instantiated for it.
// The per-example loss (BB_LOSS_PER_EXAMPLE, bb_trainer_set_loss; opt-in) is a compile-time argument LOSS of the prep and grad
// kernels; the BB_LOSS_REFERENCE instances are the text above, untouched by it.  With it
//   lossPolicy = -(1/n) sum_b sum_a pi_b[a] log_softmax(lg_b)[a],   d loss / d lg_b[a] = (softmax_b[a] T_b - pi_b[a]) / n,   T_b = sum_a pi_b[a]
//   lossParam  = l2 * sum over the kind-1 variables of sum(v^2) / 2,   its gradient l2 * v (k_train_apply, a run-time argument there)
// so a row reads its OWN label (Src::label_of, both sources), nothing couples the rows, and the prep kernels form the L2 sum
// alone: no noise, no L (k_train_prep_wide runs one workgroup instead of 17: its 4032 x n label sweep is gone).  Dense games: lane
// 0's head block, the serial orders of k_train_eval (max, sum of expf, lse, an fmaf chain for the loss piece and for T, a
// ascending).  Wide game: thread tid's 16 labels a = tid + 256 k take the place of m[] (no register is added), the loss piece
// sum_a pi[a] (lg[a] - max), T and the sum of expf are per-thread chains over k ascending in one pass and one tr_tree_sum;
// the row's piece is that sum - lse T (both terms of one sign: nothing cancels).  A row without a label adds 0 and has d lg = 0.
// No float atomics here either.  The step counter that keys the noise stream still advances once per step.
#pragma once
#include "../../include/blackbird_hip.h"
#include "examples.hip.h"
#include "games.hip.h"
#include "rng.hip.h"

#define BB_TRAIN_F 16            // filters
#define BB_TRAIN_WROW 17         // row stride of a staged conv kernel: [tap*CIN + ci][f], read along f (forward, weight
                                 // gradient) and along ci (input gradient) -- an odd stride keeps both off one bank
#define BB_TRAIN_SMALL 896       // floats of the dense games' planes and head scratch (TrainScratch)
#define BB_TRAIN_THREADS 256

struct TrainLayout {
    int R, D;
    // where each block starts, in floats: one member per row of BB_NET_BLOCKS (blackbird_hip.h), named like its field
#define X(name, kind, units, per) int name;
    BB_NET_BLOCKS(X)
#undef X
    int count;
    int n_l2; // trainable variables whose name does not contain `bias`: the N of the L2 mean
};

struct TrainAux {
    float noise[16]; // the step's noise (zeros when epsilon == 0)
    float L[16];     // sum over the batch of the policy labels
    float logS;      // log of the batch-wide normaliser
    float l2;        // lossParam
};

__device__ __forceinline__ float tr_bn_inv(float var) { return 1.0f / sqrtf(var + 1e-3f); }

// The workgroup's sum of every array s[BB_TRAIN_THREADS] given (LDS), left in its [0]: [t] += [t + w] for w = 128, 64, ... 1, a
// barrier after each level.  The caller stores the partial sums and makes the barrier before the call.  One order, so one rounding.
template <class... T>
__device__ __forceinline__ void tr_tree_sum(int tid, T *...s) {
    for (int w = BB_TRAIN_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) ((s[tid] += s[tid + w]), ...);
        __syncthreads();
    }
}
__device__ __forceinline__ void tr_tree_max(int tid, float *s) { // tr_tree_sum's shape with fmaxf
    for (int w = BB_TRAIN_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) s[tid] = fmaxf(s[tid], s[tid + w]);
        __syncthreads();
    }
}

// ---- where a step's examples come from: the Src of k_train_prep and k_train_grad, chosen at compile time ------------------
// A source answers, for row j of the batch: label(j, a), the policy label's entry a (k_train_prep); row(j), whatever it keeps
// of the row in registers, then plane(row, i), element i of the planes [H][W][C], and value(row) (k_train_grad); count(row,
// tid) reports a rejected row.  TrainTensors is bb_trainer_step's three float32 tensors.  TrainRecords is bb_trainer_epoch's:
// row j is example record order[first + j] (nullptr: record first + j) under symmetry sym[first + j] (nullptr: the identity),
// decoded by the functions k_examples_to_batch writes its rows with (examples.hip.h) -- the same floats, never stored; a
// malformed row is zeros there and here, and one integer atomicAdd from one thread of its workgroup counts it in *bad.
// label_of(row, a) and valid(row) serve the forward-only scoring of train_eval.hip.h, which keeps the row it made.
template <class G>
struct TrainTensors {
    const float *__restrict__ boards, *__restrict__ value, *__restrict__ policy;
    struct Row { int j; };
    __device__ __forceinline__ float label(int j, int a) const { return policy[(size_t)j * G::A + a]; }
    __device__ __forceinline__ Row row(int j) const { return {j}; }
    __device__ __forceinline__ float plane(const Row &r, int i) const { return boards[(size_t)r.j * G::H * G::W * G::C + i]; }
    __device__ __forceinline__ float value_of(const Row &r) const { return value[r.j]; }
    __device__ __forceinline__ float label_of(const Row &r, int a) const { return policy[(size_t)r.j * G::A + a]; }
    __device__ __forceinline__ bool valid(const Row &) const { return true; }
    __device__ __forceinline__ void count(const Row &, int) const {}
};

template <class G>
struct TrainRecords {
    int n_records;
    const uint8_t *records;
    const int64_t *order;
    const uint8_t *sym;
    size_t first;
    int32_t *bad;
    using Row = ExampleRow<G>;
    __device__ __forceinline__ Row row(int j) const { return example_row<G>(n_records, records, order, sym, first + (size_t)j); }
    __device__ __forceinline__ float label(int j, int a) const { return example_share<G>(row(j), a); }
    __device__ __forceinline__ float plane(const Row &r, int i) const { return example_plane<G>(r, i); }
    __device__ __forceinline__ float value_of(const Row &r) const { return example_value<G>(r); }
    __device__ __forceinline__ float label_of(const Row &r, int a) const { return example_share<G>(r, a); }
    __device__ __forceinline__ bool valid(const Row &r) const { return r.ok; }
    __device__ __forceinline__ void count(const Row &r, int tid) const {
        if (tid == 0 && !r.ok && bad) atomicAdd(bad, 1);
    }
};

// ---- k_train_prep, k_train_prep_wide ------------------------------------------------------------------------------------
// The L2 sum, every prep path's: thread tid's sum of squares of the kind-1 parameters i = tid, tid + 256, ... ascending, in
// double, into s_sq[tid] for tr_tree_sum.
__device__ __forceinline__ void tr_l2_partial(int tid, int count, const float *params, const uint8_t *kind, double *s_sq) {
    double sq = 0.0;
    for (int i = tid; i < count; i += BB_TRAIN_THREADS)
        if (kind[i] == 1) sq += (double)params[i] * (double)params[i];
    s_sq[tid] = sq;
}
// Thread 0's epilogue of every prep path: log S from the noise sum sn (reference loss) and lossParam from the reduced L2 sum sq.
template <int LOSS>
__device__ __forceinline__ void tr_prep_finish(TrainAux *aux, int n, int n_l2, float eps, float l2c, float sn, double sq) {
    if constexpr (LOSS == BB_LOSS_PER_EXAMPLE) {
        aux->logS = 0.f;
        aux->l2 = (float)((double)l2c * (0.5 * sq));
    } else {
        const float S = (float)n * (1.0f - eps) + (float)n * eps * sn;
        aux->logS = logf(S);
        aux->l2 = (float)(0.5 * sq / (double)n_l2);
    }
}

// The dense games: one workgroup.
template <class G, class Src, int LOSS = BB_LOSS_REFERENCE>
__global__ void __launch_bounds__(BB_TRAIN_THREADS) k_train_prep(int n, int count, int n_l2, const float *params, const uint8_t *kind,
                                                                Src src, const float *noise_in, float eps, float alpha, uint64_t seed,
                                                                uint64_t calls, float l2c, TrainAux *aux) {
    constexpr int A = G::A;
    __shared__ double s_sq[BB_TRAIN_THREADS];
    const int tid = threadIdx.x;
    if constexpr (LOSS == BB_LOSS_PER_EXAMPLE) { // no noise, no label sum: the L2 term alone
        tr_l2_partial(tid, count, params, kind, s_sq);
        __syncthreads();
        tr_tree_sum(tid, s_sq);
        if (tid < 16) {
            aux->noise[tid] = 0.f;
            aux->L[tid] = 0.f;
        }
        if (tid == 0) tr_prep_finish<LOSS>(aux, n, n_l2, eps, l2c, 0.f, s_sq[0]);
        return;
    }
    __shared__ float s_part[BB_TRAIN_THREADS];
    __shared__ float s_noise[16];
    if (tid < 16) {
        float z = 0.f;
        if (tid < A && eps != 0.f)
            z = noise_in ? noise_in[tid] : bb_beta_noise(seed, (uint32_t)calls, (uint32_t)(calls >> 32), (uint32_t)tid, alpha);
        s_noise[tid] = z;
        aux->noise[tid] = z;
    }
    { // L[a]: 16 strided partial sums per action, then those in order
        const int a = tid & 15, c = tid >> 4;
        float acc = 0.f;
        if (a < A)
            for (int j = c; j < n; j += 16) acc += src.label(j, a);
        s_part[tid] = acc;
    }
    tr_l2_partial(tid, count, params, kind, s_sq);
    __syncthreads();
    tr_tree_sum(tid, s_sq);
    if (tid < 16) {
        float acc = 0.f;
        for (int c = 0; c < 16; c++) acc += s_part[c * 16 + tid];
        aux->L[tid] = tid < A ? acc : 0.f;
    }
    if (tid == 0) {
        float sn = 0.f;
        for (int a = 0; a < A; a++) sn += s_noise[a];
        tr_prep_finish<LOSS>(aux, n, n_l2, eps, l2c, sn, s_sq[0]);
    }
}

// The wide game, 1 + ceil(A / 256) workgroups (per example: one).  The noise and L are A floats each in an allocation of their
// own (aux_noise, aux_L); TrainAux keeps logS and l2 (k_train_apply reads them).
//   workgroup 0      noise[a] for a = tid, tid + 256, ... (the caller's, or the Philox draw keyed (seed, calls, a)); the noise sum:
//                    each thread its own a ascending, then tr_tree_sum; log S; the L2 term as k_train_prep takes it
//   workgroup 1 + w  L[a] for a = 256 w + tid: the rows j = 0 .. n-1 ascending, one thread per action (loads contiguous along a)
template <class G, class Src, int LOSS = BB_LOSS_REFERENCE>
__global__ void __launch_bounds__(BB_TRAIN_THREADS) k_train_prep_wide(int n, int count, int n_l2, const float *params, const uint8_t *kind,
                                                                     Src src, const float *noise_in, float eps, float alpha, uint64_t seed,
                                                                     uint64_t calls, float l2c, TrainAux *aux, float *aux_noise, float *aux_L) {
    constexpr int A = G::A;
    const int tid = threadIdx.x;
    if constexpr (LOSS == BB_LOSS_PER_EXAMPLE) { // one workgroup: no noise, no label sweep; the L2 term alone
        if (blockIdx.x > 0) return;
        __shared__ double s_sq1[BB_TRAIN_THREADS];
        for (int a = tid; a < A; a += BB_TRAIN_THREADS) aux_noise[a] = 0.f;
        tr_l2_partial(tid, count, params, kind, s_sq1);
        __syncthreads();
        tr_tree_sum(tid, s_sq1);
        if (tid == 0) tr_prep_finish<LOSS>(aux, n, n_l2, eps, l2c, 0.f, s_sq1[0]);
        return;
    }
    if (blockIdx.x > 0) { // L[a]: rows ascending
        const int a = ((int)blockIdx.x - 1) * BB_TRAIN_THREADS + tid;
        if (a < A) {
            float acc = 0.f;
            for (int j = 0; j < n; j++) acc += src.label(j, a);
            aux_L[a] = acc;
        }
        return;
    }
    __shared__ double s_sq[BB_TRAIN_THREADS];
    __shared__ float s_noise[BB_TRAIN_THREADS];
    float sn = 0.f;
    for (int a = tid; a < A; a += BB_TRAIN_THREADS) {
        float z = 0.f;
        if (eps != 0.f) z = noise_in ? noise_in[a] : bb_beta_noise(seed, (uint32_t)calls, (uint32_t)(calls >> 32), (uint32_t)a, alpha);
        aux_noise[a] = z;
        sn += z;
    }
    s_noise[tid] = sn;
    tr_l2_partial(tid, count, params, kind, s_sq);
    __syncthreads();
    tr_tree_sum(tid, s_sq, s_noise);
    if (tid == 0) tr_prep_finish<LOSS>(aux, n, n_l2, eps, l2c, s_noise[0], s_sq[0]);
}

// ---- pieces of k_train_grad: the convolutions --------------------------------------------------------------------------
// a conv kernel [9*CIN][16] into LDS rows of BB_TRAIN_WROW, each column times scale[f] (gamma / sqrt(var + eps)) when SCALED
template <int CIN, bool SCALED>
__device__ __forceinline__ void tr_stage(float *wst, const float *k, const float *bn, int tid) {
    const int f = tid & 15;
    float s = 1.f;
    if constexpr (SCALED) s = bn[f] * tr_bn_inv(bn[3 * BB_TRAIN_F + f]);
    for (int row = tid >> 4; row < 9 * CIN; row += BB_TRAIN_THREADS / 16) {
        const float w = k[row * BB_TRAIN_F + f];
        wst[row * BB_TRAIN_WROW + f] = SCALED ? w * s : w;
    }
}

// conv 3x3 SAME + bias, inference batch norm, (+ residual), ReLU.  Thread (f = tid & 15, pg = tid >> 4) owns the pixels
// pg, pg + 16, ...; the sum over (tap, ci) is one fmaf chain in that order, padding skipped.  NRM: the normalised conv output
// is stored too (the backward pass reads it; the forward-only k_train_eval passes nrm = nullptr).  res == act is allowed: a
// thread reads and writes its own elements only.
template <class G, int CIN, bool NRM>
__device__ __forceinline__ void tr_conv_fwd(const float *X, const float *wst, const float *bias, const float *bn, const float *res,
                                            float *nrm, float *act, int tid) {
    constexpr int P = G::H * G::W, NP = (P + 15) / 16;
    const int f = tid & 15, pg = tid >> 4;
    float acc[NP];
    int pr[NP], pc[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) {
        const int p = pg + 16 * k;
        acc[k] = 0.f;
        pr[k] = p / G::W;
        pc[k] = p % G::W;
    }
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        bool ok[NP];
        int q[NP];
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const int r = pr[k] + dy, c = pc[k] + dx;
            ok[k] = pg + 16 * k < P && r >= 0 && r < G::H && c >= 0 && c < G::W;
            q[k] = ok[k] ? r * G::W + c : 0;
        }
        if constexpr (CIN % 4 == 0) {
#pragma unroll
            for (int c4 = 0; c4 < CIN / 4; c4++) {
                float w[4];
#pragma unroll
                for (int j = 0; j < 4; j++) w[j] = wst[(tap * CIN + 4 * c4 + j) * BB_TRAIN_WROW + f];
#pragma unroll
                for (int k = 0; k < NP; k++)
                    if (ok[k]) {
                        const float4 x = ((const float4 *)(X + q[k] * CIN))[c4];
                        acc[k] = __builtin_fmaf(x.x, w[0], acc[k]);
                        acc[k] = __builtin_fmaf(x.y, w[1], acc[k]);
                        acc[k] = __builtin_fmaf(x.z, w[2], acc[k]);
                        acc[k] = __builtin_fmaf(x.w, w[3], acc[k]);
                    }
            }
        } else {
#pragma unroll
            for (int ci = 0; ci < CIN; ci++) {
                const float w = wst[(tap * CIN + ci) * BB_TRAIN_WROW + f];
#pragma unroll
                for (int k = 0; k < NP; k++)
                    if (ok[k]) acc[k] = __builtin_fmaf(X[q[k] * CIN + ci], w, acc[k]);
            }
        }
    }
    const float b = bias[f], g = bn[f], be = bn[BB_TRAIN_F + f], mu = bn[2 * BB_TRAIN_F + f], inv = tr_bn_inv(bn[3 * BB_TRAIN_F + f]);
#pragma unroll
    for (int k = 0; k < NP; k++) {
        const int p = pg + 16 * k;
        if (p < P) {
            const float xh = ((acc[k] + b) - mu) * inv;
            float y = __builtin_fmaf(g, xh, be);
            if (res) y += res[p * BB_TRAIN_F + f];
            if constexpr (NRM) nrm[p * BB_TRAIN_F + f] = xh;
            act[p * BB_TRAIN_F + f] = fmaxf(y, 0.f);
        }
    }
}

// gradient of a conv's input: dX[q][ci] = sum_tap sum_f dy[q - off(tap)][f] * wst[tap][ci][f] (wst already holds the
// batch-norm scale).  Thread (ci = tid & 15, pg).  MASKED: out = act_mask > 0 ? dX : 0; else out += dX.
template <class G, bool MASKED>
__device__ __forceinline__ void tr_conv_dx(const float *dy, const float *wst, const float *act_mask, float *out, int tid) {
    constexpr int P = G::H * G::W, NP = (P + 15) / 16;
    const int ci = tid & 15, pg = tid >> 4;
    float acc[NP];
    int pr[NP], pc[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) {
        const int p = pg + 16 * k;
        acc[k] = 0.f;
        pr[k] = p / G::W;
        pc[k] = p % G::W;
    }
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const int oy = tap / 3 - 1, ox = tap % 3 - 1;
        bool ok[NP];
        int q[NP];
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const int r = pr[k] - oy, c = pc[k] - ox; // the output pixel this tap fed from here
            ok[k] = pg + 16 * k < P && r >= 0 && r < G::H && c >= 0 && c < G::W;
            q[k] = ok[k] ? r * G::W + c : 0;
        }
#pragma unroll
        for (int f4 = 0; f4 < BB_TRAIN_F / 4; f4++) {
            float w[4];
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = wst[(tap * BB_TRAIN_F + ci) * BB_TRAIN_WROW + 4 * f4 + j];
#pragma unroll
            for (int k = 0; k < NP; k++)
                if (ok[k]) {
                    const float4 d = ((const float4 *)(dy + q[k] * BB_TRAIN_F))[f4];
                    acc[k] = __builtin_fmaf(d.x, w[0], acc[k]);
                    acc[k] = __builtin_fmaf(d.y, w[1], acc[k]);
                    acc[k] = __builtin_fmaf(d.z, w[2], acc[k]);
                    acc[k] = __builtin_fmaf(d.w, w[3], acc[k]);
                }
        }
    }
#pragma unroll
    for (int k = 0; k < NP; k++) {
        const int p = pg + 16 * k;
        if (p < P) {
            const int e = p * BB_TRAIN_F + ci;
            if (MASKED)
                out[e] = act_mask[e] > 0.f ? acc[k] : 0.f;
            else
                out[e] += acc[k];
        }
    }
}

// gradients of one conv layer's variables from dy (gradient at the batch-norm output, ReLU mask applied):
//   kernel[tap][ci][f] = scale[f] * sum_p X[p + off(tap)][ci] dy[p][f]   thread (f = tid & 15, ci = tid >> 4), p ascending
//   gamma[f] = sum_p dy xhat, beta[f] = sum_p dy, bias[f] = scale[f] * beta[f]                       threads 0..15
// CIN > 16 (DragonChess's 17 planes): the channels ci = c0 + (tid >> 4) for c0 = 0, 16, ..., one pass each -- every (ci, f) pair
// is written, and the chain of a pair is the same p-ascending one whichever pass holds it.
template <class G, int CIN>
__device__ __forceinline__ void tr_conv_dw(const float *X, const float *dy, const float *nrm, const float *bn, float *slab_k,
                                           float *slab_b, float *slab_bn, int tid) {
    constexpr int P = G::H * G::W;
    const int f = tid & 15;
    const float s = bn[f] * tr_bn_inv(bn[3 * BB_TRAIN_F + f]);
#pragma unroll
    for (int c0 = 0; c0 < CIN; c0 += BB_TRAIN_THREADS / 16) {
        const int ci = c0 + (tid >> 4);
        if (ci < CIN) {
            float acc[9];
#pragma unroll
            for (int t = 0; t < 9; t++) acc[t] = 0.f;
            for (int r = 0; r < G::H; r++)
                for (int c = 0; c < G::W; c++) {
                    const float d = dy[(r * G::W + c) * BB_TRAIN_F + f];
#pragma unroll
                    for (int t = 0; t < 9; t++) {
                        const int rr = r + t / 3 - 1, cc = c + t % 3 - 1;
                        if (rr >= 0 && rr < G::H && cc >= 0 && cc < G::W)
                            acc[t] = __builtin_fmaf(X[(rr * G::W + cc) * CIN + ci], d, acc[t]);
                    }
                }
#pragma unroll
            for (int t = 0; t < 9; t++) slab_k[(t * CIN + ci) * BB_TRAIN_F + f] = acc[t] * s;
        }
    }
    if (tid < BB_TRAIN_F) {
        float dg = 0.f, db = 0.f;
        for (int p = 0; p < P; p++) {
            const float d = dy[p * BB_TRAIN_F + f];
            dg = __builtin_fmaf(d, nrm[p * BB_TRAIN_F + f], dg);
            db += d;
        }
        slab_bn[f] = dg;
        slab_bn[BB_TRAIN_F + f] = db;
        slab_b[f] = db * s;
    }
}

// ---- the heads' forward pass, one output element a call: THE text of these expressions ------------------------------------
// k_train_grad and k_train_eval (train_eval.hip.h) map the elements to their own threads and keep the results in their own
// scratch; the arithmetic is here once, so a scored row's value and logits are the step's bits by construction.  x: the tower's
// output [P][16]; vy [P], py [P][2]: the head convs' activations; h [D]: dense_1's.  xh: the normalised conv output, which the
// backward pass reads and the scorer drops.
// value/convolution (1x1, one filter), batch norm, ReLU at square p: one fmaf chain over f ascending
__device__ __forceinline__ float tr_head_value_conv(const TrainLayout &lay, const float *prm, const float *x, int p, float &xh) {
    float acc = 0.f;
    for (int f = 0; f < BB_TRAIN_F; f++) acc = __builtin_fmaf(x[p * BB_TRAIN_F + f], prm[lay.v_conv_k + f], acc);
    xh = ((acc + prm[lay.v_conv_b]) - prm[lay.v_bn + 2]) * tr_bn_inv(prm[lay.v_bn + 3]);
    return fmaxf(__builtin_fmaf(prm[lay.v_bn], xh, prm[lay.v_bn + 1]), 0.f);
}
// policy/convolution (1x1, two filters), batch norm, ReLU at square p, filter j: one fmaf chain over f ascending
__device__ __forceinline__ float tr_head_policy_conv(const TrainLayout &lay, const float *prm, const float *x, int p, int j, float &xh) {
    float acc = 0.f;
    for (int f = 0; f < BB_TRAIN_F; f++) acc = __builtin_fmaf(x[p * BB_TRAIN_F + f], prm[lay.p_conv_k + f * 2 + j], acc);
    xh = ((acc + prm[lay.p_conv_b + j]) - prm[lay.p_bn + 4 + j]) * tr_bn_inv(prm[lay.p_bn + 6 + j]);
    return fmaxf(__builtin_fmaf(prm[lay.p_bn + j], xh, prm[lay.p_bn + 2 + j]), 0.f);
}
// value/dense_1 on every square, summed over the squares p ascending, ReLU: unit d
template <class G>
__device__ __forceinline__ float tr_head_dense_1(const TrainLayout &lay, const float *prm, const float *vy, int d) {
    const float k1 = prm[lay.v_d1_k + d], b1 = prm[lay.v_d1_b + d];
    float acc = 0.f;
    for (int p = 0; p < G::H * G::W; p++) acc += __builtin_fmaf(vy[p], k1, b1);
    return fmaxf(acc, 0.f);
}
// policy/policy on every square, summed over the squares p ascending: the logit of action a
template <class G>
__device__ __forceinline__ float tr_head_logit(const TrainLayout &lay, const float *prm, const float *py, int a) {
    const float k0 = prm[lay.p_d_k + a], k1 = prm[lay.p_d_k + G::A + a], pb = prm[lay.p_d_b + a];
    float acc = 0.f;
    for (int p = 0; p < G::H * G::W; p++) acc += __builtin_fmaf(py[2 * p + 1], k1, __builtin_fmaf(py[2 * p], k0, pb));
    return acc;
}
// value/dense_2, one fmaf chain over d ascending from the bias, tanh: the value
__device__ __forceinline__ float tr_head_value(const TrainLayout &lay, const float *prm, const float *h) {
    float z = prm[lay.v_d2_b];
    for (int d = 0; d < lay.D; d++) z = __builtin_fmaf(h[d], prm[lay.v_d2_k + d], z);
    return tanhf(z);
}

// ---- the LDS of a k_train_grad workgroup ---------------------------------------------------------------------------------
// For R blocks: the activations and normalised conv outputs of 2R + 1 layers, gA, gB, the staged conv kernel and what lies behind it.
// The staged kernel is 9 * max(C, F) rows of BB_TRAIN_WROW floats (tr_stage<C> writes 9 * C rows), in whole float4s: 2448 floats
// for 3 planes, 2604 for DragonChess's 17.
template <class G>
__host__ __device__ constexpr int train_wst_floats() {
    return (9 * (G::C > BB_TRAIN_F ? G::C : BB_TRAIN_F) * BB_TRAIN_WROW + 3) / 4 * 4;
}
// Behind it: the dense games' planes and head scratch (BB_TRAIN_SMALL floats, offsets fixed); the wide game keeps only its planes
// there (H * W * C floats: 1088) -- its head scratch lies in gB and its reduction scratch in gA, both idle until the backward pass.
template <class G>
__host__ __device__ constexpr int train_small_floats() {
    return G::A <= 16 ? BB_TRAIN_SMALL : (G::H * G::W * G::C + 3) / 4 * 4;
}
template <class G>
__host__ __device__ constexpr int train_lds_floats(int R) {
    return (2 * (2 * R + 1) + 2) * G::H * G::W * BB_TRAIN_F + train_wst_floats<G>() + train_small_floats<G>();
}
// The largest R whose workgroup fits the 160 KB of LDS a gfx950 CU has (one workgroup may take all of it).  DragonChess:
// (4R + 4) * 4096 + 4 * (2604 + 1088) bytes = 162 224 at R = 8 and 178 608 at R = 9, so 8.
#define BB_TRAIN_LDS_BYTES (160 * 1024)
template <class G>
__host__ __device__ constexpr int train_max_blocks() {
    int R = 0;
    while ((size_t)train_lds_floats<G>(R + 1) * sizeof(float) <= BB_TRAIN_LDS_BYTES) R++;
    return R;
}
static_assert(train_lds_floats<Connect4>(0) == 4 * 42 * 16 + 2448 + 896 && train_lds_floats<TicTacToe>(9) == 40 * 9 * 16 + 2448 + 896,
              "the dense games' layout does not move");
static_assert(train_max_blocks<DragonChess>() >= 6, "the DragonChess step covers at least 6 blocks");
static_assert(train_lds_floats<DragonChess>(8) * 4 == 162224, "the DragonChess layout does not move");

// Where a workgroup's head scratch lies: offsets from `sm`, one type per game.  The planes (`brd`) lie behind the staged kernel for
// every game.  Dense games: sm = brd -- the planes (at most 128 floats) and the scratch share BB_TRAIN_SMALL floats, lg and dlg hold
// the A logits and their gradients.  Wide game: sm = gB, 9P + 144 = 720 floats, and the four reduction arrays [256] of
// the wide policy head lie in gA (both idle until the backward pass; the hazards: at the head, in k_train_grad).  The planes keep a
// place of their own, because the last weight gradient reads them.  The staged 17-plane kernel has rows of BB_TRAIN_WROW = 17
// floats and the planes of a pixel are 17 floats apart: both odd, so neither walk stays on one bank.
template <class G>
struct TrainScratch {
    static constexpr bool dense = G::A <= 16; // the game family: train_small_floats' predicate
    static constexpr int P = G::H * G::W;
    static constexpr int at(int d, int w) { return dense ? d : w; }
    static constexpr int vn = at(128, 0), vy = at(192, P), pn = at(256, 2 * P), py = at(384, 4 * P), dvy = at(512, 6 * P), dpy = at(576, 7 * P),
                         hbuf = at(704, 9 * P), tmp = hbuf + 64, lg = 832, dlg = 848, misc = at(864, tmp + 64), // misc: 0 svy, 1..2 spy, 3 dz
                         end = misc + 16;
    static_assert(P <= 64 && 2 * P <= 128, "head scratch sizes");
    static_assert(dense ? P * G::C <= vn && G::A <= 16 && end <= BB_TRAIN_SMALL : end <= P * BB_TRAIN_F && 4 * BB_TRAIN_THREADS <= P * BB_TRAIN_F,
                  "the dense scratch fits BB_TRAIN_SMALL; the wide one fits gB, its reductions gA");
};

// ---- pieces of k_train_grad: what every game runs ------------------------------------------------------------------------
// The forward tower: the row's planes into brd, then 2R + 1 layers, each staged and convolved; returns the tower's output.
template <class G, class Src>
__device__ __forceinline__ const float *tr_tower_fwd(const TrainLayout &lay, const float *prm, const Src &src, const typename Src::Row &row,
                                                     float *brd, float *wst, float *act, float *nrm, int tid) {
    constexpr int P = G::H * G::W, C = G::C, F = BB_TRAIN_F, LF = P * F;
    const int NL = 2 * lay.R + 1;
    for (int i = tid; i < P * C; i += BB_TRAIN_THREADS) brd[i] = src.plane(row, i);
    tr_stage<C, false>(wst, prm + lay.conv0_k, nullptr, tid);
    __syncthreads();
    tr_conv_fwd<G, C, true>(brd, wst, prm + lay.conv0_b, prm + lay.conv0_bn, nullptr, nrm, act, tid);
    __syncthreads();
    for (int l = 1; l < NL; l++) { // layer l: conv_{1,2} of block (l-1)/2; conv_2 adds the block's input
        tr_stage<F, false>(wst, prm + lay.blk_k + (l - 1) * 9 * F * F, nullptr, tid);
        __syncthreads();
        tr_conv_fwd<G, F, true>(act + (l - 1) * LF, wst, prm + lay.blk_b + (l - 1) * F, prm + lay.blk_bn + (l - 1) * 4 * F,
                          (l & 1) ? nullptr : act + (l - 2) * LF, nrm + l * LF, act + l * LF, tid);
        __syncthreads();
    }
    return act + (NL - 1) * LF;
}

// The head convolutions at the tower's output x: vn, vy, pn, py.  The caller makes the barrier.
template <class G>
__device__ __forceinline__ void tr_heads_conv(const TrainLayout &lay, const float *prm, const float *x, float *sm, int tid) {
    using S = TrainScratch<G>;
    constexpr int P = G::H * G::W;
    if (tid < P) { // value/convolution
        float xh;
        const float y = tr_head_value_conv(lay, prm, x, tid, xh);
        sm[S::vn + tid] = xh;
        sm[S::vy + tid] = y;
    } else if (tid >= 64 && tid < 64 + 2 * P) { // policy/convolution
        const int e = tid - 64;
        float xh;
        const float y = tr_head_policy_conv(lay, prm, x, e >> 1, e & 1, xh);
        sm[S::pn + e] = xh;
        sm[S::py + e] = y;
    }
}

// value/dense_1 (threads 0 .. D-1) and the three sums over the squares the dense gradients need (threads 128 .. 130).  The policy
// head calls it next to its logits; the barrier after both is the head's.
template <class G>
__device__ __forceinline__ void tr_heads_dense(const TrainLayout &lay, const float *prm, float *sm, int tid) {
    using S = TrainScratch<G>;
    constexpr int P = G::H * G::W;
    if (tid < lay.D) { // value/dense_1
        sm[S::hbuf + tid] = tr_head_dense_1<G>(lay, prm, sm + S::vy, tid);
    } else if (tid >= 128 && tid < 131) {
        const int j = tid - 128;
        float acc = 0.f;
        for (int p = 0; p < P; p++) acc += j == 0 ? sm[S::vy + p] : sm[S::py + 2 * p + (j - 1)];
        sm[S::misc + j] = acc;
    }
}

// The value, the example's value loss piece and d loss / d pre-tanh value: one thread's work (thread 0 of the policy head, at
// the place between the barriers that its head gives it).
template <class G>
__device__ __forceinline__ void tr_value_loss(const TrainLayout &lay, const float *prm, float *sm, float target, int n, float *le) {
    using S = TrainScratch<G>;
    const float val = tr_head_value(lay, prm, sm + S::hbuf), diff = val - target;
    *le = diff * diff;
    sm[S::misc + 3] = 2.0f * diff * (1.0f - val * val) / (float)n;
}

// ---- the policy head of the dense games -----------------------------------------------------------------------------------
// From the head convolutions (a barrier behind them) to d logit in sm[dlg] and policy/policy's gradients in the slab: the logits one
// thread an action, then lane 0 serially over the A actions -- max, sum of expf, the loss piece and t as fmaf chains, a ascending.
template <class G, class Src, int LOSS>
__device__ __forceinline__ void tr_policy_dense(const TrainLayout &lay, const float *prm, const TrainAux *aux, const float *noise, const float *L,
                                                const Src &src, const typename Src::Row &row, int n, float eps, float *sm, float *slab,
                                                float *le, float *lp, int tid) {
    using S = TrainScratch<G>;
    constexpr int P = G::H * G::W, A = G::A;
    if (tid >= 64 && tid < 64 + A) sm[S::lg + tid - 64] = tr_head_logit<G>(lay, prm, sm + S::py, tid - 64); // policy/policy
    tr_heads_dense<G>(lay, prm, sm, tid);
    __syncthreads();
    if (tid == 0) { // value, softmax, the example's loss pieces, d loss / d (pre-tanh value, logits)
        tr_value_loss<G>(lay, prm, sm, src.value_of(row), n, le);
        float mx = sm[S::lg];
        for (int a = 1; a < A; a++) mx = fmaxf(mx, sm[S::lg + a]);
        float e[A], sum = 0.f;
        for (int a = 0; a < A; a++) {
            e[a] = expf(sm[S::lg + a] - mx);
            sum += e[a];
        }
        if constexpr (LOSS == BB_LOSS_PER_EXAMPLE) { // the row's own label: k_train_eval's ce, and T = sum_a pi[a]
            const float lse = logf(sum);
            float pi[A], ce = 0.f, t = 0.f;
            for (int a = 0; a < A; a++) {
                pi[a] = src.label_of(row, a);
                ce = __builtin_fmaf(pi[a], (sm[S::lg + a] - mx) - lse, ce);
                t = __builtin_fmaf(pi[a], 1.0f, t);
            }
            *lp = t != 0.f ? ce : 0.f; // (a row without a label -- the terminal example -- adds 0)
            for (int a = 0; a < A; a++) sm[S::dlg + a] = ((e[a] / sum) * t - pi[a]) / (float)n;
        } else {
            float ce = 0.f, t = 0.f, r[A];
            for (int a = 0; a < A; a++) {
                e[a] = e[a] / sum; // softmax
                const float q = __builtin_fmaf(eps, noise[a], (1.0f - eps) * e[a]), La = L[a];
                if (La != 0.f) ce = __builtin_fmaf(La, logf(q) - aux->logS, ce);
                r[a] = q > 0.f ? (1.0f - eps) * e[a] / q : 0.f;
                t = __builtin_fmaf(La, r[a], t);
            }
            *lp = ce;
            const float inv_n2 = 1.0f / ((float)n * (float)n);
            for (int a = 0; a < A; a++) sm[S::dlg + a] = -inv_n2 * (L[a] * r[a] - e[a] * t);
        }
    }
    __syncthreads();
    if (tid >= 64 && tid < 64 + A) {
        const int a = tid - 64;
        const float dl = sm[S::dlg + a];
        slab[lay.p_d_b + a] = dl * (float)P;
        slab[lay.p_d_k + a] = dl * sm[S::misc + 1];
        slab[lay.p_d_k + A + a] = dl * sm[S::misc + 2];
    }
}

// ---- the policy head of the wide game: what the shared backward pass needs of it --------------------------------------------
// The head itself stands in k_train_grad's body, with its sum orders and hazards written there.  It leaves g_0 in red[0] and g_1 in
// tr_wide_g1(red)[0], red being its four reduction arrays [256] (gA); which array holds g_1 depends on the loss (the reason: at
// rg1 in k_train_grad).
template <int LOSS>
__device__ __forceinline__ float *tr_wide_g1(float *red) {
    return red + (LOSS == BB_LOSS_PER_EXAMPLE ? 2 : 1) * BB_TRAIN_THREADS;
}

// g_j as the game's policy head left it: formed from sm[dlg] (an fmaf chain, a ascending) by the dense games, read by the wide one
template <class G, int LOSS>
__device__ __forceinline__ float tr_policy_g(const TrainLayout &lay, const float *prm, const float *sm, float *red, int j) {
    using S = TrainScratch<G>;
    if constexpr (S::dense) {
        float g = 0.f;
        for (int a = 0; a < G::A; a++) g = __builtin_fmaf(sm[S::dlg + a], prm[lay.p_d_k + j * G::A + a], g);
        return g;
    } else {
        return (j ? tr_wide_g1<LOSS>(red) : red)[0];
    }
}

// ---- pieces of k_train_grad: the backward pass, every game's -----------------------------------------------------------------
// The heads once d logit is known: the value head's dense gradients, dvy / dpy, the head batch-norm and conv gradients, and the
// gradient at the tower's output x into gA (the wide head's reductions in gA are over: a barrier lies between their last read and
// this write).
template <class G, int LOSS>
__device__ __forceinline__ void tr_heads_bwd(const TrainLayout &lay, const float *prm, const float *x, float *sm, float *gA, float *slab, int tid) {
    using S = TrainScratch<G>;
    constexpr int P = G::H * G::W, F = BB_TRAIN_F, LF = P * F;
    const int D = lay.D;
    const float dz = sm[S::misc + 3];
    if (tid < D) {
        const float h = sm[S::hbuf + tid], dh = h > 0.f ? dz * prm[lay.v_d2_k + tid] : 0.f;
        slab[lay.v_d2_k + tid] = dz * h;
        slab[lay.v_d1_k + tid] = dh * sm[S::misc];
        slab[lay.v_d1_b + tid] = dh * (float)P;
        sm[S::tmp + tid] = dh * prm[lay.v_d1_k + tid];
    } else if (tid == 128) {
        slab[lay.v_d2_b] = dz;
    }
    __syncthreads();
    if (tid < P) { // every square's value-head activation gets the same gradient, through its own ReLU
        float g1 = 0.f;
        for (int d = 0; d < D; d++) g1 += sm[S::tmp + d];
        sm[S::dvy + tid] = sm[S::vy + tid] > 0.f ? g1 : 0.f;
    } else if (tid >= 64 && tid < 64 + 2 * P) { // ... and every square's policy-head activation j its g_j
        const int e = tid - 64;
        const float g = tr_policy_g<G, LOSS>(lay, prm, sm, gA, e & 1);
        sm[S::dpy + e] = sm[S::py + e] > 0.f ? g : 0.f;
    }
    __syncthreads();
    const float v_s = prm[lay.v_bn] * tr_bn_inv(prm[lay.v_bn + 3]);
    const float p_s0 = prm[lay.p_bn] * tr_bn_inv(prm[lay.p_bn + 6]), p_s1 = prm[lay.p_bn + 1] * tr_bn_inv(prm[lay.p_bn + 7]);
    if (tid == 0) {
        float dg = 0.f, db = 0.f;
        for (int p = 0; p < P; p++) {
            dg = __builtin_fmaf(sm[S::dvy + p], sm[S::vn + p], dg);
            db += sm[S::dvy + p];
        }
        slab[lay.v_bn] = dg;
        slab[lay.v_bn + 1] = db;
        slab[lay.v_conv_b] = db * v_s;
    } else if (tid < 3) {
        const int j = tid - 1;
        float dg = 0.f, db = 0.f;
        for (int p = 0; p < P; p++) {
            dg = __builtin_fmaf(sm[S::dpy + 2 * p + j], sm[S::pn + 2 * p + j], dg);
            db += sm[S::dpy + 2 * p + j];
        }
        slab[lay.p_bn + j] = dg;
        slab[lay.p_bn + 2 + j] = db;
        slab[lay.p_conv_b + j] = db * (j ? p_s1 : p_s0);
    } else if (tid >= 16 && tid < 32) {
        const int f = tid - 16;
        float acc = 0.f;
        for (int p = 0; p < P; p++) acc = __builtin_fmaf(sm[S::dvy + p], x[p * F + f], acc);
        slab[lay.v_conv_k + f] = acc * v_s;
    } else if (tid >= 32 && tid < 64) {
        const int e = tid - 32, f = e >> 1, j = e & 1;
        float acc = 0.f;
        for (int p = 0; p < P; p++) acc = __builtin_fmaf(sm[S::dpy + 2 * p + j], x[p * F + f], acc);
        slab[lay.p_conv_k + e] = acc * (j ? p_s1 : p_s0);
    }
    for (int e = tid; e < LF; e += BB_TRAIN_THREADS) { // gradient at the tower's output
        const int p = e / F, f = e % F;
        float g = (sm[S::dvy + p] * v_s) * prm[lay.v_conv_k + f];
        g = __builtin_fmaf(sm[S::dpy + 2 * p] * p_s0, prm[lay.p_conv_k + 2 * f], g);
        g = __builtin_fmaf(sm[S::dpy + 2 * p + 1] * p_s1, prm[lay.p_conv_k + 2 * f + 1], g);
        gA[e] = g;
    }
    __syncthreads();
}

// The backward tower and the conv0 weight gradient.  gA: gradient at the current block's output; gB is free from here (the wide
// game's head scratch is done).
template <class G>
__device__ __forceinline__ void tr_tower_bwd(const TrainLayout &lay, const float *prm, const float *brd, float *wst, const float *act,
                                             const float *nrm, float *gA, float *gB, float *slab, int tid) {
    constexpr int P = G::H * G::W, C = G::C, F = BB_TRAIN_F, LF = P * F;
    for (int i = lay.R - 1; i >= 0; i--) {
        const int l1 = 1 + 2 * i, l2 = 2 + 2 * i; // layers of conv_1 and conv_2; the block's input is layer l1 - 1
        const float *k1 = prm + lay.blk_k + (l1 - 1) * 9 * F * F, *k2 = prm + lay.blk_k + (l2 - 1) * 9 * F * F;
        const float *bn1 = prm + lay.blk_bn + (l1 - 1) * 4 * F, *bn2 = prm + lay.blk_bn + (l2 - 1) * 4 * F;
        // through the block's last ReLU: this is the gradient at batch_norm_2's output and at the skip connection
        for (int e = tid; e < LF; e += BB_TRAIN_THREADS) gA[e] = act[l2 * LF + e] > 0.f ? gA[e] : 0.f;
        tr_stage<F, true>(wst, k2, bn2, tid);
        __syncthreads();
        tr_conv_dw<G, F>(act + l1 * LF, gA, nrm + l2 * LF, bn2, slab + lay.blk_k + (l2 - 1) * 9 * F * F, slab + lay.blk_b + (l2 - 1) * F,
                         slab + lay.blk_bn + (l2 - 1) * 4 * F, tid);
        tr_conv_dx<G, true>(gA, wst, act + l1 * LF, gB, tid);
        __syncthreads();
        tr_stage<F, true>(wst, k1, bn1, tid);
        tr_conv_dw<G, F>(act + (l1 - 1) * LF, gB, nrm + l1 * LF, bn1, slab + lay.blk_k + (l1 - 1) * 9 * F * F,
                         slab + lay.blk_b + (l1 - 1) * F, slab + lay.blk_bn + (l1 - 1) * 4 * F, tid);
        __syncthreads();
        tr_conv_dx<G, false>(gB, wst, nullptr, gA, tid);
        __syncthreads();
    }
    for (int e = tid; e < LF; e += BB_TRAIN_THREADS) gA[e] = act[e] > 0.f ? gA[e] : 0.f;
    __syncthreads();
    tr_conv_dw<G, C>(brd, gA, nrm, prm + lay.conv0_bn, slab + lay.conv0_k, slab + lay.conv0_b, slab + lay.conv0_bn, tid);
}

// ---- k_train_grad: one workgroup per example, every game --------------------------------------------------------------------
// noise, L: A floats each (TrainAux's for the dense games).
template <class G, class Src, int LOSS = BB_LOSS_REFERENCE>
__global__ void __launch_bounds__(BB_TRAIN_THREADS) k_train_grad(TrainLayout lay, const float *__restrict__ prm, const TrainAux *__restrict__ aux,
                                                                const float *__restrict__ noise, const float *__restrict__ L, Src src, int n,
                                                                float eps, float *__restrict__ slabs, float *__restrict__ le_out,
                                                                float *__restrict__ lp_out) {
    using S = TrainScratch<G>;
    constexpr int LF = G::H * G::W * BB_TRAIN_F;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (b >= n) return;
    const int NL = 2 * lay.R + 1;
    float *act = lds, *nrm = act + NL * LF, *gA = nrm + NL * LF, *gB = gA + LF, *wst = gB + LF, *brd = wst + train_wst_floats<G>();
    float *sm = S::dense ? brd : gB;
    float *slab = slabs + (size_t)b * lay.count;

    const typename Src::Row row = src.row(b);
    src.count(row, tid);
    const float *x = tr_tower_fwd<G>(lay, prm, src, row, brd, wst, act, nrm, tid);
    tr_heads_conv<G>(lay, prm, x, sm, tid);
    __syncthreads();
    if constexpr (S::dense)
        tr_policy_dense<G, Src, LOSS>(lay, prm, aux, noise, L, src, row, n, eps, sm, slab, le_out + b, lp_out + b, tid);
    else {
        // ---- the policy head of the wide game: tr_policy_dense's span with the head spread over the workgroup ----
        //   thread tid owns the actions a = tid + 256 k, k = 0 .. 15 (4032 = 15.75 * 256: a < A guards the last 192 threads' k = 15);
        //   logit[a] from tr_head_logit, kept in registers
        //   max: each thread over its k ascending, then tr_tree_max;  sum of exp, the loss piece sum_a L[a] (log q[a] - log S) (an fmaf
        //   chain, entries with L[a] = 0 skipped) and t = sum_a L[a] r[a] (an fmaf chain): each thread over its k ascending, then tr_tree_sum
        //   d logit[a] as tr_policy_dense forms it; policy/policy's kernel and bias gradients from it, stored along a
        //   g_j = sum_a d logit[a] K[j][a], the gradient at every square's policy/convolution activation j before its ReLU mask: an fmaf
        //   chain per thread over its k ascending, then tr_tree_sum -- it does not depend on the square
        // LDS: the head scratch sm lies in gB and the four reduction arrays [256] (red) in gA.  The forward pass and the heads use
        // neither; tr_heads_bwd writes the gradient at the tower's output to gA only after the last reduction was read (a barrier in
        // between), and gB is first written by the backward tower.
        // The text stands here, in the else branch that the dense games discard, and not in a __forceinline__ function of its own: as
        // one, the same text compiled with 194 / 220 AGPRs (VGPR spill copies; reference / per-example loss) where it has 60 / 59
        // here and had 62 / 62 before the kernels were merged (`make resource-usage`; the timings: DESIGN.md section 10a).  Why the
        // register allocator answers differently was not traced to a cause.
        float *red = gA, *le = le_out + b, *lp = lp_out + b;
        constexpr int P = G::H * G::W, A = G::A, T = BB_TRAIN_THREADS, NK = (A + T - 1) / T;
        static_assert(A >= T, "every thread owns action tid");
        float *red0 = red, *red1 = red + T, *red2 = red + 2 * T, *red3 = red + 3 * T;
        // g_1's partial sums: red1 -- per example red2, because other waves may still be reading the sum of exp in red1[0] when
        // they are stored (red2[0] is read by thread 0 alone, which is the one that writes it there)
        float *rg1 = tr_wide_g1<LOSS>(red);
        float e[NK]; // the thread's logits, then their exponentials, then its softmax entries
#pragma unroll
        for (int k = 0; k < NK; k++) { // policy/policy
            const int a = tid + T * k;
            e[k] = a < A ? tr_head_logit<G>(lay, prm, sm + S::py, a) : 0.f;
        }
        tr_heads_dense<G>(lay, prm, sm, tid);
        {
            float mx = e[0]; // (A >= T: every thread owns action tid)
#pragma unroll
            for (int k = 1; k < NK; k++)
                if (tid + T * k < A) mx = fmaxf(mx, e[k]);
            red0[tid] = mx;
        }
        __syncthreads();
        tr_tree_max(tid, red0);
        if (tid == 0) tr_value_loss<G>(lay, prm, sm, src.value_of(row), n, le);
        float m[NK]; // reference: L[a] * r[a]; per example: the row's label pi[a]
        if constexpr (LOSS == BB_LOSS_PER_EXAMPLE) {
            // the sum of exp, the loss piece and T in one pass over the thread's k ascending (each an fmaf chain or a plain sum), then
            // one tr_tree_sum: sum_a pi[a] ((logit[a] - mx) - lse) = sum_a pi[a] (logit[a] - mx) - lse T, both terms of one sign
            const float mx = red0[0];
            float se = 0.f, ce = 0.f, t = 0.f;
#pragma unroll
            for (int k = 0; k < NK; k++) {
                const int a = tid + T * k;
                m[k] = 0.f;
                if (a < A) {
                    const float d = e[k] - mx;
                    m[k] = src.label_of(row, a);
                    ce = __builtin_fmaf(m[k], d, ce);
                    t = __builtin_fmaf(m[k], 1.0f, t);
                    e[k] = expf(d);
                    se += e[k];
                }
            }
            red1[tid] = se;
            red2[tid] = ce;
            red3[tid] = t;
            __syncthreads();
            tr_tree_sum(tid, red1, red2, red3);
            if (tid == 0) *lp = red3[0] != 0.f ? red2[0] - logf(red1[0]) * red3[0] : 0.f; // (no label: the row adds 0)
        } else {
            {
                const float mx = red0[0];
                float se = 0.f;
#pragma unroll
                for (int k = 0; k < NK; k++)
                    if (tid + T * k < A) {
                        e[k] = expf(e[k] - mx);
                        se += e[k];
                    }
                red1[tid] = se;
            }
            __syncthreads();
            tr_tree_sum(tid, red1);
            {
                const float sum = red1[0], logS = aux->logS;
                float ce = 0.f, t = 0.f;
#pragma unroll
                for (int k = 0; k < NK; k++) {
                    const int a = tid + T * k;
                    m[k] = 0.f;
                    if (a < A) {
                        e[k] = e[k] / sum; // softmax
                        const float q = __builtin_fmaf(eps, noise[a], (1.0f - eps) * e[k]), La = L[a];
                        if (La != 0.f) ce = __builtin_fmaf(La, logf(q) - logS, ce);
                        const float r = q > 0.f ? (1.0f - eps) * e[k] / q : 0.f;
                        t = __builtin_fmaf(La, r, t);
                        m[k] = La * r;
                    }
                }
                red2[tid] = ce;
                red3[tid] = t;
            }
            __syncthreads();
            tr_tree_sum(tid, red2, red3);
            if (tid == 0) *lp = red2[0];
        }
        {
            const float t = red3[0], sum = red1[0], inv_n2 = 1.0f / ((float)n * (float)n), spy0 = sm[S::misc + 1], spy1 = sm[S::misc + 2];
            float g0 = 0.f, g1 = 0.f;
#pragma unroll
            for (int k = 0; k < NK; k++) {
                const int a = tid + T * k;
                if (a < A) {
                    float dl;
                    if constexpr (LOSS == BB_LOSS_PER_EXAMPLE)
                        dl = ((e[k] / sum) * t - m[k]) / (float)n;
                    else
                        dl = -inv_n2 * (m[k] - e[k] * t);
                    slab[lay.p_d_b + a] = dl * (float)P;
                    slab[lay.p_d_k + a] = dl * spy0;
                    slab[lay.p_d_k + A + a] = dl * spy1;
                    g0 = __builtin_fmaf(dl, prm[lay.p_d_k + a], g0);
                    g1 = __builtin_fmaf(dl, prm[lay.p_d_k + A + a], g1);
                }
            }
            red0[tid] = g0;
            rg1[tid] = g1;
        }
        __syncthreads();
        tr_tree_sum(tid, red0, rg1);
    }
    tr_heads_bwd<G, LOSS>(lay, prm, x, sm, gA, slab, tid);
    tr_tower_bwd<G>(lay, prm, brd, wst, act, nrm, gA, gB, slab, tid);
}

// ---- k_train_apply ---------------------------------------------------------------------------------------------------
// One thread per parameter element: slabs summed b = 0 .. n-1, the L2 part, the update.  The workgroup after the last
// element reduces the loss pieces: loss[4] = total, evaluation, policy, parameter term.
__global__ void __launch_bounds__(BB_TRAIN_THREADS) k_train_apply(int count, int n, int n_l2, int loss_kind, float l2c, const float *__restrict__ slabs,
                                                                 const uint8_t *__restrict__ kind, float *__restrict__ prm,
                                                                 float *__restrict__ slot_m, float *__restrict__ slot_v, float *__restrict__ grads,
                                                                 int opt, float lr, float momentum, int apply, const float *le,
                                                                 const float *lp, const TrainAux *aux, float *loss, float *loss_out) {
    const int tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ double s_e[BB_TRAIN_THREADS], s_p[BB_TRAIN_THREADS];
        double e = 0.0, p = 0.0;
        for (int i = tid; i < n; i += BB_TRAIN_THREADS) {
            e += (double)le[i];
            p += (double)lp[i];
        }
        s_e[tid] = e;
        s_p[tid] = p;
        __syncthreads();
        tr_tree_sum(tid, s_e, s_p);
        if (tid == 0) {
            // reference: the B x B cross matrix's mean; per example: the mean over the rows
            const float l_e = (float)(s_e[0] / (double)n), l_w = aux->l2,
                        l_p = (float)(-s_p[0] / (loss_kind == BB_LOSS_PER_EXAMPLE ? (double)n : (double)n * (double)n));
            const float total = l_e + l_p + l_w;
            loss[0] = total; loss[1] = l_e; loss[2] = l_p; loss[3] = l_w;
            if (loss_out) {
                loss_out[0] = total; loss_out[1] = l_e; loss_out[2] = l_p; loss_out[3] = l_w;
            }
        }
        return;
    }
    const int i = blockIdx.x * BB_TRAIN_THREADS + tid;
    if (i >= count) return;
    const int kd = kind[i];
    if (kd == 0) {
        grads[i] = 0.f;
        return;
    }
    float g = 0.f;
    for (int b = 0; b < n; b++) g += slabs[(size_t)b * count + i];
    const float p = prm[i];
    if (kd == 1) g += loss_kind == BB_LOSS_PER_EXAMPLE ? l2c * p : p / (float)n_l2;
    grads[i] = g;
    if (!apply) return;
    if (opt == BB_OPT_ADAM) { // lr is lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); epsilon outside the bias correction (TF1)
        const float m = __builtin_fmaf(g, 0.1f, slot_m[i] * 0.9f), v = __builtin_fmaf(g * g, 0.001f, slot_v[i] * 0.999f);
        slot_m[i] = m;
        slot_v[i] = v;
        prm[i] = p - (lr * m) / (sqrtf(v) + 1e-8f);
    } else if (opt == BB_OPT_MOMENTUM) {
        const float m = __builtin_fmaf(momentum, slot_m[i], g);
        slot_m[i] = m;
        prm[i] = p - lr * m;
    } else {
        prm[i] = p - lr * g;
    }
}
