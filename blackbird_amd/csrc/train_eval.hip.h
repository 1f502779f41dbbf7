// train_eval.hip.h -- score rows with the trainer's current device parameters, forward only (bb_trainer_eval,
// bb_trainer_eval_tensors): no step, no noise, no export.  Two launches:
//   k_train_eval         one workgroup per row: the forward pass of k_train_grad -- its tr_conv_fwd and its tr_head_* (train.hip.h),
//                        not a copy of them --, then the row's value, squared error, cross entropy against its own label and a
//                        flags byte
//   k_train_eval_totals  one workgroup, after the rows: integer counts and the two double sums
// The rows come through the sources of train.hip.h (TrainTensors: three tensors; TrainRecords: the records themselves, in any
// order and under any symmetry, decoded by example_row / example_plane / example_share / example_value), so what is scored is
// what bb_examples_to_batch_sym would have written.  Both kernels read the parameters and write their outputs, nothing else:
// not the optimiser slots, the gradient buffer, TrainAux or a counter of the trainer.
//
// Layout.  Forward only, so a residual block needs two activation buffers, not one per layer: conv_1 reads A and writes B, conv_2
// reads B, adds A and writes A in place (a thread reads and writes its own element only).  LDS does not depend on R:
//     2 buffers x P*16 floats + one staged conv kernel 9*16 rows of BB_TRAIN_WROW floats, static: a plain launch
//     Connect4 (P = 42):  2*672 + 2448 = 3792 floats = 15168 bytes
//     TicTacToe (P = 9):  2*144 + 2448 = 2736 floats = 10944 bytes
// The row's planes wait in B until conv_block has read them, and the head scratch (3P + 80 floats) lies there once the tower is
// done.  The conv is k_train_grad's, thread for thread (filter f = tid & 15, pixel group pg = tid >> 4: TicTacToe's 9 pixels leave
// 7 of the 16 groups idle).  LDS banks: the 16 lanes of a group read one 16-byte piece of a pixel (a broadcast), the four groups
// of a wave pixels 64 bytes apart -- 4 x 4 different banks --, and the weights come along f with BB_TRAIN_WROW's odd row stride.
// The heads take the first wave.
// Several rows per workgroup, sharing each staged conv kernel, measured slower on the MI355X and were retired: 13 107 Connect4
// records (4 blocks, dense 16) take 0.82 / 1.03 / 2.43 ms at 1 / 2 / 4 rows, 256 VGPRs and one wave per SIMD at 4; that variant
// (-DBB_TRAIN_EVAL_E) was last present at 3be01a0.
//
// Arithmetic: float32, every fused multiply-add explicit; the orders are written where the expressions are (tr_conv_fwd,
// tr_head_*).  The row's figures are taken by one lane: score_value_part and score_policy_serial below, the one statement of a
// scored row, which k_score_rows (examples_score.hip.h) takes for the engine's outputs too.
// (A <= 16: the serial form of k_train_grad's loss; a tree over 16 lanes was not built.)
#pragma once
#include "train.hip.h"

struct EvalTotals { // bb_eval_totals
    int64_t rows, policy_rows, top1, decided, sign_ok;
    double se_sum, ce_sum;
};

// ---- one scored row (the flags byte: BB_ROW_* of include/blackbird_hip.h) ---------------------------------------------
// A well-formed row's value part: out[0] = val, out[1] = se = (val - target)^2, one subtraction and one multiplication.
// COUNTED: the row is well-formed; DECIDED: target != 0; SIGN_OK: val and target both > 0 or both < 0.
__device__ __forceinline__ void score_value_part(float val, float target, float out[3], int &flags) {
    const float diff = val - target;
    out[0] = val;
    out[1] = diff * diff;
    flags = BB_ROW_COUNTED;
    if (target != 0.f) flags |= BB_ROW_DECIDED;
    if ((val > 0.f && target > 0.f) || (val < 0.f && target < 0.f)) flags |= BB_ROW_SIGN_OK;
}

// The policy part of a row of A <= 16 actions, by one lane, every loop a ascending; logit(a), label(a): the row's entries.
//     mx = max_a logit[a];  sum = sum_a expf(logit[a] - mx);  lse = logf(sum)                               (all A logits)
//     out[2] = ce = -(fmaf chain of pi[a] * ((logit[a] - mx) - lse)), left 0 for a row without a label
// HAS_POLICY: some pi[a] != 0; TOP1: first maximum of the logits == first maximum of the label, both in action order.
template <int A, class Logit, class Label>
__device__ __forceinline__ void score_policy_serial(Logit logit, Label label, float out[3], int &flags) {
    float pi[A];
    int best_pi = 0, best_lg = 0;
    bool any = false;
    float mx = logit(0), top_pi = 0.f, top_lg = logit(0);
    for (int a = 0; a < A; a++) { // (first maxima: a later equal entry does not replace an earlier one)
        pi[a] = label(a);
        any = any || pi[a] != 0.f; // (a record's share visits / total is 0 only for visits == 0: at least 2^-32 otherwise)
        if (a == 0 || pi[a] > top_pi) { top_pi = pi[a]; best_pi = a; }
        if (logit(a) > top_lg) { top_lg = logit(a); best_lg = a; }
        mx = fmaxf(mx, logit(a));
    }
    if (!any) return;
    float sum = 0.f;
    for (int a = 0; a < A; a++) sum += expf(logit(a) - mx);
    const float lse = logf(sum);
    float acc = 0.f;
    for (int a = 0; a < A; a++) acc = __builtin_fmaf(pi[a], (logit(a) - mx) - lse, acc);
    out[2] = -acc;
    flags |= BB_ROW_HAS_POLICY;
    if (best_pi == best_lg) flags |= BB_ROW_TOP1;
}

// ---- k_train_eval: one workgroup per row ------------------------------------------------------------------------------
template <class G, class Src>
__global__ void __launch_bounds__(BB_TRAIN_THREADS) k_train_eval(TrainLayout lay, const float *__restrict__ prm, Src src, int n,
                                                                float *__restrict__ rows_out, uint8_t *__restrict__ flags_out) {
    constexpr int P = G::H * G::W, C = G::C, A = G::A, F = BB_TRAIN_F, LF = P * F;
    constexpr int VY = 0, PY = P, HB = 3 * P, LG = 3 * P + 64; // the head scratch, in B
    static_assert(P <= 64 && P * C <= LF && LG + 16 <= LF && A <= 16 && LF % 4 == 0, "the planes and the head scratch fit B");
    __shared__ __attribute__((aligned(16))) float bufA[LF], bufB[LF], wst[9 * F * BB_TRAIN_WROW];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (b >= n) return;
    const int R = lay.R, D = lay.D;

    // ---- tower ----
    for (int i = tid; i < P * C; i += BB_TRAIN_THREADS) bufB[i] = src.plane(src.row(b), i);
    tr_stage<C, false>(wst, prm + lay.conv0_k, nullptr, tid);
    __syncthreads();
    tr_conv_fwd<G, C, false>(bufB, wst, prm + lay.conv0_b, prm + lay.conv0_bn, nullptr, nullptr, bufA, tid);
    __syncthreads();
    for (int l = 1; l <= 2 * R; l++) { // layer l: conv_{1,2} of block (l-1)/2; conv_1 A -> B, conv_2 B (+ A) -> A
        tr_stage<F, false>(wst, prm + lay.blk_k + (l - 1) * 9 * F * F, nullptr, tid);
        __syncthreads();
        const float *bias = prm + lay.blk_b + (l - 1) * F, *bn = prm + lay.blk_bn + (l - 1) * 4 * F;
        if (l & 1)
            tr_conv_fwd<G, F, false>(bufA, wst, bias, bn, nullptr, nullptr, bufB, tid);
        else
            tr_conv_fwd<G, F, false>(bufB, wst, bias, bn, bufA, nullptr, bufA, tid);
        __syncthreads();
    }

    // ---- heads: the first wave ----
    float *sc = bufB;
    float xh; // (the normalised head conv outputs: the backward pass's, not kept here)
    if (tid < P) sc[VY + tid] = tr_head_value_conv(lay, prm, bufA, tid, xh);
    if (tid < 64)
        for (int el = tid; el < 2 * P; el += 64) sc[PY + el] = tr_head_policy_conv(lay, prm, bufA, el >> 1, el & 1, xh);
    __syncthreads();
    if (tid < D) sc[HB + tid] = tr_head_dense_1<G>(lay, prm, sc + VY, tid);
    if (tid < A) sc[LG + tid] = tr_head_logit<G>(lay, prm, sc + PY, tid);
    __syncthreads();
    if (tid != 0) return;
    const typename Src::Row row = src.row(b);
    float out[3] = {0.f, 0.f, 0.f};
    int flags = 0;
    if (src.valid(row)) {
        score_value_part(tr_head_value(lay, prm, sc + HB), src.value_of(row), out, flags);
        score_policy_serial<A>([=](int a) { return sc[LG + a]; }, [=](int a) { return src.label_of(row, a); }, out, flags);
    } else {
        src.count(row, 0);
    }
    rows_out[(size_t)b * 3] = out[0];
    rows_out[(size_t)b * 3 + 1] = out[1];
    rows_out[(size_t)b * 3 + 2] = out[2];
    flags_out[b] = (uint8_t)flags;
}

// ---- k_train_eval_totals: one workgroup ------------------------------------------------------------------------------
// Thread t takes rows t, t + 256, ... in order: five integer counts and two double partial sums; then tr_tree_sum, the tree of
// k_train_apply's loss reduction.  No atomics: the same rows give the same bits.
__global__ void __launch_bounds__(BB_TRAIN_THREADS) k_train_eval_totals(int n, const float *__restrict__ rows, const uint8_t *__restrict__ flags,
                                                                       EvalTotals *__restrict__ out) {
    __shared__ double s_se[BB_TRAIN_THREADS], s_ce[BB_TRAIN_THREADS];
    __shared__ long long s_cnt[5][BB_TRAIN_THREADS];
    const int tid = threadIdx.x;
    double se = 0.0, ce = 0.0;
    long long cnt[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += BB_TRAIN_THREADS) {
        const int fl = flags[i];
        if (!(fl & BB_ROW_COUNTED)) continue;
        cnt[0]++;
        se += (double)rows[(size_t)i * 3 + 1];
        if (fl & BB_ROW_HAS_POLICY) {
            cnt[1]++;
            cnt[2] += (fl & BB_ROW_TOP1) != 0;
            ce += (double)rows[(size_t)i * 3 + 2];
        }
        if (fl & BB_ROW_DECIDED) {
            cnt[3]++;
            cnt[4] += (fl & BB_ROW_SIGN_OK) != 0;
        }
    }
    s_se[tid] = se;
    s_ce[tid] = ce;
    for (int c = 0; c < 5; c++) s_cnt[c][tid] = cnt[c];
    __syncthreads();
    tr_tree_sum(tid, s_se, s_ce, s_cnt[0], s_cnt[1], s_cnt[2], s_cnt[3], s_cnt[4]);
    if (tid == 0) {
        out->rows = s_cnt[0][0];
        out->policy_rows = s_cnt[1][0];
        out->top1 = s_cnt[2][0];
        out->decided = s_cnt[3][0];
        out->sign_ok = s_cnt[4][0];
        out->se_sum = s_se[0];
        out->ce_sum = s_ce[0];
    }
}
