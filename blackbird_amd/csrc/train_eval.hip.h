// train_eval.hip.h -- score rows with the trainer's current device parameters, forward only (bb_trainer_eval,
// bb_trainer_eval_tensors): no step, no noise, no export.  Two launches:
//   k_train_eval         one workgroup per BB_TRAIN_EVAL_E rows: the forward half of k_train_grad (train.hip.h), then per row the value,
//                        the squared error, the cross entropy against the row's own label and a flags byte
//   k_train_eval_totals  one workgroup, after the rows: integer counts and the two double sums
// The rows come through the sources of train.hip.h (TrainTensors: three tensors; TrainRecords: the records themselves, in any
// order and under any symmetry, decoded by example_row / example_plane / example_share / example_value), so what is scored is
// what bb_examples_to_batch_sym would have written.  Both kernels read the parameters and write their outputs, nothing else:
// not the optimiser slots, the gradient buffer, TrainAux or a counter of the trainer.
//
// Layout.  Forward only, so a residual block needs two activation buffers per row, not one per layer: conv_1 reads A and writes
// B, conv_2 reads B, adds A and writes A in place (a thread reads and writes its own element only).  LDS does not depend on R:
//     2 buffers x E rows x P*16 floats + one staged conv kernel 9*16 rows of BB_TRAIN_WROW floats, static: a plain launch
//     Connect4 (P = 42):  E = 1: 2*672 + 2448 = 3792 floats = 15168 bytes;  E = 4: 2*4*672 + 2448 = 7824 floats = 31296 bytes
//     TicTacToe (P = 9):  E = 1: 2*144 + 2448 = 2736 floats = 10944 bytes;  E = 4: 2*4*144 + 2448 = 3600 floats = 14400 bytes
// The planes of a row wait in its part of B until conv_block has read them, and the head scratch (3P + 80 floats a row) lies
// there once the tower is done.  The E rows of a workgroup share every staged conv kernel: one tr_stage per layer per workgroup.
// The conv spreads the E*P pixels of the workgroup over the 16 pixel groups (thread: filter f = tid & 15, group pg = tid >> 4;
// slot s = pg + 16 k is pixel s % P of row s / P), so a thread loads a weight once for all its slots.  LDS banks: the 16 lanes
// of a group read one 16-byte piece of a pixel (a broadcast), the four groups of a wave pixels 64 bytes apart -- 4 x 4 different
// banks --, and the weights come along f with BB_TRAIN_WROW's odd row stride, as in k_train_grad.
// The heads take one wave per row (wave w: rows w, w + 4, ...), with k_train_grad's expressions.
// E = BB_TRAIN_EVAL_E = 1, because that is what measured fastest on the MI355X: 13 107 Connect4 records (4 blocks, dense 16) take
// 0.82 ms at E = 1, 1.03 ms at E = 2 and 2.43 ms at E = 4.  Sharing the staged kernels does not pay for what it costs in registers:
// the 11 slots a Connect4 thread owns at E = 4, unrolled over nine taps, need 256 VGPRs -- one wave per SIMD, one workgroup per
// CU -- where the 3 slots of E = 1 need 90 and leave room for five waves per SIMD.  The kernel is written over E so that the
// comparison can be repeated (-DBB_TRAIN_EVAL_E=4); at E = 1 TicTacToe (9 slots) leaves 7 of its 16 pixel groups idle.
//
// Arithmetic: float32, every fused multiply-add explicit.  A conv output is one fmaf chain over (tap, ci) in that order, padding
// skipped; the head convs chain over f, dense_1 and policy/policy sum their squares in order, dense_2 chains over d: the
// orders of k_train_grad's forward half, so value and logits are its bits.  The row's figures are taken by one lane, in order:
//     mx = max_a logit[a] (a ascending);  sum = sum_a expf(logit[a] - mx) (a ascending);  lse = logf(sum)
//     ce = -(fmaf chain over a ascending of pi[a] * ((logit[a] - mx) - lse)), 0 for a row without a label
// (A <= 16: the serial form of k_train_grad's loss; a tree over 16 lanes was not built.)
#pragma once
#include "train.hip.h"

#ifndef BB_TRAIN_EVAL_E
#define BB_TRAIN_EVAL_E 1 // rows per workgroup (the header comment says why; -DBB_TRAIN_EVAL_E=2, 4: several, for comparison)
#endif

// (the flags byte of a row: BB_ROW_* of include/blackbird_hip.h)

struct EvalTotals { // bb_eval_totals
    int64_t rows, policy_rows, top1, decided, sign_ok;
    double se_sum, ce_sum;
};

// k_train_grad's tr_conv_fwd for E rows at once and without the normalised output: X is [E][xs] floats (pixel-major, CIN
// values a pixel), res and act [E][P*16].  res == act is allowed.
template <class G, int CIN, int E>
__device__ __forceinline__ void tr_eval_conv(const float *X, int xs, const float *wst, const float *bias, const float *bn,
                                             const float *res, float *act, int tid) {
    constexpr int P = G::H * G::W, F = BB_TRAIN_F, NS = (E * P + 15) / 16;
    const int f = tid & 15, pg = tid >> 4;
    float acc[NS];
    int base[NS], pr[NS], pc[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) {
        const int s = pg + 16 * k, e = s / P, p = s % P;
        acc[k] = 0.f;
        base[k] = e * xs;
        pr[k] = p / G::W;
        pc[k] = p % G::W;
    }
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        bool ok[NS];
        int q[NS];
#pragma unroll
        for (int k = 0; k < NS; k++) {
            const int r = pr[k] + dy, c = pc[k] + dx;
            ok[k] = pg + 16 * k < E * P && r >= 0 && r < G::H && c >= 0 && c < G::W;
            q[k] = ok[k] ? base[k] + (r * G::W + c) * CIN : 0;
        }
        if constexpr (CIN % 4 == 0) {
#pragma unroll
            for (int c4 = 0; c4 < CIN / 4; c4++) {
                float w[4];
#pragma unroll
                for (int j = 0; j < 4; j++) w[j] = wst[(tap * CIN + 4 * c4 + j) * BB_TRAIN_WROW + f];
#pragma unroll
                for (int k = 0; k < NS; k++)
                    if (ok[k]) {
                        const float4 x = ((const float4 *)(X + q[k]))[c4];
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
                for (int k = 0; k < NS; k++)
                    if (ok[k]) acc[k] = __builtin_fmaf(X[q[k] + ci], w, acc[k]);
            }
        }
    }
    const float b = bias[f], g = bn[f], be = bn[F + f], mu = bn[2 * F + f], inv = tr_bn_inv(bn[3 * F + f]);
#pragma unroll
    for (int k = 0; k < NS; k++) {
        const int s = pg + 16 * k;
        if (s < E * P) {
            const float xh = ((acc[k] + b) - mu) * inv;
            float y = __builtin_fmaf(g, xh, be);
            if (res) y += res[s * F + f];
            act[s * F + f] = fmaxf(y, 0.f);
        }
    }
}

// ---- k_train_eval: one workgroup per E rows ---------------------------------------------------------------------------
template <class G, class Src>
__global__ void __launch_bounds__(BB_TRAIN_THREADS) k_train_eval(TrainLayout lay, const float *__restrict__ prm, Src src, int n,
                                                                float *__restrict__ rows_out, uint8_t *__restrict__ flags_out) {
    constexpr int P = G::H * G::W, C = G::C, A = G::A, F = BB_TRAIN_F, LF = P * F, E = BB_TRAIN_EVAL_E;
    constexpr int VY = 0, PY = P, HB = 3 * P, LG = 3 * P + 64; // the head scratch of a row, in its part of B
    static_assert(P * C <= LF && LG + 16 <= LF && A <= 16 && LF % 4 == 0, "a row's planes and head scratch fit its part of B");
    __shared__ __attribute__((aligned(16))) float bufA[E * LF], bufB[E * LF], wst[9 * F * BB_TRAIN_WROW];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t first = (size_t)blockIdx.x * E; // (rows first .. first + E - 1; those >= n are computed as zeros and not written)
    const int R = lay.R, D = lay.D;

    // ---- tower ----
    for (int i = tid; i < E * P * C; i += BB_TRAIN_THREADS) {
        const int e = i / (P * C), el = i % (P * C);
        float v = 0.f;
        if (first + e < (size_t)n) v = src.plane(src.row((int)(first + e)), el);
        bufB[e * LF + el] = v;
    }
    tr_stage<C, false>(wst, prm + lay.conv0_k, nullptr, tid);
    __syncthreads();
    tr_eval_conv<G, C, E>(bufB, LF, wst, prm + lay.conv0_b, prm + lay.conv0_bn, nullptr, bufA, tid);
    __syncthreads();
    for (int l = 1; l <= 2 * R; l++) { // layer l: conv_{1,2} of block (l-1)/2; conv_1 A -> B, conv_2 B (+ A) -> A
        tr_stage<F, false>(wst, prm + lay.blk_k + (l - 1) * 9 * F * F, nullptr, tid);
        __syncthreads();
        if (l & 1)
            tr_eval_conv<G, F, E>(bufA, LF, wst, prm + lay.blk_b + (l - 1) * F, prm + lay.blk_bn + (l - 1) * 4 * F, nullptr, bufB, tid);
        else
            tr_eval_conv<G, F, E>(bufB, LF, wst, prm + lay.blk_b + (l - 1) * F, prm + lay.blk_bn + (l - 1) * 4 * F, bufA, bufA, tid);
        __syncthreads();
    }

    // ---- heads: wave w takes rows w, w + 4, ...; the expressions of k_train_grad ----
    for (int e = wave; e < E; e += BB_TRAIN_THREADS / 64) {
        const float *x = bufA + e * LF;
        float *sc = bufB + e * LF;
        if (lane < P) { // value/convolution (1x1, one filter), batch norm, ReLU
            float acc = 0.f;
            for (int f = 0; f < F; f++) acc = __builtin_fmaf(x[lane * F + f], prm[lay.v_conv_k + f], acc);
            const float xh = ((acc + prm[lay.v_conv_b]) - prm[lay.v_bn + 2]) * tr_bn_inv(prm[lay.v_bn + 3]);
            sc[VY + lane] = fmaxf(__builtin_fmaf(prm[lay.v_bn], xh, prm[lay.v_bn + 1]), 0.f);
        }
        for (int el = lane; el < 2 * P; el += 64) { // policy/convolution (1x1, two filters)
            const int p = el >> 1, j = el & 1;
            float acc = 0.f;
            for (int f = 0; f < F; f++) acc = __builtin_fmaf(x[p * F + f], prm[lay.p_conv_k + f * 2 + j], acc);
            const float xh = ((acc + prm[lay.p_conv_b + j]) - prm[lay.p_bn + 4 + j]) * tr_bn_inv(prm[lay.p_bn + 6 + j]);
            sc[PY + el] = fmaxf(__builtin_fmaf(prm[lay.p_bn + j], xh, prm[lay.p_bn + 2 + j]), 0.f);
        }
    }
    __syncthreads();
    for (int e = wave; e < E; e += BB_TRAIN_THREADS / 64) {
        float *sc = bufB + e * LF;
        if (lane < D) { // value/dense_1 on every square, summed over the squares, ReLU
            const float k1 = prm[lay.v_d1_k + lane], b1 = prm[lay.v_d1_b + lane];
            float acc = 0.f;
            for (int p = 0; p < P; p++) acc += __builtin_fmaf(sc[VY + p], k1, b1);
            sc[HB + lane] = fmaxf(acc, 0.f);
        }
        if (lane < A) { // policy/policy on every square, summed
            const float k0 = prm[lay.p_d_k + lane], k1 = prm[lay.p_d_k + A + lane], pb = prm[lay.p_d_b + lane];
            float acc = 0.f;
            for (int p = 0; p < P; p++)
                acc += __builtin_fmaf(sc[PY + 2 * p + 1], k1, __builtin_fmaf(sc[PY + 2 * p], k0, pb));
            sc[LG + lane] = acc;
        }
    }
    __syncthreads();
    for (int e = wave; e < E; e += BB_TRAIN_THREADS / 64) {
        if (lane != 0 || first + e >= (size_t)n) continue;
        const size_t j = first + e;
        const float *sc = bufB + e * LF;
        const typename Src::Row row = src.row((int)j);
        float out[3] = {0.f, 0.f, 0.f};
        uint8_t flags = 0;
        if (src.valid(row)) {
            float z = prm[lay.v_d2_b];
            for (int d = 0; d < D; d++) z = __builtin_fmaf(sc[HB + d], prm[lay.v_d2_k + d], z);
            const float val = tanhf(z), target = src.value_of(row), diff = val - target;
            out[0] = val;
            out[1] = diff * diff;
            flags = BB_ROW_COUNTED;
            if (target != 0.f) flags |= BB_ROW_DECIDED;
            if ((val > 0.f && target > 0.f) || (val < 0.f && target < 0.f)) flags |= BB_ROW_SIGN_OK;
            float pi[A];
            int best_pi = 0, best_lg = 0;
            bool any = false;
            float mx = sc[LG], top_pi = 0.f, top_lg = sc[LG];
            for (int a = 0; a < A; a++) { // (first maxima: a later equal entry does not replace an earlier one)
                pi[a] = src.label_of(row, a);
                any = any || pi[a] != 0.f;
                if (a == 0 || pi[a] > top_pi) { top_pi = pi[a]; best_pi = a; }
                if (sc[LG + a] > top_lg) { top_lg = sc[LG + a]; best_lg = a; }
                mx = fmaxf(mx, sc[LG + a]);
            }
            if (any) {
                float sum = 0.f;
                for (int a = 0; a < A; a++) sum += expf(sc[LG + a] - mx);
                const float lse = logf(sum);
                float acc = 0.f;
                for (int a = 0; a < A; a++) acc = __builtin_fmaf(pi[a], (sc[LG + a] - mx) - lse, acc);
                out[2] = -acc;
                flags |= BB_ROW_HAS_POLICY;
                if (best_pi == best_lg) flags |= BB_ROW_TOP1;
            }
        } else {
            src.count(row, 0);
        }
        rows_out[j * 3] = out[0];
        rows_out[j * 3 + 1] = out[1];
        rows_out[j * 3 + 2] = out[2];
        flags_out[j] = flags;
    }
}

// ---- k_train_eval_totals: one workgroup ------------------------------------------------------------------------------
// Thread t takes rows t, t + 256, ... in order: five integer counts and two double partial sums; then the tree of
// k_train_apply's loss reduction (w = 128, 64, ... 1: [t] += [t + w]).  No atomics: the same rows give the same bits.
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
    for (int w = BB_TRAIN_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_se[tid] += s_se[tid + w];
            s_ce[tid] += s_ce[tid + w];
            for (int c = 0; c < 5; c++) s_cnt[c][tid] += s_cnt[c][tid + w];
        }
        __syncthreads();
    }
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
