// net_pack.hip.h -- the operand images of net_pack.h, packed on the device from weights that are in device memory
// (bb_load_weights_device).  No layout is stated here: every kernel is one thread per call of a body of net_pack.h, so what it
// writes is the host image byte for byte -- the bf16 split is integer arithmetic, the batch-norm fold one correctly rounded
// float32 operation per step (-ffp-contract=off; hipcc keeps the float32 divide and square root of HIP code correctly rounded
// and float32 subnormals as they are).  16 filters, one filter block: the fused tower's operands in both net forms.
#pragma once
#include "net_pack.h"

#define NET_PACK_THREADS 256

// the float32 image: w0 (one thread per K step and lane), wt (per layer, tap and lane), epi (per layer record)
static __global__ void k_pack_f32(bb_net_weights w, float *w0, float *wt, float *epi) {
    const int n_w0 = f32_steps0(w.C) * 64, n_wt = 2 * w.R * 9 * 64, n_epi = 1 + 2 * w.R;
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_w0) return pack_f32_w0(&w, 1, 0, i >> 6, i & 63, w0);
    i -= n_w0;
    if (i < n_wt) return pack_f32_wt(&w, 1, i / (9 * 64), 0, 0, (i >> 6) % 9, i & 63, wt);
    i -= n_wt;
    if (i < n_epi) pack_f32_epi(&w, 1, i, 0, epi);
}
static inline int pack_f32_threads(int C, int R) { return f32_steps0(C) * 64 + 2 * R * 9 * 64 + 1 + 2 * R; }

// the head: one thread per float of the array, its padding included
static __global__ void k_pack_head(bb_net_weights w, NetHeadOff off, float *head) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < off.floats) head[i] = pack_head_float(&w, off, i);
}

// the five bf16 images: w0 (wide: one thread per tap and lane; narrow: per lane), wh (per lane), the tower (per layer and lane)
static __global__ void k_pack_x3(bb_net_weights w, uint16_t *w0, uint16_t *wt12, uint16_t *wt3, uint16_t *wt8, uint16_t *wh) {
    const bool wide = x3_wide(w.C);
    const int n_w0 = wide ? 9 * 64 : 64, n_t = 2 * w.R * 64;
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_w0) {
        if (wide) pack_x3_w0_wide(&w, i >> 6, i & 63, w0);
        else pack_x3_w0_narrow(&w, i, w0);
        return;
    }
    i -= n_w0;
    if (i < 64) return pack_x3_wh(&w, i, wh);
    i -= 64;
    if (i < n_t) pack_x3_tower(&w, i >> 6, i & 63, wt12, wt3, wt8);
}
static inline int pack_x3_threads(int C, int R) { return (x3_wide(C) ? 9 * 64 : 64) + 64 + 2 * R * 64; }
