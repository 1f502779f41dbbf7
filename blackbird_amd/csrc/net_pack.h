// net_pack.h -- bb_net_weights -> the operand images the network kernels read.  Plain C++17 and nothing of HIP: a layout is
// stated here once, in the body that fills one piece of it, and tests/test_net_pack_cpu.py unpacks every image on the CPU.  A body
// is a function of the loop indices, marked NET_PACK_HD: the host loops below call it (bb_load_weights uploads their images byte
// for byte) and so do the kernels of net_pack.hip.h (bb_load_weights_device: the same images from weights in device memory).  A
// body writes every element of its piece, zeros included, so an image is complete whatever its buffer held before.
#pragma once
#include "../../include/blackbird_hip.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define NET_PACK_HD __host__ __device__
#else
#define NET_PACK_HD
#endif

// scale and shift of filters f0 .. f0 + n - 1 of a batch norm [4][F]: gamma, beta, moving mean, moving variance
// (float32, each operation rounded once: the build keeps the divide and the square root correctly rounded and contracts nothing)
NET_PACK_HD static inline void bn_fold(const float *bn, int F, int f0, int n, float *scale, float *shift) {
    for (int f = f0; f < f0 + n; f++) {
        float g = bn[0 * F + f], b = bn[1 * F + f], m = bn[2 * F + f], v = bn[3 * F + f];
        float s = g / sqrtf(v + 1e-3f); // tf.layers.batch_normalization default epsilon
        float t = m * s;
        scale[f - f0] = s;
        shift[f - f0] = b - t;
    }
}

// ---- bf16: every weight as three planes, w = w1 + w2 + w3 exactly ---------------------------------------------------
NET_PACK_HD static inline uint16_t bf16_rne(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
NET_PACK_HD static inline float bf16_value(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
NET_PACK_HD static inline void bf16_split3(float v, uint16_t out[3]) {
    out[0] = bf16_rne(v);
    float r = v - bf16_value(out[0]);
    out[1] = bf16_rne(r);
    r = r - bf16_value(out[1]);
    out[2] = bf16_rne(r);
}

// taps 0 .. 7 of a 3x3 tower convolution as four K = 32 slices of two taps x 16 channels -- (0, 1), (3, 4), (6, 7), (2, 5) --;
// tap 8 goes alone.  Tap h (0, 1) of slice sl:
NET_PACK_HD static inline int slice_tap(int sl, int h) { return sl < 3 ? 3 * sl + h : 2 + 3 * h; }

// weight of tower layer l (0 .. 2R - 1), tap, input channel c, filter f of an F-filter network
NET_PACK_HD static inline float tower_k(const bb_net_weights *w, int F, int l, int tap, int c, int f) {
    return w->blk_k[(((size_t)l * 9 + tap) * F + c) * F + f];
}

// ---- float32 MFMA operands (net.hip.h NetDev, gnet.hip.h GNetDev), NCB = F / 16 filter blocks --------------------------
// w0:  [NCB(fb)][steps0][64]: lane (f = lane & 15, j = lane >> 4) of K step s holds row k = 4s + j of the first convolution
//      ([9C][F], k = tap * C + channel) at filter 16 fb + f; rows >= 9C are zero
// wt:  [2R][NCB(fb)][NCB(cb)][9][64][4]: lane (f, j), element r = W[layer][tap][16 cb + 4j + r][16 fb + f]
// epi: [1 + 2R][NCB][3][16]: bias, batch-norm scale, batch-norm shift of the layer's filters 16 fb .. + 15
// The fused 16-filter tower (net.hip.h) reads the same image with NCB = 1.
NET_PACK_HD static inline int f32_steps0(int C) { return (9 * C + 3) / 4; }
NET_PACK_HD static inline size_t f32_w0_floats(int C, int NCB) { return (size_t)NCB * f32_steps0(C) * 64; }
NET_PACK_HD static inline size_t f32_wt_floats(int R, int NCB) { return (size_t)2 * R * NCB * NCB * 9 * 64 * 4; }
NET_PACK_HD static inline size_t f32_epi_floats(int R, int NCB) { return (size_t)(1 + 2 * R) * NCB * 48; }
// one (filter block, K step, lane) of w0
NET_PACK_HD static inline void pack_f32_w0(const bb_net_weights *w, int NCB, int fb, int s, int lane, float *w0) {
    (void)NCB;
    const int F = w->F, C = w->C, f = lane & 15, j = lane >> 4, k = 4 * s + j;
    w0[((size_t)fb * f32_steps0(C) + s) * 64 + lane] = k < 9 * C ? w->conv0_k[(size_t)k * F + 16 * fb + f] : 0.f;
}
// one (layer, filter block, channel block, tap, lane) of wt: its four channels
NET_PACK_HD static inline void pack_f32_wt(const bb_net_weights *w, int NCB, int l, int fb, int cb, int tap, int lane, float *wt) {
    const int F = w->F, f = lane & 15, j = lane >> 4;
    for (int r = 0; r < 4; r++)
        wt[((((((size_t)l * NCB + fb) * NCB + cb) * 9 + tap) * 64) + lane) * 4 + r] = tower_k(w, F, l, tap, 16 * cb + 4 * j + r, 16 * fb + f);
}
// one (layer, filter block) record of epi; layer 0 is the first convolution
NET_PACK_HD static inline void pack_f32_epi(const bb_net_weights *w, int NCB, int l, int fb, float *epi) {
    const int F = w->F;
    const float *b = l == 0 ? w->conv0_b : w->blk_b + (size_t)(l - 1) * F;
    const float *bn = l == 0 ? w->conv0_bn : w->blk_bn + (size_t)(l - 1) * 4 * F;
    float *rec = &epi[((size_t)l * NCB + fb) * 48];
    for (int f = 0; f < 16; f++) rec[f] = b[16 * fb + f];
    bn_fold(bn, F, 16 * fb, 16, rec + 16, rec + 32);
}
struct NetF32 {
    std::vector<float> w0, wt, epi;
    NetF32(int C, int R, int NCB) // zero-filled: what the fused tower's buffers hold while a wider network is loaded
        : w0(f32_w0_floats(C, NCB)), wt(f32_wt_floats(R, NCB)), epi(f32_epi_floats(R, NCB)) {}
};
static NetF32 pack_f32(const bb_net_weights *w, int NCB) {
    const int C = w->C, R = w->R, steps0 = f32_steps0(C);
    NetF32 o(C, R, NCB);
    for (int fb = 0; fb < NCB; fb++)
        for (int s = 0; s < steps0; s++)
            for (int lane = 0; lane < 64; lane++) pack_f32_w0(w, NCB, fb, s, lane, o.w0.data());
    for (int l = 0; l < 2 * R; l++)
        for (int fb = 0; fb < NCB; fb++)
            for (int cb = 0; cb < NCB; cb++)
                for (int tap = 0; tap < 9; tap++)
                    for (int lane = 0; lane < 64; lane++) pack_f32_wt(w, NCB, l, fb, cb, tap, lane, o.wt.data());
    for (int l = 0; l < 1 + 2 * R; l++)
        for (int fb = 0; fb < NCB; fb++) pack_f32_epi(w, NCB, l, fb, o.epi.data());
    return o;
}

// ---- the head parameters, back to back, each array padded with zeros to a multiple of 4 floats --------------------------
// v3 = value conv bias, batch-norm scale, shift; p6 = the two policy conv biases, scales, shifts
struct NetHeadOff {
    int off_vk, off_v3, off_d1k, off_d1b, off_d2k, off_d2b, off_pk, off_p6, off_pdk, off_pdb;
    int floats; // of the whole array
};
NET_PACK_HD static inline NetHeadOff head_offsets(int F, int D, int A) {
    NetHeadOff o;
    int at = 0;
    auto take = [&](int n) {
        int off = at;
        at += (n + 3) / 4 * 4;
        return off;
    };
    o.off_vk = take(F);
    o.off_v3 = take(3);
    o.off_d1k = take(D);
    o.off_d1b = take(D);
    o.off_d2k = take(D);
    o.off_d2b = take(1);
    o.off_pk = take(2 * F);
    o.off_p6 = take(6);
    o.off_pdk = take(2 * A);
    o.off_pdb = take(A);
    o.floats = at;
    return o;
}
// float i of the array: an element of the array it falls into, or the zero of that array's padding
NET_PACK_HD static inline float pack_head_float(const bb_net_weights *w, const NetHeadOff &o, int i) {
    const int F = w->F, D = w->D, A = w->A;
    auto in = [&](int off, const float *p, int n) { return i - off < n ? p[i - off] : 0.f; };
    if (i >= o.off_pdb) return in(o.off_pdb, w->p_d_b, A);
    if (i >= o.off_pdk) return in(o.off_pdk, w->p_d_k, 2 * A);
    if (i >= o.off_p6) { // the two biases, the two scales, the two shifts, two zeros
        const int j = i - o.off_p6;
        if (j < 2) return w->p_conv_b[j];
        if (j >= 6) return 0.f;
        float s, t;
        bn_fold(w->p_bn, 2, j & 1, 1, &s, &t);
        return j < 4 ? s : t;
    }
    if (i >= o.off_pk) return in(o.off_pk, w->p_conv_k, 2 * F);
    if (i >= o.off_d2b) return in(o.off_d2b, w->v_d2_b, 1);
    if (i >= o.off_d2k) return in(o.off_d2k, w->v_d2_k, D);
    if (i >= o.off_d1b) return in(o.off_d1b, w->v_d1_b, D);
    if (i >= o.off_d1k) return in(o.off_d1k, w->v_d1_k, D);
    if (i >= o.off_v3) { // the bias, the scale, the shift, a zero
        const int j = i - o.off_v3;
        if (j == 0) return w->v_conv_b[0];
        if (j >= 3) return 0.f;
        float s, t;
        bn_fold(w->v_bn, 1, 0, 1, &s, &t);
        return j == 1 ? s : t;
    }
    return in(o.off_vk, w->v_conv_k, F);
}
struct NetHead : NetHeadOff {
    std::vector<float> v;
};
static NetHead pack_head(const bb_net_weights *w) {
    NetHead o;
    static_cast<NetHeadOff &>(o) = head_offsets(w->F, w->D, w->A);
    o.v.resize((size_t)o.floats);
    for (int i = 0; i < o.floats; i++) o.v[i] = pack_head_float(w, o, i);
    return o;
}

// ---- operands of net_x3.hip.h: the 16-filter network as three bf16 planes, in A-operand lane order ----------------------
// (lane = 16 g + f: filter f, lane group g)
// w0:   narrow input: [plane][lane][8] (taps 2g, 2g + 1 x 4 input planes), then ONE operand [lane][8] for tap 8: lane group 0
//       = [w1 | w2] (4 input planes each), group 1 = [w3 | 0], groups 2, 3 zero -- against B = [x | x] that is all three planes
//       of the tap in one K = 32 product.  Wide input (DragonChess): [tap][plane][lane][8], lane group g = input planes 8g .. 8g + 7
// wt12: per layer [slice 0..3][plane 0..1][lane][8] (slices = taps (0,1), (3,4), (6,7), (2,5); lane group g: tap g >> 1 of the
//       slice, channels 8 (g & 1) .. + 7) then tap 8: [plane 0..1][channel half][filter][8] (what both halves of the lane groups read)
// wt3:  per layer [slice][lane][8] (the third plane alone) then [lane][8] = tap 8's operand [w1 | w3]: lane groups 0, 1 plane 1,
//       groups 2, 3 plane 3, channels 8 (g & 1) .. + 7
// wt8:  per layer [3][lane][8]: tap 8's three A operands [w1|w1], [w2|w2], [w1|w3] as 64-lane images (PP form)
// (tap 8 = three K = 32 products on plane-concatenated operands: [w1|w1].[x1;x2] + [w2|w2].[x1;x2] + [w1|w3].[x3;x1], net_x3.hip.h)
// wh:   [3][lane][8]: the head convolutions as a 16-filter K = 16 layer -- filter 0 = value conv, 4 and 8 = policy conv, the rest
//       zero (so that lane groups 0, 1, 2 of the result each hold ONE head's activation) -- in the three operands of tap 8
constexpr size_t X3_PER12 = 4 * 2 * 64 * 8 + 2 * 32 * 8, X3_PER3 = 4 * 64 * 8 + 64 * 8, X3_PER8 = 3 * 64 * 8; // uint16 of a layer
NET_PACK_HD static inline bool x3_wide(int C) { return C > 4; } // DragonChess: one K = 32 slice per tap, lane group g = input planes 8g .. 8g + 7
// uint16 counts of the five images, in NetX3's order: w0, wt12, wt3, wt8, wh
NET_PACK_HD static inline void x3_counts(int C, int R, size_t n[5]) {
    n[0] = x3_wide(C) ? (size_t)9 * 3 * 64 * 8 : (size_t)(3 * 64 * 8 + 64 * 8);
    n[1] = (size_t)2 * R * X3_PER12;
    n[2] = (size_t)2 * R * X3_PER3;
    n[3] = (size_t)2 * R * X3_PER8;
    n[4] = (size_t)3 * 64 * 8;
}
// one (tap, lane) of the wide first convolution
NET_PACK_HD static inline void pack_x3_w0_wide(const bb_net_weights *w, int tap, int lane, uint16_t *w0) {
    const int F = 16, C = w->C, f = lane & 15, g = lane >> 4;
    uint16_t h[3];
    for (int i = 0; i < 8; i++) {
        int ch = 8 * g + i;
        bf16_split3(ch < C ? w->conv0_k[((size_t)tap * C + ch) * F + f] : 0.f, h);
        for (int q = 0; q < 3; q++) w0[(((size_t)tap * 3 + q) * 64 + lane) * 8 + i] = h[q];
    }
}
// one lane of the narrow first convolution: its taps 2g, 2g + 1, and its part of tap 8's one operand
NET_PACK_HD static inline void pack_x3_w0_narrow(const bb_net_weights *w, int lane, uint16_t *w0) {
    const int F = 16, C = w->C, f = lane & 15, g = lane >> 4;
    uint16_t h[3];
    for (int i = 0; i < 8; i++) {
        int tap = 2 * g + (i >> 2), ch = i & 3;
        bf16_split3(ch < C ? w->conv0_k[((size_t)tap * C + ch) * F + f] : 0.f, h);
        for (int q = 0; q < 3; q++) w0[((size_t)q * 64 + lane) * 8 + i] = h[q];
    }
    for (int i = 0; i < 8; i++) { // tap 8: k slot i of lane group g = plane 2g + (i >> 2) of input plane i & 3; planes past the third: zero
        const int q = 2 * g + (i >> 2), ch = i & 3;
        bf16_split3(ch < C ? w->conv0_k[((size_t)8 * C + ch) * F + f] : 0.f, h);
        w0[(size_t)3 * 64 * 8 + (size_t)lane * 8 + i] = q > 2 ? (uint16_t)0 : h[q];
    }
}
// one lane of the head convolutions' three operands
NET_PACK_HD static inline void pack_x3_wh(const bb_net_weights *w, int lane, uint16_t *wh) {
    const int f = lane & 15, g = lane >> 4;
    const int head = f == 0 ? 0 : f == 4 ? 1 : f == 8 ? 2 : -1; // filter rows 0, 4, 8: the first result register of lane groups 0, 1, 2
    uint16_t h[3] = {0, 0, 0};
    for (int i = 0; i < 8; i++) {
        const int ch = 8 * (g & 1) + i;
        if (head >= 0) bf16_split3(head == 0 ? w->v_conv_k[ch] : w->p_conv_k[(size_t)ch * 2 + (head - 1)], h);
        wh[((size_t)0 * 64 + lane) * 8 + i] = h[0];
        wh[((size_t)1 * 64 + lane) * 8 + i] = h[1];
        wh[((size_t)2 * 64 + lane) * 8 + i] = g < 2 ? h[0] : h[2];
    }
}
// one (layer, lane) of the tower: its part of the layer's wt12, wt3 and wt8
NET_PACK_HD static inline void pack_x3_tower(const bb_net_weights *w, int l, int lane, uint16_t *wt12, uint16_t *wt3, uint16_t *wt8) {
    const int F = 16, f = lane & 15, g = lane >> 4;
    uint16_t *o12 = wt12 + (size_t)l * X3_PER12, *o3 = wt3 + (size_t)l * X3_PER3;
    uint16_t h[3];
    for (int sl = 0; sl < 4; sl++)
        for (int i = 0; i < 8; i++) {
            bf16_split3(tower_k(w, F, l, slice_tap(sl, g >> 1), 8 * (g & 1) + i, f), h);
            for (int q = 0; q < 2; q++) o12[(((size_t)sl * 2 + q) * 64 + lane) * 8 + i] = h[q];
            o3[((size_t)sl * 64 + lane) * 8 + i] = h[2];
        }
    for (int i = 0; i < 8; i++) { // tap 8, channels 8 (g & 1) .. + 7
        bf16_split3(tower_k(w, F, l, 8, 8 * (g & 1) + i, f), h);
        if (g < 2)
            for (int q = 0; q < 2; q++) o12[(size_t)4 * 2 * 64 * 8 + (((size_t)q * 2 + g) * 16 + f) * 8 + i] = h[q];
        const uint16_t a3 = g < 2 ? h[0] : h[2];
        o3[(size_t)4 * 64 * 8 + (size_t)lane * 8 + i] = a3;
        wt8[(((size_t)l * 3 + 0) * 64 + lane) * 8 + i] = h[0];
        wt8[(((size_t)l * 3 + 1) * 64 + lane) * 8 + i] = h[1];
        wt8[(((size_t)l * 3 + 2) * 64 + lane) * 8 + i] = a3;
    }
}
struct NetX3Image {
    std::vector<uint16_t> w0, wt12, wt3, wt8, wh; // uploaded back to back in this order (NetX3's pointers)
};
static NetX3Image pack_x3(const bb_net_weights *w) {
    const int C = w->C, R = w->R;
    NetX3Image o;
    auto &[w0, wt12, wt3, wt8, wh] = o;
    size_t n[5];
    x3_counts(C, R, n);
    w0.assign(n[0], 0);
    wt12.assign(n[1], 0);
    wt3.assign(n[2], 0);
    wt8.assign(n[3], 0);
    wh.assign(n[4], 0);
    for (int lane = 0; lane < 64; lane++) {
        if (x3_wide(C))
            for (int tap = 0; tap < 9; tap++) pack_x3_w0_wide(w, tap, lane, w0.data());
        else
            pack_x3_w0_narrow(w, lane, w0.data());
        pack_x3_wh(w, lane, wh.data());
    }
    for (int l = 0; l < 2 * R; l++)
        for (int lane = 0; lane < 64; lane++) pack_x3_tower(w, l, lane, wt12.data(), wt3.data(), wt8.data());
    return o;
}

// ---- tower operands of gnet_x3.hip.h: any filter count, three bf16 planes ------------------------------------------------
// [2R][NCB(fb)][NCB(cb)] blocks of GNET_X3_BLOCK uint16 (GX3_PAIR_B bytes), one per (filter block, channel block):
//   [slice 0..3][plane 0..2][lane][8]: lane (f, g) = filter 16 fb + f, tap g >> 1 of the slice, channels 16 cb + 8 (g & 1) .. + 7
//   then tap 8: [plane 0..2][lane][4]: channels 16 cb + 4g .. + 3
constexpr size_t GNET_X3_BLOCK = 4 * 3 * 64 * 8 + 3 * 64 * 4;
static std::vector<uint16_t> pack_gnet_x3(const bb_net_weights *w, int NCB) {
    const int F = w->F, R = w->R;
    std::vector<uint16_t> x((size_t)2 * R * NCB * NCB * GNET_X3_BLOCK);
    uint16_t h[3];
    for (int l = 0; l < 2 * R; l++)
        for (int fb = 0; fb < NCB; fb++)
            for (int cb = 0; cb < NCB; cb++) {
                uint16_t *o = x.data() + (((size_t)l * NCB + fb) * NCB + cb) * GNET_X3_BLOCK;
                for (int lane = 0; lane < 64; lane++) {
                    const int f = lane & 15, g = lane >> 4;
                    for (int sl = 0; sl < 4; sl++)
                        for (int i = 0; i < 8; i++) {
                            bf16_split3(tower_k(w, F, l, slice_tap(sl, g >> 1), 16 * cb + 8 * (g & 1) + i, 16 * fb + f), h);
                            for (int q = 0; q < 3; q++) o[(((size_t)sl * 3 + q) * 64 + lane) * 8 + i] = h[q];
                        }
                    for (int i = 0; i < 4; i++) {
                        bf16_split3(tower_k(w, F, l, 8, 16 * cb + 4 * g + i, 16 * fb + f), h);
                        for (int q = 0; q < 3; q++) o[(size_t)4 * 3 * 64 * 8 + ((size_t)q * 64 + lane) * 4 + i] = h[q];
                    }
                }
            }
    return x;
}
