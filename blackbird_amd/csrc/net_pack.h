// net_pack.h -- bb_net_weights -> the operand images the network kernels read.  Host only, plain C++17 and nothing of HIP: a
// layout is stated here once, next to the loop that fills it, and tests/test_net_pack_cpu.py unpacks every image on the CPU.
// engine.hip (bb_load_weights) owns the device buffers and uploads these images byte for byte.
#pragma once
#include "../../include/blackbird_hip.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// scale and shift of filters f0 .. f0 + n - 1 of a batch norm [4][F]: gamma, beta, moving mean, moving variance
static void bn_fold(const float *bn, int F, int f0, int n, float *scale, float *shift) {
    for (int f = f0; f < f0 + n; f++) {
        float g = bn[0 * F + f], b = bn[1 * F + f], m = bn[2 * F + f], v = bn[3 * F + f];
        float s = g / sqrtf(v + 1e-3f); // tf.layers.batch_normalization default epsilon
        float t = m * s;
        scale[f - f0] = s;
        shift[f - f0] = b - t;
    }
}

// ---- bf16: every weight as three planes, w = w1 + w2 + w3 exactly ---------------------------------------------------
static uint16_t bf16_rne(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static float bf16_value(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static void bf16_split3(float v, uint16_t out[3]) {
    out[0] = bf16_rne(v);
    float r = v - bf16_value(out[0]);
    out[1] = bf16_rne(r);
    r = r - bf16_value(out[1]);
    out[2] = bf16_rne(r);
}

// taps 0 .. 7 of a 3x3 tower convolution as four K = 32 slices of two taps x 16 channels; tap 8 goes alone
static const int slice_taps[4][2] = {{0, 1}, {3, 4}, {6, 7}, {2, 5}};

// weight of tower layer l (0 .. 2R - 1), tap, input channel c, filter f of an F-filter network
static inline float tower_k(const bb_net_weights *w, int F, int l, int tap, int c, int f) {
    return w->blk_k[(((size_t)l * 9 + tap) * F + c) * F + f];
}

// ---- float32 MFMA operands (net.hip.h NetDev, gnet.hip.h GNetDev), NCB = F / 16 filter blocks --------------------------
// w0:  [NCB(fb)][steps0][64]: lane (f = lane & 15, j = lane >> 4) of K step s holds row k = 4s + j of the first convolution
//      ([9C][F], k = tap * C + channel) at filter 16 fb + f; rows >= 9C are zero
// wt:  [2R][NCB(fb)][NCB(cb)][9][64][4]: lane (f, j), element r = W[layer][tap][16 cb + 4j + r][16 fb + f]
// epi: [1 + 2R][NCB][3][16]: bias, batch-norm scale, batch-norm shift of the layer's filters 16 fb .. + 15
// The fused 16-filter tower (net.hip.h) reads the same image with NCB = 1.
struct NetF32 {
    std::vector<float> w0, wt, epi;
    NetF32(int C, int R, int NCB) // zero-filled: what the fused tower's buffers hold while a wider network is loaded
        : w0((size_t)NCB * ((9 * C + 3) / 4) * 64), wt((size_t)2 * R * NCB * NCB * 9 * 64 * 4), epi((size_t)(1 + 2 * R) * NCB * 48) {}
};
static NetF32 pack_f32(const bb_net_weights *w, int NCB) {
    const int F = w->F, C = w->C, R = w->R, steps0 = (9 * C + 3) / 4;
    NetF32 o(C, R, NCB);
    for (int fb = 0; fb < NCB; fb++)
        for (int s = 0; s < steps0; s++)
            for (int lane = 0; lane < 64; lane++) {
                int f = lane & 15, j = lane >> 4, k = 4 * s + j;
                o.w0[((size_t)fb * steps0 + s) * 64 + lane] = k < 9 * C ? w->conv0_k[(size_t)k * F + 16 * fb + f] : 0.f;
            }
    for (int l = 0; l < 2 * R; l++)
        for (int fb = 0; fb < NCB; fb++)
            for (int cb = 0; cb < NCB; cb++)
                for (int tap = 0; tap < 9; tap++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int r = 0; r < 4; r++) {
                            int f = lane & 15, j = lane >> 4;
                            o.wt[((((((size_t)l * NCB + fb) * NCB + cb) * 9 + tap) * 64) + lane) * 4 + r] =
                                tower_k(w, F, l, tap, 16 * cb + 4 * j + r, 16 * fb + f);
                        }
    for (int l = 0; l < 1 + 2 * R; l++) {
        const float *b = l == 0 ? w->conv0_b : w->blk_b + (size_t)(l - 1) * F;
        const float *bn = l == 0 ? w->conv0_bn : w->blk_bn + (size_t)(l - 1) * 4 * F;
        for (int fb = 0; fb < NCB; fb++) {
            float *rec = &o.epi[((size_t)l * NCB + fb) * 48];
            memcpy(rec, b + 16 * fb, 64);
            bn_fold(bn, F, 16 * fb, 16, rec + 16, rec + 32);
        }
    }
    return o;
}

// ---- the head parameters, back to back, each array padded with zeros to a multiple of 4 floats --------------------------
// v3 = value conv bias, batch-norm scale, shift; p6 = the two policy conv biases, scales, shifts
struct NetHead {
    std::vector<float> v;
    int off_vk, off_v3, off_d1k, off_d1b, off_d2k, off_d2b, off_pk, off_p6, off_pdk, off_pdb;
};
static NetHead pack_head(const bb_net_weights *w) {
    const int F = w->F, D = w->D, A = w->A;
    NetHead o;
    auto push = [&](const float *p, int n) {
        int off = (int)o.v.size();
        o.v.insert(o.v.end(), p, p + n);
        while (o.v.size() % 4) o.v.push_back(0.f);
        return off;
    };
    float v3[3], p6[6], s1, t1, s2[2], t2[2];
    bn_fold(w->v_bn, 1, 0, 1, &s1, &t1);
    bn_fold(w->p_bn, 2, 0, 2, s2, t2);
    v3[0] = w->v_conv_b[0]; v3[1] = s1; v3[2] = t1;
    p6[0] = w->p_conv_b[0]; p6[1] = w->p_conv_b[1]; p6[2] = s2[0]; p6[3] = s2[1]; p6[4] = t2[0]; p6[5] = t2[1];
    o.off_vk = push(w->v_conv_k, F);
    o.off_v3 = push(v3, 3);
    o.off_d1k = push(w->v_d1_k, D);
    o.off_d1b = push(w->v_d1_b, D);
    o.off_d2k = push(w->v_d2_k, D);
    o.off_d2b = push(w->v_d2_b, 1);
    o.off_pk = push(w->p_conv_k, 2 * F);
    o.off_p6 = push(p6, 6);
    o.off_pdk = push(w->p_d_k, 2 * A);
    o.off_pdb = push(w->p_d_b, A);
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
struct NetX3Image {
    std::vector<uint16_t> w0, wt12, wt3, wt8, wh; // uploaded back to back in this order (NetX3's pointers)
};
static NetX3Image pack_x3(const bb_net_weights *w) {
    const int F = 16, C = w->C, R = w->R;
    const bool wide = C > 4; // DragonChess: one K = 32 slice per tap, lane group g = input planes 8g .. 8g + 7
    NetX3Image o;
    auto &[w0, wt12, wt3, wt8, wh] = o;
    w0.assign(wide ? (size_t)9 * 3 * 64 * 8 : (size_t)(3 * 64 * 8 + 64 * 8), 0);
    const size_t per12 = 4 * 2 * 64 * 8 + 2 * 32 * 8, per3 = 4 * 64 * 8 + 64 * 8;
    wt12.assign((size_t)2 * R * per12, 0);
    wt3.assign((size_t)2 * R * per3, 0);
    wt8.assign((size_t)2 * R * 3 * 64 * 8, 0);
    uint16_t h[3];
    for (int lane = 0; wide && lane < 64; lane++) {
        const int f = lane & 15, g = lane >> 4;
        for (int tap = 0; tap < 9; tap++)
            for (int i = 0; i < 8; i++) {
                int ch = 8 * g + i;
                bf16_split3(ch < C ? w->conv0_k[((size_t)tap * C + ch) * F + f] : 0.f, h);
                for (int q = 0; q < 3; q++) w0[(((size_t)tap * 3 + q) * 64 + lane) * 8 + i] = h[q];
            }
    }
    for (int lane = 0; !wide && lane < 64; lane++) {
        const int f = lane & 15, g = lane >> 4;
        for (int i = 0; i < 8; i++) {
            int tap = 2 * g + (i >> 2), ch = i & 3;
            bf16_split3(ch < C ? w->conv0_k[((size_t)tap * C + ch) * F + f] : 0.f, h);
            for (int q = 0; q < 3; q++) w0[((size_t)q * 64 + lane) * 8 + i] = h[q];
        }
        for (int i = 0; i < 8 && g < 2; i++) { // tap 8: k slot i of lane group g = plane 2g + (i >> 2) of input plane i & 3
            const int q = 2 * g + (i >> 2), ch = i & 3;
            if (q > 2) continue;
            bf16_split3(ch < C ? w->conv0_k[((size_t)8 * C + ch) * F + f] : 0.f, h);
            w0[(size_t)3 * 64 * 8 + (size_t)lane * 8 + i] = h[q];
        }
    }
    wh.assign((size_t)3 * 64 * 8, 0);
    for (int lane = 0; lane < 64; lane++) {
        const int f = lane & 15, g = lane >> 4;
        const int head = f == 0 ? 0 : f == 4 ? 1 : f == 8 ? 2 : -1; // filter rows 0, 4, 8: the first result register of lane groups 0, 1, 2
        for (int i = 0; i < 8 && head >= 0; i++) {
            const int ch = 8 * (g & 1) + i;
            bf16_split3(head == 0 ? w->v_conv_k[ch] : w->p_conv_k[(size_t)ch * 2 + (head - 1)], h);
            wh[((size_t)0 * 64 + lane) * 8 + i] = h[0];
            wh[((size_t)1 * 64 + lane) * 8 + i] = h[1];
            wh[((size_t)2 * 64 + lane) * 8 + i] = g < 2 ? h[0] : h[2];
        }
    }
    for (int l = 0; l < 2 * R; l++) {
        uint16_t *o12 = wt12.data() + (size_t)l * per12, *o3 = wt3.data() + (size_t)l * per3;
        for (int lane = 0; lane < 64; lane++) {
            const int f = lane & 15, g = lane >> 4;
            for (int sl = 0; sl < 4; sl++)
                for (int i = 0; i < 8; i++) {
                    bf16_split3(tower_k(w, F, l, slice_taps[sl][g >> 1], 8 * (g & 1) + i, f), h);
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
    }
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
                            bf16_split3(tower_k(w, F, l, slice_taps[sl][g >> 1], 16 * cb + 8 * (g & 1) + i, 16 * fb + f), h);
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
