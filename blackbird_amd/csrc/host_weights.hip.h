// host_weights.hip.h -- the weight loads (host-packed and on the device), the network launches (launch_gnet, launch_net) and
// the bb_net_eval* / bb_hash_eval entry points.
#pragma once
extern "C" int bb_net_form(bb_engine *e) {
    if (!e) return fail(BB_ERR_ARG, "null engine");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    if (e->general_net) return e->gx3.wt ? 3 : 1;
    return e->x3.w0 ? 2 : 0;
}

// ---- weights: pack on the host (net_pack.h), keep or reallocate the operand buffers, upload ---------------------------
static_assert(GNET_X3_BLOCK * 2 == GX3_PAIR_B, "net_pack.h and gnet_x3.hip.h must agree on the tower's weight block");
template <class T>
static int upload(void *dst, const std::vector<T> &v) {
    if (!v.empty()) HIPCHK(hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return BB_OK;
}

// ---- general-F network (gnet.hip.h): buffers, weights, launch sequence -------------------------------------------------
template <class G>
static int gnet_reserve(bb_engine *e, int n) {
    using GG = GNetGeom<G>;
    GNetDev &g = e->gnet;
    int cap = (n + GG::PPB - 1) / GG::PPB * GG::PPB;
    if (cap <= g.cap) return BB_OK;
    HIPCHK(sync_all(e));
    size_t pos_floats = (size_t)g.NCB * 4 * GG::PLANE;
    if (e->own.alloc(g.inp, (size_t)cap * GG::SLOTS * GG::CP) || e->own.alloc(g.act[0], (size_t)cap * pos_floats))
        return BB_ERR_HIP; // zero-filled: the halo ring of every position stays zero for the buffers' lifetime
    if (e->gx3.wt) { // bf16-pipe tower: two buffers of three bf16 planes; the float32 buffer above only carries the last layer
        const size_t pos_bytes = (size_t)g.NCB * GG::SLOTS * 96;
        if (e->own.alloc(e->gx3.act3[0], (size_t)cap * pos_bytes) || e->own.alloc(e->gx3.act3[1], (size_t)cap * pos_bytes)) return BB_ERR_HIP;
    } else if (e->own.alloc(g.act[1], (size_t)cap * pos_floats)) {
        return BB_ERR_HIP;
    }
    HIPCHK(sync_all(e)); // the fills ran on the engine stream; the caller may launch on another one
    g.cap = cap;
    return BB_OK;
}

// img: pack_f32 at F / 16 filter blocks
static int load_general_weights(bb_engine *e, const bb_net_weights *w, const NetF32 &img) {
    const int F = w->F, C = w->C, R = w->R, NCB = F / 16;
    // the tower layers' operands as three bf16 planes (gnet_x3.hip.h); BB_NET_FORM_F32 keeps the float32-MFMA layers
    const bool want3 = R > 0 && e->cfg.net_form != BB_NET_FORM_F32;
    const std::vector<uint16_t> x = want3 ? pack_gnet_x3(w, NCB) : std::vector<uint16_t>();
    GNetDev &g = e->gnet;
    // weights are reloaded after every training step: keep the device buffers (operands and activation scratch) when
    // the network shape is unchanged instead of allocating new ones each time
    const bool same = g.F == F && g.R == R && g.NCB == NCB && g.w0 && e->gnet_C == C;
    float *d_w0 = (float *)g.w0, *d_wt = (float *)g.wt, *d_epi = (float *)g.epi;
    if (!same) {
        g = GNetDev{};
        g.F = F;
        g.NCB = NCB;
        g.R = R;
        e->gnet_C = C;
        if (e->own.alloc(d_w0, img.w0.size(), false) || e->own.alloc(d_wt, img.wt.size(), false) || e->own.alloc(d_epi, img.epi.size(), false))
            return BB_ERR_HIP;
    }
    HIPCHK(sync_all(e));
    if (upload(d_w0, img.w0) || upload(d_wt, img.wt) || upload(d_epi, img.epi)) return BB_ERR_HIP;
    g.w0 = d_w0;
    g.wt = (const f32x4 *)d_wt;
    g.epi = d_epi;
    if (want3) {
        unsigned char *d_x = (unsigned char *)e->gx3.wt;
        if (!d_x || x.size() * 2 != e->gx3_bytes) {
            if (e->own.alloc(d_x, x.size() * 2 + 16, false)) return BB_ERR_HIP;
            e->gx3_bytes = x.size() * 2;
            g.cap = 0; // (the activation buffers of the other form are re-reserved on the next launch)
        }
        if (upload(d_x, x)) return BB_ERR_HIP;
        e->gx3.wt = d_x;
    } else {
        if (e->gx3.wt) g.cap = 0;
        e->gx3.wt = nullptr;
    }
    return BB_OK;
}

// How launch_gnet cuts a call of up to n_max positions at NCB filter blocks -- the ONE place that decides it.  Small batch: one
// position x one filter block per wave (latency of a lone evaluation: 40 layers x ~25 us instead of x ~170 us at 256 filters);
// every larger call, and every call whose size lives on the device (n_ptr), takes PPB positions x FBW filter blocks per wave.
// bb_net_eval_structure reports it for a host-sized call.
static bool gnet_small_launch(int n_max, int NCB, const int *n_ptr) { return (long)n_max * NCB <= 2048 && !n_ptr; }

// n_ptr != nullptr: the batch size lives in device memory (<= n_max); slot_list maps batch entries to mailbox slots
template <class G>
static int launch_gnet(bb_engine *e, int n_max, const int *n_ptr, const int *slot_list, const typename G::State *states,
                       const int8_t *planes, const uint32_t *game_id, const int32_t *serial, int noise, float *value,
                       float *logits, float *policy, int pstride, hipStream_t st, int buf_offset = 0,
                       EvalCache store = {nullptr, 0}) {
    // store: the evaluation cache the heads fill (the batch is a round's miss list: eval_probe.hip.h)
    // buf_offset: first position of the activation buffers this call may use (the two slot-range views of pipelined
    // rounds run on two streams at once and must not share scratch)
    using GG = GNetGeom<G>;
    buf_offset = (buf_offset + GG::PPB - 1) / GG::PPB * GG::PPB;
    int rc = gnet_reserve<G>(e, buf_offset + n_max);
    if (rc) return rc;
    GNetDev g = e->gnet;
    {
        const size_t pos_floats = (size_t)g.NCB * 4 * GG::PLANE;
        g.inp += (size_t)buf_offset * GG::SLOTS * GG::CP;
        g.act[0] += (size_t)buf_offset * pos_floats;
        if (g.act[1]) g.act[1] += (size_t)buf_offset * pos_floats; // (not allocated when the tower layers run in the split-operand form)
    }
    k_gnet_input<G><<<nblk((size_t)n_max * GG::HW), 256, 0, st>>>(g, n_max, n_ptr, slot_list, states, planes);
    GNetX3 gx = e->gx3; // wt != nullptr: tower layers on the bf16 matrix pipe (gnet_x3.hip.h); first conv in float32 MFMA, writing the split form
    if (gx.wt) {
        const size_t pos_bytes = (size_t)g.NCB * GG::SLOTS * 96;
        gx.act3[0] += (size_t)buf_offset * pos_bytes;
        gx.act3[1] += (size_t)buf_offset * pos_bytes;
    }
    const bool small = gnet_small_launch(n_max, g.NCB, n_ptr);
    constexpr int FBW3 = 4;
    // a workgroup's four waves take `per` neighbours along y (filter blocks, or groups of FBW of them) and 4 / per along x
    // (positions, or groups of PPB of them)
    const int nx = small ? n_max : (n_max + GG::PPB - 1) / GG::PPB;
    auto cut = [&](int fbw, int &per) {
        const int ny = small ? g.NCB : (g.NCB + fbw - 1) / fbw;
        per = ny >= 4 ? 4 : (ny >= 2 ? 2 : 1);
        return dim3((nx + 4 / per - 1) / (4 / per), (ny + per - 1) / per);
    };
    int per0, per;
    const dim3 grid0 = cut(GN_FBW, per0), grid = cut(gx.wt ? FBW3 : GN_FBW, per); // first convolution, tower
    auto *conv0 = small ? k_gnet_conv<G, true, 1, 1> : k_gnet_conv<G, true>;
    conv0<<<grid0, 256, 0, st>>>(g, 0, n_max, n_ptr, nullptr, g.act[0], 0, per0, gx.wt ? gx.act3[0] : nullptr);
    const int L = 2 * g.R;
    if (gx.wt) {
        auto *mid = small ? k_gnet_conv_x3<G, 1, 1, false> : k_gnet_conv_x3<G, GG::PPB, FBW3, false>;
        auto *last = small ? k_gnet_conv_x3<G, 1, 1, true> : k_gnet_conv_x3<G, GG::PPB, FBW3, true>; // writes float32, for the heads
        for (int l = 0; l < L; l++)
            (l + 1 < L ? mid : last)<<<grid, 256, 0, st>>>(g, gx, 1 + l, n_max, n_ptr, gx.act3[l & 1], gx.act3[(l & 1) ^ 1],
                                                           l + 1 < L ? nullptr : g.act[0], l & 1, per);
    } else {
        auto *conv = small ? k_gnet_conv<G, false, 1, 1> : k_gnet_conv<G, false>;
        for (int l = 0; l < L; l++)
            conv<<<grid, 256, 0, st>>>(g, 1 + l, n_max, n_ptr, g.act[l & 1], g.act[(l & 1) ^ 1], l & 1, per, nullptr);
    }
    k_gnet_heads<G><<<(n_max + 3) / 4, 256, 0, st>>>(g, e->net, n_max, n_ptr, slot_list, g.act[0], game_id, serial, noise, value,
                                                     logits, policy, pstride, store, planes ? nullptr : states);
    HIPCHK(hipGetLastError());
    return BB_OK;
}

// What every entry point asks of a bb_net_weights before anything else: the game's planes and actions, and every block the
// shape needs (net_blocks.h).  `who`, where given, goes in front of the message.
static int check_weights(const bb_net_weights *w, const bb_game_info &gi, const char *who = nullptr) {
    const std::string pre = who ? std::string(who) + ": " : "";
    if (w->H != gi.H || w->W != gi.W || w->C != gi.C || w->A != gi.A)
        return fail(BB_ERR_ARG, "%sweights are for a %dx%dx%d/%d network, game needs %dx%dx%d/%d", pre.c_str(), w->H, w->W, w->C, w->A,
                    gi.H, gi.W, gi.C, gi.A);
    if (net_block_missing(*w)) return fail(BB_ERR_ARG, "%sa weight block is missing", pre.c_str());
    return BB_OK;
}

extern "C" int bb_load_weights(bb_engine *e, const bb_net_weights *w) {
    if (!e || !w) return fail(BB_ERR_ARG, "null argument");
    if (int rc = check_weights(w, e->info)) return rc;
    if (w->F <= 0 || w->F % 16 != 0 || w->F > 1024)
        return fail(BB_ERR_ARG, "filters must be a multiple of 16 (MFMA tile), got %d", w->F);
    if (w->D <= 0 || w->D > 64 || w->R < 0) return fail(BB_ERR_ARG, "unsupported dense/blocks");
    HIPCHK(hipSetDevice(e->cfg.device));
    // no evaluation outlives the weights (or the network form) it was made with
    if (e->eval_cache_bytes) HIPCHK(hipMemsetAsync(e->dev.eval_cache, 0, e->eval_cache_bytes, e->stream));
    const int F = w->F, C = w->C, R = w->R;
    e->general_net = F != 16 || e->cfg.general_net != 0;
    // operands of the fused single-wave tower (net.hip.h): the one-block image; a wider network leaves them zero
    const NetF32 img = F == 16 ? pack_f32(w, 1) : NetF32(C, R, 1);
    if (e->general_net) {
        int rc = load_general_weights(e, w, F == 16 ? img : pack_f32(w, F / 16));
        if (rc) return rc;
    }
    const NetHead head = pack_head(w);
    // the bf16-pipe form of the same network (every game, 16 filters); BB_NET_FORM_F32 keeps the float32 MFMA path
    const bool want3 = F == 16 && C <= 32 && !e->general_net && e->cfg.net_form != BB_NET_FORM_F32;
    const NetX3Image x = want3 ? pack_x3(w) : NetX3Image();
    NetDev &nd = e->net;
    // (weights are reloaded after every training step: the operand buffers are reused while their sizes stay the same)
    float *d_w0 = (float *)nd.w0, *d_wt = (float *)nd.wt, *d_epi = (float *)nd.epi, *d_head = (float *)nd.head;
    const size_t sizes[4] = {img.w0.size(), img.wt.size(), img.epi.size(), head.v.size()};
    if (!d_w0 || memcmp(sizes, e->net_sizes, sizeof(sizes)) != 0) {
        if (e->own.alloc(d_w0, sizes[0], false) || e->own.alloc(d_wt, sizes[1], false) || e->own.alloc(d_epi, sizes[2], false) ||
            e->own.alloc(d_head, sizes[3], false))
            return BB_ERR_HIP;
        memcpy(e->net_sizes, sizes, sizeof(sizes));
    }
    HIPCHK(sync_all(e));
    if (upload(d_w0, img.w0) || upload(d_wt, img.wt) || upload(d_epi, img.epi) || upload(d_head, head.v)) return BB_ERR_HIP;
    if (want3) { // one buffer, the five images back to back
        const std::vector<uint16_t> *part[5] = {&x.w0, &x.wt12, &x.wt3, &x.wt8, &x.wh};
        size_t at[6] = {0};
        for (int i = 0; i < 5; i++) at[i + 1] = at[i] + part[i]->size() * 2;
        unsigned char *d_x = (unsigned char *)e->x3.w0;
        if (!d_x || at[5] != e->x3_bytes) {
            if (e->own.alloc(d_x, at[5] + 16, false)) return BB_ERR_HIP;
            e->x3_bytes = at[5];
        }
        for (int i = 0; i < 5; i++)
            if (upload(d_x + at[i], *part[i])) return BB_ERR_HIP;
        e->x3 = NetX3{d_x + at[0], d_x + at[1], d_x + at[2], d_x + at[3], d_x + at[4]};
    } else {
        e->x3 = NetX3{nullptr, nullptr, nullptr, nullptr, nullptr};
    }
    nd.R = R;
    nd.D = w->D;
    nd.A = w->A;
    nd.w0 = d_w0;
    nd.wt = (const f32x4 *)d_wt;
    nd.epi = d_epi;
    nd.head = d_head;
    nd.head_floats = (int)head.v.size();
    nd.off_vk = head.off_vk; nd.off_v3 = head.off_v3; nd.off_d1k = head.off_d1k; nd.off_d1b = head.off_d1b; nd.off_d2k = head.off_d2k;
    nd.off_d2b = head.off_d2b; nd.off_pk = head.off_pk; nd.off_p6 = head.off_p6; nd.off_pdk = head.off_pdk; nd.off_pdb = head.off_pdb;
    nd.seed = e->cfg.seed;
    nd.alpha = e->cfg.alpha;
    nd.eps = e->cfg.epsilon;
    nd.inv_alpha = 1.0f / nd.alpha;
    nd.inv_beta = 1.0f / (1.0f - nd.alpha);
    nd.dbg = 0; // (ablation switches exist in diagnostic builds only: bb_timing_net, stamps.hip.h)
    e->has_weights = true;
    e->net_F = F;
    e->net_C = C;
    return BB_OK;
}

// ---- weights that are in device memory already: pack on the device (net_pack.hip.h) into the buffers bb_load_weights made ----
static int load_weights_device(bb_engine *e, const bb_net_weights *w, hipStream_t stream, const char *who) {
    if (int rc = check_weights(w, e->info, who)) return rc;
    if (!e->has_weights || !e->net.w0 || !e->net.head)
        return fail(BB_ERR_STATE, "%s: the engine has no weight buffers yet -- its first load is bb_load_weights, which allocates them", who);
    if (e->general_net)
        return fail(BB_ERR_STATE, "%s covers the fused 16-filter tower; this engine runs its %d-filter network through the "
                    "launch-per-layer kernels", who, e->net_F);
    const bool want3 = w->C <= 32 && e->cfg.net_form != BB_NET_FORM_F32;
    if (w->F != 16 || e->net_F != 16 || w->C != e->net_C || w->R != e->net.R || w->D != e->net.D || w->A != e->net.A ||
        want3 != (e->x3.w0 != nullptr))
        return fail(BB_ERR_STATE, "%s: the engine's buffers hold a network of %d planes, %d filters, %d blocks, dense %d, %d actions "
                    "(%s); the weights given have %d, %d, %d, %d, %d", who, e->net_C, e->net_F, e->net.R, e->net.D, e->net.A,
                    e->x3.w0 ? "split form" : "float32 form", w->C, w->F, w->R, w->D, w->A);
    NetDev &nd = e->net;
    const NetHeadOff off = head_offsets(16, w->D, w->A);
    if (off.floats != nd.head_floats || (size_t)off.floats != e->net_sizes[3])
        return fail(BB_ERR_STATE, "%s: the head array holds %d floats, these weights need %d", who, nd.head_floats, off.floats);
    if (int rc = engine_on_current_device(e, who, "weights")) return rc;
    // weights must not change under a running search; behind whatever `stream` has queued (the steps that made these weights) ...
    if (int rc = engine_stream_after(e, stream)) return rc;
    // ... no evaluation outlives the weights it was made with ...
    if (e->eval_cache_bytes) HIPCHK(hipMemsetAsync(e->dev.eval_cache, 0, e->eval_cache_bytes, e->stream));
    auto blocks = [](int threads) { return (unsigned)((threads + NET_PACK_THREADS - 1) / NET_PACK_THREADS); };
    k_pack_f32<<<blocks(pack_f32_threads(w->C, w->R)), NET_PACK_THREADS, 0, e->stream>>>(*w, (float *)nd.w0, (float *)nd.wt, (float *)nd.epi);
    k_pack_head<<<blocks(off.floats), NET_PACK_THREADS, 0, e->stream>>>(*w, off, (float *)nd.head);
    if (e->x3.w0)
        k_pack_x3<<<blocks(pack_x3_threads(w->C, w->R)), NET_PACK_THREADS, 0, e->stream>>>(
            *w, (uint16_t *)e->x3.w0, (uint16_t *)e->x3.wt12, (uint16_t *)e->x3.wt3, (uint16_t *)e->x3.wt8, (uint16_t *)e->x3.wh);
    HIPCHK(hipGetLastError());
    // ... and everything else waits for the images: the engine's second stream, and `stream` itself, so that the weights may be
    // freed or stepped on as soon as `stream` has come this far
    return engine_stream_release(e, stream, true);
}

extern "C" int bb_load_weights_device(bb_engine *e, const bb_net_weights *w_dev, void *stream) {
    if (!e || !w_dev) return fail(BB_ERR_ARG, "null argument");
    return load_weights_device(e, w_dev, (hipStream_t)stream, "bb_load_weights_device");
}

extern "C" int bb_weights_read(bb_engine *e, int which, void *host_out, int64_t capacity, int64_t *bytes_out) {
    if (!e || (!host_out && !bytes_out)) return fail(BB_ERR_ARG, "null argument");
    if (which < BB_WEIGHTS_W0 || which > BB_WEIGHTS_X3) return fail(BB_ERR_ARG, "unknown image %d", which);
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    const void *src[5] = {e->net.w0, e->net.wt, e->net.epi, e->net.head, e->x3.w0};
    const int64_t bytes = which == BB_WEIGHTS_X3 ? (e->x3.w0 ? (int64_t)e->x3_bytes : 0) : (int64_t)(e->net_sizes[which] * sizeof(float));
    if (bytes_out) *bytes_out = bytes;
    if (!host_out) return BB_OK;
    if (capacity < bytes) return fail(BB_ERR_ARG, "image %d has %lld bytes, the buffer %lld", which, (long long)bytes, (long long)capacity);
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(sync_all(e));
    if (bytes) HIPCHK(hipMemcpy(host_out, src[which], (size_t)bytes, hipMemcpyDeviceToHost));
    return BB_OK;
}

// positions per wave of the fused tower, chosen so that 4 waves' activations fill the 160 KiB LDS
template <class G> struct NetPW;
template <> struct NetPW<Connect4> { static constexpr int v = 4; };
template <> struct NetPW<TicTacToe> { static constexpr int v = 12; };
template <> struct NetPW<DragonChess> { static constexpr int v = 1; }; // 64 pixels = 4 full tiles; 1024 games fill 256 CUs

template <class G>
static int launch_net(bb_engine *e, int n, const typename G::State *states, const int8_t *planes,
                      const uint32_t *game_id, const int32_t *serial, int noise, float *value, float *logits,
                      float *policy, int pstride, hipStream_t st) {
    if (e->general_net)
        return launch_gnet<G>(e, n, nullptr, nullptr, states, planes, game_id, serial, noise, value, logits, policy, pstride, st);
    // positions per wave: the fewest that still put a wave on every SIMD (1024 waves) -- a single FindMove position
    // must not pay for the 11 MFMA tiles of a 4-position wave
    constexpr int PW = NetPW<G>::v;
    {
        if (e->x3.w0) { // one position per wave on the bf16 pipe: the same arithmetic everywhere (bb_net_eval, search, self-play)
            k_net_x3<G><<<(n + 3) / 4, 256, 0, st>>>(e->net, e->x3, n, nullptr, nullptr, states, planes, game_id, serial, noise, value,
                                                     logits, policy, pstride, EvalCache{nullptr, 0});
            HIPCHK(hipGetLastError());
            return BB_OK;
        }
    }
    if (PW > 1 && n <= 1024) {
        k_net_fused16<G, 1><<<(n + 3) / 4, 256, 0, st>>>(e->net, n, states, planes, game_id, serial, noise, value, logits, policy,
                                                         pstride);
    } else if (PW > 2 && n <= 2048) {
        k_net_fused16<G, 2><<<(n + 7) / 8, 256, 0, st>>>(e->net, n, states, planes, game_id, serial, noise, value, logits, policy,
                                                         pstride);
    } else {
        int blocks = (n + 4 * PW - 1) / (4 * PW);
        k_net_fused16<G, PW><<<blocks, 256, 0, st>>>(e->net, n, states, planes, game_id, serial, noise, value, logits,
                                                      policy, pstride);
    }
    HIPCHK(hipGetLastError());
    return BB_OK;
}

template <class G>
static int net_eval(bb_engine *e, int n, const void *states, const int8_t *planes, float *value, float *logits,
                    float *policy, int noise, const uint32_t *game_ids = nullptr, const int32_t *serials = nullptr) {
    const int A = G::A;
    Staged<typename G::State> dst; // the input: one of the two is allocated, the other stays null
    Staged<int8_t> dpl;
    Staged<float> dv, dl, dp;
    Staged<uint32_t> dg;
    Staged<int32_t> dser;
    if ((states ? dst.alloc((size_t)n) : dpl.alloc((size_t)n * G::H * G::W * G::C)) || dv.alloc((size_t)n) || dl.alloc((size_t)n * A) ||
        dp.alloc((size_t)n * A) || dg.alloc((size_t)n) || dser.alloc((size_t)n))
        return BB_ERR_HIP;
    if (int rc = states ? dst.from_host(states) : dpl.from_host(planes)) return rc;
    if (game_ids)
        if (int rc = dg.from_host(game_ids)) return rc;
    if (serials)
        if (int rc = dser.from_host(serials)) return rc;
    int rc = launch_net<G>(e, n, dst.get(), dpl.get(), game_ids ? dg.get() : nullptr, serials ? dser.get() : nullptr, noise, dv.get(),
                           dl.get(), dp.get(), A, e->stream);
    if (rc) return rc;
    HIPCHK(sync_all(e));
    if (value)
        if (int rc = dv.to_host(value)) return rc;
    if (logits)
        if (int rc = dl.to_host(logits)) return rc;
    return policy ? dp.to_host(policy) : BB_OK;
}

extern "C" int bb_net_eval(bb_engine *e, int n, const void *states, const int8_t *planes, float *value_out,
                           float *logits_out, float *policy_out, int noise) {
    if (e && n == 0) return BB_OK; // an empty batch is a no-op
    if (!e || n < 0 || (!states == !planes)) return fail(BB_ERR_ARG, "bad arguments (exactly one of states/planes)");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    HIPCHK(hipSetDevice(e->cfg.device));
    GAME_SWITCH(e->cfg.game, return net_eval<G>(e, n, states, planes, value_out, logits_out, policy_out, noise));
}

extern "C" int bb_net_eval_structure(bb_engine *e, int n, int32_t *out) {
    if (!e || !out || n < 0) return fail(BB_ERR_ARG, "bb_net_eval_structure: an engine, n >= 0 and a place for the answer");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    *out = !e->general_net ? BB_NET_EVAL_FUSED : gnet_small_launch(n, e->gnet.NCB, nullptr) ? BB_NET_EVAL_SMALL : BB_NET_EVAL_BATCH;
    return BB_OK;
}

extern "C" int bb_net_eval_keyed(bb_engine *e, int n, const void *states, const int8_t *planes, const uint32_t *game_ids,
                                 const int32_t *node_serials, float *value_out, float *logits_out, float *policy_out) {
    if (e && n == 0) return BB_OK;
    if (!e || n < 0 || (!states == !planes) || !game_ids || !node_serials)
        return fail(BB_ERR_ARG, "bad arguments (exactly one of states/planes; game_ids and node_serials are required)");
    if (!e->has_weights) return fail(BB_ERR_WEIGHTS, "bb_load_weights has not been called");
    HIPCHK(hipSetDevice(e->cfg.device));
    GAME_SWITCH(e->cfg.game, return net_eval<G>(e, n, states, planes, value_out, logits_out, policy_out, 1, game_ids, node_serials));
}

template <class G>
static int hash_eval(bb_engine *e, int n, const void *states, float *value, float *policy) {
    Staged<typename G::State> ds;
    Staged<float> dv, dp;
    if (ds.alloc((size_t)n) || dv.alloc((size_t)n) || dp.alloc((size_t)n * G::A)) return BB_ERR_HIP;
    if (int rc = ds.from_host(states)) return rc;
    Launch<G>::hash(e->stream, n, ds.get(), nullptr, e->cfg.hash_salt, 0, 0, dv.get(), dp.get(), G::A);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_all(e));
    if (value)
        if (int rc = dv.to_host(value)) return rc;
    return policy ? dp.to_host(policy) : BB_OK;
}

extern "C" int bb_hash_eval(bb_engine *e, int n, const void *states, float *value_out, float *policy_out) {
    if (e && n == 0) return BB_OK;
    if (!e || n < 0 || !states) return fail(BB_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->cfg.device));
    GAME_SWITCH(e->cfg.game, return hash_eval<G>(e, n, states, value_out, policy_out));
}
