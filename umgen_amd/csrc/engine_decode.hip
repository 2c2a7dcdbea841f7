// One decode step: decode_path, the one statement of which path takes a step of B scenes (batched layer, chip-wide engine, XCD-resident engine, five
// launches per layer); the BlockOAR layers on the path they are handed (oar_layers), the head and sampler behind them (enqueue_step) -- both on the DecView they
// are handed: its stream, its buffers, its flags, nothing read from or swapped into the engine; a decode lane's view of the batch (lane_view); the drain launch of
// the background workers; and the test hooks on a live handle (one step on the path that was asked for, K/V cache rows in and out, the tag epoch).
#include "engine_state.h"

// host arithmetic stays unfused in every engine file, as it was while they were one file behind the numpy-faithful helpers (engine_weights.hip)
#pragma clang fp contract(off)

namespace {

// one OAR decode step through the 36 BlockOAR layers (module.py:402-416) for the B scenes of v, on `path` (decode_path's answer, or the path a test hook asks for)
template <typename T>
int oar_layers(umgen_engine* e, const DecView& v, int B, int ns, DecodePath path) {
    const int E = e->E, H = e->H;
    const int* d_len = &v.d_state->step;
    if constexpr (sizeof(T) == 2) {
        if (path == PATH_BATCHED) {      // five launches per layer for the whole batch: LN + q|k|v, attention, c_proj (+x), LN + c_fc + GELU, mlp c_proj (+x)
            // activations between the launches are fragment-major (decode_batched.hip); x also stays row-major in xdec (sampler, residual)
            launch_rows_to_frag(v.stream, v.xdec, E, B, E, v.xfrag);
            for (size_t li = 0; li < e->oar.size(); ++li) {
                const SubW& w = e->oar[e->dbg_same_layer ? 0 : li];
                T* cache = reinterpret_cast<T*>(v.kvcache) + (long)li * e->kv_layer_stride;
                RowsArgs r{};
                r.x = v.xfrag; r.M = B; r.ln_w = w.ln_a; r.W = w.attn.Wqkv; r.bias = w.attn.bqkv; r.N = 3 * E; r.K = E; r.mode = ROWS_QKV;
                r.out = v.qdec; r.ldo = E; r.cache = cache; r.scene_stride = e->kv_scene_stride; r.d_len = d_len; r.Lmax = e->Lmax; r.E = E;
                launch_rows_mfma<T>(v.stream, r);
                launch_attn_decode_batched<T>(v.stream, v.qdec, cache, e->kv_scene_stride, B, H, e->Lmax, d_len, v.afrag);
                RowsArgs p{};
                p.x = v.afrag; p.M = B; p.W = w.attn.Wo; p.bias = w.attn.bo; p.N = E; p.K = E; p.mode = ROWS_RESID; p.out = v.xdec; p.ldo = E; p.out_frag = v.xfrag; p.E = E;
                launch_rows_mfma<T>(v.stream, p);
                RowsArgs f{};
                f.x = v.xfrag; f.M = B; f.ln_w = w.ln_b; f.W = w.mlp.Wfc; f.N = 4 * E; f.K = E; f.mode = ROWS_GELU; f.out_frag = v.hfrag; f.E = E;
                launch_rows_mfma<T>(v.stream, f);
                RowsArgs q{};
                q.x = v.hfrag; q.M = B; q.W = w.mlp.Wproj; q.N = E; q.K = 4 * E; q.mode = ROWS_RESID; q.out = v.xdec; q.ldo = E; q.out_frag = v.xfrag; q.E = E;
                launch_rows_mfma<T>(v.stream, q);
            }
            return 0;
        }
    }
    if (path == PATH_WIDE) {
        OarWideArgs a{};
        a.layers = e->d_layers_wide; a.n_layers = (int)e->oar.size();
        a.kvcache = reinterpret_cast<bf16_t*>(v.kvcache); a.kv_layer_stride = e->kv_layer_stride; a.kv_scene_stride = e->kv_scene_stride; a.Lmax = e->Lmax;
        a.xdec = v.xdec; a.st = v.d_state; a.gran = e->wide_gran; a.ticket = e->wide_ticket; a.err = e->wide_err;
        a.fp16 = std::is_same<T, f16_t>::value ? 1 : 0;
        a.stamps = e->wide_stamps;
        for (int b = 0; b < B; ++b) {
            a.scene = b;
            HIPCHK(e, launch_oar_engine_wide(v.stream, a));
        }
        return 0;
    }
    if (path == PATH_ENGINE) {
        const umgen_engine::EngStream* es = e->eng_for(v.stream);
        if (!es) return e->fail(UMGEN_E_UNSUPPORTED, "the XCD-resident decode engine has no census for this stream");
        OarEngineArgs a{};
        a.layers = e->d_layers; a.n_layers = (int)e->oar.size();
        a.kvcache = reinterpret_cast<bf16_t*>(v.kvcache); a.kv_layer_stride = e->kv_layer_stride; a.kv_scene_stride = e->kv_scene_stride; a.Lmax = e->Lmax;
        a.xdec = v.xdec; a.st = v.d_state; a.gx = e->eng_gx; a.gloc = e->eng_gloc; a.ticket = e->eng_ticket; a.err = e->eng_err;
        a.B = B; a.NG = es->NG;
        a.R = es->NG;
        for (int r = 1; r <= es->NG; ++r)
            if (es->NG % r == 0 && r >= std::min(B, es->NG)) { a.R = r; break; }
        if (const char* dd = getenv("UMGEN_DEBUG_ENGINE_D")) {   // debugging: fewer groups per scene than the batch size asks for
            const int want = atoi(dd);
            if (want >= 1 && es->NG % want == 0 && es->NG / want >= std::min(B, es->NG)) a.R = es->NG / want;
        }
        a.D = es->NG / a.R;
        if (e->bg_engine && B == 1 && es->NG == 8 && !e->eng_stamps) {      // one scene on 4 XCD groups, the other 4 XCDs' workgroups are background workers (bg_worker.h)
            a.R = 2; a.D = 4;
            a.bg = e->d_bgq;
        }
        memcpy(a.xcc_group, es->map, 16);
        if (const char* bs = getenv("UMGEN_DEBUG_BURN")) {      // measurement builds (-DUMGEN_ENG_BURN): "us,mfma,sleep,kb"
            int us = 0, mf = 0, sl = 0, kb = 0;
            if (sscanf(bs, "%d,%d,%d,%d", &us, &mf, &sl, &kb) >= 1) {
                a.burn_ticks = us * 100; a.burn_mfma = mf; a.burn_sleep = sl; a.burn_kb = e->burn_buf ? kb : 0; a.burn_buf = e->burn_buf;
            }
        }
        a.stamps = e->eng_stamps;
        a.fp16 = std::is_same<T, f16_t>::value ? 1 : 0;
        // More than 4 scenes: the systolic schedule (oar_engine.hip) -- the scenes flow through the 8 groups, group g working on layers
        // g, g + 8, ...; up to 4 scenes keep disjoint group sets per scene (8 / 4 / 2 groups each), whose per-scene latency is lower.
        // Measured (profiles/r03_systolic.txt): 5 scenes 704 vs 1014 us per step, 8 scenes 1034 vs 1037 us (the register file cannot
        // keep a layer resident, so every item still streams 11 of its 14 MB).  UMGEN_ENGINE_SYSTOLIC=0/1 forces either form.
        static const char* sys_env = getenv("UMGEN_ENGINE_SYSTOLIC");
        a.systolic = sys_env ? (sys_env[0] == '1' && B > 1) : (B > 4);
        if (a.systolic && B > kEngMaxSystolic) a.systolic = 0;
        // hand-off tags of one step: (round or scene, layer, edge) must fit kEpochPerStep (umgen_create bounds n_oar_layer and max_batch)
        const int slots = a.systolic ? B : (B + a.R - 1) / a.R;
        if ((unsigned)(slots * 64 * 8) > kEpochPerStep) return e->fail(UMGEN_E_UNSUPPORTED, "decode engine: %d scenes need more hand-off tags than one step has", B);
        HIPCHK(e, launch_oar_engine(v.stream, a));
        return 0;
    }
    for (size_t li = 0; li < e->oar.size(); ++li) {
        const SubW& w = e->oar[e->dbg_same_layer ? 0 : li];
        DecodeLayerArgs d{};
        d.ln_a = w.ln_a; d.Wqkv = w.attn.Wqkv; d.bqkv = w.attn.bqkv; d.Wo = w.attn.Wo; d.bo = w.attn.bo; d.ln_b = w.ln_b; d.Wfc = w.mlp.Wfc;
        d.Wproj = w.mlp.Wproj; d.x = v.xdec; d.q = v.qdec; d.h = e->hdec; d.part = e->part;
        d.cache = reinterpret_cast<T*>(v.kvcache) + (long)li * e->kv_layer_stride; d.scene_stride = e->kv_scene_stride; d.Lmax = e->Lmax;
        d.d_len = d_len; d.B = B; d.E = E; d.H = H; d.ns = ns; d.rows_per_block = rows_per_block_for(e, B);
        launch_decode_layer<T>(v.stream, d);
    }
    return 0;
}

// kernels of one decode step of kind mod (0 fixed token, 1 map, 2 bbox3d, 3 image) for B scenes
template <typename T>
int enqueue_step(umgen_engine* e, const DecView& v, int B, int mod, int ns, const umgen_trace* tr, int j) {
    const int E = e->E;
    hipStream_t st = v.stream;
    const DecodePath path = decode_path(e, B, st, v.lane);
    const bool time_layers = e->profiling && !v.capture && !v.lane;
    if (time_layers) {
        if (e->layer_ev_used == e->layer_ev.size()) {
            hipEvent_t a0, a1;
            hipEventCreate(&a0);
            hipEventCreate(&a1);
            e->layer_ev.emplace_back(a0, a1);
        }
        hipEventRecord(e->layer_ev[e->layer_ev_used].first, st);
    }
    if (int rc = oar_layers<T>(e, v, B, ns, path)) return rc;
    if (time_layers) hipEventRecord(e->layer_ev[e->layer_ev_used++].second, st);
    static FILE* dump = getenv("UMGEN_DEBUG_DUMP_X") ? fopen(getenv("UMGEN_DEBUG_DUMP_X"), "wb") : nullptr;   // debugging only (eager launches)
    if (dump && tr == nullptr && !e->cfg.use_graphs) {
        std::vector<float> hx((size_t)E);
        hipMemcpyAsync(hx.data(), v.xdec, (size_t)E * 4, hipMemcpyDeviceToHost, st);
        hipStreamSynchronize(st);
        fwrite(hx.data(), 4, E, dump);
        fflush(dump);
    }
    SampleArgs sa{};
    sa.st = v.d_state; sa.tb = e->tb; sa.logits = v.logits; sa.logits_tar = v.logits_tar; sa.ld_logits = 8192; sa.ld_tar = e->cfg.bbox3d_vocab;
    sa.cond = v.cond; sa.x_next = v.xdec; sa.tokens = v.d_tokens; sa.prev_box = v.d_prev_box; sa.control_slot = v.d_control;
    sa.boxes = v.d_boxes; sa.n_boxes = v.d_nboxes; sa.seeds = v.d_seeds; sa.forced = e->d_forced; sa.counters = e->d_counters;
    sa.side = v.d_side;      // (always set: what a step writes of it are the device-side switches of OarState, so one captured graph serves every kind of call)
    sa.plan = v.d_plan;      // (likewise: OarState::plan)
    if (mod == 0) {
        launch_fixed_token(st, sa, B);
    } else {
        const void* head = mod == 1 ? e->head_ar_map : (mod == 2 ? e->head_ar_box : e->head_ar_img);
        const int V = mod == 1 ? e->cfg.map_vocab : (mod == 2 ? e->cfg.bbox3d_vocab : e->cfg.img_vocab);
        bool head_done = false;
        if constexpr (sizeof(T) == 2) {
            if (path == PATH_BATCHED) {
                RowsArgs r{};
                r.x = v.xfrag; r.M = B; r.ln_w = e->ln_oar; r.W = head; r.N = V; r.K = E; r.mode = ROWS_F32; r.out = v.logits; r.ldo = sa.ld_logits; r.E = E;   // (xfrag: the last layer's copy of x)
                launch_rows_mfma<T>(v.stream, r);
                head_done = true;
            }
        }
        if (!head_done) gemv_any(e, Place{st, &e->w_main, v.capture}, v.xdec, E, e->ln_oar, head, nullptr, V, E, B, GEMV_OUT_F32, v.logits, sa.ld_logits);
        // (head_tar_bbox3d on the conditioning rows, UMGen.py:1087,1103: the rows do not depend on the decoded tokens, so all 660
        //  positions were multiplied once before the loop -- tar_head_logits -- instead of one GEMV launch per bbox3d step)
        if (tr) {
            float* dst = mod == 1 ? tr->logits_map : (mod == 2 ? tr->logits_bbox3d : tr->logits_image);
            const int k = mod == 1 ? j - kMapC0 : (mod == 2 ? j - kBoxC0 : j - kImgC0);
            if (dst) HIPCHK(e, hipMemcpyAsync(dst + (size_t)k * V, v.logits, (size_t)V * 4, hipMemcpyDeviceToHost, st));
        }
        sa.mod = mod;
        sa.vocab = V;
        launch_sample_token(st, sa, B);
    }
    return 0;
}

}  // namespace

namespace umgen {

DecodePath decode_path(const umgen_engine* e, int B, hipStream_t st, bool lane) {
    if (e->tsz != 2) return PATH_LAUNCHES;      // fp32: five launches per layer
    if (e->use_batched(B, lane)) return PATH_BATCHED;
    if (e->use_wide(B)) return PATH_WIDE;
    return e->eng_for(st) ? PATH_ENGINE : PATH_LAUNCHES;
}

DecView lane_view(const umgen_engine* e, const umgen_engine::DecLane& ln, int b0) {
    const long E = e->E;
    DecView v = e->dv;      // (only what a lane offsets or replaces is named below)
    v.stream = ln.s; v.lane = true; v.d_state = ln.st; v.xfrag = ln.xfrag; v.afrag = ln.afrag; v.hfrag = ln.hfrag;
    v.xdec += b0 * E; v.qdec += b0 * E; v.logits += (long)b0 * 8192;
    v.logits_tar += (long)b0 * kNBox * e->cfg.bbox3d_vocab; v.cond += (long)b0 * kSeq * E;
    v.kvcache = static_cast<unsigned char*>(v.kvcache) + (size_t)b0 * e->kv_scene_stride * e->tsz;
    v.d_tokens += (long)b0 * kTokPerFrame; v.d_prev_box += (long)b0 * kNBox; v.d_nboxes += b0;
    v.d_control += (long)b0 * kSlots; v.d_boxes += (long)b0 * 64 * 10; v.d_seeds += b0;
    v.d_side = side_at(v.d_side, b0);
    v.d_plan = plan_at(v.d_plan, b0);
    return v;
}

int launch_bg_drain(umgen_engine* e, hipStream_t st) {
    OarEngineArgs a{};
    a.NG = 8; a.R = 2; a.D = 4; a.B = 1; a.bg = e->d_bgq; a.bg_only = 1;
    a.st = e->dv.d_state; a.ticket = e->eng_ticket; a.err = e->eng_err;
    memcpy(a.xcc_group, e->eng_fg.map, 16);
    a.fp16 = e->cfg.precision == UMGEN_PREC_FP16 ? 1 : 0;
    HIPCHK(e, launch_oar_engine(st, a));
    return 0;
}

int enqueue_step_any(umgen_engine* e, const DecView& v, int B, int mod, int ns, const umgen_trace* tr, int j) {
    return with_precision(e, [&](auto t) { return enqueue_step<decltype(t)>(e, v, B, mod, ns, tr, j); });
}

}  // namespace umgen

extern "C" {

// Test hook: ONE decode step through the BlockOAR layers (no head, no sampler) on caller-provided inputs, either as the five-launch
// layer form (use_engine 0), the XCD-resident engine (1), the batched decode layer (2) or the chip-wide engine (3).  The K/V rows of position L are
// appended to the cache: a test drives L = 0, 1, 2, ... or sets the history with umgen_dbg_oar_cache.  A path that oar_layers would not take for this
// B is refused: 2 runs exactly when decode_path gives the batched layer on this handle, 0 / 1 / 3 exactly when it does not.
// x_frag (umgen_dbg_oar_step_frag; use_engine 2 only): the fragment-major copy of x behind the step -- dv.xfrag, the buffer the head's launch
// would stream (enqueue_step) -- downloaded as it is and put into rows [B][E] on the host with frag_index.
static int oar_step_hook(umgen_engine* e, int32_t B, int32_t L, const float* x_in, float* x_out, float* x_frag, int32_t use_engine, int32_t unmasked) {
    if (!e || !x_in || !x_out) return UMGEN_E_INVALID;
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_finalize_weights has not been called");
    if (e->cfg.precision == UMGEN_PREC_FP32) return e->fail(UMGEN_E_UNSUPPORTED, "16-bit engines only");
    if (B < 1 || B > e->cfg.max_batch || L < 0 || L >= e->Lmax) return e->fail(UMGEN_E_INVALID, "B=%d L=%d", B, L);
    if (use_engine < 0 || use_engine > 3)
        return e->fail(UMGEN_E_INVALID, "use_engine %d (0: five launches per layer, 1: XCD-resident engine, 2: batched decode layer, 3: chip-wide engine)", use_engine);
    if (x_frag && use_engine != 2) return e->fail(UMGEN_E_INVALID, "only the batched decode layer (use_engine 2) keeps a fragment-major copy of x");
    if (use_engine == 1 && !e->eng_enabled) return e->fail(UMGEN_E_UNSUPPORTED, "decode engine not available on this engine");
    if (use_engine == 3 && !e->wide_enabled) return e->fail(UMGEN_E_UNSUPPORTED, "chip-wide decode engine not available on this engine");
    // the step runs on the path that was asked for or not at all: oar_layers decides by B, and a test must not measure another path's arithmetic
    hipStream_t const st = (unmasked && e->full_stream) ? e->full_stream : e->stream;
    const DecodePath own = decode_path(e, B, st, false);
    if (use_engine == 2 && own != PATH_BATCHED)
        return e->fail(UMGEN_E_UNSUPPORTED, "%d scenes do not take the batched decode layer on this engine (UMGEN_DECODE_BATCHED)", B);
    if (use_engine != 2 && own == PATH_BATCHED)
        return e->fail(UMGEN_E_UNSUPPORTED, "%d scenes take the batched decode layer on this engine (UMGEN_DECODE_BATCHED), not %s", B,
                       use_engine == 0 ? "five launches per layer" : "a decode engine");
    if (use_engine == 3 && own != PATH_WIDE) return e->fail(UMGEN_E_UNSUPPORTED, "the chip-wide decode engine takes at most 4 scenes per call, not %d", B);
    if (use_engine == 1 && !e->eng_for(st)) return e->fail(UMGEN_E_UNSUPPORTED, "the XCD-resident decode engine has no census for this stream");
    if (e->eng_epoch > 0xE0000000u) {   // same wrap rule as run_frame, for both engines' granule buffers
        HIPCHK(e, hipDeviceSynchronize());
        if (e->eng_enabled) {
            HIPCHK(e, hipMemset(e->eng_gx, 0, (size_t)e->cfg.max_batch * kEngE * 8));
            HIPCHK(e, hipMemset(e->eng_gloc, 0, e->eng_gloc_bytes));
        }
        if (e->wide_enabled) HIPCHK(e, hipMemset(e->wide_gran, 0, oar_engine_wide_granules() * 8));
        e->eng_epoch = 16u;
    }
    const unsigned epoch = e->eng_epoch;   // tags never repeat across calls
    e->eng_epoch += kEpochPerStep;
    DecView v = e->dv;      // the whole batch's buffers on the stream that was asked for
    v.stream = st;
    OarState s0{L, 0, 0, 0, 0, epoch, SamplerParams{}};
    HIPCHK(e, hipMemcpyAsync(v.d_state, &s0, sizeof(s0), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(v.xdec, x_in, (size_t)B * e->E * 4, hipMemcpyHostToDevice, st));
    const DecodePath path = (DecodePath)use_engine;      // (the refusals above: a path this handle and B can take)
    const int lrc = e->cfg.precision == UMGEN_PREC_FP16 ? oar_layers<f16_t>(e, v, B, attn_nsplit(L + 1), path) : oar_layers<bf16_t>(e, v, B, attn_nsplit(L + 1), path);
    if (lrc) return lrc;
    HIPCHK(e, hipMemcpyAsync(x_out, v.xdec, (size_t)B * e->E * 4, hipMemcpyDeviceToHost, st));
    std::vector<float> hfrag(x_frag ? (size_t)kRowsMaxM * e->E : 0);
    if (x_frag) HIPCHK(e, hipMemcpyAsync(hfrag.data(), v.xfrag, hfrag.size() * 4, hipMemcpyDeviceToHost, st));
    unsigned eng_err = 0;
    if (use_engine == 1 || use_engine == 3)
        HIPCHK(e, hipMemcpyAsync(&eng_err, use_engine == 3 ? e->wide_err : e->eng_err, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    if (x_frag)
        for (int m = 0; m < B; ++m)
            for (int k = 0; k < e->E; ++k) x_frag[(size_t)m * e->E + k] = hfrag[frag_index(m, k)];
    if (eng_err) {      // clear the word of the engine that ran (the other engine's may not exist: ADVICE r5)
        (void)hipMemset(use_engine == 3 ? e->wide_err : e->eng_err, 0, sizeof(unsigned));
        return e->fail(UMGEN_E_HIP, "decode engine gave up waiting for hand-off tag 0x%08x", eng_err);
    }
    return UMGEN_OK;
}

int umgen_dbg_oar_step(umgen_engine* e, int32_t B, int32_t L, const float* x_in, float* x_out, int32_t use_engine, int32_t unmasked) {
    return oar_step_hook(e, B, L, x_in, x_out, nullptr, use_engine, unmasked);
}

// the same step with the second output x_frag [B][E] (may be null)
int umgen_dbg_oar_step_frag(umgen_engine* e, int32_t B, int32_t L, const float* x_in, float* x_out, float* x_frag, int32_t use_engine, int32_t unmasked) {
    return oar_step_hook(e, B, L, x_in, x_out, x_frag, use_engine, unmasked);
}

// Test hook: rows [row0, row0 + n_rows) of every (K / V, head) of one (layer, scene) block of the decode K/V cache, device [layer][scene][2][H][Lmax][48],
// to (upload 0) or from (upload 1) host [2][H][n_rows][48] in the cache type's bits.  16-bit engines only.
int umgen_dbg_oar_cache(umgen_engine* e, int32_t layer, int32_t scene, int32_t row0, int32_t n_rows, void* host, int32_t upload) {
    if (!e || !host) return UMGEN_E_INVALID;
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_finalize_weights has not been called");
    if (e->cfg.precision == UMGEN_PREC_FP32) return e->fail(UMGEN_E_UNSUPPORTED, "16-bit engines only");
    if (layer < 0 || layer >= (int)e->oar.size() || scene < 0 || scene >= e->cfg.max_batch || row0 < 0 || n_rows < 1 || (long)row0 + n_rows > e->Lmax)
        return e->fail(UMGEN_E_INVALID, "layer=%d scene=%d rows [%d, %d + %d) of %d", layer, scene, row0, row0, n_rows, e->Lmax);
    unsigned char* dev = static_cast<unsigned char*>(e->dv.kvcache) + ((size_t)layer * e->kv_layer_stride + (size_t)scene * e->kv_scene_stride + (size_t)row0 * kHeadDim) * e->tsz;
    const size_t dpitch = (size_t)e->Lmax * kHeadDim * e->tsz, width = (size_t)n_rows * kHeadDim * e->tsz, height = (size_t)2 * e->H;
    if (upload) HIPCHK(e, hipMemcpy2DAsync(dev, dpitch, host, width, width, height, hipMemcpyHostToDevice, e->stream));
    else HIPCHK(e, hipMemcpy2DAsync(host, width, dev, dpitch, width, height, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return UMGEN_OK;
}

// Test hook: moves the hand-off tag epoch of the decode engines FORWARD (towards the wrap that run_frame and umgen_dbg_oar_step handle).  Backwards is
// refused: tags below the current epoch may still lie in the granule buffers, which only the wrap clears.
int umgen_dbg_oar_epoch(umgen_engine* e, uint32_t epoch) {
    if (!e) return UMGEN_E_INVALID;
    if (epoch < e->eng_epoch) return e->fail(UMGEN_E_INVALID, "epoch 0x%08x is below the current 0x%08x", epoch, e->eng_epoch);
    e->eng_epoch = epoch;
    return UMGEN_OK;
}

}  // extern "C"
