// The templated compute path on whole windows: GEMM / attention launch helpers, the BlockTAR sub-block and the four stacks, the ego
// decoder, the given-token prefix as one pass, the recorder / launcher of the next frame's background pass (its known slots one gather_windows of
// the frame's TokenView, token_windows.h, kept in px.win and staged in px_up), and the GMLP tables.
// Other files enter through the *_any dispatchers at the end.
#include "engine_frame.h"      // (upload_tokens)

// host arithmetic stays unfused in every engine file, as it was while they were one file behind the numpy-faithful helpers (engine_weights.hip)
#pragma clang fp contract(off)

namespace {

// ---- templated compute path ---------------------------------------------------------------------------------
template <typename T> struct Path;
template <> struct Path<float> {
    static void gemm(hipStream_t s, const GemmArgs& a) { launch_gemm_valu<float, float>(s, a); }
    static void attn_spatial(hipStream_t s, const float* qk, const float* vt, float* y, int F, int S, int Sp, int H) {
        launch_attn_spatial_f32_mfma(s, qk, vt, y, F, S, Sp, H);
    }
    static void attn_causal(hipStream_t s, const float* qk, const float* vt, float* y, int F, int S, int Sp, int H) {
        launch_attn_causal_f32(s, qk, vt, y, F, S, Sp, H);
    }
    static void gemm_w_f32act(hipStream_t s, const GemmArgs& a) { launch_gemm_valu<float, float>(s, a); }
};
template <typename TT> struct Path16 {   // bf16_t / f16_t: the same matrix-core kernels with the other operand type
    static void gemm(hipStream_t s, const GemmArgs& a) { launch_gemm_mfma<TT>(s, a); }
    static void attn_spatial(hipStream_t s, const TT* qk, const TT* vt, TT* y, int F, int S, int Sp, int H) {
        launch_attn_spatial_mfma<TT>(s, qk, vt, y, F, S, Sp, H);
    }
    static void attn_causal(hipStream_t s, const TT* qk, const TT* vt, TT* y, int F, int S, int Sp, int H) {
        launch_attn_causal_mfma<TT>(s, qk, vt, y, F, S, Sp, H);
    }
    static void gemm_w_f32act(hipStream_t s, const GemmArgs& a) { launch_gemm_valu<TT, float>(s, a); }
};
template <> struct Path<bf16_t> : Path16<bf16_t> {};
template <> struct Path<f16_t> : Path16<f16_t> {};

template <typename T>
void gemm_timed(umgen_engine* e, const Place& pl, const GemmArgs& a) {
    if (e->profiling) {
        if (e->gemm_ev_used == e->gemm_ev.size()) {
            hipEvent_t a0, a1;
            hipEventCreate(&a0);
            hipEventCreate(&a1);
            e->gemm_ev.emplace_back(a0, a1);
        }
        auto& pr = e->gemm_ev[e->gemm_ev_used++];
        hipEventRecord(pr.first, pl.stream);
        Path<T>::gemm(pl.stream, a);
        hipEventRecord(pr.second, pl.stream);
        e->gemm_flops_pending += 2.0 * (double)a.Mi * (double)a.Nj * (double)a.K * (double)a.batch;
    } else {
        Path<T>::gemm(pl.stream, a);
    }
    // a refused launch (e.g. a dynamic-LDS attribute missing on this device) would leave stale workspace data behind: never silently
    if (!pl.capture) { const hipError_t le = hipGetLastError(); if (le != hipSuccess && e->launch_status == hipSuccess) e->launch_status = le; }
}

// out[tokens R][N] (T) = A[R][K] . W[N][K]^T + bias  (optionally GELU)
template <typename T>
void linear_store(umgen_engine* e, const Place& pl, const void* W, const float* bias, int N, int K, const void* A, long R, void* out, long ldo, int gelu) {
    GemmArgs g{};
    g.P = W; g.Q = A; g.Mi = N; g.Nj = (int)R; g.K = K; g.ldp = K; g.ldq = K; g.batch = 1;
    g.mode = GEMM_STORE; g.bias = bias; g.gelu = gelu; g.out = out; g.ldo = ldo;
    gemm_timed<T>(e, pl, g);
}
// X[R][N] (fp32) += A[R][K] . W[N][K]^T + bias
template <typename T>
void linear_resid(umgen_engine* e, const Place& pl, const void* W, const float* bias, int N, int K, const void* A, long R, float* X) {
    GemmArgs g{};
    g.P = W; g.Q = A; g.Mi = N; g.Nj = (int)R; g.K = K; g.ldp = K; g.ldq = K; g.batch = 1;
    g.mode = GEMM_RESID; g.bias = bias; g.out = X; g.ldo = N;
    gemm_timed<T>(e, pl, g);
}

// one (LayerNorm -> attention -> residual -> LayerNorm -> MLP -> residual) sub-block of BlockTAR (module.py:332-359)
//
// `tail`: the reference consumes only the LAST frame of every stack's output (UMGen.py:1227-1231 takes
// [:, -1] of each TAR output, 1002 of the ego stack), the spatial attention / LayerNorm / MLPs are frame-local and the temporal
// attention is causal (module.py:332-359) -- so in a stack's FINAL block everything behind the temporal attention's k | v rows is
// evaluated for the last frame only: identical outputs (per-row arithmetic does not depend on which other rows are in the launch).
//   tail 0: all rows;  tail 1 (temporal sub-block): LN + k|v of all rows, q / attention output / projection / MLP of the last frame;
//   tail 2 (the spatial sub-block behind it): the whole sub-block on the last frame's rows.
template <typename T>
void tar_sub(umgen_engine* e, const Place& pl, const SubW& w, int B, int Tn, int S, bool temporal, TemporalRange tr = TemporalRange{0, nullptr, 0, 0}, int tail = 0,
             int fan = 0, int fan_scenes = 0) {
    const int E = e->E, H = e->H;
    const long R = (long)B * Tn * S;
    T* A = reinterpret_cast<T*>(pl.work->A);
    T* QKV = reinterpret_cast<T*>(pl.work->QKV);
    T* Hb = reinterpret_cast<T*>(pl.work->Hb);
    const char* Wqkv = reinterpret_cast<const char*>(w.attn.Wqkv);
    const size_t wrow = (size_t)E * sizeof(T);                      // bytes of one weight row of c_attn
    // row ranges the "rest" of the sub-block (projection, MLP) runs on: everything, or the last frame of each scene
    struct Range { long row0, rows; };
    std::vector<Range> rest;
    if (tail == 0) rest.push_back(Range{0, R});
    else for (int b = 0; b < B; ++b) rest.push_back(Range{((long)b * Tn + (Tn - 1)) * S, (long)S});
    auto spatial_attention = [&](long frame0, int frames) {         // q | k row-major, V transposed per (frame, head) for the attention kernel
        const long r0 = frame0 * S;
        linear_store<T>(e, pl, Wqkv, w.attn.bqkv, 2 * E, E, A + r0 * E, (long)frames * S, QKV + r0 * 2 * E, 2L * E, 0);
        T* vt = reinterpret_cast<T*>(pl.work->VT) + frame0 * (long)E * e->S_pad;
        GemmArgs g{};
        g.P = A + r0 * E; g.Q = Wqkv + (size_t)2 * E * wrow;
        g.Mi = S; g.Nj = E; g.K = E; g.ldp = E; g.ldq = E; g.strideP = (long)S * E; g.strideQ = 0; g.batch = frames;
        g.mode = GEMM_VT; g.bias = w.attn.bqkv + 2 * E; g.out = vt; g.ldo = e->S_pad; g.H = H;
        gemm_timed<T>(e, pl, g);
        hipEvent_t t0 = nullptr, t1 = nullptr;
        if (e->profiling) {
            if (e->attn_ev_used == e->attn_ev.size()) {
                hipEvent_t a0, a1;
                hipEventCreate(&a0);
                hipEventCreate(&a1);
                e->attn_ev.emplace_back(a0, a1);
            }
            auto& pr = e->attn_ev[e->attn_ev_used++];
            t0 = pr.first; t1 = pr.second;
            hipEventRecord(t0, pl.stream);
            e->attn_flops_pending += 4.0 * (double)S * (double)S * kHeadDim * (double)H * (double)frames;
        }
        Path<T>::attn_spatial(pl.stream, QKV + r0 * 2 * E, vt, A + r0 * E, frames, S, e->S_pad, H);
        if (t1) hipEventRecord(t1, pl.stream);
    };
    if (temporal) {
        launch_layernorm<T>(pl.stream, pl.work->X, E, R, E, w.ln_a, A);
        if (tail == 0) {
            linear_store<T>(e, pl, Wqkv, w.attn.bqkv, 3 * E, E, A, R, QKV, 3L * E, 0);
        } else {   // k | v rows of every frame, q rows of the last frame only (the same [R][3E] row layout)
            linear_store<T>(e, pl, Wqkv + (size_t)E * wrow, w.attn.bqkv + E, 2 * E, E, A, R, QKV + E, 3L * E, 0);
            for (const Range& r : rest) linear_store<T>(e, pl, Wqkv, w.attn.bqkv, E, E, A + r.row0 * E, r.rows, QKV + r.row0 * 3 * E, 3L * E, 0);
            tr.q0 = tr.t0 + Tn - 1;
        }
        // fan: the B rows-of-one-slot are items that share their scenes' cached slots [0, tr.t0) (CACHE_SHARED_ITEMS); 2: item i also leaves its own
        // k | v rows in block i, slot tr.t0 (CACHE_SHARED_ITEMS_APPEND); 3: the items bring Tn slots [tr.t0, tr.t0 + Tn) each (CACHE_SHARED_ITEMS_TAIL; the
        // caller has asked attn_temporal_fan_tail_heads, so a refusal here is a refused launch like any other)
        if (fan == 2) launch_attn_temporal_fan_write<T>(pl.stream, QKV, A, B, e->d_item_scene, fan_scenes, S, H, tr.t0, reinterpret_cast<T*>(tr.cache), tr.Tcap);
        else if (fan == 3) {
            if (launch_attn_temporal_fan_tail<T>(pl.stream, QKV, A, B, Tn, e->d_item_scene, fan_scenes, S, H, tr.t0, tr.q0, reinterpret_cast<const T*>(tr.cache), tr.Tcap) &&
                e->launch_status == hipSuccess)
                e->launch_status = hipErrorInvalidConfiguration;
        } else if (fan) launch_attn_temporal_fan<T>(pl.stream, QKV, A, B, e->d_item_scene, fan_scenes, S, H, tr.t0, reinterpret_cast<const T*>(tr.cache), tr.Tcap);
        else launch_attn_temporal<T>(pl.stream, QKV, A, B, Tn, S, H, tr);
    } else if (tail == 0) {
        launch_layernorm<T>(pl.stream, pl.work->X, E, R, E, w.ln_a, A);
        spatial_attention(0, B * Tn);
    } else {
        for (const Range& r : rest) {
            launch_layernorm<T>(pl.stream, pl.work->X + r.row0 * E, E, r.rows, E, w.ln_a, A + r.row0 * E);
            spatial_attention(r.row0 / S, 1);
        }
    }
    for (const Range& r : rest) {
        float* X = pl.work->X + r.row0 * E;
        linear_resid<T>(e, pl, w.attn.Wo, w.attn.bo, E, E, A + r.row0 * E, r.rows, X);
        launch_layernorm<T>(pl.stream, X, E, r.rows, E, w.ln_b, A + r.row0 * E);
        linear_store<T>(e, pl, w.mlp.Wfc, nullptr, 4 * E, E, A + r.row0 * E, r.rows, Hb + r.row0 * 4 * E, 4L * E, 1);
        linear_resid<T>(e, pl, w.mlp.Wproj, nullptr, E, 4 * E, Hb + r.row0 * 4 * E, r.rows, X);
    }
}

// cache_mode: enum CacheMode (engine_state.h).
// fan_scenes (the CACHE_SHARED_ITEMS modes): the scenes whose slot caches the w.B items share, item i those of scene e->d_item_scene[i].
// tail: TAIL_AUTO = the final block's last-frame shortcut wherever it applies (below); TAIL_NONE = every block on every slot (umgen_score_clip reads all of
// them).  warped_all (STACK_MAP, or nullptr): [w.B][w.T][1024][E], the warped map of every slot beside warped_last.
template <typename T>
void run_stack(umgen_engine* e, const Place& pl, int stack, const WindowTokens& w, CacheMode cache_mode, int tail = TAIL_AUTO, float* warped_all = nullptr,
               int fan_scenes = 0) {
    const int S = stack_len(stack);
    launch_embed_stack(pl.stream, stack, e->tb, w, pl.work->X, pl.work->mapfeat);
    if (stack != STACK_EGO) launch_warp_map(pl.stream, stack, e->tb, w.B, w.T, pl.work->mapfeat, e->pose_diff, pl.work->X,
                                            stack == STACK_MAP ? e->warped_last : nullptr, w.Tfull, w.t0, stack == STACK_MAP ? warped_all : nullptr);
    static const bool no_tail = getenv("UMGEN_NO_TAIL") != nullptr;   // measurement: evaluate every block on every frame like the reference
    for (size_t i = 0; i < e->stk[stack].size(); ++i) {
        const TarW& blk = e->stk[stack][i];
        TemporalRange tr{w.t0, cache_mode != CACHE_NONE ? e->tcache[stack][i] : nullptr, e->cfg.max_cond_frames, cache_writes(cache_mode) ? 1 : 0};
        // the final block's tail on the last frame only (f-3): whole-window passes with more than one slot (the temporal sub-block still
        // evaluates the k | v rows of every slot, so a pass that fills the slot caches keeps the shortcut)
        const bool last = i + 1 == e->stk[stack].size() && cache_last_frame_shortcut(cache_mode) && w.T > 1 && !no_tail && tail == TAIL_AUTO;
        tar_sub<T>(e, pl, blk.sub[0], w.B, w.T, S, false);
        tar_sub<T>(e, pl, blk.sub[1], w.B, w.T, S, true, tr, last ? 1 : 0, cache_fan_form(cache_mode), fan_scenes);
        tar_sub<T>(e, pl, blk.sub[2], w.B, w.T, S, false, TemporalRange{0, nullptr, 0, 0}, last ? 2 : 0);
    }
}

// GemvArgs helpers
template <typename T>
void gemv(umgen_engine* e, const Place& pl, const float* x, long ldx, const float* ln_w, const void* W, const float* bias, int N, int K, int M,
          int mode, float* out, long ldo) {
    GemvArgs a{};
    a.rows_per_block = rows_per_block_for(e, M);
    a.x = x; a.ldx = ldx; a.ln_w = ln_w; a.W = W; a.bias = bias; a.N = N; a.K = K; a.M = M; a.out_mode = mode; a.out = out; a.ldo = ldo;
    a.E = e->E;
    launch_gemv<T>(pl.stream, a);
}
template <typename T>
void gemv_resid(umgen_engine* e, const Place& pl, const float* a_in, long lda, const float* part, const void* W, const float* bias, int N, int K, int M,
                float* x, long ldx, int ns = 1) {
    GemvResidArgs a{};
    a.rows_per_block = rows_per_block_for(e, M);
    a.a = a_in; a.lda = lda; a.part = part; a.H = e->H; a.ns = ns; a.W = W; a.bias = bias; a.N = N; a.K = K; a.M = M; a.x = x; a.ldx = ldx;
    launch_gemv_resid<T>(pl.stream, a);
}

// The ego decoder (Decoder.forward_func, module.py:662-683) and head_ego on n items (n <= max_batch): item i reads the frame whose 2207 rows start at row
// frame_of[i] * 2207 of X (the ego stack's output) and takes the ego queries of window length Tq -- or of its own, d_item_T[i] (device, [n]), when given.
// -> e->dv.logits [3 n][pose_vocab]
template <typename T>
void ego_decoder(umgen_engine* e, const Place& pl, int n, const long* frame_of, int Tq, const int* d_item_T) {
    const int E = e->E, H = e->H, B = n;
    // p = ln_ego_tar(x) of the item's frame, kept in fp32 (every decoder block re-normalises it with its own ln_3)
    for (int b = 0; b < B; ++b)
        launch_layernorm<float>(pl.stream, pl.work->X + (frame_of[b] * kSeq) * E, E, kSeq, E, e->ln_ego_tar,
                                e->pego + (long)b * kSeq * E);
    float* x = e->dv.xdec;   // [3B][E] ego queries
    launch_ego_queries(pl.stream, e->tb, B, Tq, x, d_item_T);
    const int M = 3 * B;
    T* PN = reinterpret_cast<T*>(pl.work->A);         // ln_3(p)           [B*2207][E]
    T* KV = reinterpret_cast<T*>(pl.work->QKV);       // k | v of ln_3(p)  [B*2207][2E]
    for (const DecW& d : e->dec) {               // Decoder.forward_func (module.py:662-683)
        gemv<T>(e, pl, x, E, d.ln1, d.self.Wqkv, d.self.bqkv, 3 * E, E, M, GEMV_OUT_F32, e->qkv3, 3L * E);
        // self-attention among the 3 ego queries of a scene (non-causal); q rows gathered out of the packed q|k|v rows
        hipMemcpy2DAsync(e->dv.qdec, (size_t)E * 4, e->qkv3, (size_t)3 * E * 4, (size_t)E * 4, M, hipMemcpyDeviceToDevice, pl.stream);
        launch_ego_self_attn(pl.stream, e->dv.qdec, e->qkv3, M, H, e->part);
        gemv_resid<T>(e, pl, nullptr, 0, e->part, d.self.Wo, d.self.bo, E, E, M, x, E, 1);
        // cross attention to the frame's 2207 scene tokens (FlashCrossAttention.forward, module.py:482-509)
        gemv<T>(e, pl, x, E, d.ln2, d.Wq, d.bq, E, E, M, GEMV_OUT_F32, e->dv.qdec, E);
        launch_layernorm<T>(pl.stream, e->pego, E, (long)B * kSeq, E, d.ln3, PN);
        linear_store<T>(e, pl, d.Wkv, d.bkv, 2 * E, E, PN, (long)B * kSeq, KV, 2L * E, 0);
        launch_ego_cross_attn<T>(pl.stream, e->dv.qdec, KV, M, H, e->part);
        gemv_resid<T>(e, pl, nullptr, 0, e->part, d.Wco, d.bco, E, E, M, x, E, ego_cross_nsplit());
        gemv<T>(e, pl, x, E, d.ln4, d.mlp.Wfc, nullptr, 4 * E, E, M, GEMV_OUT_GELU, e->hdec, 4L * E);
        gemv_resid<T>(e, pl, e->hdec, 4L * E, nullptr, d.mlp.Wproj, nullptr, E, 4 * E, M, x, E);
    }
    gemv<T>(e, pl, x, E, e->ln_ego, e->head_ego, nullptr, e->cfg.pose_vocab, E, M, GEMV_OUT_F32, e->dv.logits, e->cfg.pose_vocab);
}

// infer_ego_net / forward_ego_net (UMGen.py:994-1005, 634-687).  The Decoder is frame-local and only t = -1 is consumed
// (UMGen.py:1002), so the 12 decoder blocks run on the last frame only -- identical outputs, 1/T of the work.
template <typename T>
void run_ego(umgen_engine* e, const Place& pl, const WindowTokens& w, const SamplerParams& sp, int frame_idx, bool forced, float* trace_logits,
             CacheMode cache_mode, const EgoSide& es) {
    const int B = w.B, Tn = w.T;   // Tn: slots in this pass (the last one is the window's last frame)
    run_stack<T>(e, pl, STACK_EGO, w, cache_mode);
    std::vector<long> last(B);
    for (int b = 0; b < B; ++b) last[b] = (long)b * Tn + (Tn - 1);
    ego_decoder<T>(e, pl, B, last.data(), w.Tfull ? w.Tfull : Tn, nullptr);
    if (trace_logits) hipMemcpyAsync(trace_logits, e->dv.logits, (size_t)3 * e->cfg.pose_vocab * 4, hipMemcpyDeviceToHost, pl.stream);
    launch_sample_ego(pl.stream, e->dv.logits, e->cfg.pose_vocab, sp, e->dv.d_seeds, frame_idx, forced ? e->d_forced : nullptr, e->d_ego_tok, B,
                      e->d_counters + 7, es);
}

// run_ego for the fan frame of umgen_rollout_fan: the ego stack and decoder once per scene (the w.B scenes' whole windows), then every branch (b, s) -- item
// b*N + s of e->dv.d_seeds / e->d_ego_tok / logp -- draws its own pose from its scene's three head_ego rows with its own seed.  The rows are copied to the items'
// places in e->dv.logits scene by scene in DESCENDING b: scene b's rows lie where item b's go, and every destination of scene b is >= b*N, above every lower scene
// whose rows are still unread (b == 0, s == 0 is the self-copy that is skipped).  The sampler and its logp then read the rows the replicated call's would.
template <typename T>
void run_ego_fan(umgen_engine* e, const Place& pl, const WindowTokens& w, int N, const SamplerParams& sp, int frame_idx, CacheMode cache_mode, const EgoSide& es) {
    const int B = w.B, Tn = w.T;
    run_stack<T>(e, pl, STACK_EGO, w, cache_mode);
    std::vector<long> last(B);
    for (int b = 0; b < B; ++b) last[b] = (long)b * Tn + (Tn - 1);
    ego_decoder<T>(e, pl, B, last.data(), w.Tfull ? w.Tfull : Tn, nullptr);
    const size_t row3 = (size_t)3 * e->cfg.pose_vocab;
    for (int b = B - 1; b >= 0; --b)
        for (int s = N - 1; s >= 0; --s)
            if (b * N + s != b)
                hipMemcpyAsync(e->dv.logits + (size_t)(b * N + s) * row3, e->dv.logits + (size_t)b * row3, row3 * sizeof(float), hipMemcpyDeviceToDevice, pl.stream);
    launch_sample_ego(pl.stream, e->dv.logits, e->cfg.pose_vocab, sp, e->dv.d_seeds, frame_idx, nullptr, e->d_ego_tok, B * N, e->d_counters + 7, es);
}

// The GIVEN-token prefix of a frame as ONE forward pass (infer_oar_net's first iteration pushes the whole predefined prefix through the 36
// layers, UMGen.py:1184-1201, 1234-1237; rounds 1-4 replayed it as up to 1693 single decode steps, ~0.46 s per frame for a given map).
// Positions 0 .. P - 2 of every scene are the rows of the TAR stacks' own kernels -- LayerNorm, q|k and V^T GEMMs, S x S attention with the
// causal mask, projection + MLP with the residual epilogues -- in the stacks' workspaces (idle while the decode runs); every layer leaves its
// k | v rows in the decode cache.  Position P - 1 stays a decode step: its input goes to xdec and the step loop starts there.
// Arithmetic: the stacks' contract (16-bit GEMM operands in the 16-bit modes, exact fp32 chains in fp32 mode) instead of the decode
// step's fp32 activations -- the reference computes the prefix in one fp16-autocast pass as well.
// src (umgen_score_clip; nullptr: the engine's own buffers): conditioning rows [B][2207][E], tokens [B][2199] and a [B][E] row buffer for position P - 1 that
// may hold more than max_batch scenes (B <= max_batch * max_cond_frames: what the stacks' workspaces hold), and whether the decode cache, which holds
// max_batch scenes, is left alone
template <typename T>
int run_prefix_prefill(umgen_engine* e, const Place& pl, int B, int P, const PrefillSrc* src = nullptr) {
    const int E = e->E, H = e->H, S = P - 1;
    if (S < 1 || S > e->S_pad) return e->fail(UMGEN_E_INVALID, "prefix pass over %d positions", S);
    hipStream_t st = pl.stream;
    const long R = (long)B * S;
    T* A = reinterpret_cast<T*>(pl.work->A);
    T* QKV = reinterpret_cast<T*>(pl.work->QKV);
    T* Hb = reinterpret_cast<T*>(pl.work->Hb);
    T* vt = reinterpret_cast<T*>(pl.work->VT);
    launch_prefix_rows(st, e->tb, e->tb.tske + (long)e->cfg.task_id * E, src ? src->cond : e->dv.cond, src ? src->tokens : e->dv.d_tokens, B, P, pl.work->X,
                       src ? src->x_last : e->dv.xdec);
    const size_t wrow = (size_t)E * sizeof(T);
    for (size_t li = 0; li < e->oar.size(); ++li) {
        const SubW& w = e->oar[li];
        const char* Wqkv = reinterpret_cast<const char*>(w.attn.Wqkv);
        launch_layernorm<T>(st, pl.work->X, E, R, E, w.ln_a, A);
        linear_store<T>(e, pl, Wqkv, w.attn.bqkv, 2 * E, E, A, R, QKV, 2L * E, 0);           // q | k rows
        GemmArgs g{};                                                                     // V^T per (scene, head): [B][H][48][S_pad]
        g.P = A; g.Q = Wqkv + (size_t)2 * E * wrow;
        g.Mi = S; g.Nj = E; g.K = E; g.ldp = E; g.ldq = E; g.strideP = (long)S * E; g.strideQ = 0; g.batch = B;
        g.mode = GEMM_VT; g.bias = w.attn.bqkv + 2 * E; g.out = vt; g.ldo = e->S_pad; g.H = H;
        gemm_timed<T>(e, pl, g);
        if (!src || !src->skip_cache)
            launch_prefix_kv_to_cache<T>(st, QKV, vt, B, S, e->S_pad, H, e->Lmax, reinterpret_cast<T*>(e->dv.kvcache) + (long)li * e->kv_layer_stride,
                                         e->kv_scene_stride);
        Path<T>::attn_causal(st, QKV, vt, A, B, S, e->S_pad, H);
        linear_resid<T>(e, pl, w.attn.Wo, w.attn.bo, E, E, A, R, pl.work->X);
        launch_layernorm<T>(st, pl.work->X, E, R, E, w.ln_b, A);
        linear_store<T>(e, pl, w.mlp.Wfc, nullptr, 4 * E, E, A, R, Hb, 4L * E, 1);
        linear_resid<T>(e, pl, w.mlp.Wproj, nullptr, E, 4 * E, Hb, R, pl.work->X);
    }
    return 0;
}

// Background pass for the NEXT frame of the rollout: its window is this window moved on by one frame, and all its slots but the
// last are known now (the new frame's pose tokens `ego` included).  They run through the four stacks on bg_stream while the
// decode loop of the current frame owns the other CUs; the temporal k | v rows of every layer land in the slot caches.
// pl: the frame's decode stream (the foreground) and the main workspaces, which the pass works in whichever stream it takes.
// dbg (the test hooks of debug_bg.hip; nullptr in the product): the very same pass either as stand-alone launches on pl.stream, synchronised
// (foreground), or recorded and uploaded with every op's chunk / the margin overridden; a pass the recorder refuses is then an error, not a frame on the plain path.
template <typename T>
int launch_prefix(umgen_engine* e, const Place& pl, const FrameIO& io, const std::vector<int>& ego, const BgPassDebug* dbg) {
    const int B = io.B, Tn = io.T;
    const int Tnext = std::min(Tn + 1, io.cond_cap);
    const int off = (Tn + 1 > io.cond_cap) ? 1 : 0;     // the window slides (UMGen.py:1600-1603) or still grows
    const int P = Tnext - 1;
    if (P < 1 || Tnext > e->cfg.max_cond_frames) return 0;
    umgen_engine::Prefix& px = e->px;
    px.valid = false;
    px.B = B; px.P = P; px.Tfull = Tnext; px.has_ego = !io.next_has_ctrl_pose;
    // the known slots [B][P][S_mod], kept for prefix_matches, and as the first P of Tnext slots in the upload: slot P is zero but for the new pose
    TokenSeqs& up = e->px_up;
    gather_windows(io.win, B, off, P, px.win);
    up.resize(B, Tnext);
    for (int m = 0; m < 4; ++m) {
        std::fill(up.mod[m].begin(), up.mod[m].end(), 0);
        for (int b = 0; b < B; ++b) memcpy(up.at(m, b, 0), px.win.at(m, b, 0), (size_t)P * kModLen[m] * sizeof(int));
    }
    px.pose_next.assign(ego.begin(), ego.end());
    for (int b = 0; b < B; ++b) memcpy(up.at(0, b, P), &ego[(size_t)b * 3], 3 * sizeof(int));
    std::vector<int> zero((size_t)B * 3, 0);
    decode_pose_shift(up.mod[0].data(), zero.data(), B, Tnext, e->px_pshift, e->px_pdiff);   // slot P (unknown) is not touched by this pass

    hipStream_t fg = pl.stream, bg = e->bg_engine ? fg : e->bg_stream;
    if (!e->bg_engine) {
        HIPCHK(e, hipEventRecord(e->ev_tar_done, fg));
        HIPCHK(e, hipStreamWaitEvent(bg, e->ev_tar_done, 0));
    }
    if (int rc = upload_tokens(e, bg, up.view(), (size_t)B * Tnext)) return rc;
    HIPCHK(e, hipMemcpyAsync(e->d_pose_shift, e->px_pshift.data(), e->px_pshift.size() * 4, hipMemcpyHostToDevice, bg));
    HIPCHK(e, hipMemcpyAsync(e->pose_diff, e->px_pdiff.data(), e->px_pdiff.size() * 4, hipMemcpyHostToDevice, bg));
    const WindowTokens ws{e->d_pose_shift, e->d_map, e->d_box, e->d_img, B, P, Tnext, 0};
    // on bg in the main workspaces: the pass owns them until it is done (ev_bg_done on a second stream; the drain behind the frame's last step on the workers)
    const Place pass{bg, &e->w_main};
    auto run_pass = [&]() {      // recorded, or launched on bg
        if (px.has_ego) run_stack<T>(e, pass, STACK_EGO, WindowTokens{e->d_pose, e->d_map, e->d_box, e->d_img, B, P, Tnext, 0}, CACHE_FILL_PREFIX);
        run_stack<T>(e, pass, STACK_MAP, ws, CACHE_FILL_PREFIX);
        run_stack<T>(e, pass, STACK_BOX, ws, CACHE_FILL_PREFIX);
        run_stack<T>(e, pass, STACK_TAR, ws, CACHE_FILL_PREFIX);
    };
    if (dbg && dbg->foreground) {      // the reference of tests/test_gpu_bg_pass.py: the stand-alone kernels (bg == the caller's stream here); nothing stays pending
        run_pass();
        HIPCHK(e, hipStreamSynchronize(bg));
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) return e->fail(UMGEN_E_HIP, "a kernel launch of the pass was refused: %s", hipGetErrorString(le));
        return 0;
    }
    if (e->bg_engine) {
        // the pass as an op list for the decode engine's background workers: the same run_stack calls, with the launchers recording instead of launching
        BgRecorder rec;
        g_bg_rec = &rec;
        run_pass();
        g_bg_rec = nullptr;
        if (rec.failed || rec.ops.empty() || rec.ops.size() > (size_t)kBgMaxOps) {
            if (dbg) return e->fail(UMGEN_E_UNSUPPORTED, "background pass not recordable (%s)", rec.failed ? rec.failed : "op count");
            if (getenv("UMGEN_DEBUG_TIMING")) fprintf(stderr, "[umgen] background pass not recordable (%s): this frame's successor computes its whole window\n", rec.failed ? rec.failed : "op count");
            return 0;      // (px.valid stays false: the next frame takes the plain path)
        }
        // unit times: the workers' own measurements survive from pass to pass while the list keeps its shape; a new shape starts from the host's guesses
        bool same = rec.ops.size() == e->bg_rec.ops.size();
        for (size_t i = 0; same && i < rec.ops.size(); ++i) same = memcmp(&rec.ops[i].h, &e->bg_rec.ops[i].h, sizeof(BgOpHead)) == 0;
        e->bg_rec = std::move(rec);
        if (dbg && dbg->chunk > 0) for (BgOp& o : e->bg_rec.ops) o.h.chunk = dbg->chunk;
        // header: op count, engine_ticks = 0 (the first launch measures, the workers start with the second), margin 10 us, the embedding tables
        e->bg_head.w[0] = (unsigned)e->bg_rec.ops.size(); e->bg_head.w[1] = 0u; e->bg_head.w[2] = (unsigned)(getenv("UMGEN_BG_MARGIN_US") ? atoi(getenv("UMGEN_BG_MARGIN_US")) * 100 : 1000); e->bg_head.w[3] = 0u;
        if (dbg && dbg->margin_ticks >= 0) e->bg_head.w[2] = (unsigned)dbg->margin_ticks;
        e->bg_head.tb = e->tb;
        static_assert(offsetof(BgQueue, tb) == 16 && offsetof(BgQueue, state) == 16 + sizeof(EmbedTables), "BgQueue header layout");
        HIPCHK(e, hipMemcpyAsync(&e->d_bgq->n_ops, &e->bg_head, sizeof(e->bg_head), hipMemcpyHostToDevice, fg));
        HIPCHK(e, hipMemsetAsync(&e->d_bgq->state[0][0], 0, sizeof(e->d_bgq->state) + sizeof(e->d_bgq->arrive), fg));
        if (!same || dbg) HIPCHK(e, hipMemcpyAsync(&e->d_bgq->est[0], e->bg_rec.est.data(), e->bg_rec.est.size() * sizeof(unsigned), hipMemcpyHostToDevice, fg));
        HIPCHK(e, hipMemcpyAsync(&e->d_bgq->ops[0], e->bg_rec.ops.data(), e->bg_rec.ops.size() * sizeof(BgOp), hipMemcpyHostToDevice, fg));
        e->bg_pending = true;      // (px.valid: once the drain behind the frame's last step has seen every worker at the end of the list, run_frame)
        return 0;
    }
    HIPCHK(e, hipEventRecord(e->ev_bg0, bg));
    run_pass();
    HIPCHK(e, hipEventRecord(e->ev_bg_done, bg));
    e->bg_pending = true;
    px.valid = true;
    return 0;
}

template <typename T>
int build_tables(umgen_engine* e, const Place& pl) {
    // GMLP(codebook) rows (module.py:710-743 applied once to each of the 8192 codes): fp32 activations, exact FMA chain
    const int E = e->E;
    for (int which = 0; which < 2; ++which) {
        const int V = which ? e->cfg.img_vocab : e->cfg.map_vocab;
        const int C = which ? e->cfg.n_img_embd : e->cfg.n_map_embd;
        float* table;
        if (int rc = dalloc(e, &table, (size_t)V * E)) return rc;
        float* hid;
        HIPCHK(e, hipMalloc(&hid, (size_t)V * 4 * E * 4));
        GemmArgs g{};
        g.P = which ? e->img_fc : e->map_fc; g.Q = which ? e->img_cb : e->map_cb; g.Mi = 4 * E; g.Nj = V; g.K = C; g.ldp = C; g.ldq = C;
        g.batch = 1; g.mode = GEMM_STORE; g.gelu = 1; g.out = hid; g.ldo = 4L * E;
        Path<T>::gemm_w_f32act(pl.stream, g);
        GemmArgs g2{};
        g2.P = which ? e->img_proj : e->map_proj; g2.Q = hid; g2.Mi = E; g2.Nj = V; g2.K = 4 * E; g2.ldp = 4 * E; g2.ldq = 4 * E;
        g2.batch = 1; g2.mode = GEMM_STORE; g2.out = table; g2.ldo = E;
        Path<T>::gemm_w_f32act(pl.stream, g2);
        HIPCHK(e, hipStreamSynchronize(pl.stream));
        HIPCHK(e, hipFree(hid));
        if (which) e->tb.gimg = table; else e->tb.gmap = table;
    }
    return 0;
}

}  // namespace

namespace umgen {

// by-precision dispatchers: templates on T do not cross files
void run_stack_any(umgen_engine* e, const Place& pl, int stack, const WindowTokens& w, CacheMode cache_mode, int tail, float* warped_all, int fan_scenes) {
    with_precision(e, [&](auto t) { run_stack<decltype(t)>(e, pl, stack, w, cache_mode, tail, warped_all, fan_scenes); });
}
void ego_decoder_any(umgen_engine* e, const Place& pl, int n, const long* frame_of, int Tq, const int* d_item_T) {
    with_precision(e, [&](auto t) { ego_decoder<decltype(t)>(e, pl, n, frame_of, Tq, d_item_T); });
}
void run_ego_any(umgen_engine* e, const Place& pl, const WindowTokens& w, const SamplerParams& sp, int frame_idx, bool forced, float* trace_logits, CacheMode cache_mode,
                 const EgoSide& es) {
    with_precision(e, [&](auto t) { run_ego<decltype(t)>(e, pl, w, sp, frame_idx, forced, trace_logits, cache_mode, es); });
}
void run_ego_fan_any(umgen_engine* e, const Place& pl, const WindowTokens& w, int N, const SamplerParams& sp, int frame_idx, CacheMode cache_mode, const EgoSide& es) {
    with_precision(e, [&](auto t) { run_ego_fan<decltype(t)>(e, pl, w, N, sp, frame_idx, cache_mode, es); });
}
int run_prefix_prefill_any(umgen_engine* e, const Place& pl, int B, int P, const PrefillSrc* src) {
    return with_precision(e, [&](auto t) { return run_prefix_prefill<decltype(t)>(e, pl, B, P, src); });
}
int launch_prefix_any(umgen_engine* e, const Place& pl, const FrameIO& io, const std::vector<int>& ego, const BgPassDebug* dbg) {
    return with_precision(e, [&](auto t) { return launch_prefix<decltype(t)>(e, pl, io, ego, dbg); });
}
void gemv_any(umgen_engine* e, const Place& pl, const float* x, long ldx, const float* ln_w, const void* W, const float* bias, int N, int K, int M, int mode, float* out, long ldo) {
    with_precision(e, [&](auto t) { gemv<decltype(t)>(e, pl, x, ldx, ln_w, W, bias, N, K, M, mode, out, ldo); });
}
int build_tables_any(umgen_engine* e, const Place& pl) {
    return with_precision(e, [&](auto t) { return build_tables<decltype(t)>(e, pl); });
}

}  // namespace umgen
