// Kernel-level test hooks of the decode step (host pointers in, host pointers out): the batched decode layer (decode_batched.hip), the sampler
// and the collision test (frame.hip), and the five-launch decode layer with the ego decoder's attention (gemv.hip).  Each launches what the
// decode step launches, through the same launchers and argument layout as oar_layers (engine_decode.hip), run_ego (engine_stacks.hip) and
// sample_token_kernel (frame.hip).  Every output buffer carries a guard band (Scratch::out); every location the kernel must not write holds
// NaN and is checked where it comes back.  Used only by tests/; never called by the product path.
#include "debug_util.h"

extern "C" {

// launch_rows_to_frag + launch_rows_mfma on x [M][K] (row-major fp32) and W [N][K] (16-bit bits of precision code prec: 1 bf16, 2 fp16).
//   ROWS_QKV   out [M][ldo]: q columns 0 .. E-1; cache [M][2][H][Lmax][48] (16-bit, H = E / 48, output only: NaN before the launch) gets its
//              K / V rows at position pos
//   ROWS_GELU  out_rows [M][N]: gelu(LN(x) W^T + bias), converted from the fragment-major output
//   ROWS_RESID out [M][ldo] (in/out): out + x W^T + bias; out_rows [M][N]: the fragment-major copy, un-permuted
//   ROWS_F32   out [M][ldo]: LN(x) W^T + bias
// The fragment columns m >= M of the input, the row-major output columns the mode does not write (up to ldo) and the whole cache hold NaN
// at the launch; out and cache come back whole, so that the caller sees whether any of them changed.
int umgen_dbg_rows(int prec, int mode, const float* x, const float* ln_w, const void* W, const float* bias, int M, int N, int K, int E, float* out,
                   long ldo, float* out_rows, void* cache, int Lmax, int pos) {
    if ((prec != 1 && prec != 2) || mode < ROWS_F32 || mode > ROWS_RESID) return UMGEN_E_INVALID;
    if (M < 1 || M > kRowsMaxM || N < 1 || K < 32 || K % 32 || !x || !W) return UMGEN_E_INVALID;
    const bool ln = mode != ROWS_RESID, has_out = mode != ROWS_GELU, has_frag = mode == ROWS_GELU || mode == ROWS_RESID;
    if (ln && (!ln_w || K > 768)) return UMGEN_E_INVALID;        // the LayerNorm prologue keeps every k-step of a wave in registers
    const long ncol = mode == ROWS_QKV ? E : N;                   // row-major columns the kernel writes
    if (has_out && (!out || ldo < ncol)) return UMGEN_E_INVALID;
    if (has_frag && !out_rows) return UMGEN_E_INVALID;
    if (mode == ROWS_QKV && (E < kHeadDim || E % kHeadDim || N != 3 * E || !cache || Lmax < 1 || pos < 0 || pos >= Lmax)) return UMGEN_E_INVALID;
    const size_t cstride = mode == ROWS_QKV ? (size_t)2 * (E / kHeadDim) * Lmax * kHeadDim : 0;   // 16-bit elements per scene
    const size_t osz = has_out ? (size_t)M * ldo * 4 : 0, csz = (size_t)M * cstride * 2;
    std::vector<float> ho(osz / 4);                               // out at the launch: the caller's values where ROWS_RESID adds to them, else NaN
    const float qnan = __builtin_bit_cast(float, kNaN32);
    for (int m = 0; m < M && has_out; ++m)
        for (long n = 0; n < ldo; ++n) ho[(size_t)m * ldo + n] = (mode == ROWS_RESID && n < ncol) ? out[(size_t)m * ldo + n] : qnan;
    Scratch s;
    const float* dX = s.in(x, (size_t)M * K * 4);
    float* dXf = s.raw(frag_floats(K) * 4);
    RowsArgs r{};
    r.x = dXf; r.M = M; r.ln_w = s.in(ln ? ln_w : nullptr, (size_t)K * 4); r.W = s.in(W, (size_t)N * K * 2); r.bias = s.in(bias, (size_t)N * 4);
    r.N = N; r.K = K; r.mode = mode; r.ldo = ldo; r.scene_stride = (long)cstride; r.d_len = s.in(&pos, 4); r.Lmax = Lmax; r.E = E;
    float* dO = s.inout(ho.data(), osz, scene_band((size_t)ldo * 4, M));
    float* dF = s.out(has_frag ? frag_floats(N) * 4 : 0);
    void* dC = s.out(csz, scene_band(cstride * 2, M));
    if (s.rc) return s.rc;
    r.out = has_out ? dO : nullptr; r.out_frag = has_frag ? dF : nullptr; r.cache = csz ? dC : nullptr;
    if (fill_nan(dXf, frag_floats(K), 0) || (has_frag && fill_nan(dF, frag_floats(N), 0)) || (csz && fill_nan(dC, csz / 2, prec))) return UMGEN_E_HIP;
    launch_rows_to_frag(nullptr, dX, K, M, K, dXf);
    by_prec16(prec, [&](auto t) { launch_rows_mfma<decltype(t)>(nullptr, r); });
    if (int rc = s.finish()) return rc;
    if (has_out && down(out, dO, osz)) return UMGEN_E_HIP;
    if (csz && down(cache, dC, csz)) return UMGEN_E_HIP;
    return has_frag ? frag_down(dF, M, N, out_rows) : UMGEN_OK;
}

// launch_attn_decode_batched on q [M][H * 48] (fp32) against the cache image [M][2][H][Lmax][48] (16-bit bits of prec) with *d_len = len, i.e.
// keys 0 .. len; y [M][H * 48] row-major (converted from the kernel's fragment-major output)
int umgen_dbg_attn_decode_batched(int prec, const float* q, const void* cache, int M, int H, int Lmax, int len, float* y) {
    if ((prec != 1 && prec != 2) || M < 1 || M > kRowsMaxM || H < 1 || len < 0 || len >= Lmax || !q || !cache || !y) return UMGEN_E_INVALID;
    const int E = H * kHeadDim;
    const size_t cstride = (size_t)2 * H * Lmax * kHeadDim, csz = (size_t)M * cstride * 2;
    Scratch s;
    const float* dQ = s.in(q, (size_t)M * E * 4);
    const void* dC = s.in(cache, csz);
    const int* dlen = s.in(&len, 4);
    float* dY = s.out(frag_floats(E) * 4);
    if (s.rc) return s.rc;
    if (int rc = fill_nan(dY, frag_floats(E), 0)) return rc;
    by_prec16(prec, [&](auto t) {
        typedef decltype(t) T;
        launch_attn_decode_batched<T>(nullptr, dQ, (const T*)dC, (long)cstride, M, H, Lmax, dlen, dY);
    });
    if (int rc = s.finish()) return rc;
    return frag_down(dY, M, E, y);
}

// block_sample (frame.hip; method 0 top-k with k, 1 top-p with p; temperature temp) on n rows of V <= 8192 logits, one block per row, with the
// uniforms u[n] and the masked index mask_idx (-1: none) -> tokens[n]
int umgen_dbg_sample(int method, const float* logits, int n, int V, int k, float p, float temp, int mask_idx, const float* u, int32_t* tokens) {
    if ((method != 0 && method != 1) || V < 1 || V > 8192 || n < 1 || k < 1 || mask_idx < -1 || mask_idx >= V) return UMGEN_E_INVALID;
    Scratch s;
    const float *dL = s.in(logits, (size_t)n * V * 4), *dU = s.in(u, (size_t)n * 4);
    int *dO = s.raw(4), *dT = s.out((size_t)n * 4);
    if (s.rc) return s.rc;
    if (hipMemset(dO, 0, 4) != hipSuccess) return UMGEN_E_HIP;
    SamplerParams sp{};
    sp.method = method; sp.top_k = sp.top_k_map = sp.topk_image = k; sp.p = sp.p_map = p; sp.temperature = temp;
    launch_sample_dbg(nullptr, dL, V, sp, k, p, dU, mask_idx, dT, dO, n);
    if (int rc = s.finish()) return rc;
    return down(tokens, dT, (size_t)n * 4);
}

// block_sample on the rows w = logits + bias (bias [n][V]: every row its own, entries finite or -inf with one allowed entry that is not mask_idx),
// formed on the device in a scratch row per block like the samplers of a biased call form them -> tokens[n]
int umgen_dbg_sample_biased(int method, const float* logits, const float* bias, int n, int V, int k, float p, float temp, int mask_idx, const float* u,
                            int32_t* tokens) {
    if ((method != 0 && method != 1) || !logits || !bias || !u || !tokens || V < 1 || V > 8192 || n < 1 || k < 1 || mask_idx < -1 || mask_idx >= V)
        return UMGEN_E_INVALID;
    for (int i = 0; i < n; ++i) {
        int allowed = 0;
        for (int c = 0; c < V; ++c) {
            const float v = bias[(size_t)i * V + c];
            if (v != v || v == INFINITY) return UMGEN_E_INVALID;
            allowed += (v != -INFINITY && c != mask_idx);
        }
        if (!allowed) return UMGEN_E_INVALID;
    }
    Scratch s;
    const float *dL = s.in(logits, (size_t)n * V * 4), *dB = s.in(bias, (size_t)n * V * 4), *dU = s.in(u, (size_t)n * 4);
    float* dW = s.out((size_t)n * kBiasRowLen * 4);
    int *dO = s.raw(4), *dT = s.out((size_t)n * 4);
    if (s.rc) return s.rc;
    if (hipMemset(dO, 0, 4) != hipSuccess) return UMGEN_E_HIP;
    SamplerParams sp{};
    sp.method = method; sp.top_k = sp.top_k_map = sp.topk_image = k; sp.p = sp.p_map = p; sp.temperature = temp;
    launch_sample_dbg_biased(nullptr, dL, dB, dW, V, sp, k, p, dU, mask_idx, dT, dO, n);
    if (int rc = s.finish()) return rc;
    return down(tokens, dT, (size_t)n * 4);
}

// check_collision_dev (frame.hip) on n_sets box sets: boxes [n_sets][max_n][10] fp64, set i = its first counts[i] boxes -> out[i] 0 / 1
int umgen_dbg_collision(const double* boxes, const int32_t* counts, int n_sets, int max_n, int32_t* out) {
    if (n_sets < 1 || max_n < 1 || max_n > 64 || !boxes || !counts || !out) return UMGEN_E_INVALID;     // the sampler's corner table holds 64 boxes
    for (int i = 0; i < n_sets; ++i)
        if (counts[i] < 1 || counts[i] > max_n) return UMGEN_E_INVALID;
    Scratch s;
    const double* dB = s.in(boxes, (size_t)n_sets * max_n * 10 * 8);
    const int* dN = s.in(counts, (size_t)n_sets * 4);
    int* dO = s.out((size_t)n_sets * 4);
    if (s.rc) return s.rc;
    launch_collision_rows(nullptr, dB, dN, max_n, dO, n_sets);
    if (int rc = s.finish()) return rc;
    return down(out, dO, (size_t)n_sets * 4);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The five-launch decode layer and the ego decoder's attention (gemv.hip).  Operands of type T by precision code prec (0 fp32, 1 bf16 bits,
// 2 fp16 bits); activations, biases and LayerNorm weights fp32.
// ---------------------------------------------------------------------------------------------------------------------------

// launch_gemv in output mode `mode` (GEMV_OUT_F32 / _GELU / _QKV) with rows_per_block rpb (0: row loop, 1, 2) on W [N][K]; ln_w nullable.
//   x: xoff < 0: the rows [M][K]; xoff >= 0: [xoff + M][K], the input rows addressed through the device-side offset d_xoff (= xoff rows)
//   out [M][ldo]: returned whole; NaN at the launch, the kernel writes columns < N (QKV: < E)
//   cache (QKV only) [M][2][H][Lmax][48] of T, in / out: the kernel may change row pos of every (scene, K / V, head) only
int umgen_dbg_gemv_modes(int prec, int mode, int rpb, const float* x, int xoff, const float* ln_w, const void* W, const float* bias, int M, int N,
                         int K, int E, float* out, long ldo, void* cache, int Lmax, int pos) {
    if (prec < 0 || prec > 2 || mode < GEMV_OUT_F32 || mode > GEMV_OUT_QKV || rpb < 0 || rpb > 2) return UMGEN_E_INVALID;
    if (M < 1 || N < 1 || K < 8 || K % 8 || K > 1536 || !x || !W || !out) return UMGEN_E_INVALID;
    const bool qkv = mode == GEMV_OUT_QKV;
    if (ldo < (qkv ? E : N)) return UMGEN_E_INVALID;
    if (qkv && (E < kHeadDim || E % kHeadDim || N != 3 * E || !cache || Lmax < 1 || pos < 0 || pos >= Lmax)) return UMGEN_E_INVALID;
    const size_t es = prec ? 2 : 4, rows = (size_t)M + std::max(xoff, 0);
    const size_t cstride = qkv ? (size_t)2 * (E / kHeadDim) * Lmax * kHeadDim : 0, csz = (size_t)M * cstride * es, osz = (size_t)M * ldo * 4;
    Scratch s;
    GemvArgs a{};
    a.x = s.in(x, rows * K * 4); a.ldx = K; a.ln_w = s.in(ln_w, (size_t)K * 4); a.W = s.in(W, (size_t)N * K * es); a.bias = s.in(bias, (size_t)N * 4);
    const int *dOff = s.in(&xoff, 4), *dlen = s.in(&pos, 4);
    if (xoff >= 0) { a.d_xoff = dOff; a.xoff_mul = K; }
    a.N = N; a.K = K; a.M = M; a.out_mode = mode; a.out = s.out(osz, scene_band((size_t)ldo * 4, M)); a.ldo = ldo;
    void* dC = s.inout(cache, csz, scene_band(cstride * es, M));
    a.cache = csz ? dC : nullptr; a.scene_stride = (long)cstride;
    a.d_len = qkv ? dlen : nullptr; a.Lmax = Lmax; a.E = qkv ? E : K; a.rows_per_block = rpb;
    if (s.rc) return s.rc;
    if (int rc = fill_nan(a.out, osz / 4, 0)) return rc;
    by_prec(prec, [&](auto t) { launch_gemv<decltype(t)>(nullptr, a); });
    if (int rc = s.finish()) return rc;
    if (down(out, a.out, osz)) return UMGEN_E_HIP;
    return csz ? down(cache, dC, csz) : UMGEN_OK;
}

// The plain form of launch_gemv_resid (MLP down-projection): x [M][N] (in / out) += a[:, :K] . W[N][K]^T + bias, a [M][lda]; rpb as above.
int umgen_dbg_gemv_resid(int prec, int rpb, const float* a_in, long lda, const void* W, const float* bias, int M, int N, int K, float* x) {
    if (prec < 0 || prec > 2 || rpb < 0 || rpb > 2 || M < 1 || N < 1 || K < 8 || K % 8 || K > 12 * 512 || lda < K || lda % 4 || !a_in || !W || !x)
        return UMGEN_E_INVALID;
    const size_t es = prec ? 2 : 4, xsz = (size_t)M * N * 4;
    Scratch s;
    GemvResidArgs r{};
    r.rows_per_block = rpb; r.a = s.in(a_in, (size_t)M * lda * 4); r.lda = lda; r.H = 1; r.ns = 1; r.W = s.in(W, (size_t)N * K * es);
    r.bias = s.in(bias, (size_t)N * 4); r.N = N; r.K = K; r.M = M; r.x = s.inout(x, xsz, scene_band((size_t)N * 4, M)); r.ldx = N;
    if (s.rc) return s.rc;
    by_prec(prec, [&](auto t) { launch_gemv_resid<decltype(t)>(nullptr, r); });
    if (int rc = s.finish()) return rc;
    return down(x, r.x, xsz);
}

// One attention site -- launch_attn_partial with the product's geometry -- and its projection with the split merge (launch_gemv_resid,
// part != nullptr, rows_per_block rpb): x [M][E] (in / out) += merge(partials) . Wo[E][E]^T + bo.  E = H * 48.  geom:
//   0  decode step (launch_decode_layer): M = B; q [B][E]; kv = cache [B][2][H][Lmax][48] of T, keys 0 .. pos (*d_len = pos); ns splits
//   1  ego self-attention (launch_ego_self_attn): M = 3B; q = the packed q|k|v rows qkv3 [3B][3E] (fp32 in every mode); kv unused
//   2  ego cross-attention (launch_ego_cross_attn): M = 3B; q [3B][E]; kv [B * kSeq][2E] of T
// The partials start as finite garbage (the product's buffer keeps the values of earlier launches): slots >= ns must weigh 0.
int umgen_dbg_attn_partial(int prec, int geom, int rpb, const float* q, const void* kv, int B, int H, int Lmax, int pos, int ns, const void* Wo,
                           const float* bo, float* x) {
    if (prec < 0 || prec > 2 || geom < 0 || geom > 2 || rpb < 0 || rpb > 2 || B < 1 || H < 1 || H > 32 || !q || !Wo || !x) return UMGEN_E_INVALID;
    if (geom != 1 && !kv) return UMGEN_E_INVALID;
    if (geom == 0 && (Lmax < kAttnSplit * kAttnChunk || pos < 0 || pos >= kAttnSplit * kAttnChunk || ns < attn_nsplit(pos + 1) || ns > kAttnSplit))
        return UMGEN_E_INVALID;                    // the loads are clamped to kAttnSplit * kAttnChunk rows per (scene, head)
    const int E = H * kHeadDim, M = geom == 0 ? B : 3 * B;
    const size_t es = prec ? 2 : 4, xsz = (size_t)M * E * 4, psz = (size_t)M * H * kAttnRec;
    const size_t qsz = (size_t)M * (geom == 1 ? 3 : 1) * E * 4;
    const size_t kvsz = geom == 0 ? (size_t)B * 2 * H * Lmax * kHeadDim * es : (geom == 2 ? (size_t)B * kSeq * 2 * E * es : 0);
    Scratch s;
    const float* dq = s.in(q, qsz);
    const void* dKV = s.in(kvsz ? kv : nullptr, kvsz);
    float *dQ = s.raw((size_t)M * E * 4), *dP = s.raw(psz * 4);
    const int* dlen = s.in(&pos, 4);
    GemvResidArgs r{};
    r.rows_per_block = rpb; r.part = dP; r.H = H; r.W = s.in(Wo, (size_t)E * E * es); r.bias = s.in(bo, (size_t)E * 4);
    r.N = E; r.K = E; r.M = M; r.x = s.inout(x, xsz, scene_band((size_t)E * 4, M)); r.ldx = E;
    if (s.rc) return s.rc;
    if (int rc = fill_stale(dP, psz)) return rc;
    by_prec(prec, [&](auto t) {
        typedef decltype(t) T;
        if (geom == 0) {
            launch_attn_partial<T>(nullptr, dq, (const T*)dKV, (long)2 * H * Lmax * kHeadDim, (long)Lmax * kHeadDim, kHeadDim,
                                   (long)H * Lmax * kHeadDim, B, 1, H, dlen, 1, ns, dP);
            r.ns = ns;
        } else if (geom == 1) {                    // run_ego: the q rows gathered out of the packed q|k|v rows first
            (void)hipMemcpy2DAsync(dQ, (size_t)E * 4, dq, (size_t)3 * E * 4, (size_t)E * 4, M, hipMemcpyDeviceToDevice, nullptr);
            launch_ego_self_attn(nullptr, dQ, dq, M, H, dP);
            r.ns = 1;
        } else {
            launch_ego_cross_attn<T>(nullptr, dq, (const T*)dKV, M, H, dP);
            r.ns = ego_cross_nsplit();
        }
        launch_gemv_resid<T>(nullptr, r);
    });
    if (int rc = s.finish()) return rc;
    return down(x, r.x, xsz);
}

// One whole BlockOAR layer of the decode step through launch_decode_layer (what oar_layers launches per layer) for B scenes at position pos:
// x [B][E] (in / out), q [B][E] (out: the q rows), cache [B][2][H][kAttnSplit * kAttnChunk][48] of T (in / out; the layer writes row pos).
// Weights Wqkv [3E][E], Wo [E][E], Wfc [4E][E], Wproj [E][4E] of T; bqkv [3E], bo [E], ln_a, ln_b [E].
int umgen_dbg_decode_layer(int prec, int rpb, int B, int E, int pos, int ns, const float* ln_a, const void* Wqkv, const float* bqkv, const void* Wo,
                           const float* bo, const float* ln_b, const void* Wfc, const void* Wproj, float* x, float* q, void* cache) {
    const int Lmax = kAttnSplit * kAttnChunk, H = E / kHeadDim;
    if (prec < 0 || prec > 2 || rpb < 0 || rpb > 2 || B < 1 || E < kHeadDim || E % kHeadDim || E > 1536 || pos < 0 || pos >= Lmax) return UMGEN_E_INVALID;
    if (ns < attn_nsplit(pos + 1) || ns > kAttnSplit || !ln_a || !Wqkv || !bqkv || !Wo || !bo || !ln_b || !Wfc || !Wproj || !x || !q || !cache)
        return UMGEN_E_INVALID;
    const size_t es = prec ? 2 : 4, EE = (size_t)E * E, xsz = (size_t)B * E * 4, cstride = (size_t)2 * H * Lmax * kHeadDim, csz = B * cstride * es;
    const size_t psz = (size_t)B * H * kAttnRec;
    Scratch s;
    DecodeLayerArgs d{};
    d.ln_a = s.in(ln_a, (size_t)E * 4); d.Wqkv = s.in(Wqkv, 3 * EE * es); d.bqkv = s.in(bqkv, (size_t)3 * E * 4); d.Wo = s.in(Wo, EE * es);
    d.bo = s.in(bo, (size_t)E * 4); d.ln_b = s.in(ln_b, (size_t)E * 4); d.Wfc = s.in(Wfc, 4 * EE * es); d.Wproj = s.in(Wproj, 4 * EE * es);
    d.h = s.raw((size_t)B * 4 * E * 4); d.part = s.raw(psz * 4); d.d_len = s.in(&pos, 4);
    d.x = s.inout(x, xsz, scene_band((size_t)E * 4, B)); d.q = s.out(xsz, scene_band((size_t)E * 4, B));
    d.cache = s.inout(cache, csz, scene_band(cstride * es, B));
    d.scene_stride = (long)cstride; d.Lmax = Lmax; d.B = B; d.E = E; d.H = H; d.ns = ns; d.rows_per_block = rpb;
    if (s.rc) return s.rc;
    if (fill_nan(d.q, xsz / 4, 0) || fill_stale(d.part, psz)) return UMGEN_E_HIP;
    by_prec(prec, [&](auto t) { launch_decode_layer<decltype(t)>(nullptr, d); });
    if (int rc = s.finish()) return rc;
    if (down(x, d.x, xsz) || down(q, d.q, xsz)) return UMGEN_E_HIP;
    return down(cache, d.cache, csz);
}

// Self-test of what the hooks above rely on, without a kernel: Scratch's guard bands must notice one changed byte at either end of a band,
// and frag_down one written word in a scene column >= M or a pad column >= C.  0, or the number (from 1) of the first step that gave
// another answer than expected.
int umgen_dbg_guard_selftest(void) {
    Scratch s;
    const size_t n1 = 1000, n2 = 4096, band2 = (size_t)1 << 20;
    char *b1 = s.out(n1), *b2 = s.out(n2, band2);
    const int M = 17, C = 40;
    float* dF = s.raw(frag_floats(C) * 4);
    auto set_byte = [](char* p, int v) { return hipMemset(p, v, 1) == hipSuccess; };
    if (s.rc) return 1;
    if (!s.intact()) return 2;
    if (!set_byte(b1 + n1, 0) || s.intact()) return 3;                       // first byte of the first band
    if (!set_byte(b1 + n1, kGuardByte) || !s.intact()) return 4;
    if (!set_byte(b2 + n2 + band2 - 1, 0) || s.intact()) return 5;           // last byte of the second band
    if (!set_byte(b2 + n2 + band2 - 1, kGuardByte) || !s.intact()) return 6;
    // fragment-major [kRowsMaxM][C]: NaN everywhere, then value m * C + c at (m < M, c < C)
    std::vector<float> h(frag_floats(C)), rows((size_t)M * C, -1.f);
    if (fill_nan(dF, h.size(), 0) || down(h.data(), dF, h.size() * 4)) return 7;
    for (int m = 0; m < M; ++m)
        for (int c = 0; c < C; ++c) h[frag_index(m, c)] = (float)(m * C + c);
    if (up(dF, h.data(), h.size() * 4) || frag_down(dF, M, C, rows.data()) != UMGEN_OK) return 7;
    for (size_t i = 0; i < rows.size(); ++i)
        if (rows[i] != (float)i) return 7;
    const float one = 1.f, qnan = __builtin_bit_cast(float, kNaN32);
    if (up(dF + frag_index(M, 0), &one, 4) || frag_down(dF, M, C, rows.data()) != UMGEN_E_STATE) return 8;    // a scene column >= M
    if (up(dF + frag_index(M, 0), &qnan, 4) || frag_down(dF, M, C, rows.data()) != UMGEN_OK) return 9;
    if (up(dF + frag_index(0, C), &one, 4) || frag_down(dF, M, C, rows.data()) != UMGEN_E_STATE) return 10;   // a pad column >= C
    return 0;
}

}  // extern "C"
