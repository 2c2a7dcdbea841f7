// Kernel-level test hooks of libumgen_hip.so (host pointers in, host pointers out) for the GEMMs, the stack attentions, the few-row GEMV and the
// top-k sampler, and the timing hooks of tools/.  Used only by tests/ and tools/ to pin each HIP kernel against the CPU oracle at production
// width; never called by the product path.  Like those of debug_decode.hip and debug_frame.hip, the hooks of this file put a guard band behind every
// output and start it as NaN (in / out buffers as the caller's values); the timing hooks, which return no output, do neither.
#include "debug_util.h"

namespace {
// out[R][N] = act[R][K] . W[N][K]^T as the engine's linears launch it (weights as the P operand)
GemmArgs linear_args(const void* dW, const void* dA, int R, int N, int K, void* dO) {
    GemmArgs g{};
    g.P = dW; g.Q = dA; g.Mi = N; g.Nj = R; g.K = K; g.ldp = K; g.ldq = K; g.batch = 1; g.out = dO; g.ldo = N;
    return g;
}
// the V^T GEMM of the spatial attention: F frames of S rows -> out [F][N][S_pad]
GemmArgs vt_args(const void* dA, const void* dW, int F, int S, int S_pad, int N, int K, void* dO) {
    GemmArgs g{};
    g.P = dA; g.Q = dW; g.Mi = S; g.Nj = N; g.K = K; g.ldp = K; g.ldq = K; g.strideP = (long)S * K; g.strideQ = 0; g.batch = F;
    g.mode = GEMM_VT; g.out = dO; g.ldo = S_pad; g.H = N / kHeadDim;
    return g;
}
inline int pad64(int S) { return ((S + 63) / 64) * 64; }
constexpr int kTemporalSlots = 32;   // attn.hip's kTmax: the temporal kernels take up to twice as many slots (their 64-slot variants)
// random bf16 operands of the GEMM timing hooks: act [na] in [-1, 1), then W [nw] in [-0.05, 0.05), one sequence
void lcg_operands(Scratch& s, size_t na, size_t nw, DevPtr& dA, DevPtr& dW) {
    std::vector<bf16_t> h;
    unsigned x = 12345u;
    fill_lcg(h, na, x, 1.0f);
    dA = s.in(h.data(), na * 2);
    fill_lcg(h, nw, x, 0.05f);
    dW = s.in(h.data(), nw * 2);
}
}  // namespace

extern "C" {

// out[R][N] = act[R][K] . W[N][K]^T + bias (+gelu) (+ residual into out when resid != 0).  bf16 != 0: operands are raw
// bf16 bits (bf16 == 2: IEEE half bits) and the MFMA kernel runs; else fp32 operands and the exact VALU kernel.  out is fp32 for resid, operand dtype otherwise.
int umgen_dbg_linear(int flags, const void* act, const void* W, const float* bias, int R, int N, int K, int gelu, int resid, void* out) {
    const int bf16 = flags & 3;                 // precision code; flag 16: force the 256 x 256 kernel, 32: never use it
    const size_t es = bf16 ? 2 : 4, osz = (size_t)R * N * (resid ? 4 : es);
    Scratch s;
    const void *dA = s.in(act, (size_t)R * K * es), *dW = s.in(W, (size_t)N * K * es);
    const float* dB = s.in(bias, (size_t)N * 4);
    void* dO = resid ? s.inout(out, osz) : s.out(osz);
    if (s.rc) return s.rc;
    if (!resid)
        if (int rc = fill_nan(dO, (size_t)R * N, bf16)) return rc;   // a tile the kernel leaves out comes back as NaN
    GemmArgs g = linear_args(dW, dA, R, N, K, dO);
    g.mode = resid ? GEMM_RESID : GEMM_STORE; g.bias = dB; g.gelu = gelu;
    g.tile256 = (flags & 16) ? 1 : ((flags & 32) ? -1 : 0);
    if (bf16) by_prec16(bf16, [&](auto t) { launch_gemm_mfma<decltype(t)>(nullptr, g); });
    else launch_gemm_valu<float, float>(nullptr, g);
    if (int rc = s.finish()) return rc;
    return down(out, dO, osz);
}

// V^T GEMM of the spatial attention (GEMM_VT): act [F*S][K] rows, W [N][K], bias [N] -> out [F][N][S_pad] of the operand type
// (S_pad = S rounded up to 64; pad columns are zero).  flag 16: force the 256 x 256 kernel, 32: the 128-tile kernels only.
int umgen_dbg_linear_vt(int flags, const void* act, const void* W, const float* bias, int F, int S, int N, int K, void* out) {
    const int prec = flags & 3;
    if (prec != 1 && prec != 2) return UMGEN_E_UNSUPPORTED;
    const int S_pad = pad64(S);
    const size_t R = (size_t)F * S, osz = (size_t)F * N * S_pad * 2;
    Scratch s;
    const void *dA = s.in(act, R * K * 2), *dW = s.in(W, (size_t)N * K * 2);
    const float* dB = s.in(bias, (size_t)N * 4);
    std::vector<unsigned short> h0((size_t)F * N * S_pad, nan16(prec));   // columns < S start as NaN, the pad columns as the zeros they must stay
    for (size_t r = 0; r < (size_t)F * N; ++r) std::fill(h0.begin() + r * S_pad + S, h0.begin() + (r + 1) * S_pad, (unsigned short)0);
    void* dO = s.inout(h0.data(), osz);
    if (s.rc) return s.rc;
    GemmArgs g = vt_args(dA, dW, F, S, S_pad, N, K, dO);
    g.bias = dB;
    g.tile256 = (flags & 16) ? 1 : ((flags & 32) ? -1 : 0);
    by_prec16(prec, [&](auto t) { launch_gemm_mfma<decltype(t)>(nullptr, g); });
    if (int rc = s.finish()) return rc;
    return down(out, dO, osz);
}

// One GEMM launch in the full GemmArgs geometry (kernels.h), for the forms the stacks launch and umgen_dbg_linear cannot express: a strided,
// column-offset output, batches with operand and output strides, weights and activations of different types.  precP / precQ: precision codes
// of P and Q (fp32 x fp32, 16-bit x fp32, or the same 16-bit type twice); mfma != 0 (two 16-bit operands): launch_gemm_mfma, else
// launch_gemm_valu.  P [nP], Q [nQ] elements; bias [Mi] ([Nj] for GEMM_VT), nullable.  `out` is the caller's WHOLE buffer of out_n elements
// (the operand type of the activations for GEMM_STORE / GEMM_VT, fp32 otherwise), uploaded as it is (NaN bits, residual values) and
// downloaded whole; the GEMM's out pointer is element out_off of it.  Every address the geometry reaches is checked here first.
// Mi need not be a multiple of 4 on the launch_gemm_valu path (its kernel stores the last 1 - 3 features one at a time); ldo must be.
int umgen_dbg_gemm(int precP, int precQ, int mfma, const void* P, long nP, const void* Q, long nQ, const float* bias, int Mi, int Nj, int K,
                   long ldp, long ldq, long strideP, long strideQ, int batch, int mode, int gelu, long ldo, long strideO, int H, int tile256,
                   void* out, long out_off, long out_n) {
    const bool pair_ok = (precQ == 0 && precP >= 0 && precP <= 2) || (precP == precQ && (precP == 1 || precP == 2));
    if (!pair_ok || !P || !Q || !out || Mi < 1 || Nj < 1 || K < 1 || batch < 1 || mode < GEMM_STORE || mode > GEMM_VT) return UMGEN_E_INVALID;
    if (ldp < K || ldq < K || strideP < 0 || strideQ < 0 || strideO < 0 || out_off < 0) return UMGEN_E_INVALID;
    const bool use_mfma = mfma && precP == precQ && precP != 0;
    if (mfma && !use_mfma) return UMGEN_E_INVALID;
    if (use_mfma && K % 8 != 0) return UMGEN_E_INVALID;                             // the matrix-core kernels load K in 16-byte pieces
    if ((batch - 1) * strideP + (long)(Mi - 1) * ldp + K > nP || (batch - 1) * strideQ + (long)(Nj - 1) * ldq + K > nQ) return UMGEN_E_INVALID;
    const int prec_o = mode == GEMM_STORE ? precQ : (mode == GEMM_VT ? precP : 0);   // output type: the activations' (Q; P for GEMM_VT), fp32 otherwise
    const long al = prec_o ? 8 : 4;                                                 // 16-byte stores
    if (ldo % al != 0 || strideO % al != 0 || out_off % al != 0 || ldo < Mi) return UMGEN_E_INVALID;
    if (mode == GEMM_VT) {
        if (H < 1 || Nj > H * kHeadDim || out_off + (long)batch * H * kHeadDim * ldo > out_n) return UMGEN_E_INVALID;
    } else if ((Mi % 4 != 0 && use_mfma) || (batch > 1 && strideO < (long)(Nj - 1) * ldo + Mi) || out_off + (batch - 1) * strideO + (long)(Nj - 1) * ldo + Mi > out_n) {
        return UMGEN_E_INVALID;
    }
    const size_t esP = precP ? 2 : 4, esQ = precQ ? 2 : 4, esO = prec_o ? 2 : 4;
    Scratch s;
    const void *dP = s.in(P, (size_t)nP * esP), *dQ = s.in(Q, (size_t)nQ * esQ);
    const float* dB = s.in(bias, (size_t)(mode == GEMM_VT ? Nj : Mi) * 4);
    unsigned char* dO = s.inout(out, (size_t)out_n * esO);
    if (s.rc) return s.rc;
    GemmArgs g{};
    g.P = dP; g.Q = dQ; g.Mi = Mi; g.Nj = Nj; g.K = K; g.ldp = ldp; g.ldq = ldq; g.strideP = strideP; g.strideQ = strideQ; g.batch = batch;
    g.mode = mode; g.bias = dB; g.gelu = gelu; g.out = dO + (size_t)out_off * esO; g.ldo = ldo; g.strideO = strideO; g.H = H; g.tile256 = tile256;
    if (use_mfma) by_prec16(precP, [&](auto t) { launch_gemm_mfma<decltype(t)>(nullptr, g); });
    else if (precP == 0) launch_gemm_valu<float, float>(nullptr, g);
    else if (precQ == 0) by_prec16(precP, [&](auto t) { launch_gemm_valu<decltype(t), float>(nullptr, g); });
    else by_prec16(precP, [&](auto t) { launch_gemm_valu<decltype(t), decltype(t)>(nullptr, g); });
    if (int rc = s.finish()) return rc;
    return down(out, dO, (size_t)out_n * esO);
}

// spatial attention on q|k rows [F*S][2E] and v rows [F*S][E] (both row-major on the host; V is transposed on the device
// through the same GEMM_VT-layout the engine uses).  y [F*S][E].  flag 64: causal (query i sees keys 0 .. i), else every key.
// flag 128: the pad columns [S, S_pad) of V^T hold 7.0 instead of the zeros the product keeps there -- a finite guard value: the kernels load
// the pad with the ragged last key tile and must give it the weight 0 (the masked probabilities are exactly 0; 0 x NaN / inf would not be 0,
// and "pad columns are zero" stays the product's contract), so the result must not change by a bit.
int umgen_dbg_attn_spatial(int flags, const void* qk, const void* v, int F, int S, int H, void* y) {
    const int bf16 = flags & 3;                 // precision code; flag 32 (fp32 only): the VALU kernel instead of the matrix-core one
    if ((flags & 64) && (flags & 32)) return UMGEN_E_UNSUPPORTED;   // the causal launchers have no kernel choice
    const int E = H * kHeadDim, S_pad = pad64(S);
    const size_t es = bf16 ? 2 : 4, R = (size_t)F * S;
    // host-side transpose of V into [F][H][48][S_pad]
    std::vector<unsigned char> vt((size_t)F * E * S_pad * es, 0);
    const unsigned char* vs = (const unsigned char*)v;
    if (flags & 128) {                          // 7.0 in the operand type: fp32 | bf16 | IEEE half
        const unsigned guard = bf16 == 0 ? 0x40E00000u : (bf16 == 1 ? 0x40E0u : 0x4700u);
        for (size_t r = 0; r < (size_t)F * E; ++r)
            for (int sr = S; sr < S_pad; ++sr) memcpy(&vt[(r * S_pad + sr) * es], &guard, es);
    }
    for (int f = 0; f < F; ++f)
        for (int sr = 0; sr < S; ++sr)
            for (int c = 0; c < E; ++c)
                memcpy(&vt[(((size_t)f * E + c) * S_pad + sr) * es], &vs[(((size_t)f * S + sr) * E + c) * es], es);
    Scratch s;
    const void *dQK = s.in(qk, R * 2 * E * es), *dVT = s.in(vt.data(), vt.size());
    void* dY = s.out(R * E * es);
    if (s.rc) return s.rc;
    if (int rc = fill_nan(dY, R * E, bf16)) return rc;   // a row the kernel leaves out comes back as NaN
    by_prec(bf16, [&](auto t) {
        typedef decltype(t) T;
        const T *q = (const T*)dQK, *vtp = (const T*)dVT;
        if constexpr (std::is_same<T, float>::value) {
            if (flags & 64) launch_attn_causal_f32(nullptr, q, vtp, (T*)dY, F, S, S_pad, H);
            else if (flags & 32) launch_attn_spatial_valu<float>(nullptr, q, vtp, (T*)dY, F, S, S_pad, H);   // flag 32: the VALU kernel
            else launch_attn_spatial_f32_mfma(nullptr, q, vtp, (T*)dY, F, S, S_pad, H);
        } else if (flags & 64) {                // flag 64: the causal S x S form of the OAR prefix pass (run_prefix_prefill)
            launch_attn_causal_mfma<T>(nullptr, q, vtp, (T*)dY, F, S, S_pad, H);
        } else {
            launch_attn_spatial_mfma<T>(nullptr, q, vtp, (T*)dY, F, S, S_pad, H);
        }
    });
    if (int rc = s.finish()) return rc;
    return down(y, dY, R * E * es);
}

// temporal causal attention on qkv rows [B*T*S][3E] -> y [B*T*S][E].  split = P > 0: slots 0..P-1 first (k | v appended to a
// slot cache), then slots P..T-1 against that cache -- must equal the single pass bit for bit.
int umgen_dbg_attn_temporal(int bf16, const void* qkv, int B, int T, int S, int H, int split, void* y) {
    const int E = H * kHeadDim;
    const size_t es = bf16 ? 2 : 4, row = (size_t)3 * E * es, orow = (size_t)E * es;
    // one launch on the slots [t0, t0 + Tn) of every scene, gathered into a compact [B][Tn][S] block and scattered back into y
    auto pass = [&](int t0, int Tn, TemporalRange tr) -> int {
        const size_t Rn = (size_t)B * Tn * S;
        std::vector<unsigned char> hq(Rn * row), hy(Rn * orow);
        for (int b = 0; b < B; ++b)
            memcpy(&hq[(size_t)b * Tn * S * row], (const unsigned char*)qkv + ((size_t)b * T + t0) * S * row, (size_t)Tn * S * row);
        Scratch s;
        const void* dQ = s.in(hq.data(), hq.size());
        void* dY = s.out(hy.size());
        if (s.rc) return s.rc;
        if (int rc = fill_nan(dY, Rn * E, bf16)) return rc;
        by_prec(bf16, [&](auto t) { typedef decltype(t) TT; launch_attn_temporal<TT>(nullptr, (const TT*)dQ, (TT*)dY, B, Tn, S, H, tr); });
        if (int rc = s.finish()) return rc;
        if (down(hy.data(), dY, hy.size())) return UMGEN_E_HIP;
        for (int b = 0; b < B; ++b)
            memcpy((unsigned char*)y + ((size_t)b * T + t0) * S * orow, &hy[(size_t)b * Tn * S * orow], (size_t)Tn * S * orow);
        return UMGEN_OK;
    };
    if (split <= 0 || split >= T) return pass(0, T, TemporalRange{0, nullptr, 0, 0});
    const int Tcap = T + 1;
    Scratch s;
    const size_t cn = (size_t)B * Tcap * S * 2 * E;
    void* dC = s.out(cn * es);
    if (s.rc) return s.rc;
    if (int rc = fill_nan(dC, cn, bf16)) return rc;               // a slot the second pass reads and the first did not write is NaN
    if (int rc = pass(0, split, TemporalRange{0, dC, Tcap, 1})) return rc;
    if (int rc = pass(split, T - split, TemporalRange{split, dC, Tcap, 0})) return rc;
    return s.finish();
}

// ONE launch_attn_temporal call on an arbitrary slot range (TemporalRange, kernels.h): qkv [B][Tn][S][3E] holds the slots [t0, t0 + Tn), the
// k | v rows of slots [0, t0) are read from cache [B][Tcap][S][2E], write != 0 appends the new slots' k | v rows to it, only query slots >= q0
// are evaluated.  cache (nullable when t0 == 0 and write == 0) and y [B][Tn][S][E] are in / out: whatever the launch leaves alone keeps the
// caller's fill.
int umgen_dbg_attn_temporal_range(int prec, const void* qkv, int B, int Tn, int S, int H, int t0, int q0, int write, int Tcap, void* cache, void* y) {
    if (prec < 0 || prec > 2 || !qkv || !y || B < 1 || Tn < 1 || S < 1 || H < 1 || t0 < 0 || q0 < 0 || q0 >= t0 + Tn || t0 + Tn > 2 * kTemporalSlots)
        return UMGEN_E_INVALID;
    if (cache ? Tcap < t0 + Tn : (t0 > 0 || write)) return UMGEN_E_INVALID;
    const int E = H * kHeadDim;
    const size_t es = prec ? 2 : 4, Rn = (size_t)B * Tn * S;
    const size_t csz = cache ? (size_t)B * Tcap * S * 2 * E * es : 0;
    Scratch s;
    const void* dQ = s.in(qkv, Rn * 3 * E * es);
    void* dY = s.inout(y, Rn * E * es);
    void* dC = cache ? (void*)s.inout(cache, csz) : nullptr;
    if (s.rc) return s.rc;
    TemporalRange tr{t0, dC, Tcap, write};
    tr.q0 = q0;
    by_prec(prec, [&](auto t) { typedef decltype(t) TT; launch_attn_temporal<TT>(nullptr, (const TT*)dQ, (TT*)dY, B, Tn, S, H, tr); });
    if (int rc = s.finish()) return rc;
    if (cache && down(cache, dC, csz)) return UMGEN_E_HIP;
    return down(y, dY, Rn * E * es);
}

// ONE launch_attn_temporal_fan call (kernels.h): qkv [N][S][3E] holds slot P of N items, item i reads the k | v rows of slots [0, P) from block
// scene_of_item[i] of cache [B][Tcap][S][2E].  cache and y [N][S][E] are in / out: the cache must come back as it went in, and whatever the launch
// leaves alone of y keeps the caller's fill.  The scene list is checked here (in range, every scene's items contiguous) before anything is launched.
int umgen_dbg_attn_temporal_fan(int prec, const void* qkv, int N, const int32_t* scene_of_item, int B, int S, int H, int P, int Tcap, void* cache, void* y) {
    if (prec < 0 || prec > 2 || !qkv || !y || !cache || !scene_of_item || N < 1 || B < 1 || S < 1 || H < 1 || P < 1 || P + 1 > 2 * kTemporalSlots || Tcap < P)
        return UMGEN_E_INVALID;
    std::vector<char> seen(B, 0);
    for (int i = 0; i < N; ++i) {
        const int sc = scene_of_item[i];
        if (sc < 0 || sc >= B || (seen[sc] && scene_of_item[i - 1] != sc)) return UMGEN_E_INVALID;
        seen[sc] = 1;
    }
    const int E = H * kHeadDim;
    const size_t es = prec ? 2 : 4, Rn = (size_t)N * S, csz = (size_t)B * Tcap * S * 2 * E * es;
    Scratch s;
    const void* dQ = s.in(qkv, Rn * 3 * E * es);
    const int* dS = s.in(scene_of_item, (size_t)N * 4);
    void* dY = s.inout(y, Rn * E * es);
    void* dC = s.inout(cache, csz);
    if (s.rc) return s.rc;
    by_prec(prec, [&](auto t) { typedef decltype(t) TT; launch_attn_temporal_fan<TT>(nullptr, (const TT*)dQ, (TT*)dY, N, dS, B, S, H, P, (const TT*)dC, Tcap); });
    if (int rc = s.finish()) return rc;
    if (down(cache, dC, csz)) return UMGEN_E_HIP;
    return down(y, dY, Rn * E * es);
}

// ONE launch_attn_temporal_fan_write call (kernels.h): umgen_dbg_attn_temporal_fan's arguments, but the cache has `blocks` >= max(B, N) blocks and Tcap > P:
// item i also leaves its k | v rows of slot P in block i.  cache and y are in / out: whatever the launch leaves alone keeps the caller's fill.
int umgen_dbg_attn_temporal_fan_write(int prec, const void* qkv, int N, const int32_t* scene_of_item, int B, int S, int H, int P, int Tcap, int blocks, void* cache,
                                      void* y) {
    if (prec < 0 || prec > 2 || !qkv || !y || !cache || !scene_of_item || N < 1 || B < 1 || S < 1 || H < 1 || P < 1 || P + 1 > 2 * kTemporalSlots || Tcap < P + 1 ||
        blocks < std::max(B, N))
        return UMGEN_E_INVALID;
    std::vector<char> seen(B, 0);
    for (int i = 0; i < N; ++i) {
        const int sc = scene_of_item[i];
        if (sc < 0 || sc >= B || (seen[sc] && scene_of_item[i - 1] != sc)) return UMGEN_E_INVALID;
        seen[sc] = 1;
    }
    const int E = H * kHeadDim;
    const size_t es = prec ? 2 : 4, Rn = (size_t)N * S, csz = (size_t)blocks * Tcap * S * 2 * E * es;
    Scratch s;
    const void* dQ = s.in(qkv, Rn * 3 * E * es);
    const int* dS = s.in(scene_of_item, (size_t)N * 4);
    void* dY = s.inout(y, Rn * E * es);
    void* dC = s.inout(cache, csz);
    if (s.rc) return s.rc;
    by_prec(prec, [&](auto t) { typedef decltype(t) TT; launch_attn_temporal_fan_write<TT>(nullptr, (const TT*)dQ, (TT*)dY, N, dS, B, S, H, P, (TT*)dC, Tcap); });
    if (int rc = s.finish()) return rc;
    if (down(cache, dC, csz)) return UMGEN_E_HIP;
    return down(y, dY, Rn * E * es);
}

// ONE launch_attn_temporal_fan_tail call (kernels.h): qkv [N][Wt][S][3E] holds the slots [P, P + Wt) of N items, item i reads the k | v rows of slots [0, P)
// from block scene_of_item[i] of cache [B][Tcap][S][2E]; only tail slots >= q0 have a query.  cache and y [N][Wt][S][E] are in / out, as for
// umgen_dbg_attn_temporal_fan.  A tail no form of the kernel holds is refused with UMGEN_E_UNSUPPORTED before any buffer is made or anything is launched.
int umgen_dbg_attn_temporal_fan_tail(int prec, const void* qkv, int N, int Wt, const int32_t* scene_of_item, int B, int S, int H, int P, int q0, int Tcap,
                                     void* cache, void* y) {
    if (prec < 0 || prec > 2 || !qkv || !y || !cache || !scene_of_item || N < 1 || Wt < 1 || B < 1 || S < 1 || H < 1 || P < 1 || q0 < 0 || q0 >= P + Wt || Tcap < P)
        return UMGEN_E_INVALID;
    if (!attn_temporal_fan_tail_heads(H, P, Wt)) return UMGEN_E_UNSUPPORTED;
    std::vector<char> seen(B, 0);
    for (int i = 0; i < N; ++i) {
        const int sc = scene_of_item[i];
        if (sc < 0 || sc >= B || (seen[sc] && scene_of_item[i - 1] != sc)) return UMGEN_E_INVALID;
        seen[sc] = 1;
    }
    const int E = H * kHeadDim;
    const size_t es = prec ? 2 : 4, Rn = (size_t)N * Wt * S, csz = (size_t)B * Tcap * S * 2 * E * es;
    Scratch s;
    const void* dQ = s.in(qkv, Rn * 3 * E * es);
    const int* dS = s.in(scene_of_item, (size_t)N * 4);
    void* dY = s.inout(y, Rn * E * es);
    void* dC = s.inout(cache, csz);
    if (s.rc) return s.rc;
    int refused = 0;
    by_prec(prec, [&](auto t) {
        typedef decltype(t) TT;
        refused = launch_attn_temporal_fan_tail<TT>(nullptr, (const TT*)dQ, (TT*)dY, N, Wt, dS, B, S, H, P, q0, (const TT*)dC, Tcap);
    });
    if (refused) return UMGEN_E_UNSUPPORTED;
    if (int rc = s.finish()) return rc;
    if (down(cache, dC, csz)) return UMGEN_E_HIP;
    return down(y, dY, Rn * E * es);
}

// ONE launch_tcache_spread call (kernels.h) on cache [blocks][Tcap][row_bytes] (in / out), blocks >= B * N: slots [0, P) of block b < B to the blocks b*N + s
int umgen_dbg_tcache_spread(void* cache, int blocks, int B, int N, int P, int Tcap, long row_bytes) {
    if (!cache || B < 1 || N < 1 || P < 1 || P > Tcap || row_bytes < 16 || row_bytes % 16 || (long)B * N > blocks) return UMGEN_E_INVALID;
    const size_t csz = (size_t)blocks * Tcap * (size_t)row_bytes;
    Scratch s;
    void* dC = s.inout(cache, csz);
    if (s.rc) return s.rc;
    launch_tcache_spread(nullptr, dC, B, N, P, Tcap, (size_t)row_bytes);
    if (int rc = s.finish()) return rc;
    return down(cache, dC, csz);
}

// decode-style attention: q [NQ][E] fp32, kv [L][2E] (k | v) of dtype bf16/fp32 shared by all queries -> y [NQ][E] fp32
// (partial pass + the combine that normally runs in the projection prologue, here through an identity projection)
int umgen_dbg_attn_decode(int bf16, const float* q, const void* kv, int NQ, int L, int H, float* y) {
    const int E = H * kHeadDim;
    const size_t es = bf16 ? 2 : 4;
    std::vector<float> eye((size_t)E * E, 0.f);
    for (int i = 0; i < E; ++i) eye[(size_t)i * E + i] = 1.f;
    Scratch s;
    const float* dQ = s.in(q, (size_t)NQ * E * 4);
    const void *dKV = s.in(kv, (size_t)L * 2 * E * es), *dW = s.in(eye.data(), eye.size() * 4);
    const size_t psz = (size_t)NQ * H * kAttnRec;
    const std::vector<float> x0((size_t)NQ * E, 0.f);            // the residual stream the projection adds into
    float *dP = s.out(psz * 4), *dX = s.inout(x0.data(), x0.size() * 4);
    if (s.rc) return s.rc;
    if (int rc = fill_stale(dP, psz)) return rc;
    by_prec(bf16, [&](auto t) {
        typedef decltype(t) T;
        launch_attn_partial<T>(nullptr, dQ, (const T*)dKV, 0, kHeadDim, 2L * E, E, NQ, NQ, H, nullptr, L, attn_nsplit(L), dP);
    });
    GemvResidArgs a{};
    a.part = dP; a.H = H; a.ns = attn_nsplit(L); a.W = dW; a.N = E; a.K = E; a.M = NQ; a.x = dX; a.ldx = E;
    launch_gemv_resid<float>(nullptr, a);
    if (int rc = s.finish()) return rc;
    return down(y, dX, (size_t)NQ * E * 4);
}

// times `iters` launches of the bf16 MFMA GEMM (mode: GEMM_STORE / GEMM_RESID) on device-resident random operands;
// returns the average milliseconds per launch through *ms.  tokens R, features N, reduction K.
int umgen_dbg_gemm_bench(int R, int N, int K, int mode, int iters, float* ms) {
    Scratch s;
    DevPtr dA, dW;
    lcg_operands(s, (size_t)R * K, (size_t)N * K, dA, dW);
    void* dO = s.raw((size_t)R * N * 4);
    if (s.rc) return s.rc;
    (void)hipMemset(dO, 0, (size_t)R * N * 4);
    GemmArgs g = linear_args(dW, dA, R, N, K, dO);
    g.mode = mode & 15; g.gelu = (mode >> 4) & 1;                             // mode bit 4: erf-GELU epilogue
    g.tile256 = (mode & 64) ? -1 : ((mode & 32) ? 1 : 0);                     // bit 5: force the 256 x 256 kernel, bit 6: 128 x 128 kernels only
    return time_launches(nullptr, 1, iters, 1, ms, [&](int) { launch_gemm_mfma<bf16_t>(nullptr, g); });
}

// timing of the V^T GEMM (GEMM_VT) of F frames x S tokens; flag 32: force the 256-tile kernel, 64: the 128-tile kernels only
int umgen_dbg_gemm_vt_bench(int F, int S, int N, int K, int flag, int iters, float* ms) {
    const int S_pad = pad64(S);
    const size_t osz = (size_t)F * N * S_pad * 2;
    Scratch s;
    DevPtr dA, dW;
    lcg_operands(s, (size_t)F * S * K, (size_t)N * K, dA, dW);
    void* dO = s.raw(osz);
    if (s.rc) return s.rc;
    (void)hipMemset(dO, 0, osz);
    GemmArgs g = vt_args(dA, dW, F, S, S_pad, N, K, dO);
    g.tile256 = (flag & 64) ? -1 : ((flag & 32) ? 1 : 0);
    return time_launches(nullptr, 1, iters, 1, ms, [&](int) { launch_gemm_mfma<bf16_t>(nullptr, g); });
}

int umgen_dbg_gemm_stamps(unsigned long long* out16) { return gemm256_read_stamps(out16); }

// few-row linear: out[M][N] = LN(x[M][K]; ln_w) . W[N][K]^T + bias, optional GELU.  W dtype bf16/fp32, activations fp32.
int umgen_dbg_gemv(int bf16, const float* x, const float* ln_w, const void* W, const float* bias, int M, int N, int K, int gelu, float* out) {
    const size_t es = bf16 ? 2 : 4, osz = (size_t)M * N * 4;
    Scratch s;
    GemvArgs a{};
    a.x = s.in(x, (size_t)M * K * 4); a.ldx = K; a.ln_w = s.in(ln_w, (size_t)K * 4); a.W = s.in(W, (size_t)N * K * es); a.bias = s.in(bias, (size_t)N * 4);
    a.N = N; a.K = K; a.M = M; a.out_mode = gelu ? GEMV_OUT_GELU : GEMV_OUT_F32; a.out = s.out(osz); a.ldo = N; a.E = K;
    if (s.rc) return s.rc;
    // the row-loop form, then (M > 1) the one-row-per-workgroup form the engine launches for several scenes: it must give the same bits
    for (int rpb = 0; rpb <= (M > 1 ? 1 : 0); ++rpb) {
        std::vector<float> got((size_t)M * N);
        if (int rc = fill_nan(a.out, (size_t)M * N, 0)) return rc;
        a.rows_per_block = rpb;
        by_prec(bf16, [&](auto t) { launch_gemv<decltype(t)>(nullptr, a); });
        if (int rc = s.finish()) return rc;
        if (int rc = down(rpb ? got.data() : out, a.out, osz)) return rc;
        if (rpb && memcmp(got.data(), out, osz) != 0) return UMGEN_E_STATE;
    }
    return UMGEN_OK;
}

// the top-k sampler (frame.hip block_sample_topk: UMGen.py:899-913 + 967-974 on the build's uniforms) on n independent rows of V <= 8192
// logits; *overflow counts the rows whose kept set (ties at the k-th value) exceeded the sampler's 64 slots
int umgen_dbg_sample_topk(const float* logits, int n, int V, int k, float temp, const float* u, int32_t* tokens, int32_t* overflow) {
    if (V > 8192 || V < 1 || n < 1) return UMGEN_E_INVALID;
    Scratch s;
    const float *dL = s.in(logits, (size_t)n * V * 4), *dU = s.in(u, (size_t)n * 4);
    int *dT = s.raw((size_t)n * 4), *dO = s.raw(4);
    if (s.rc) return s.rc;
    (void)hipMemset(dO, 0, 4);
    launch_sample_rows(nullptr, dL, V, k, temp, dU, dT, dO, n);
    if (int rc = finish()) return rc;
    if (int rc = down(tokens, dT, (size_t)n * 4)) return rc;
    return down(overflow, dO, 4);
}

// Timing hook of the batched decode layer's kernels (decode_batched.hip) on random data: one BlockOAR layer's five launches at M scenes and
// KV length L, `iters` times back to back; us[0..4] = average microseconds of q|k|v, attention, c_proj, c_fc, mlp c_proj (HIP events
// around each launch), us[5] = the five as one sequence.
int umgen_dbg_batched_layer_bench(int prec, int M, int L, int iters, float* us) {
    const int E = 768, H = 16, Lmax = 2304;
    if (prec != 1 && prec != 2) return UMGEN_E_INVALID;
    if (M < 1 || M > kRowsMaxM || L < 1 || L >= Lmax) return UMGEN_E_INVALID;
    const size_t wsz = (size_t)12 * E * E * 2, csz = (size_t)M * 2 * H * Lmax * kHeadDim * 2, xsz = (size_t)64 * E * 4;
    std::vector<unsigned short> hw(wsz / 2);
    for (size_t i = 0; i < hw.size(); ++i) hw[i] = (unsigned short)(0x3c00 + (i * 2654435761u >> 24)) & (prec == 1 ? 0x3cff : 0x2fff);   // small positive values
    std::vector<float> hx((size_t)64 * E, 0.25f), hl(E, 1.f), hb(4 * E, 0.f);
    for (size_t i = 0; i < hx.size(); ++i) hx[i] = 0.25f + 1e-3f * (float)(i % 97);
    Scratch s;
    const char* Wq = s.in(hw.data(), wsz);
    void* dC = s.raw(csz);
    float *dx = s.in(hx.data(), xsz), *dxr = s.in(hx.data(), xsz), *dq = s.raw(xsz), *da = s.raw(xsz), *dh = s.raw(4 * xsz);
    const float *dln = s.in(hl.data(), (size_t)E * 4), *db = s.in(hb.data(), (size_t)4 * E * 4);
    const int* dlen = s.in(&L, 4);
    if (s.rc) return s.rc;
    if (hipMemset(da, 0, xsz) != hipSuccess || hipMemset(dh, 0, 4 * xsz) != hipSuccess || hipMemset(dC, 0, csz) != hipSuccess) return UMGEN_E_HIP;
    Stream stream;
    if (!stream.s) return UMGEN_E_HIP;
    hipStream_t st = stream.s;
    const long cstride = (long)2 * H * Lmax * kHeadDim;
    auto run = [&](int which) {
        by_prec16(prec, [&](auto tag) {
            typedef decltype(tag) TT;
            RowsArgs r{};
            r.M = M; r.E = E;
            switch (which) {
                case 0: r.x = dx; r.ln_w = dln; r.W = Wq; r.bias = db; r.N = 3 * E; r.K = E; r.mode = ROWS_QKV; r.out = dq; r.ldo = E;
                        r.cache = dC; r.scene_stride = cstride; r.d_len = dlen; r.Lmax = Lmax; launch_rows_mfma<TT>(st, r); break;
                case 1: launch_attn_decode_batched<TT>(st, dq, (const TT*)dC, cstride, M, H, Lmax, dlen, da); break;
                case 2: r.x = da; r.W = Wq + (size_t)3 * E * E * 2; r.bias = db; r.N = E; r.K = E; r.mode = ROWS_RESID; r.out = dxr; r.ldo = E; r.out_frag = dx; launch_rows_mfma<TT>(st, r); break;
                case 3: r.x = dx; r.ln_w = dln; r.W = Wq + (size_t)4 * E * E * 2; r.N = 4 * E; r.K = E; r.mode = ROWS_GELU; r.out_frag = dh; launch_rows_mfma<TT>(st, r); break;
                default: r.x = dh; r.W = Wq + (size_t)8 * E * E * 2; r.N = E; r.K = 4 * E; r.mode = ROWS_RESID; r.out = dxr; r.ldo = E; r.out_frag = dx; launch_rows_mfma<TT>(st, r); break;
            }
        });
    };
    if (int rc = time_launches(st, 3, iters, 6, us, [&](int which) { if (which < 5) run(which); else for (int k = 0; k < 5; ++k) run(k); })) return rc;
    for (int i = 0; i < 6; ++i) us[i] *= 1000.f;
    return UMGEN_OK;
}

}  // extern "C"
