// Kernel-level test hooks of libumgen_hip.so (host pointers in, host pointers out).  Used only by tests/ to pin each
// HIP kernel against the CPU oracle at production width; never called by the product path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/umgen.h"
#include "frame.h"
#include "kernels.h"

using namespace umgen;

namespace {
struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes) { if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) p = nullptr; }
    ~DevBuf() { if (p) (void)hipFree(p); }
};
inline int up(void* d, const void* h, size_t n) { return hipMemcpy(d, h, n, hipMemcpyHostToDevice) == hipSuccess ? 0 : UMGEN_E_HIP; }
inline int down(void* h, const void* d, size_t n) { return hipMemcpy(h, d, n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : UMGEN_E_HIP; }

// Output buffer of the batched-decode and sampler hooks: `bytes` the kernel may write, then a band of `guard` bytes filled with a sentinel.
// A kernel that writes past N, M or the row changes the band; the hook then returns UMGEN_E_STATE.
constexpr unsigned char kGuardByte = 0xA7;
constexpr size_t kGuardBytes = (size_t)64 << 10;
struct GuardedBuf : DevBuf {
    size_t bytes, guard;
    explicit GuardedBuf(size_t b, size_t g = kGuardBytes) : DevBuf(b + g), bytes(b), guard(g) {
        if (p && hipMemset((char*)p + bytes, kGuardByte, guard) != hipSuccess) { (void)hipFree(p); p = nullptr; }
    }
    bool intact() const {
        std::vector<unsigned char> h(guard);
        if (hipMemcpy(h.data(), (const char*)p + bytes, guard, hipMemcpyDeviceToHost) != hipSuccess) return false;
        for (unsigned char c : h)
            if (c != kGuardByte) return false;
        return true;
    }
};
// band behind a buffer of M per-scene rows: the rows scenes M .. kRowsMaxM - 1 would take (at least 64 KB, at most 64 MB)
inline size_t scene_band(size_t row_bytes, int M) {
    return std::min(std::max(kGuardBytes, row_bytes * (size_t)(kRowsMaxM - M)), (size_t)64 << 20);
}
constexpr unsigned kNaN32 = 0x7fc00000u;
inline unsigned short nan16(int prec) { return prec == 2 ? 0x7e00 : 0x7fc0; }
// floats of a fragment-major buffer of kRowsMaxM scenes x C columns (frag_index, kernels.h)
inline size_t frag_floats(int C) { return (size_t)((C + 31) / 32) * 32 * kRowsMaxM; }
// fragment-major [kRowsMaxM][C] on the device -> row-major [M][C] on the host; UMGEN_E_STATE if a column m >= M or a pad column >= C was written
int frag_down(const void* d, int M, int C, float* rows) {
    std::vector<unsigned> h(frag_floats(C));
    if (int rc = down(h.data(), d, h.size() * 4)) return rc;
    bool clean = true;
    for (int m = 0; m < kRowsMaxM; ++m)
        for (int c = 0; c < (C + 31) / 32 * 32; ++c) {
            const unsigned v = h[frag_index(m, c)];
            if (m < M && c < C) memcpy(rows + (size_t)m * C + c, &v, 4);
            else clean = clean && v == kNaN32;
        }
    return clean ? UMGEN_OK : UMGEN_E_STATE;
}
// f(T{}) with T the operand type of precision code prec (0 fp32, 1 bf16, 2 fp16)
template <typename F>
void by_prec(int prec, F&& f) {
    if (prec == 2) f(f16_t{}); else if (prec == 1) f(bf16_t{}); else f(float{});
}
// launch errors first (a launch the runtime refused writes nothing), then the work itself
inline int finish() {
    if (hipGetLastError() != hipSuccess) return UMGEN_E_HIP;
    return hipDeviceSynchronize() == hipSuccess ? UMGEN_OK : UMGEN_E_HIP;
}
constexpr float kStalePartial = 1000.f;   // never-written slots of the attention partials: finite garbage, like the product's stale values
}  // namespace

extern "C" {

// out[R][N] = act[R][K] . W[N][K]^T + bias (+gelu) (+ residual into out when resid != 0).  bf16 != 0: operands are raw
// bf16 bits (bf16 == 2: IEEE half bits) and the MFMA kernel runs; else fp32 operands and the exact VALU kernel.  out is fp32 for resid, operand dtype otherwise.
int umgen_dbg_linear(int flags, const void* act, const void* W, const float* bias, int R, int N, int K, int gelu, int resid, void* out) {
    const int bf16 = flags & 3;                 // precision code; flag 16: force the 256 x 256 kernel, 32: never use it
    const size_t es = bf16 ? 2 : 4;
    DevBuf dA((size_t)R * K * es), dW((size_t)N * K * es), dB((size_t)N * 4), dO((size_t)R * N * 4);
    if (!dA.p || !dW.p || !dB.p || !dO.p) return UMGEN_E_NOMEM;
    if (up(dA.p, act, (size_t)R * K * es) || up(dW.p, W, (size_t)N * K * es)) return UMGEN_E_HIP;
    if (bias && up(dB.p, bias, (size_t)N * 4)) return UMGEN_E_HIP;
    const size_t osz = (size_t)R * N * (resid ? 4 : es);
    if (resid && up(dO.p, out, osz)) return UMGEN_E_HIP;
    GemmArgs g{};
    g.P = dW.p; g.Q = dA.p; g.Mi = N; g.Nj = R; g.K = K; g.ldp = K; g.ldq = K; g.batch = 1;
    g.mode = resid ? GEMM_RESID : GEMM_STORE; g.bias = bias ? (const float*)dB.p : nullptr; g.gelu = gelu; g.out = dO.p; g.ldo = N;
    g.tile256 = (flags & 16) ? 1 : ((flags & 32) ? -1 : 0);
    if (bf16 == 2) launch_gemm_mfma<f16_t>(nullptr, g); else if (bf16) launch_gemm_mfma<bf16_t>(nullptr, g); else launch_gemm_valu<float, float>(nullptr, g);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    return down(out, dO.p, osz);
}

// V^T GEMM of the spatial attention (GEMM_VT): act [F*S][K] rows, W [N][K], bias [N] -> out [F][N][S_pad] of the operand type
// (S_pad = S rounded up to 64; pad columns are zero).  flag 16: force the 256 x 256 kernel, 32: the 128-tile kernels only.
int umgen_dbg_linear_vt(int flags, const void* act, const void* W, const float* bias, int F, int S, int N, int K, void* out) {
    const int prec = flags & 3;
    if (prec != 1 && prec != 2) return UMGEN_E_UNSUPPORTED;
    const int S_pad = ((S + 63) / 64) * 64;
    const size_t R = (size_t)F * S, osz = (size_t)F * N * S_pad * 2;
    DevBuf dA(R * K * 2), dW((size_t)N * K * 2), dB((size_t)N * 4), dO(osz);
    if (!dA.p || !dW.p || !dB.p || !dO.p) return UMGEN_E_NOMEM;
    if (up(dA.p, act, R * K * 2) || up(dW.p, W, (size_t)N * K * 2)) return UMGEN_E_HIP;
    if (bias && up(dB.p, bias, (size_t)N * 4)) return UMGEN_E_HIP;
    (void)hipMemset(dO.p, 0, osz);
    GemmArgs g{};
    g.P = dA.p; g.Q = dW.p; g.Mi = S; g.Nj = N; g.K = K; g.ldp = K; g.ldq = K; g.strideP = (long)S * K; g.strideQ = 0; g.batch = F;
    g.mode = GEMM_VT; g.bias = bias ? (const float*)dB.p : nullptr; g.out = dO.p; g.ldo = S_pad; g.H = N / kHeadDim;
    g.tile256 = (flags & 16) ? 1 : ((flags & 32) ? -1 : 0);
    if (prec == 2) launch_gemm_mfma<f16_t>(nullptr, g); else launch_gemm_mfma<bf16_t>(nullptr, g);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    return down(out, dO.p, osz);
}

// spatial attention on q|k rows [F*S][2E] and v rows [F*S][E] (both row-major on the host; V is transposed on the device
// through the same GEMM_VT-layout the engine uses).  y [F*S][E].  flag 64: causal (query i sees keys 0 .. i), else every key.
int umgen_dbg_attn_spatial(int flags, const void* qk, const void* v, int F, int S, int H, void* y) {
    const int bf16 = flags & 3;                 // precision code; flag 32 (fp32 only): the VALU kernel instead of the matrix-core one
    const int E = H * kHeadDim, S_pad = ((S + 63) / 64) * 64;
    const size_t es = bf16 ? 2 : 4;
    const size_t R = (size_t)F * S;
    // host-side transpose of V into [F][H][48][S_pad]
    std::vector<unsigned char> vt((size_t)F * E * S_pad * es, 0);
    const unsigned char* vs = (const unsigned char*)v;
    for (int f = 0; f < F; ++f)
        for (int s = 0; s < S; ++s)
            for (int c = 0; c < E; ++c)
                memcpy(&vt[(((size_t)f * E + c) * S_pad + s) * es], &vs[(((size_t)f * S + s) * E + c) * es], es);
    if ((flags & 64) && (flags & 32)) return UMGEN_E_UNSUPPORTED;   // the causal launchers have no kernel choice
    DevBuf dQK(R * 2 * E * es), dVT(vt.size());
    GuardedBuf dY(R * E * es);                  // NaN at the launch: a row the kernel leaves out comes back as NaN
    if (!dQK.p || !dVT.p || !dY.p) return UMGEN_E_NOMEM;
    if (up(dQK.p, qk, R * 2 * E * es) || up(dVT.p, vt.data(), vt.size())) return UMGEN_E_HIP;
    if (bf16 ? hipMemsetD16((hipDeviceptr_t)dY.p, nan16(bf16), R * E) != hipSuccess : hipMemsetD32((hipDeviceptr_t)dY.p, (int)kNaN32, R * E) != hipSuccess)
        return UMGEN_E_HIP;
    if (flags & 64) {                           // flag 64: the causal S x S form of the OAR prefix pass (run_prefix_prefill)
        if (bf16 == 2) launch_attn_causal_mfma<f16_t>(nullptr, (const f16_t*)dQK.p, (const f16_t*)dVT.p, (f16_t*)dY.p, F, S, S_pad, H);
        else if (bf16) launch_attn_causal_mfma<bf16_t>(nullptr, (const bf16_t*)dQK.p, (const bf16_t*)dVT.p, (bf16_t*)dY.p, F, S, S_pad, H);
        else launch_attn_causal_f32(nullptr, (const float*)dQK.p, (const float*)dVT.p, (float*)dY.p, F, S, S_pad, H);
    }
    else if (bf16 == 2) launch_attn_spatial_mfma<f16_t>(nullptr, (const f16_t*)dQK.p, (const f16_t*)dVT.p, (f16_t*)dY.p, F, S, S_pad, H);
    else if (bf16) launch_attn_spatial_mfma<bf16_t>(nullptr, (const bf16_t*)dQK.p, (const bf16_t*)dVT.p, (bf16_t*)dY.p, F, S, S_pad, H);
    else if (flags & 32) launch_attn_spatial_valu<float>(nullptr, (const float*)dQK.p, (const float*)dVT.p, (float*)dY.p, F, S, S_pad, H);   // flag 32: the VALU kernel
    else launch_attn_spatial_f32_mfma(nullptr, (const float*)dQK.p, (const float*)dVT.p, (float*)dY.p, F, S, S_pad, H);
    if (int rc = finish()) return rc;
    if (!dY.intact()) return UMGEN_E_STATE;
    return down(y, dY.p, R * E * es);
}

// temporal causal attention on qkv rows [B*T*S][3E] -> y [B*T*S][E].  split = P > 0: slots 0..P-1 first (k | v appended to a
// slot cache), then slots P..T-1 against that cache -- must equal the single pass bit for bit.
int umgen_dbg_attn_temporal(int bf16, const void* qkv, int B, int T, int S, int H, int split, void* y) {
    const int E = H * kHeadDim;
    const size_t es = bf16 ? 2 : 4, R = (size_t)B * T * S;
    if (split <= 0 || split >= T) {
        DevBuf dQ(R * 3 * E * es), dY(R * E * es);
        if (!dQ.p || !dY.p) return UMGEN_E_NOMEM;
        if (up(dQ.p, qkv, R * 3 * E * es)) return UMGEN_E_HIP;
        if (bf16 == 2) launch_attn_temporal<f16_t>(nullptr, (const f16_t*)dQ.p, (f16_t*)dY.p, B, T, S, H);
        else if (bf16) launch_attn_temporal<bf16_t>(nullptr, (const bf16_t*)dQ.p, (bf16_t*)dY.p, B, T, S, H);
        else launch_attn_temporal<float>(nullptr, (const float*)dQ.p, (float*)dY.p, B, T, S, H);
        if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
        return down(y, dY.p, R * E * es);
    }
    const int Tcap = T + 1;
    DevBuf dC((size_t)B * Tcap * S * 2 * E * es);
    if (!dC.p) return UMGEN_E_NOMEM;
    const int t0s[2] = {0, split}, tns[2] = {split, T - split};
    const size_t row = (size_t)3 * E * es, orow = (size_t)E * es;
    for (int pass = 0; pass < 2; ++pass) {
        const int t0 = t0s[pass], Tn = tns[pass];
        const size_t Rn = (size_t)B * Tn * S;
        std::vector<unsigned char> hq(Rn * row), hy(Rn * orow);
        for (int b = 0; b < B; ++b)   // gather the [b][t0 .. t0+Tn) slots into a compact [B][Tn][S] block
            memcpy(&hq[(size_t)b * Tn * S * row], (const unsigned char*)qkv + ((size_t)b * T + t0) * S * row, (size_t)Tn * S * row);
        DevBuf dQ(hq.size()), dY(hy.size());
        if (!dQ.p || !dY.p) return UMGEN_E_NOMEM;
        if (up(dQ.p, hq.data(), hq.size())) return UMGEN_E_HIP;
        TemporalRange tr{t0, dC.p, Tcap, pass == 0 ? 1 : 0};
        if (bf16 == 2) launch_attn_temporal<f16_t>(nullptr, (const f16_t*)dQ.p, (f16_t*)dY.p, B, Tn, S, H, tr);
        else if (bf16) launch_attn_temporal<bf16_t>(nullptr, (const bf16_t*)dQ.p, (bf16_t*)dY.p, B, Tn, S, H, tr);
        else launch_attn_temporal<float>(nullptr, (const float*)dQ.p, (float*)dY.p, B, Tn, S, H, tr);
        if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
        if (down(hy.data(), dY.p, hy.size())) return UMGEN_E_HIP;
        for (int b = 0; b < B; ++b)
            memcpy((unsigned char*)y + ((size_t)b * T + t0) * S * orow, &hy[(size_t)b * Tn * S * orow], (size_t)Tn * S * orow);
    }
    return UMGEN_OK;
}

// decode-style attention: q [NQ][E] fp32, kv [L][2E] (k | v) of dtype bf16/fp32 shared by all queries -> y [NQ][E] fp32
// (partial pass + the combine that normally runs in the projection prologue, here through an identity projection)
int umgen_dbg_attn_decode(int bf16, const float* q, const void* kv, int NQ, int L, int H, float* y) {
    const int E = H * kHeadDim;
    const size_t es = bf16 ? 2 : 4;
    DevBuf dQ((size_t)NQ * E * 4), dKV((size_t)L * 2 * E * es), dP((size_t)NQ * H * kAttnRec * 4), dW((size_t)E * E * 4), dX((size_t)NQ * E * 4);
    if (!dQ.p || !dKV.p || !dP.p || !dW.p || !dX.p) return UMGEN_E_NOMEM;
    if (up(dQ.p, q, (size_t)NQ * E * 4) || up(dKV.p, kv, (size_t)L * 2 * E * es)) return UMGEN_E_HIP;
    std::vector<float> eye((size_t)E * E, 0.f);
    for (int i = 0; i < E; ++i) eye[(size_t)i * E + i] = 1.f;
    if (up(dW.p, eye.data(), eye.size() * 4)) return UMGEN_E_HIP;
    (void)hipMemset(dX.p, 0, (size_t)NQ * E * 4);
    if (bf16 == 2) launch_attn_partial<f16_t>(nullptr, (const float*)dQ.p, (const f16_t*)dKV.p, 0, kHeadDim, 2L * E, E, NQ, NQ, H, nullptr, L, attn_nsplit(L), (float*)dP.p);
    else if (bf16) launch_attn_partial<bf16_t>(nullptr, (const float*)dQ.p, (const bf16_t*)dKV.p, 0, kHeadDim, 2L * E, E, NQ, NQ, H, nullptr, L, attn_nsplit(L), (float*)dP.p);
    else launch_attn_partial<float>(nullptr, (const float*)dQ.p, (const float*)dKV.p, 0, kHeadDim, 2L * E, E, NQ, NQ, H, nullptr, L, attn_nsplit(L), (float*)dP.p);
    GemvResidArgs a{};
    a.part = (const float*)dP.p; a.H = H; a.ns = attn_nsplit(L); a.W = dW.p; a.N = E; a.K = E; a.M = NQ; a.x = (float*)dX.p; a.ldx = E;
    launch_gemv_resid<float>(nullptr, a);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    return down(y, dX.p, (size_t)NQ * E * 4);
}

// times `iters` launches of the bf16 MFMA GEMM (mode: GEMM_STORE / GEMM_RESID) on device-resident random operands;
// returns the average milliseconds per launch through *ms.  tokens R, features N, reduction K.
int umgen_dbg_gemm_bench(int R, int N, int K, int mode, int iters, float* ms) {
    DevBuf dA((size_t)R * K * 2), dW((size_t)N * K * 2), dO((size_t)R * N * 4);
    if (!dA.p || !dW.p || !dO.p) return UMGEN_E_NOMEM;
    std::vector<bf16_t> h((size_t)R * K);
    unsigned x = 12345u;
    for (auto& v : h) { x = x * 1664525u + 1013904223u; v = f32_to_bf16(((x >> 8) & 0xffff) / 32768.0f - 1.0f); }
    if (up(dA.p, h.data(), h.size() * 2)) return UMGEN_E_HIP;
    h.resize((size_t)N * K);
    for (auto& v : h) { x = x * 1664525u + 1013904223u; v = f32_to_bf16((((x >> 8) & 0xffff) / 32768.0f - 1.0f) * 0.05f); }
    if (up(dW.p, h.data(), h.size() * 2)) return UMGEN_E_HIP;
    (void)hipMemset(dO.p, 0, (size_t)R * N * 4);
    GemmArgs g{};
    g.P = dW.p; g.Q = dA.p; g.Mi = N; g.Nj = R; g.K = K; g.ldp = K; g.ldq = K; g.batch = 1;
    g.mode = mode & 15; g.gelu = (mode >> 4) & 1; g.out = dO.p; g.ldo = N;   // mode bit 4: erf-GELU epilogue
    g.tile256 = (mode & 64) ? -1 : ((mode & 32) ? 1 : 0);                     // bit 5: force the 256 x 256 kernel, bit 6: 128 x 128 kernels only
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    launch_gemm_mfma<bf16_t>(nullptr, g);
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; ++i) launch_gemm_mfma<bf16_t>(nullptr, g);
    (void)hipEventRecord(e1, nullptr);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    *ms = t / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

// timing of the V^T GEMM (GEMM_VT) of F frames x S tokens; flag 32: force the 256-tile kernel, 64: the 128-tile kernels only
int umgen_dbg_gemm_vt_bench(int F, int S, int N, int K, int flag, int iters, float* ms) {
    const int S_pad = ((S + 63) / 64) * 64;
    const size_t R = (size_t)F * S;
    DevBuf dA(R * K * 2), dW((size_t)N * K * 2), dO((size_t)F * N * S_pad * 2);
    if (!dA.p || !dW.p || !dO.p) return UMGEN_E_NOMEM;
    std::vector<bf16_t> h(R * K);
    unsigned x = 12345u;
    for (auto& v : h) { x = x * 1664525u + 1013904223u; v = f32_to_bf16(((x >> 8) & 0xffff) / 32768.0f - 1.0f); }
    if (up(dA.p, h.data(), h.size() * 2)) return UMGEN_E_HIP;
    h.resize((size_t)N * K);
    for (auto& v : h) { x = x * 1664525u + 1013904223u; v = f32_to_bf16((((x >> 8) & 0xffff) / 32768.0f - 1.0f) * 0.05f); }
    if (up(dW.p, h.data(), h.size() * 2)) return UMGEN_E_HIP;
    (void)hipMemset(dO.p, 0, (size_t)F * N * S_pad * 2);
    GemmArgs g{};
    g.P = dA.p; g.Q = dW.p; g.Mi = S; g.Nj = N; g.K = K; g.ldp = K; g.ldq = K; g.strideP = (long)S * K; g.strideQ = 0; g.batch = F;
    g.mode = GEMM_VT; g.out = dO.p; g.ldo = S_pad; g.H = N / kHeadDim;
    g.tile256 = (flag & 64) ? -1 : ((flag & 32) ? 1 : 0);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    launch_gemm_mfma<bf16_t>(nullptr, g);
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; ++i) launch_gemm_mfma<bf16_t>(nullptr, g);
    (void)hipEventRecord(e1, nullptr);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    *ms = t / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

int umgen_dbg_gemm_stamps(unsigned long long* out16) { return gemm256_read_stamps(out16); }

// few-row linear: out[M][N] = LN(x[M][K]; ln_w) . W[N][K]^T + bias, optional GELU.  W dtype bf16/fp32, activations fp32.
int umgen_dbg_gemv(int bf16, const float* x, const float* ln_w, const void* W, const float* bias, int M, int N, int K, int gelu, float* out) {
    const size_t es = bf16 ? 2 : 4;
    DevBuf dX((size_t)M * K * 4), dL((size_t)K * 4), dW((size_t)N * K * es), dB((size_t)N * 4), dO((size_t)M * N * 4);
    if (!dX.p || !dL.p || !dW.p || !dB.p || !dO.p) return UMGEN_E_NOMEM;
    if (up(dX.p, x, (size_t)M * K * 4) || up(dW.p, W, (size_t)N * K * es)) return UMGEN_E_HIP;
    if (ln_w && up(dL.p, ln_w, (size_t)K * 4)) return UMGEN_E_HIP;
    if (bias && up(dB.p, bias, (size_t)N * 4)) return UMGEN_E_HIP;
    GemvArgs a{};
    a.x = (const float*)dX.p; a.ldx = K; a.ln_w = ln_w ? (const float*)dL.p : nullptr; a.W = dW.p; a.bias = bias ? (const float*)dB.p : nullptr;
    a.N = N; a.K = K; a.M = M; a.out_mode = gelu ? GEMV_OUT_GELU : GEMV_OUT_F32; a.out = (float*)dO.p; a.ldo = N; a.E = K;
    if (bf16 == 2) launch_gemv<f16_t>(nullptr, a); else if (bf16) launch_gemv<bf16_t>(nullptr, a); else launch_gemv<float>(nullptr, a);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    if (int rc = down(out, dO.p, (size_t)M * N * 4)) return rc;
    if (M > 1) {   // the one-row-per-workgroup form (what the engine launches for several scenes) must give the same bits
        std::vector<float> alt((size_t)M * N);
        (void)hipMemset(dO.p, 0, (size_t)M * N * 4);
        a.rows_per_block = 1;
        if (bf16 == 2) launch_gemv<f16_t>(nullptr, a); else if (bf16) launch_gemv<bf16_t>(nullptr, a); else launch_gemv<float>(nullptr, a);
        if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
        if (int rc = down(alt.data(), dO.p, (size_t)M * N * 4)) return rc;
        if (memcmp(alt.data(), out, (size_t)M * N * 4) != 0) return UMGEN_E_STATE;
    }
    return UMGEN_OK;
}

// the top-k sampler (frame.hip block_sample_topk: UMGen.py:899-913 + 967-974 on the build's uniforms) on n independent rows of V <= 8192
// logits; *overflow counts the rows whose kept set (ties at the k-th value) exceeded the sampler's 64 slots
int umgen_dbg_sample_topk(const float* logits, int n, int V, int k, float temp, const float* u, int32_t* tokens, int32_t* overflow) {
    if (V > 8192 || V < 1 || n < 1) return UMGEN_E_INVALID;
    DevBuf dL((size_t)n * V * 4), dU((size_t)n * 4), dT((size_t)n * 4), dO(4);
    if (!dL.p || !dU.p || !dT.p || !dO.p) return UMGEN_E_NOMEM;
    if (up(dL.p, logits, (size_t)n * V * 4) || up(dU.p, u, (size_t)n * 4)) return UMGEN_E_HIP;
    (void)hipMemset(dO.p, 0, 4);
    launch_sample_rows(nullptr, (const float*)dL.p, V, k, temp, (const float*)dU.p, (int*)dT.p, (int*)dO.p, n);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    if (int rc = down(tokens, dT.p, (size_t)n * 4)) return rc;
    return down(overflow, dO.p, 4);
}

// Timing hook of the batched decode layer's kernels (decode_batched.hip) on random data: one BlockOAR layer's five launches at M scenes and
// KV length L, `iters` times back to back; us[0..4] = average microseconds of q|k|v, attention, c_proj, c_fc, mlp c_proj (HIP events
// around each launch), us[5] = the five as one sequence.
int umgen_dbg_batched_layer_bench(int prec, int M, int L, int iters, float* us) {
    const int E = 768, H = 16, Lmax = 2304;
    if (prec != 1 && prec != 2) return UMGEN_E_INVALID;
    if (M < 1 || M > kRowsMaxM || L < 1 || L >= Lmax) return UMGEN_E_INVALID;
    const size_t wsz = (size_t)12 * E * E * 2, csz = (size_t)M * 2 * H * Lmax * kHeadDim * 2;
    DevBuf dW(wsz), dC(csz), dx((size_t)64 * E * 4), dxr((size_t)64 * E * 4), dq((size_t)64 * E * 4), da((size_t)64 * E * 4), dh((size_t)64 * 4 * E * 4), dln((size_t)E * 4), db((size_t)4 * E * 4), dlen(16);
    if (!dW.p || !dC.p || !dx.p || !dxr.p || !dq.p || !da.p || !dh.p || !dln.p || !db.p || !dlen.p) return UMGEN_E_NOMEM;
    std::vector<unsigned short> hw(wsz / 2);
    for (size_t i = 0; i < hw.size(); ++i) hw[i] = (unsigned short)(0x3c00 + (i * 2654435761u >> 24)) & (prec == 1 ? 0x3cff : 0x2fff);   // small positive values
    std::vector<float> hx((size_t)64 * E, 0.25f), hl(E, 1.f), hb(4 * E, 0.f);
    for (size_t i = 0; i < hx.size(); ++i) hx[i] = 0.25f + 1e-3f * (float)(i % 97);
    if (up(dW.p, hw.data(), wsz) || up(dx.p, hx.data(), hx.size() * 4) || up(dxr.p, hx.data(), hx.size() * 4) || hipMemset(da.p, 0, (size_t)64 * E * 4) != hipSuccess || hipMemset(dh.p, 0, (size_t)64 * 4 * E * 4) != hipSuccess || up(dln.p, hl.data(), E * 4) || up(db.p, hb.data(), 4 * E * 4)) return UMGEN_E_HIP;
    if (hipMemset(dC.p, 0, csz) != hipSuccess || hipMemcpy(dlen.p, &L, 4, hipMemcpyHostToDevice) != hipSuccess) return UMGEN_E_HIP;
    hipStream_t st;
    if (hipStreamCreate(&st) != hipSuccess) return UMGEN_E_HIP;
    const char* Wq = (const char*)dW.p;
    auto run = [&](int which, auto tag) {
        typedef decltype(tag) TT;
        RowsArgs r{};
        r.M = M; r.E = E;
        switch (which) {
            case 0: r.x = (float*)dx.p; r.ln_w = (float*)dln.p; r.W = Wq; r.bias = (float*)db.p; r.N = 3 * E; r.K = E; r.mode = ROWS_QKV; r.out = (float*)dq.p; r.ldo = E;
                    r.cache = dC.p; r.scene_stride = (long)2 * H * Lmax * kHeadDim; r.d_len = (int*)dlen.p; r.Lmax = Lmax; launch_rows_mfma<TT>(st, r); break;
            case 1: launch_attn_decode_batched<TT>(st, (float*)dq.p, (const TT*)dC.p, (long)2 * H * Lmax * kHeadDim, M, H, Lmax, (int*)dlen.p, (float*)da.p); break;
            case 2: r.x = (float*)da.p; r.W = Wq + (size_t)3 * E * E * 2; r.bias = (float*)db.p; r.N = E; r.K = E; r.mode = ROWS_RESID; r.out = (float*)dxr.p; r.ldo = E; r.out_frag = (float*)dx.p; launch_rows_mfma<TT>(st, r); break;
            case 3: r.x = (float*)dx.p; r.ln_w = (float*)dln.p; r.W = Wq + (size_t)4 * E * E * 2; r.N = 4 * E; r.K = E; r.mode = ROWS_GELU; r.out_frag = (float*)dh.p; launch_rows_mfma<TT>(st, r); break;
            default: r.x = (float*)dh.p; r.W = Wq + (size_t)8 * E * E * 2; r.N = E; r.K = 4 * E; r.mode = ROWS_RESID; r.out = (float*)dxr.p; r.ldo = E; r.out_frag = (float*)dx.p; launch_rows_mfma<TT>(st, r); break;
        }
    };
    auto run_p = [&](int which) { if (prec == 2) run(which, f16_t{}); else run(which, bf16_t{}); };
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (int which = 0; which <= 5; ++which) {
        for (int w = 0; w < 3; ++w) { if (which < 5) run_p(which); else for (int k = 0; k < 5; ++k) run_p(k); }
        hipEventRecord(e0, st);
        for (int i = 0; i < iters; ++i) { if (which < 5) run_p(which); else for (int k = 0; k < 5; ++k) run_p(k); }
        hipEventRecord(e1, st);
        if (hipEventSynchronize(e1) != hipSuccess) return UMGEN_E_HIP;
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        us[which] = ms * 1000.f / (float)iters;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipStreamDestroy(st);
    return UMGEN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Kernel-level hooks of the batched decode layer (decode_batched.hip) and of the sampler (frame.hip).  Each launches what the decode step
// launches, through the same launchers and argument layout as oar_layers / sample_token_kernel (engine.hip, frame.hip).  Every output
// buffer carries a guard band (GuardedBuf); every location the kernel must not write holds NaN and is checked where it comes back.
// ---------------------------------------------------------------------------------------------------------------------------

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
    DevBuf dX((size_t)M * K * 4), dXf(frag_floats(K) * 4), dL((size_t)K * 4), dW((size_t)N * K * 2), dB((size_t)N * 4), dlen(4);
    GuardedBuf dO(osz, scene_band((size_t)ldo * 4, M)), dF(has_frag ? frag_floats(N) * 4 : 0), dC(csz, scene_band(cstride * 2, M));
    if (!dX.p || !dXf.p || !dL.p || !dW.p || !dB.p || !dlen.p || !dO.p || !dF.p || !dC.p) return UMGEN_E_NOMEM;
    if (up(dX.p, x, (size_t)M * K * 4) || up(dW.p, W, (size_t)N * K * 2) || up(dlen.p, &pos, 4)) return UMGEN_E_HIP;
    if ((ln && up(dL.p, ln_w, (size_t)K * 4)) || (bias && up(dB.p, bias, (size_t)N * 4))) return UMGEN_E_HIP;
    if (hipMemsetD32((hipDeviceptr_t)dXf.p, (int)kNaN32, frag_floats(K)) != hipSuccess) return UMGEN_E_HIP;
    if (has_frag && hipMemsetD32((hipDeviceptr_t)dF.p, (int)kNaN32, frag_floats(N)) != hipSuccess) return UMGEN_E_HIP;
    if (csz && hipMemsetD16((hipDeviceptr_t)dC.p, nan16(prec), csz / 2) != hipSuccess) return UMGEN_E_HIP;
    if (has_out) {
        std::vector<float> ho((size_t)M * ldo);
        const float qnan = __builtin_bit_cast(float, kNaN32);
        for (int m = 0; m < M; ++m)
            for (long n = 0; n < ldo; ++n) ho[(size_t)m * ldo + n] = (mode == ROWS_RESID && n < ncol) ? out[(size_t)m * ldo + n] : qnan;
        if (up(dO.p, ho.data(), osz)) return UMGEN_E_HIP;
    }
    launch_rows_to_frag(nullptr, (const float*)dX.p, K, M, K, (float*)dXf.p);
    RowsArgs r{};
    r.x = (const float*)dXf.p; r.M = M; r.ln_w = ln ? (const float*)dL.p : nullptr; r.W = dW.p; r.bias = bias ? (const float*)dB.p : nullptr;
    r.N = N; r.K = K; r.mode = mode; r.out = has_out ? (float*)dO.p : nullptr; r.ldo = ldo; r.out_frag = has_frag ? (float*)dF.p : nullptr;
    r.cache = csz ? dC.p : nullptr; r.scene_stride = (long)cstride; r.d_len = (const int*)dlen.p; r.Lmax = Lmax; r.E = E;
    if (prec == 2) launch_rows_mfma<f16_t>(nullptr, r); else launch_rows_mfma<bf16_t>(nullptr, r);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    if (!dO.intact() || !dF.intact() || !dC.intact()) return UMGEN_E_STATE;
    if (has_out && down(out, dO.p, osz)) return UMGEN_E_HIP;
    if (csz && down(cache, dC.p, csz)) return UMGEN_E_HIP;
    return has_frag ? frag_down(dF.p, M, N, out_rows) : UMGEN_OK;
}

// launch_attn_decode_batched on q [M][H * 48] (fp32) against the cache image [M][2][H][Lmax][48] (16-bit bits of prec) with *d_len = len, i.e.
// keys 0 .. len; y [M][H * 48] row-major (converted from the kernel's fragment-major output)
int umgen_dbg_attn_decode_batched(int prec, const float* q, const void* cache, int M, int H, int Lmax, int len, float* y) {
    if ((prec != 1 && prec != 2) || M < 1 || M > kRowsMaxM || H < 1 || len < 0 || len >= Lmax || !q || !cache || !y) return UMGEN_E_INVALID;
    const int E = H * kHeadDim;
    const size_t cstride = (size_t)2 * H * Lmax * kHeadDim, csz = (size_t)M * cstride * 2;
    DevBuf dQ((size_t)M * E * 4), dC(csz), dlen(4);
    GuardedBuf dY(frag_floats(E) * 4);
    if (!dQ.p || !dC.p || !dlen.p || !dY.p) return UMGEN_E_NOMEM;
    if (up(dQ.p, q, (size_t)M * E * 4) || up(dC.p, cache, csz) || up(dlen.p, &len, 4)) return UMGEN_E_HIP;
    if (hipMemsetD32((hipDeviceptr_t)dY.p, (int)kNaN32, frag_floats(E)) != hipSuccess) return UMGEN_E_HIP;
    if (prec == 2) launch_attn_decode_batched<f16_t>(nullptr, (const float*)dQ.p, (const f16_t*)dC.p, (long)cstride, M, H, Lmax, (const int*)dlen.p, (float*)dY.p);
    else launch_attn_decode_batched<bf16_t>(nullptr, (const float*)dQ.p, (const bf16_t*)dC.p, (long)cstride, M, H, Lmax, (const int*)dlen.p, (float*)dY.p);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    if (!dY.intact()) return UMGEN_E_STATE;
    return frag_down(dY.p, M, E, y);
}

// block_sample (frame.hip; method 0 top-k with k, 1 top-p with p; temperature temp) on n rows of V <= 8192 logits, one block per row, with the
// uniforms u[n] and the masked index mask_idx (-1: none) -> tokens[n]
int umgen_dbg_sample(int method, const float* logits, int n, int V, int k, float p, float temp, int mask_idx, const float* u, int32_t* tokens) {
    if ((method != 0 && method != 1) || V < 1 || V > 8192 || n < 1 || k < 1 || mask_idx < -1 || mask_idx >= V) return UMGEN_E_INVALID;
    DevBuf dL((size_t)n * V * 4), dU((size_t)n * 4), dO(4);
    GuardedBuf dT((size_t)n * 4);
    if (!dL.p || !dU.p || !dO.p || !dT.p) return UMGEN_E_NOMEM;
    if (up(dL.p, logits, (size_t)n * V * 4) || up(dU.p, u, (size_t)n * 4) || hipMemset(dO.p, 0, 4) != hipSuccess) return UMGEN_E_HIP;
    SamplerParams sp{};
    sp.method = method; sp.top_k = sp.top_k_map = sp.topk_image = k; sp.p = sp.p_map = p; sp.temperature = temp;
    launch_sample_dbg(nullptr, (const float*)dL.p, V, sp, k, p, (const float*)dU.p, mask_idx, (int*)dT.p, (int*)dO.p, n);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    if (!dT.intact()) return UMGEN_E_STATE;
    return down(tokens, dT.p, (size_t)n * 4);
}

// check_collision_dev (frame.hip) on n_sets box sets: boxes [n_sets][max_n][10] fp64, set i = its first counts[i] boxes -> out[i] 0 / 1
int umgen_dbg_collision(const double* boxes, const int32_t* counts, int n_sets, int max_n, int32_t* out) {
    if (n_sets < 1 || max_n < 1 || max_n > 64 || !boxes || !counts || !out) return UMGEN_E_INVALID;     // the sampler's corner table holds 64 boxes
    for (int i = 0; i < n_sets; ++i)
        if (counts[i] < 1 || counts[i] > max_n) return UMGEN_E_INVALID;
    const size_t bsz = (size_t)n_sets * max_n * 10 * 8;
    DevBuf dB(bsz), dN((size_t)n_sets * 4);
    GuardedBuf dO((size_t)n_sets * 4);
    if (!dB.p || !dN.p || !dO.p) return UMGEN_E_NOMEM;
    if (up(dB.p, boxes, bsz) || up(dN.p, counts, (size_t)n_sets * 4)) return UMGEN_E_HIP;
    launch_collision_rows(nullptr, (const double*)dB.p, (const int*)dN.p, max_n, (int*)dO.p, n_sets);
    if (hipDeviceSynchronize() != hipSuccess) return UMGEN_E_HIP;
    if (!dO.intact()) return UMGEN_E_STATE;
    return down(out, dO.p, (size_t)n_sets * 4);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Kernel-level hooks of the five-launch decode layer and the ego decoder's attention (gemv.hip).  Operands of type T by precision code prec
// (0 fp32, 1 bf16 bits, 2 fp16 bits); activations, biases and LayerNorm weights fp32.  Outputs carry guard bands (GuardedBuf).
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
    DevBuf dX(rows * K * 4), dL((size_t)K * 4), dW((size_t)N * K * es), dB((size_t)N * 4), dOff(4), dlen(4);
    GuardedBuf dO(osz, scene_band((size_t)ldo * 4, M)), dC(csz, scene_band(cstride * es, M));
    if (!dX.p || !dL.p || !dW.p || !dB.p || !dOff.p || !dlen.p || !dO.p || !dC.p) return UMGEN_E_NOMEM;
    if (up(dX.p, x, rows * K * 4) || up(dW.p, W, (size_t)N * K * es) || up(dOff.p, &xoff, 4) || up(dlen.p, &pos, 4)) return UMGEN_E_HIP;
    if ((ln_w && up(dL.p, ln_w, (size_t)K * 4)) || (bias && up(dB.p, bias, (size_t)N * 4)) || (csz && up(dC.p, cache, csz))) return UMGEN_E_HIP;
    if (hipMemsetD32((hipDeviceptr_t)dO.p, (int)kNaN32, osz / 4) != hipSuccess) return UMGEN_E_HIP;
    GemvArgs a{};
    a.x = (const float*)dX.p; a.ldx = K;
    if (xoff >= 0) { a.d_xoff = (const int*)dOff.p; a.xoff_mul = K; }
    a.ln_w = ln_w ? (const float*)dL.p : nullptr; a.W = dW.p; a.bias = bias ? (const float*)dB.p : nullptr; a.N = N; a.K = K; a.M = M;
    a.out_mode = mode; a.out = (float*)dO.p; a.ldo = ldo; a.cache = csz ? dC.p : nullptr; a.scene_stride = (long)cstride;
    a.d_len = qkv ? (const int*)dlen.p : nullptr; a.Lmax = Lmax; a.E = qkv ? E : K; a.rows_per_block = rpb;
    by_prec(prec, [&](auto t) { launch_gemv<decltype(t)>(nullptr, a); });
    if (int rc = finish()) return rc;
    if (!dO.intact() || !dC.intact()) return UMGEN_E_STATE;
    if (down(out, dO.p, osz)) return UMGEN_E_HIP;
    return csz ? down(cache, dC.p, csz) : UMGEN_OK;
}

// The plain form of launch_gemv_resid (MLP down-projection): x [M][N] (in / out) += a[:, :K] . W[N][K]^T + bias, a [M][lda]; rpb as above.
int umgen_dbg_gemv_resid(int prec, int rpb, const float* a_in, long lda, const void* W, const float* bias, int M, int N, int K, float* x) {
    if (prec < 0 || prec > 2 || rpb < 0 || rpb > 2 || M < 1 || N < 1 || K < 8 || K % 8 || K > 12 * 512 || lda < K || lda % 4 || !a_in || !W || !x)
        return UMGEN_E_INVALID;
    const size_t es = prec ? 2 : 4, xsz = (size_t)M * N * 4;
    DevBuf dA((size_t)M * lda * 4), dW((size_t)N * K * es), dB((size_t)N * 4);
    GuardedBuf dX(xsz, scene_band((size_t)N * 4, M));
    if (!dA.p || !dW.p || !dB.p || !dX.p) return UMGEN_E_NOMEM;
    if (up(dA.p, a_in, (size_t)M * lda * 4) || up(dW.p, W, (size_t)N * K * es) || up(dX.p, x, xsz) || (bias && up(dB.p, bias, (size_t)N * 4)))
        return UMGEN_E_HIP;
    GemvResidArgs r{};
    r.rows_per_block = rpb; r.a = (const float*)dA.p; r.lda = lda; r.H = 1; r.ns = 1; r.W = dW.p; r.bias = bias ? (const float*)dB.p : nullptr;
    r.N = N; r.K = K; r.M = M; r.x = (float*)dX.p; r.ldx = N;
    by_prec(prec, [&](auto t) { launch_gemv_resid<decltype(t)>(nullptr, r); });
    if (int rc = finish()) return rc;
    if (!dX.intact()) return UMGEN_E_STATE;
    return down(x, dX.p, xsz);
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
    DevBuf dQin(qsz), dQ((size_t)M * E * 4), dKV(kvsz), dP(psz * 4), dW((size_t)E * E * es), dB((size_t)E * 4), dlen(4);
    GuardedBuf dX(xsz, scene_band((size_t)E * 4, M));
    if (!dQin.p || !dQ.p || !dKV.p || !dP.p || !dW.p || !dB.p || !dlen.p || !dX.p) return UMGEN_E_NOMEM;
    if (up(dQin.p, q, qsz) || (kvsz && up(dKV.p, kv, kvsz)) || up(dW.p, Wo, (size_t)E * E * es) || up(dX.p, x, xsz) || up(dlen.p, &pos, 4))
        return UMGEN_E_HIP;
    if ((bo && up(dB.p, bo, (size_t)E * 4)) || hipMemsetD32((hipDeviceptr_t)dP.p, (int)__builtin_bit_cast(unsigned, kStalePartial), psz) != hipSuccess)
        return UMGEN_E_HIP;
    const float* dq = (const float*)dQin.p;
    int nsplit = ns;
    by_prec(prec, [&](auto t) {
        typedef decltype(t) T;
        if (geom == 0) {
            launch_attn_partial<T>(nullptr, dq, (const T*)dKV.p, (long)2 * H * Lmax * kHeadDim, (long)Lmax * kHeadDim, kHeadDim,
                                   (long)H * Lmax * kHeadDim, B, 1, H, (const int*)dlen.p, 1, ns, (float*)dP.p);
        } else if (geom == 1) {                    // run_ego: the q rows gathered out of the packed q|k|v rows first
            (void)hipMemcpy2DAsync(dQ.p, (size_t)E * 4, dQin.p, (size_t)3 * E * 4, (size_t)E * 4, M, hipMemcpyDeviceToDevice, nullptr);
            launch_ego_self_attn(nullptr, (const float*)dQ.p, dq, M, H, (float*)dP.p);
            nsplit = 1;
        } else {
            launch_ego_cross_attn<T>(nullptr, dq, (const T*)dKV.p, M, H, (float*)dP.p);
            nsplit = ego_cross_nsplit();
        }
        GemvResidArgs r{};
        r.rows_per_block = rpb; r.part = (const float*)dP.p; r.H = H; r.ns = nsplit; r.W = dW.p; r.bias = bo ? (const float*)dB.p : nullptr;
        r.N = E; r.K = E; r.M = M; r.x = (float*)dX.p; r.ldx = E;
        launch_gemv_resid<T>(nullptr, r);
    });
    if (int rc = finish()) return rc;
    if (!dX.intact()) return UMGEN_E_STATE;
    return down(x, dX.p, xsz);
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
    DevBuf dLa((size_t)E * 4), dLb((size_t)E * 4), dWqkv(3 * EE * es), dbqkv((size_t)3 * E * 4), dWo(EE * es), dbo((size_t)E * 4), dWfc(4 * EE * es),
        dWproj(4 * EE * es), dH((size_t)B * 4 * E * 4), dP(psz * 4), dlen(4);
    GuardedBuf dX(xsz, scene_band((size_t)E * 4, B)), dQ(xsz, scene_band((size_t)E * 4, B)), dC(csz, scene_band(cstride * es, B));
    if (!dLa.p || !dLb.p || !dWqkv.p || !dbqkv.p || !dWo.p || !dbo.p || !dWfc.p || !dWproj.p || !dH.p || !dP.p || !dlen.p || !dX.p || !dQ.p || !dC.p)
        return UMGEN_E_NOMEM;
    if (up(dLa.p, ln_a, (size_t)E * 4) || up(dLb.p, ln_b, (size_t)E * 4) || up(dWqkv.p, Wqkv, 3 * EE * es) || up(dbqkv.p, bqkv, (size_t)3 * E * 4) ||
        up(dWo.p, Wo, EE * es) || up(dbo.p, bo, (size_t)E * 4) || up(dWfc.p, Wfc, 4 * EE * es) || up(dWproj.p, Wproj, 4 * EE * es) || up(dX.p, x, xsz) ||
        up(dC.p, cache, csz) || up(dlen.p, &pos, 4))
        return UMGEN_E_HIP;
    if (hipMemsetD32((hipDeviceptr_t)dQ.p, (int)kNaN32, xsz / 4) != hipSuccess ||
        hipMemsetD32((hipDeviceptr_t)dP.p, (int)__builtin_bit_cast(unsigned, kStalePartial), psz) != hipSuccess)
        return UMGEN_E_HIP;
    DecodeLayerArgs d{};
    d.ln_a = (const float*)dLa.p; d.Wqkv = dWqkv.p; d.bqkv = (const float*)dbqkv.p; d.Wo = dWo.p; d.bo = (const float*)dbo.p; d.ln_b = (const float*)dLb.p;
    d.Wfc = dWfc.p; d.Wproj = dWproj.p; d.x = (float*)dX.p; d.q = (float*)dQ.p; d.h = (float*)dH.p; d.part = (float*)dP.p;
    d.cache = dC.p; d.scene_stride = (long)cstride; d.Lmax = Lmax; d.d_len = (const int*)dlen.p; d.B = B; d.E = E; d.H = H; d.ns = ns; d.rows_per_block = rpb;
    by_prec(prec, [&](auto t) { launch_decode_layer<decltype(t)>(nullptr, d); });
    if (int rc = finish()) return rc;
    if (!dX.intact() || !dQ.intact() || !dC.intact()) return UMGEN_E_STATE;
    if (down(x, dX.p, xsz) || down(q, dQ.p, xsz)) return UMGEN_E_HIP;
    return down(cache, dC.p, csz);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Kernel-level hooks of frame assembly (frame.hip, rowops.hip): token embedding + map warp, LayerNorm, conditioning rows, first input, ego
// queries, the given-token prefix rows and their K/V move, the per-token step (fixed / sampled token with the bbox3d control flow) and the
// ego sampler.  Each goes through the product's launcher.  Outputs start as NaN (or as the caller's buffer where they are in / out) and
// carry guard bands; every token a launch may use as a table index is checked against the table's size on the host first.
// ---------------------------------------------------------------------------------------------------------------------------
}  // extern "C"

// host image of EmbedTables: fp32 tables and raw bf16 bits, with their row counts (spe has kSeq rows, egoe 3, axe 8, grid_posi 1024)
struct umgen_dbg_tables {
    const float *egoe, *axe, *be, *tpe, *spe, *gmap, *gimg;
    const uint16_t *fouier_pe, *posi, *grid_posi;
    int32_t E, n_tpe, n_pose, n_map, n_box, n_img, n_posi;
};

// everything umgen_dbg_token_steps reads and writes (see there)
struct umgen_dbg_steps {
    const float *cond, *logits, *logits_tar;
    const int32_t* prev_box;
    const unsigned char* control_slot;
    const int32_t* forced;
    const uint64_t* seeds;
    int32_t* tokens;
    float* x_next;
    int32_t *counters, *n_boxes;
    double* boxes;
    uint32_t* state_log;
    SamplerParams sp;
    int32_t B, j0, j1, given_end, ld_logits, use_forced, use_control, frame_idx;
    uint32_t epoch0;
};

namespace {
struct TablesDev {
    std::vector<DevBuf*> bufs;
    EmbedTables tb{};
    bool ok = true;
    const void* put(const void* h, size_t bytes) {
        if (!h) return nullptr;
        bufs.push_back(new DevBuf(bytes));
        if (!bufs.back()->p || up(bufs.back()->p, h, bytes)) { ok = false; return nullptr; }
        return bufs.back()->p;
    }
    explicit TablesDev(const umgen_dbg_tables& t) {
        const size_t E = (size_t)t.E;
        tb.E = t.E;
        tb.egoe = (const float*)put(t.egoe, 3 * E * 4);
        tb.axe = (const float*)put(t.axe, 8 * E * 4);
        tb.be = (const float*)put(t.be, (size_t)t.n_box * E * 4);
        tb.tpe = (const float*)put(t.tpe, (size_t)t.n_tpe * E * 4);
        tb.spe = (const float*)put(t.spe, (size_t)kSeq * E * 4);
        tb.gmap = (const float*)put(t.gmap, (size_t)t.n_map * E * 4);
        tb.gimg = (const float*)put(t.gimg, (size_t)t.n_img * E * 4);
        tb.fouier_pe = (const bf16_t*)put(t.fouier_pe, (size_t)t.n_pose * E * 2);
        tb.posi = (const bf16_t*)put(t.posi, (size_t)t.n_posi * E * 2);
        tb.grid_posi = (const bf16_t*)put(t.grid_posi, (size_t)kNMap * E * 2);
    }
    ~TablesDev() { for (DevBuf* b : bufs) delete b; }
    TablesDev(const TablesDev&) = delete;
};
inline bool tables_sane(const umgen_dbg_tables* t) {
    return t && t->E >= 1 && t->n_tpe >= 0 && t->n_pose >= 0 && t->n_map >= 0 && t->n_box >= 0 && t->n_img >= 0 && t->n_posi >= 0;
}
inline bool in_range(const int32_t* t, size_t n, int hi) {
    for (size_t i = 0; i < n; ++i)
        if (t[i] < 0 || t[i] >= hi) return false;
    return true;
}
inline int fill_nan32(void* d, size_t n) { return hipMemsetD32((hipDeviceptr_t)d, (int)kNaN32, n) == hipSuccess ? 0 : UMGEN_E_HIP; }
inline int kind_of_pos(int j, int given_end) {    // engine.hip umgen_frame: 0 fixed token, 1 map, 2 bbox3d, 3 image
    if (j < given_end) return 0;
    return (j >= kMapC0 && j < kMapEos) ? 1 : (j >= kBoxC0 && j < kBoxEos) ? 2 : (j >= kImgC0 && j < kImgEos) ? 3 : 0;
}
}  // namespace

extern "C" {

// run_stack's first two launches (engine.hip): launch_embed_stack, then for every stack but STACK_EGO launch_warp_map.  Token arrays
// [B][Tf][3 | 1024 | 660 | 512] and pose_diff [B][Tf][3] with Tf = Tfull (0: T); the pass covers slots t0 .. t0 + T - 1.
// -> X [B][T][stack_len][E], mapfeat [B][T][1024][E], warped_last [B][1024][E] (handed to the launcher only when want_last != 0).
int umgen_dbg_embed_warp(int stack, const umgen_dbg_tables* t, const int32_t* pose, const int32_t* map, const int32_t* box, const int32_t* img, int B,
                         int T, int Tfull, int t0, const float* pose_diff, int want_last, float* X, float* mapfeat, float* warped_last) {
    if (stack < STACK_EGO || stack > STACK_TAR || !tables_sane(t) || B < 1 || T < 1 || Tfull < 0 || t0 < 0) return UMGEN_E_INVALID;
    const int Tf = Tfull ? Tfull : T;
    if (t0 + T > Tf || Tf > t->n_tpe || !pose || !map || !box || !img || !pose_diff || !X || !mapfeat || !warped_last) return UMGEN_E_INVALID;
    if (!t->axe || !t->be || !t->tpe || !t->spe || !t->gmap || !t->gimg || !t->fouier_pe || !t->posi || !t->grid_posi) return UMGEN_E_INVALID;
    const size_t F = (size_t)B * Tf, E = (size_t)t->E;
    if (!in_range(pose, F * kNPose, t->n_pose) || !in_range(map, F * kNMap, t->n_map) || !in_range(box, F * kNBox, t->n_box) ||
        !in_range(img, F * kNImg, t->n_img))
        return UMGEN_E_INVALID;
    for (size_t f = 0; f < F; ++f)
        for (int sl = 0; sl < kSlots; ++sl)
            if (box[f * kNBox + sl * kSlotLen] >= t->n_posi || box[f * kNBox + sl * kSlotLen + 1] >= t->n_posi) return UMGEN_E_INVALID;
    const size_t xn = (size_t)B * T * stack_len(stack) * E, mn = (size_t)B * T * kNMap * E, wn = (size_t)B * kNMap * E;
    TablesDev td(*t);
    DevBuf dP(F * kNPose * 4), dM(F * kNMap * 4), dB(F * kNBox * 4), dI(F * kNImg * 4), dPD(F * 3 * 4);
    GuardedBuf dX(xn * 4), dMF(mn * 4), dWL(wn * 4);
    if (!td.ok || !dP.p || !dM.p || !dB.p || !dI.p || !dPD.p || !dX.p || !dMF.p || !dWL.p) return UMGEN_E_NOMEM;
    if (up(dP.p, pose, F * kNPose * 4) || up(dM.p, map, F * kNMap * 4) || up(dB.p, box, F * kNBox * 4) || up(dI.p, img, F * kNImg * 4) ||
        up(dPD.p, pose_diff, F * 3 * 4) || fill_nan32(dX.p, xn) || fill_nan32(dMF.p, mn) || fill_nan32(dWL.p, wn))
        return UMGEN_E_HIP;
    WindowTokens w{};
    w.pose = (const int*)dP.p; w.map = (const int*)dM.p; w.box = (const int*)dB.p; w.img = (const int*)dI.p; w.B = B; w.T = T; w.Tfull = Tfull; w.t0 = t0;
    launch_embed_stack(nullptr, stack, td.tb, w, (float*)dX.p, (float*)dMF.p);
    if (stack != STACK_EGO)
        launch_warp_map(nullptr, stack, td.tb, B, T, (const float*)dMF.p, (const float*)dPD.p, (float*)dX.p, want_last ? (float*)dWL.p : nullptr, Tfull, t0);
    if (int rc = finish()) return rc;
    if (!dX.intact() || !dMF.intact() || !dWL.intact()) return UMGEN_E_STATE;
    if (down(X, dX.p, xn * 4) || down(mapfeat, dMF.p, mn * 4)) return UMGEN_E_HIP;
    return down(warped_last, dWL.p, wn * 4);
}

// launch_layernorm<T> (T by prec) on n_rows rows of x (row r at x + r * row_stride, E <= 1536 columns) -> out [out_rows][E] of T, out_rows >= n_rows:
// NaN at the launch, so rows >= n_rows come back as NaN
int umgen_dbg_layernorm(int prec, const float* x, long row_stride, long n_rows, int E, const float* w, void* out, long out_rows) {
    if (prec < 0 || prec > 2 || !x || !w || !out || E < 1 || E > 64 * 24 || row_stride < E || n_rows < 1 || out_rows < n_rows) return UMGEN_E_INVALID;
    const size_t es = prec ? 2 : 4, xsz = (size_t)n_rows * row_stride * 4, on = (size_t)out_rows * E;
    DevBuf dXi(xsz), dW((size_t)E * 4);
    GuardedBuf dO(on * es);
    if (!dXi.p || !dW.p || !dO.p) return UMGEN_E_NOMEM;
    if (up(dXi.p, x, xsz) || up(dW.p, w, (size_t)E * 4)) return UMGEN_E_HIP;
    if (prec ? hipMemsetD16((hipDeviceptr_t)dO.p, nan16(prec), on) != hipSuccess : fill_nan32(dO.p, on) != 0) return UMGEN_E_HIP;
    by_prec(prec, [&](auto tag) { launch_layernorm<decltype(tag)>(nullptr, (const float*)dXi.p, row_stride, n_rows, E, (const float*)dW.p, (decltype(tag)*)dO.p); });
    if (int rc = finish()) return rc;
    if (!dO.intact()) return UMGEN_E_STATE;
    return down(out, dO.p, on * es);
}

// launch_cond_rows of one stack: X [B][T][stack_len][E], ln_w [E], warped_last [B][1024][E] or NULL (required for STACK_MAP) -> cond
// [B][kSeq][E], in / out: the launch changes the stack's own rows only
int umgen_dbg_cond_rows(int stack, int B, int T, int E, const float* X, const float* ln_w, const float* warped_last, float* cond) {
    if (stack < STACK_MAP || stack > STACK_TAR || B < 1 || T < 1 || E < 1 || !X || !ln_w || !cond || (stack == STACK_MAP && !warped_last)) return UMGEN_E_INVALID;
    const size_t xn = (size_t)B * T * stack_len(stack) * E, wn = (size_t)B * kNMap * E, cn = (size_t)B * kSeq * E;
    DevBuf dXi(xn * 4), dW((size_t)E * 4), dWL(wn * 4);
    GuardedBuf dC(cn * 4);
    if (!dXi.p || !dW.p || !dWL.p || !dC.p) return UMGEN_E_NOMEM;
    if (up(dXi.p, X, xn * 4) || up(dW.p, ln_w, (size_t)E * 4) || up(dC.p, cond, cn * 4) || (warped_last && up(dWL.p, warped_last, wn * 4))) return UMGEN_E_HIP;
    launch_cond_rows(nullptr, stack, B, T, E, (const float*)dXi.p, (const float*)dW.p, warped_last ? (const float*)dWL.p : nullptr, (float*)dC.p);
    if (int rc = finish()) return rc;
    if (!dC.intact()) return UMGEN_E_STATE;
    return down(cond, dC.p, cn * 4);
}

// launch_first_input: x [B][E] = row [E] + cond[b][0] (cond [B][kSeq][E])
int umgen_dbg_first_input(int B, int E, const float* row, const float* cond, float* x) {
    if (B < 1 || E < 1 || !row || !cond || !x) return UMGEN_E_INVALID;
    const size_t cn = (size_t)B * kSeq * E, xn = (size_t)B * E;
    DevBuf dR((size_t)E * 4), dC(cn * 4);
    GuardedBuf dXo(xn * 4);
    if (!dR.p || !dC.p || !dXo.p) return UMGEN_E_NOMEM;
    if (up(dR.p, row, (size_t)E * 4) || up(dC.p, cond, cn * 4) || fill_nan32(dXo.p, xn)) return UMGEN_E_HIP;
    launch_first_input(nullptr, B, E, (const float*)dR.p, (const float*)dC.p, (float*)dXo.p);
    if (int rc = finish()) return rc;
    if (!dXo.intact()) return UMGEN_E_STATE;
    return down(x, dXo.p, xn * 4);
}

// launch_ego_queries: x [B][3][E] = (egoe[j] + spe[j]) + tpe[T - 1]
int umgen_dbg_ego_queries(const umgen_dbg_tables* t, int B, int T, float* x) {
    if (!tables_sane(t) || B < 1 || T < 1 || T > t->n_tpe || !t->egoe || !t->spe || !t->tpe || !x) return UMGEN_E_INVALID;
    const size_t xn = (size_t)B * 3 * t->E;
    TablesDev td(*t);
    GuardedBuf dXo(xn * 4);
    if (!td.ok || !dXo.p) return UMGEN_E_NOMEM;
    if (fill_nan32(dXo.p, xn)) return UMGEN_E_HIP;
    launch_ego_queries(nullptr, td.tb, B, T, (float*)dXo.p);
    if (int rc = finish()) return rc;
    if (!dXo.intact()) return UMGEN_E_STATE;
    return down(x, dXo.p, xn * 4);
}

// launch_prefix_rows: the decode inputs of the given positions 0 .. P - 1 (tske_row [E], cond [B][kSeq][E], tokens [B][2199]) ->
// X [B][P - 1][E] (rows 0 .. P - 2) and x_last [B][E] (row P - 1)
int umgen_dbg_prefix_rows(const umgen_dbg_tables* t, const float* tske_row, const float* cond, const int32_t* tokens, int B, int P, float* X, float* x_last) {
    if (!tables_sane(t) || B < 1 || P < 2 || P > kBoxEos + 2 || !tske_row || !cond || !tokens || !X || !x_last) return UMGEN_E_INVALID;
    if (!t->axe || !t->be || !t->gmap || !t->fouier_pe) return UMGEN_E_INVALID;
    for (int b = 0; b < B; ++b) {
        const int32_t* tk = tokens + (size_t)b * kTokPerFrame;
        if (!in_range(tk, kNPose, t->n_pose) || !in_range(tk + kOffMap, kNMap, t->n_map) || !in_range(tk + kOffBox, kNBox, t->n_box)) return UMGEN_E_INVALID;
    }
    const size_t E = (size_t)t->E, cn = (size_t)B * kSeq * E, xn = (size_t)B * (P - 1) * E, ln = (size_t)B * E, tn = (size_t)B * kTokPerFrame;
    TablesDev td(*t);
    DevBuf dR(E * 4), dC(cn * 4), dT(tn * 4);
    GuardedBuf dXo(xn * 4), dL(ln * 4);
    if (!td.ok || !dR.p || !dC.p || !dT.p || !dXo.p || !dL.p) return UMGEN_E_NOMEM;
    if (up(dR.p, tske_row, E * 4) || up(dC.p, cond, cn * 4) || up(dT.p, tokens, tn * 4) || fill_nan32(dXo.p, xn) || fill_nan32(dL.p, ln)) return UMGEN_E_HIP;
    launch_prefix_rows(nullptr, td.tb, (const float*)dR.p, (const float*)dC.p, (const int*)dT.p, B, P, (float*)dXo.p, (float*)dL.p);
    if (int rc = finish()) return rc;
    if (!dXo.intact() || !dL.intact()) return UMGEN_E_STATE;
    if (down(X, dXo.p, xn * 4)) return UMGEN_E_HIP;
    return down(x_last, dL.p, ln * 4);
}

// launch_prefix_kv_to_cache<T>: qk [B * S][2E] (q | k rows) and vt [B][H][48][S_pad] of T -> cache [B][2][H][Lmax][48] of T (NaN at the launch) with
// the product's scene stride 2 * H * Lmax * 48
int umgen_dbg_prefix_kv_to_cache(int prec, const void* qk, const void* vt, int B, int S, int S_pad, int H, int Lmax, void* cache) {
    if (prec < 0 || prec > 2 || !qk || !vt || !cache || B < 1 || S < 1 || S > S_pad || S > Lmax || H < 1) return UMGEN_E_INVALID;
    const size_t es = prec ? 2 : 4, E = (size_t)H * kHeadDim, qn = (size_t)B * S * 2 * E, vn = (size_t)B * E * S_pad, stride = (size_t)2 * H * Lmax * kHeadDim;
    const size_t cn = (size_t)B * stride;
    DevBuf dQ(qn * es), dV(vn * es);
    GuardedBuf dC(cn * es, scene_band(stride * es, B));
    if (!dQ.p || !dV.p || !dC.p) return UMGEN_E_NOMEM;
    if (up(dQ.p, qk, qn * es) || up(dV.p, vt, vn * es)) return UMGEN_E_HIP;
    if (prec ? hipMemsetD16((hipDeviceptr_t)dC.p, nan16(prec), cn) != hipSuccess : fill_nan32(dC.p, cn) != 0) return UMGEN_E_HIP;
    by_prec(prec, [&](auto tag) {
        typedef decltype(tag) TT;
        launch_prefix_kv_to_cache<TT>(nullptr, (const TT*)dQ.p, (const TT*)dV.p, B, S, S_pad, H, Lmax, (TT*)dC.p, (long)stride);
    });
    if (int rc = finish()) return rc;
    if (!dC.intact()) return UMGEN_E_STATE;
    return down(cache, dC.p, cn * es);
}

// The sampler kernels of decode steps j0 .. j1 - 1 of one frame for B scenes, on an OarState and a SampleArgs of the hook's own: what enqueue_step
// (engine.hip) launches behind the head at position j -- launch_fixed_token for bos / eos / the pose prefix and every position < given_end, else
// launch_sample_token with the position's mod and vocabulary (tables: n_map | n_box | n_img) -- with that step's logits [B][ld_logits]
// (logits [j1 - j0][B][ld_logits]).  logits_tar [B][660][n_box], prev_box [B][660], control_slot [B][60], forced [B][2199] (or NULL), seeds [B].
// In / out: tokens [B][2199], counters [8], n_boxes [B], boxes [B][64][10].  Out: x_next [j1 - j0][B][E] (NaN before every step) and
// state_log [j1 - j0][3] = OarState step, epoch, done behind every step.
int umgen_dbg_token_steps(const umgen_dbg_tables* t, const umgen_dbg_steps* a) {
    if (!tables_sane(t) || !a || a->B < 1 || a->j0 < 0 || a->j1 <= a->j0 || a->j1 > kImgEos) return UMGEN_E_INVALID;
    // given tokens end behind the pose prefix, the map or the boxes (umgen_frame's given_end): fixed_token_kernel knows no given image token
    if (a->given_end != kPoseEos + 1 && a->given_end != kMapEos + 1 && a->given_end != kBoxEos + 1) return UMGEN_E_INVALID;
    if (!a->cond || !a->logits || !a->logits_tar || !a->prev_box || !a->control_slot || !a->seeds || !a->tokens || !a->x_next || !a->counters ||
        !a->n_boxes || !a->boxes || !a->state_log || (a->use_forced && !a->forced))
        return UMGEN_E_INVALID;
    if (!t->axe || !t->be || !t->gmap || !t->gimg || !t->fouier_pe || t->E > 6 * 256) return UMGEN_E_INVALID;   // CondRow: E <= 1536
    const int vmax = std::max(t->n_map, std::max(t->n_box, t->n_img));
    if (vmax > 8192 || a->ld_logits < vmax || t->n_map < 1 || t->n_img < 1 || t->n_box <= kBoxPad) return UMGEN_E_INVALID;
    if (a->sp.method < 0 || a->sp.method > 1 || a->sp.top_k < 1 || a->sp.top_k_map < 1 || a->sp.topk_image < 1 || !(a->sp.temperature > 0.f)) return UMGEN_E_INVALID;
    const int B = a->B, n = a->j1 - a->j0;
    for (int b = 0; b < B; ++b) {
        const int32_t* tk = a->tokens + (size_t)b * kTokPerFrame;
        if (!in_range(tk, kNPose, t->n_pose) || !in_range(tk + kOffMap, kNMap, t->n_map) || !in_range(tk + kOffBox, kNBox, t->n_box) ||
            !in_range(tk + kOffImg, kNImg, t->n_img))
            return UMGEN_E_INVALID;
        if (a->use_forced) {
            const int32_t* ft = a->forced + (size_t)b * kTokPerFrame;
            if (!in_range(ft, kNPose, t->n_pose)) return UMGEN_E_INVALID;
            if (!in_range(ft + kOffMap, kNMap, t->n_map) || !in_range(ft + kOffBox, kNBox, t->n_box) || !in_range(ft + kOffImg, kNImg, t->n_img)) return UMGEN_E_INVALID;
        }
        if (a->n_boxes[b] < 0 || a->n_boxes[b] > 30) return UMGEN_E_INVALID;     // the kernel's box list and corner table hold 64
    }
    const size_t E = (size_t)t->E, cn = (size_t)B * kSeq * E, ln = (size_t)B * a->ld_logits, tarn = (size_t)B * kNBox * t->n_box, tn = (size_t)B * kTokPerFrame;
    const size_t bn = (size_t)B * 64 * 10;
    TablesDev td(*t);
    DevBuf dSt(sizeof(OarState)), dC(cn * 4), dLg(ln * 4), dTar(tarn * 4), dPrev((size_t)B * kNBox * 4), dCtl((size_t)B * kSlots), dF(tn * 4), dSeed((size_t)B * 8);
    GuardedBuf dXn((size_t)B * E * 4), dTok(tn * 4), dCnt(8 * 4), dNb((size_t)B * 4), dBx(bn * 8);
    if (!td.ok || !dSt.p || !dC.p || !dLg.p || !dTar.p || !dPrev.p || !dCtl.p || !dF.p || !dSeed.p || !dXn.p || !dTok.p || !dCnt.p || !dNb.p || !dBx.p)
        return UMGEN_E_NOMEM;
    OarState s0{};
    s0.step = a->j0; s0.frame_idx = a->frame_idx; s0.use_forced = a->use_forced ? 1 : 0; s0.use_control = a->use_control ? 1 : 0; s0.done = 0;
    s0.epoch = a->epoch0; s0.sp = a->sp;
    if (up(dSt.p, &s0, sizeof(s0)) || up(dC.p, a->cond, cn * 4) || up(dTar.p, a->logits_tar, tarn * 4) || up(dPrev.p, a->prev_box, (size_t)B * kNBox * 4) ||
        up(dCtl.p, a->control_slot, (size_t)B * kSlots) || up(dSeed.p, a->seeds, (size_t)B * 8) || up(dTok.p, a->tokens, tn * 4) ||
        up(dCnt.p, a->counters, 8 * 4) || up(dNb.p, a->n_boxes, (size_t)B * 4) || up(dBx.p, a->boxes, bn * 8) || (a->use_forced && up(dF.p, a->forced, tn * 4)))
        return UMGEN_E_HIP;
    SampleArgs sa{};
    sa.st = (OarState*)dSt.p; sa.tb = td.tb; sa.logits = (const float*)dLg.p; sa.logits_tar = (const float*)dTar.p; sa.ld_logits = a->ld_logits;
    sa.ld_tar = t->n_box; sa.cond = (const float*)dC.p; sa.x_next = (float*)dXn.p; sa.tokens = (int*)dTok.p; sa.prev_box = (const int*)dPrev.p;
    sa.control_slot = (const unsigned char*)dCtl.p; sa.boxes = (double*)dBx.p; sa.n_boxes = (int*)dNb.p; sa.seeds = (const unsigned long long*)dSeed.p;
    sa.forced = (const int*)dF.p; sa.counters = (int*)dCnt.p;
    for (int i = 0; i < n; ++i) {
        const int j = a->j0 + i, mod = kind_of_pos(j, a->given_end);
        if (fill_nan32(dXn.p, (size_t)B * E)) return UMGEN_E_HIP;
        if (mod == 0) {
            launch_fixed_token(nullptr, sa, B);
        } else {
            if (up(dLg.p, a->logits + (size_t)i * ln, ln * 4)) return UMGEN_E_HIP;
            sa.mod = mod;
            sa.vocab = mod == 1 ? t->n_map : (mod == 2 ? t->n_box : t->n_img);
            launch_sample_token(nullptr, sa, B);
        }
        if (int rc = finish()) return rc;
        OarState s1{};
        if (down(&s1, dSt.p, sizeof(s1)) || down(a->x_next + (size_t)i * B * E, dXn.p, (size_t)B * E * 4)) return UMGEN_E_HIP;
        a->state_log[3 * i] = (uint32_t)s1.step; a->state_log[3 * i + 1] = s1.epoch; a->state_log[3 * i + 2] = (uint32_t)s1.done;
    }
    if (!dXn.intact() || !dTok.intact() || !dCnt.intact() || !dNb.intact() || !dBx.intact()) return UMGEN_E_STATE;
    if (down(a->tokens, dTok.p, tn * 4) || down(a->counters, dCnt.p, 8 * 4) || down(a->n_boxes, dNb.p, (size_t)B * 4)) return UMGEN_E_HIP;
    return down(a->boxes, dBx.p, bn * 8);
}

// launch_sample_ego: logits [3 B][V] -> out_tokens [B][3]; the draw of row (b, jq) is rng_uniform(seeds[b], frame_idx, kSeq + jq, DRAW_MAIN); forced
// [B][2199] (or NULL) overrides with its pose tokens
int umgen_dbg_sample_ego(const float* logits, int V, const SamplerParams* sp, const uint64_t* seeds, int frame_idx, const int32_t* forced, int B,
                         int32_t* out_tokens) {
    if (!logits || !sp || !seeds || !out_tokens || B < 1 || V < 1 || V > 8192 || sp->method < 0 || sp->method > 1 || sp->top_k < 1 || !(sp->temperature > 0.f))
        return UMGEN_E_INVALID;
    const size_t ln = (size_t)B * 3 * V, tn = (size_t)B * kTokPerFrame;
    DevBuf dL(ln * 4), dS((size_t)B * 8), dF(tn * 4), dOv(4);
    GuardedBuf dT((size_t)B * 3 * 4);
    if (!dL.p || !dS.p || !dF.p || !dOv.p || !dT.p) return UMGEN_E_NOMEM;
    if (up(dL.p, logits, ln * 4) || up(dS.p, seeds, (size_t)B * 8) || (forced && up(dF.p, forced, tn * 4)) || hipMemset(dOv.p, 0, 4) != hipSuccess ||
        hipMemset(dT.p, 0xff, (size_t)B * 3 * 4) != hipSuccess)
        return UMGEN_E_HIP;
    launch_sample_ego(nullptr, (const float*)dL.p, V, *sp, (const unsigned long long*)dS.p, frame_idx, forced ? (const int*)dF.p : nullptr, (int*)dT.p, B, (int*)dOv.p);
    if (int rc = finish()) return rc;
    int ovf = 0;
    if (down(&ovf, dOv.p, 4)) return UMGEN_E_HIP;
    if (!dT.intact() || ovf != 0) return UMGEN_E_STATE;      // (the overflow word is unused since the exhaustive tie walk: it must stay 0)
    return down(out_tokens, dT.p, (size_t)B * 3 * 4);
}

}  // extern "C"
