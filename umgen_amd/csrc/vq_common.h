// What the VQ decoder (vqdec.hip) and the VQ encoder (vqenc.hip) share: the building blocks of projects/tokenizer/vq_modules.py
// (ResnetBlock / AttnBlock / Normalize / nonlinearity, vq_modules.py:14-22, 63-176) on channels-last fp32 activations, the
// state-dict slots both handles fill, and the one-frame workspace they run in.
//
// Layout: activations are channels-last fp32 [pixel][channel] (one frame at a time), so every convolution is ONE GEMM of this
// library: a 3 x 3 convolution = im2col ([pixel][9 C_in], zero padded) x the repacked kernel [C_out][(ky, kx, c_in)], a 1 x 1
// convolution = the GEMM on the activation rows themselves; the residual add of a ResnetBlock is the GEMM's residual epilogue.
// Arithmetic: exact fp32 FMA chains (launch_gemm_valu<float, float>), fp32 GroupNorm statistics, expf-based sigmoid / softmax.
// The attention block (single head of C channels over H*W positions) is three GEMMs + a row softmax.
//
// Kernels and host helpers are internal to each translation unit that includes this header (anonymous namespace / static).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/umgen.h"
#include "kernels.h"

namespace umgen {
namespace vqc {

struct Conv { float* w = nullptr; float* b = nullptr; int cin = 0, cout = 0, cout_pad = 0, ks = 0, pad = 0; bool loaded_w = false, loaded_b = false; int cin_src = 0; };   // cout_pad: rows of w / b (multiple of 4, zero rows behind cout: the GEMM epilogues write 4 features at a time); cin_src: input channels of the checkpoint's kernel (<= cin: the columns behind it stay zero)
struct Norm { float* g = nullptr; float* b = nullptr; int c = 0; bool loaded_g = false, loaded_b = false; };
struct Res { Norm n1, n2; Conv c1, c2, nin; bool has_nin = false; };
struct Attn { Norm n; Conv q, k, v, proj; };

// the part of a handle the shared helpers work on
struct Ctx {
    std::string err;
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;
    // what load_tensor fills: key -> (destination, expected shape, conv to repack or nullptr, flag)
    struct Slot { float* dst; std::vector<int64_t> shape; Conv* repack; bool* flag; };
    std::map<std::string, Slot> slots;
    bool finalized = false;
    // workspace (one frame)
    float *x = nullptr, *h = nullptr, *t = nullptr, *col = nullptr, *stats = nullptr, *scores = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr;

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

}  // namespace vqc
}  // namespace umgen

#define VQCHK(e, call)                                                                               \
    do {                                                                                             \
        hipError_t _err = (call);                                                                    \
        if (_err != hipSuccess) return (e)->fail(UMGEN_E_HIP, "%s -> %s", #call, hipGetErrorString(_err)); \
    } while (0)

namespace {

using namespace umgen;
using namespace umgen::vqc;

// ---------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------
// col[p][(ky * KS + kx) * C + c] = x[y + ky - pad][x + kx - pad][c]   (zero outside), KS x KS kernel, stride 1
__global__ void vq_im2col_kernel(const float* __restrict__ x, int H, int W, int C, int KS, int pad, float* __restrict__ col) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // one float4 of 4 channels
    const int C4 = C >> 2;
    const long total = (long)H * W * KS * KS * C4;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const long r = i / C4;
    const int kk = (int)(r % (KS * KS));
    const long p = r / (KS * KS);
    const int px = (int)(p % W), py = (int)(p / W);
    const int sy = py + kk / KS - pad, sx = px + kk % KS - pad;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (sy >= 0 && sy < H && sx >= 0 && sx < W) v = reinterpret_cast<const float4*>(x + ((long)sy * W + sx) * C)[c4];
    reinterpret_cast<float4*>(col + (p * KS * KS + kk) * C)[c4] = v;
}

// GroupNorm(32 groups, eps 1e-6, affine) statistics of one frame: stats[g] = (mean, rstd) over H*W x (C/32) values
__global__ __launch_bounds__(256) void vq_gn_stats_kernel(const float* __restrict__ x, long n_px, int C, float* __restrict__ stats) {
    __shared__ double s_sum[4], s_sq[4];
    const int g = blockIdx.x, cg = C / 32;
    const long n = n_px * cg;
    double sum = 0.0, sq = 0.0;      // (torch accumulates GroupNorm statistics in a wider type on the CPU too)
    for (long i = threadIdx.x; i < n; i += 256) {
        const float v = x[(i / cg) * C + g * cg + (i % cg)];
        sum += v;
        sq += (double)v * v;
    }
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o); sq += __shfl_xor(sq, o); }
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = sum; s_sq[threadIdx.x >> 6] = sq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3], q = s_sq[0] + s_sq[1] + s_sq[2] + s_sq[3];
        const double mean = s / (double)n;
        const double var = q / (double)n - mean * mean;
        stats[2 * g] = (float)mean;
        stats[2 * g + 1] = (float)(1.0 / sqrt(var + 1e-6));
    }
}
// y = GroupNorm(x) * gamma + beta, optionally followed by x * sigmoid(x) (nonlinearity, vq_modules.py:14-16)
__global__ void vq_gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, long n_px, int C, int swish, float* __restrict__ y) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px * C) return;
    const int c = (int)(i % C), g = c / (C / 32);
    float v = (x[i] - stats[2 * g]) * stats[2 * g + 1] * gamma[c] + beta[c];
    if (swish) v = v / (1.0f + expf(-v));
    y[i] = v;
}

// row softmax of the attention scores: w[i][:] = softmax(s[i][:] * scale)  (AttnBlock, vq_modules.py:158-160); one wave per row of
// n scores, rows ld floats apart (columns n .. ld - 1 are left alone)
__global__ __launch_bounds__(256) void vq_softmax_kernel(float* __restrict__ s, int n, int ld, float scale) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    float* r = s + (long)row * ld;
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) mx = fmaxf(mx, r[j] * scale);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < n; j += 64) { const float e = expf(r[j] * scale - mx); r[j] = e; sum += e; }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    for (int j = lane; j < n; j += 64) r[j] *= inv;
}

// nearest-neighbour x2 upsampling (F.interpolate(scale_factor=2, mode="nearest")), channels last
__global__ void vq_upsample_kernel(const float* __restrict__ x, int H, int W, int C, float* __restrict__ y) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int C4 = C >> 2;
    const long total = (long)4 * H * W * C4;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const long p = i / C4;
    const int ox = (int)(p % (2 * W)), oy = (int)(p / (2 * W));
    reinterpret_cast<float4*>(y + p * C)[c4] = reinterpret_cast<const float4*>(x + ((long)(oy >> 1) * W + (ox >> 1)) * C)[c4];
}

// out[c][p] (channels first, the reference's output layout) = x[p][c]
__global__ void vq_to_nchw_kernel(const float* __restrict__ x, long n_px, int C, int ldx, float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px * C) return;
    const long p = i % n_px;
    const int c = (int)(i / n_px);
    out[i] = x[p * ldx + c];
}

// y[p][c] = x[c][p] for c < C_in, 0 for the pad lanes C_in <= c < C (C a multiple of 4: the im2col kernels move float4s)
__global__ void vq_from_nchw_kernel(const float* __restrict__ x, long n_px, int C_in, int C, float* __restrict__ y) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px * C) return;
    const long p = i / C;
    const int c = (int)(i % C);
    y[i] = c < C_in ? x[(long)c * n_px + p] : 0.f;
}

// Downsample: col[(oy, ox)][(ky * 3 + kx) * C + c] = x[2 oy + ky][2 ox + kx][c], zero where that is the pad column right of the
// frame or the pad row below it (F.pad(x, (0, 1, 0, 1)), then a 3 x 3 stride-2 convolution without padding).  H, W even.
__global__ void vq_im2col_s2_kernel(const float* __restrict__ x, int H, int W, int C, float* __restrict__ col) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // one float4 of 4 channels
    const int C4 = C >> 2, Ho = H >> 1, Wo = W >> 1;
    const long total = (long)Ho * Wo * 9 * C4;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const long r = i / C4;
    const int kk = (int)(r % 9);
    const long p = r / 9;
    const int ox = (int)(p % Wo), oy = (int)(p / Wo);
    const int sy = 2 * oy + kk / 3, sx = 2 * ox + kk % 3;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (sy < H && sx < W) v = reinterpret_cast<const float4*>(x + ((long)sy * W + sx) * C)[c4];
    reinterpret_cast<float4*>(col + (p * 9 + kk) * C)[c4] = v;
}

// e2[n] = |e_n|^2 of every codebook row (once, at finalize)
__global__ void vq_code_norms_kernel(const float* __restrict__ emb, int N, int D, float* __restrict__ e2) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int c = 0; c < D; ++c) s = fmaf(emb[(long)n * D + c], emb[(long)n * D + c], s);
    e2[n] = s;
}

// NormEMAVectorQuantizer.forward up to the arg-min (quantize.py:417-429): one wave per token position.
//   z = row / max(|row|_2, 1e-12);   d_n = |z|^2 + |e_n|^2 - 2 z.e_n  (three terms, fp32);   code = first n with the smallest d_n
// The codebook streams through LDS in tiles of `tile` rows (row stride D + 4 floats: a lane's float4 reads of its own row then
// spread over the banks); lane l of a wave looks at rows l, l + 64, ... of every tile in ascending order and keeps the first
// minimum, the wave reduction keeps the lower index on equal distance: torch.argmin's answer.  4 positions per workgroup.
constexpr int kQuantMaxD = 64;
__global__ __launch_bounds__(256) void vq_quantize_kernel(const float* __restrict__ h, int ldh, const float* __restrict__ emb,
                                                          const float* __restrict__ e2, int N, int D, int tile, long n_pos,
                                                          long long* __restrict__ codes, float* __restrict__ zn) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int LD = D + 4;
    float* sE = smem;                        // [tile][LD]
    float* sE2 = sE + (long)tile * LD;       // [tile]
    float* sZ = sE2 + tile;                  // [4][kQuantMaxD]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long pos = (long)blockIdx.x * 4 + wave;
    const bool live = pos < n_pos;           // (every wave stays for the barriers below)
    float zz = 0.f;
    if (live) {
        const float* row = h + pos * ldh;
        float ss = 0.f;
        for (int c = 0; c < D; ++c) ss = fmaf(row[c], row[c], ss);
        const float den = fmaxf(sqrtf(ss), 1e-12f);                       // F.normalize(p=2, dim=-1, eps=1e-12)
        if (lane < D) {
            const float v = row[lane] / den;
            sZ[wave * kQuantMaxD + lane] = v;
            zn[pos * D + lane] = v;
        }
    }
    __syncthreads();
    if (live)
        for (int c = 0; c < D; ++c) zz = fmaf(sZ[wave * kQuantMaxD + c], sZ[wave * kQuantMaxD + c], zz);
    float best = INFINITY;
    int best_n = 0x7fffffff;
    const int D4 = D >> 2;
    for (int n0 = 0; n0 < N; n0 += tile) {
        const int rows = min(tile, N - n0);
        for (int i = threadIdx.x; i < rows * D4; i += 256) {
            const int r = i / D4, c4 = i % D4;
            *reinterpret_cast<float4*>(sE + r * LD + 4 * c4) = reinterpret_cast<const float4*>(emb + (long)(n0 + r) * D)[c4];
        }
        for (int i = threadIdx.x; i < rows; i += 256) sE2[i] = e2[n0 + i];
        __syncthreads();
        if (live)
            for (int r = lane; r < rows; r += 64) {
                float dot = 0.f;
                for (int c4 = 0; c4 < D4; ++c4) {
                    const float4 ev = *reinterpret_cast<const float4*>(sE + r * LD + 4 * c4);
                    const float4 zv = *reinterpret_cast<const float4*>(sZ + wave * kQuantMaxD + 4 * c4);
                    dot = fmaf(zv.x, ev.x, dot); dot = fmaf(zv.y, ev.y, dot); dot = fmaf(zv.z, ev.z, dot); dot = fmaf(zv.w, ev.w, dot);
                }
                const float d = (zz + sE2[r]) - 2.0f * dot;
                if (d < best) { best = d; best_n = n0 + r; }             // ascending n per lane: the first minimum stays
            }
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(best, o);
        const int on = __shfl_xor(best_n, o);
        if (od < best || (od == best && on < best_n)) { best = od; best_n = on; }
    }
    if (live && lane == 0) codes[pos] = best_n == 0x7fffffff ? 0 : best_n;     // (no row compared below +inf: only a non-finite z)
}

inline dim3 grid1d(long n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }

// the one launch of each kernel above (the handles and the test hooks of debug_vq.hip go through these)
inline void launch_im2col(hipStream_t s, const float* x, int H, int W, int C, int KS, int pad, float* col) {
    hipLaunchKernelGGL(vq_im2col_kernel, grid1d((long)H * W * KS * KS * (C / 4)), dim3(256), 0, s, x, H, W, C, KS, pad, col);
}
inline void launch_im2col_s2(hipStream_t s, const float* x, int H, int W, int C, float* col) {
    hipLaunchKernelGGL(vq_im2col_s2_kernel, grid1d((long)(H / 2) * (W / 2) * 9 * (C / 4)), dim3(256), 0, s, x, H, W, C, col);
}
inline void launch_upsample(hipStream_t s, const float* x, int H, int W, int C, float* y) {
    hipLaunchKernelGGL(vq_upsample_kernel, grid1d((long)4 * H * W * (C / 4)), dim3(256), 0, s, x, H, W, C, y);
}
inline void launch_from_nchw(hipStream_t s, const float* x, long n_px, int C_in, int C, float* y) {
    hipLaunchKernelGGL(vq_from_nchw_kernel, grid1d(n_px * C), dim3(256), 0, s, x, n_px, C_in, C, y);
}
inline void launch_to_nchw(hipStream_t s, const float* x, long n_px, int C, int ldx, float* out) {
    hipLaunchKernelGGL(vq_to_nchw_kernel, grid1d(n_px * C), dim3(256), 0, s, x, n_px, C, ldx, out);
}
// softmax(scores * C^-0.5) over the n columns of n rows, ld floats apart: int(c) ** (-0.5)
inline void launch_softmax(hipStream_t s, float* scores, int n, int ld, int C) {
    hipLaunchKernelGGL(vq_softmax_kernel, dim3((n + 3) / 4), dim3(256), 0, s, scores, n, ld, 1.0f / sqrtf((float)C));
}
inline void launch_code_norms(hipStream_t s, const float* emb, int N, int D, float* e2) {
    hipLaunchKernelGGL(vq_code_norms_kernel, grid1d(N), dim3(256), 0, s, emb, N, D, e2);
}
// codebook tile of the quantiser: at most 512 rows and 40 KB of LDS, a multiple of 64 rows
inline int quant_tile(int D) { return std::max(64, std::min(512, (10240 / (D + 4)) & ~63)); }
inline size_t quant_lds(int D) { return ((size_t)quant_tile(D) * (D + 4) + quant_tile(D) + 4 * kQuantMaxD) * sizeof(float); }
inline void launch_quantize(hipStream_t s, const float* h, int ldh, const float* emb, const float* e2, int N, int D, long n_pos, long long* codes, float* zn) {
    hipLaunchKernelGGL(vq_quantize_kernel, dim3((unsigned)((n_pos + 3) / 4)), dim3(256), quant_lds(D), s, h, ldh, emb, e2, N, D, quant_tile(D), n_pos, codes, zn);
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
int vq_alloc(Ctx* e, float** p, size_t n) {
    VQCHK(e, hipMalloc(reinterpret_cast<void**>(p), (n ? n : 4) * sizeof(float)));
    e->allocs.push_back(*p);
    return 0;
}
// cin_src: input channels of the checkpoint's kernel when the activations carry zero pad lanes behind them (0: cin)
int reg_conv(Ctx* e, const std::string& key, Conv& c, int cin, int cout, int ks, int pad, int cin_src = 0) {
    c.cin = cin; c.cout = cout; c.cout_pad = (cout + 3) & ~3; c.ks = ks; c.pad = pad; c.cin_src = cin_src ? cin_src : cin;
    if (int rc = vq_alloc(e, &c.w, (size_t)c.cout_pad * cin * ks * ks)) return rc;
    if (int rc = vq_alloc(e, &c.b, (size_t)c.cout_pad)) return rc;
    VQCHK(e, hipMemset(c.w, 0, (size_t)c.cout_pad * cin * ks * ks * 4));
    VQCHK(e, hipMemset(c.b, 0, (size_t)c.cout_pad * 4));
    e->slots[key + ".weight"] = Ctx::Slot{c.w, {cout, c.cin_src, ks, ks}, &c, &c.loaded_w};
    e->slots[key + ".bias"] = Ctx::Slot{c.b, {cout}, nullptr, &c.loaded_b};
    return 0;
}
int reg_norm(Ctx* e, const std::string& key, Norm& n, int c) {
    n.c = c;
    if (int rc = vq_alloc(e, &n.g, (size_t)c)) return rc;
    if (int rc = vq_alloc(e, &n.b, (size_t)c)) return rc;
    e->slots[key + ".weight"] = Ctx::Slot{n.g, {c}, nullptr, &n.loaded_g};
    e->slots[key + ".bias"] = Ctx::Slot{n.b, {c}, nullptr, &n.loaded_b};
    return 0;
}
int reg_res(Ctx* e, const std::string& key, Res& r, int cin, int cout) {
    if (int rc = reg_norm(e, key + ".norm1", r.n1, cin)) return rc;
    if (int rc = reg_conv(e, key + ".conv1", r.c1, cin, cout, 3, 1)) return rc;
    if (int rc = reg_norm(e, key + ".norm2", r.n2, cout)) return rc;
    if (int rc = reg_conv(e, key + ".conv2", r.c2, cout, cout, 3, 1)) return rc;
    r.has_nin = cin != cout;
    if (r.has_nin) { if (int rc = reg_conv(e, key + ".nin_shortcut", r.nin, cin, cout, 1, 0)) return rc; }
    return 0;
}
int reg_attn(Ctx* e, const std::string& key, Attn& a, int c) {
    if (int rc = reg_norm(e, key + ".norm", a.n, c)) return rc;
    if (int rc = reg_conv(e, key + ".q", a.q, c, c, 1, 0)) return rc;
    if (int rc = reg_conv(e, key + ".k", a.k, c, c, 1, 0)) return rc;
    if (int rc = reg_conv(e, key + ".v", a.v, c, c, 1, 0)) return rc;
    return reg_conv(e, key + ".proj_out", a.proj, c, c, 1, 0);
}

// one state-dict entry into its slot (1: not a key of this handle); convolution kernels are repacked to the im2col column order
int load_slot(Ctx* e, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
    auto it = e->slots.find(key);
    if (it == e->slots.end()) return 1;
    Ctx::Slot& s = it->second;
    if ((size_t)ndim != s.shape.size()) return e->fail(UMGEN_E_INVALID, "%s: ndim %d, expected %zu", key, ndim, s.shape.size());
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] != s.shape[i]) return e->fail(UMGEN_E_INVALID, "%s: dim %d is %lld, expected %lld", key, i, (long long)shape[i], (long long)s.shape[i]);
        n *= (size_t)shape[i];
    }
    if (s.repack && (s.repack->ks > 1 || s.repack->cin_src != s.repack->cin)) {     // [C_out][C_in][ky][kx] -> [C_out][(ky, kx, c_in)]: the im2col column order
        const Conv& c = *s.repack;
        const int kk = c.ks * c.ks;
        std::vector<float> r((size_t)c.cout * kk * c.cin, 0.f);
        for (int o = 0; o < c.cout; ++o)
            for (int i = 0; i < c.cin_src; ++i)
                for (int k = 0; k < kk; ++k) r[((size_t)o * kk + k) * c.cin + i] = data[((size_t)o * c.cin_src + i) * kk + k];
        VQCHK(e, hipMemcpy(s.dst, r.data(), r.size() * 4, hipMemcpyHostToDevice));
    } else {
        VQCHK(e, hipMemcpy(s.dst, data, n * 4, hipMemcpyHostToDevice));
    }
    *s.flag = true;
    e->finalized = false;
    return UMGEN_OK;
}
// UMGEN_E_STATE while a slot is still empty
int check_slots(Ctx* e, const char* what) {
    int nmiss = 0;
    std::string first;
    for (auto& kv : e->slots)
        if (!*kv.second.flag) { if (!nmiss) first = kv.first; ++nmiss; }
    if (nmiss) return e->fail(UMGEN_E_STATE, "%d %s tensors not loaded (e.g. %s)", nmiss, what, first.c_str());
    return UMGEN_OK;
}

// out[p][cout] (= or +=) sum_k act[p][k] w[cout][k] + bias: the GEMM behind every convolution (act: activation rows or im2col rows)
void conv_gemm(Ctx* e, const Conv& c, const float* act, int K, long n_px, float* out, bool residual) {
    GemmArgs g{};
    g.P = c.w; g.Q = act; g.Mi = c.cout_pad; g.Nj = (int)n_px; g.K = K; g.ldp = K; g.ldq = K; g.batch = 1;
    g.mode = residual ? GEMM_RESID : GEMM_STORE; g.bias = c.b; g.out = out; g.ldo = c.cout_pad;
    launch_gemm_valu<float, float>(e->stream, g);
}
// out[p][cout] (= or +=) conv(x)[p][cout] + bias, stride 1
void conv(Ctx* e, const Conv& c, const float* x, int H, int W, float* out, bool residual) {
    const long n_px = (long)H * W;
    const float* act = x;
    int K = c.cin;
    if (c.ks > 1) {
        launch_im2col(e->stream, x, H, W, c.cin, c.ks, c.pad, e->col);
        act = e->col;
        K = c.cin * c.ks * c.ks;
    }
    conv_gemm(e, c, act, K, n_px, out, residual);
}
void group_norm(Ctx* e, const Norm& n, const float* x, long n_px, bool swish, float* y) {
    hipLaunchKernelGGL(vq_gn_stats_kernel, dim3(32), dim3(256), 0, e->stream, x, n_px, n.c, e->stats);
    hipLaunchKernelGGL(vq_gn_apply_kernel, grid1d(n_px * n.c), dim3(256), 0, e->stream, x, e->stats, n.g, n.b, n_px, n.c, swish ? 1 : 0, y);
}
// ResnetBlock.forward (vq_modules.py:108-128), temb = None, dropout 0: x (in e->x, C_in) -> e->x (C_out)
void res_block(Ctx* e, const Res& r, int H, int W) {
    const long n_px = (long)H * W;
    group_norm(e, r.n1, e->x, n_px, true, e->h);
    conv(e, r.c1, e->h, H, W, e->t, false);
    group_norm(e, r.n2, e->t, n_px, true, e->h);
    if (r.has_nin) {
        conv(e, r.nin, e->x, H, W, e->t, false);      // x = nin_shortcut(x)
        std::swap(e->x, e->t);
    }
    conv(e, r.c2, e->h, H, W, e->x, true);            // x + conv2(h)
}
// AttnBlock.forward (vq_modules.py:150-176): x += proj_out(softmax(q k^T / sqrt(C)) v)
// The rows of the scores and of v^T are ld = n rounded up to 4 floats apart: the GEMM epilogues store 16 bytes at a time, and a row
// of n floats would start off that alignment whenever n is no multiple of 4 (the columns n .. ld - 1 are never read)
inline long attn_ld(long n) { return (n + 3) & ~3L; }
void attn_block(Ctx* e, const Attn& a, int H, int W) {
    const int n = H * W, C = a.n.c, ld = (int)attn_ld(n);
    group_norm(e, a.n, e->x, n, false, e->h);
    conv(e, a.q, e->h, H, W, e->q, false);
    conv(e, a.k, e->h, H, W, e->k, false);
    {   // v^T[c][j] = sum_k Wv[c][k] h[j][k] + bv[c]: channels-first so that it is the K-contiguous operand of the second product
        GemmArgs g{};
        g.P = e->h; g.Q = a.v.w; g.Mi = n; g.Nj = C; g.K = C; g.ldp = C; g.ldq = C; g.batch = 1;
        g.mode = GEMM_VT; g.bias = a.v.b; g.out = e->vt; g.ldo = ld; g.H = C / kHeadDim;   // (row index (j / 48) * 48 + j % 48 = j)
        launch_gemm_valu<float, float>(e->stream, g);
    }
    {   // scores[i][j] = sum_c q[i][c] k[j][c]
        GemmArgs g{};
        g.P = e->k; g.Q = e->q; g.Mi = n; g.Nj = n; g.K = C; g.ldp = C; g.ldq = C; g.batch = 1;
        g.mode = GEMM_STORE; g.out = e->scores; g.ldo = ld;
        launch_gemm_valu<float, float>(e->stream, g);
    }
    launch_softmax(e->stream, e->scores, n, ld, C);
    {   // h[i][c] = sum_j w[i][j] v^T[c][j]
        GemmArgs g{};
        g.P = e->vt; g.Q = e->scores; g.Mi = C; g.Nj = n; g.K = n; g.ldp = ld; g.ldq = ld; g.batch = 1;
        g.mode = GEMM_STORE; g.out = e->h; g.ldo = C;
        launch_gemm_valu<float, float>(e->stream, g);
    }
    conv(e, a.proj, e->h, H, W, e->x, true);
}

}  // namespace
