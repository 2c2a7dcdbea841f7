// Scoring a GIVEN frame (umgen_score, engine_score.hip run_score): log p(target) of many rows under one AR head without ever holding their logits.
//   head_nll_kernel     one workgroup = 16 rows x one split of the vocabulary.  Prologue: LayerNorm of the 16 rows (weight only, eps 1e-5, fp32
//                       two-pass statistics like gemv_ln_kernel), left in LDS -- in the 16-bit modes as the hi + lo 16-bit pairs the matrix cores
//                       consume (activations stay fp32-accurate, like rows_mfma_kernel: two MFMAs per k-step on the weights as stored), in fp32
//                       mode as fp32 rows for an FMA chain.  The split's vocabulary columns are swept in tiles of 16 (v_mfma_f32_16x16x32: 16
//                       head rows x 16 activation rows) or 4 (fp32: one wave, K over its lanes); every lane keeps the running (max, sum-exp,
//                       arg-max, target logit) of its activation row, folded at the end over the lanes of the row, the 4 waves and -- by
//                       nll_combine_kernel -- the splits, each in a fixed order.  One record of 16 bytes per (row, split) is all that reaches memory.
//   logits_nll_kernel   the same statistics for rows whose logits exist already (the ego head's three rows per scene, run_ego).
//   head_detail_kernel  umgen_score_detail's second sweep behind head_nll_kernel, through the same prologue and tile products (nll_ln_rows,
//                       nll_tile16, nll_cols4): rank, mass above, entropy and the 16 best tokens of every row; logits_detail_kernel likewise.
// A row's result is a function of its own values, V and K only: the split of V (head_nll_tiles_per_split) and every reduction order are fixed
// by (V, K), a row never mixes with its tile neighbours (the MFMA's columns do not mix), so M and the other rows of a launch do not matter.
#include "kernels.h"

namespace umgen {

namespace {

constexpr int kNllThreads = 256, kNllWaves = 4, kNllRows = 16;

// running statistics of one row over the columns seen so far
struct NllStat {
    float m, s, t;      // max logit; sum of exp(logit - m); the target's logit (-inf: not seen)
    int arg;            // lowest index among the maxima
};
__device__ inline NllStat nll_init() { return NllStat{-INFINITY, 0.f, -INFINITY, 0x7fffffff}; }
__device__ inline void nll_add(NllStat& st, float v, int n, int target) {
    if (v > st.m) {
        st.s = st.s * expf(st.m - v) + 1.f;
        st.m = v;
        st.arg = n;
    } else {
        st.s += expf(v - st.m);
    }
    if (n == target) st.t = v;
}
// a then b; the index sets may interleave
__device__ inline NllStat nll_merge(const NllStat& a, const NllStat& b) {
    NllStat o;
    o.m = fmaxf(a.m, b.m);
    const float ea = a.m == o.m ? 1.f : expf(a.m - o.m), eb = b.m == o.m ? 1.f : expf(b.m - o.m);
    o.s = a.s * ea + b.s * eb;
    o.arg = (b.m > a.m || (b.m == a.m && b.arg < a.arg)) ? b.arg : a.arg;
    o.t = fmaxf(a.t, b.t);
    return o;
}
__device__ inline NllStat nll_shfl_xor(const NllStat& a, int mask) {
    return NllStat{__shfl_xor(a.m, mask), __shfl_xor(a.s, mask), __shfl_xor(a.t, mask), __shfl_xor(a.arg, mask)};
}
__device__ inline void nll_finish(const NllStat& st, long r, float* logp, int* argmax, float* lse, float* tlogit, float* rmax = nullptr,
                                  float* sumexp = nullptr) {
    const float l = st.m + logf(st.s);
    if (logp) logp[r] = st.t - l;
    if (argmax) argmax[r] = st.arg;
    if (lse) lse[r] = l;
    if (tlogit) tlogit[r] = st.t;
    if (rmax) rmax[r] = st.m;
    if (sumexp) sumexp[r] = st.s;
}

__device__ inline const float* nll_row(const HeadNllArgs& a, int r) {
    return a.x + (long)(r / a.rows_per_group) * a.group_stride + (long)(r % a.rows_per_group) * a.ldx;
}
__device__ inline int nll_target(const HeadNllArgs& a, int r) {
    return a.target[(long)(r / a.rows_per_group) * a.target_group_stride + r % a.rows_per_group];
}

template <typename TT>
__device__ inline void nll_split8(const float (&v)[8], typename Mma16<TT>::vec& hi, typename Mma16<TT>::vec& lo) {
    typedef typename Mma16<TT>::elem elem;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const auto h = Cvt<TT>::from_f(v[e]);
        hi[e] = __builtin_bit_cast(elem, h);
        lo[e] = __builtin_bit_cast(elem, Cvt<TT>::from_f(v[e] - Cvt<TT>::to_f(h)));
    }
}

// LDS image of the 16 normalised rows, 64 K bytes in either form:
//   16-bit: [k-step s][hi | lo][64 lanes][8]: lane l of k-step s holds k = 32 s + 8 (l / 16) .. + 7 of row l % 16 -- the MFMA's B operand, one ds_read_b128
//   fp32:   [16 rows][K]
// nll_ln_rows writes it: LayerNorm of rows r0 .. r0 + 15 (rows >= M: zeros), 4 rows per wave, a lane owns the 8-value chunks lane, lane + 64, lane + 128
template <typename T>
__device__ inline void nll_ln_rows(const HeadNllArgs& a, int r0, unsigned char* nll_smem) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = a.K, M = a.M;
#pragma unroll 1
    for (int q = 0; q < kNllRows / kNllWaves; ++q) {
        const int rl = wave * (kNllRows / kNllWaves) + q, r = r0 + rl;
        const float* xr = nll_row(a, min(r, M - 1));
        float v[3][8];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int c = lane + 64 * i;
            if (8 * c < K && r < M) load8(xr + 8 * c, v[i]);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
            }
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[i][e];
        const float mean = wave_sum(s) / (float)K;
        float qq = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (8 * (lane + 64 * i) < K) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; qq += d * d; }
            }
        const float rstd = 1.0f / sqrtf(wave_sum(qq) / (float)K + 1e-5f);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int c = lane + 64 * i;
            if (8 * c < K) {
                float lw[8], y[8];
                load8(a.ln_w + 8 * c, lw);
#pragma unroll
                for (int e = 0; e < 8; ++e) y[e] = (v[i][e] - mean) * rstd * lw[e];
                if constexpr (sizeof(T) == 2) {
                    typedef typename Mma16<T>::vec vec;
                    vec hi, lo;
                    nll_split8<T>(y, hi, lo);
                    vec* f = reinterpret_cast<vec*>(nll_smem) + (long)(c >> 2) * 128 + (c & 3) * 16 + rl;
                    f[0] = hi;
                    f[64] = lo;
                } else {
                    float* xs = reinterpret_cast<float*>(nll_smem) + (long)rl * K + 8 * c;
                    *reinterpret_cast<float4*>(xs) = make_float4(y[0], y[1], y[2], y[3]);
                    *reinterpret_cast<float4*>(xs + 4) = make_float4(y[4], y[5], y[6], y[7]);
                }
            }
        }
    }
}

// one tile of the 16-bit sweep: head rows n0 .. n0 + 15 (clamped to V - 1) x the 16 activation rows of the LDS image; lane (col, kg) gets rows n0 + 4 kg .. + 3 of activation row col
template <typename T>
__device__ inline f32x4_t nll_tile16(const T* W, const typename Mma16<T>::vec* frag, int n0, int col, int kg, int K, int V) {
    typedef typename Mma16<T>::vec vec;
    const int nsteps = K >> 5;
    const T* wrow = W + (long)min(n0 + col, V - 1) * K + 8 * kg;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < nsteps; s0 += 3) {               // (K = 96, 768, 1536: 3, 24, 48 k-steps; three weight loads in flight)
        vec wf[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) wf[u] = *reinterpret_cast<const vec*>(wrow + 32 * (s0 + u));
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            acc = Mma16<T>::mfma(wf[u], frag[(long)(s0 + u) * 128], acc);
            acc = Mma16<T>::mfma(wf[u], frag[(long)(s0 + u) * 128 + 64], acc);
        }
    }
    return acc;
}

// the fp32 sweep's step: head rows g .. g + 3 (clamped to V - 1) x the 16 rows of the LDS image, K over the lanes; f(c, v): v is, in lane r < 16, row r's logit of head row g + c
template <typename F>
__device__ inline void nll_cols4(const float* W, const float* xs, int g, int K, int V, int lane, F&& f) {
    float acc[4][kNllRows];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < kNllRows; ++r) acc[c][r] = 0.f;
    for (int k = 4 * lane; k < K; k += 256) {
        float4 w[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = *reinterpret_cast<const float4*>(W + (long)min(g + c, V - 1) * K + k);
#pragma unroll
        for (int r = 0; r < kNllRows; ++r) {
            const float4 xv = *reinterpret_cast<const float4*>(xs + (long)r * K + k);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc[c][r] = fmaf(w[c].w, xv.w, fmaf(w[c].z, xv.z, fmaf(w[c].y, xv.y, fmaf(w[c].x, xv.x, acc[c][r]))));
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float mine = 0.f;
#pragma unroll
        for (int r = 0; r < kNllRows; ++r) {
            const float tot = wave_sum(acc[c][r]);
            mine = lane == r ? tot : mine;
        }
        f(c, mine);
    }
}

template <typename T>
__global__ __launch_bounds__(kNllThreads) void head_nll_kernel(HeadNllArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nll_smem[];
    __shared__ NllStat s_st[kNllWaves][kNllRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, V = a.V, M = a.M;
    const int split = blockIdx.x, r0 = blockIdx.y * kNllRows;
    nll_ln_rows<T>(a, r0, nll_smem);
    __syncthreads();
    // ---- the split's columns
    const int ntiles = (V + 15) / 16, tps = head_nll_tiles_per_split(V);
    const int t0 = split * tps, t1 = min(ntiles, t0 + tps);
    const T* W = reinterpret_cast<const T*>(a.W);
    NllStat st = nll_init();
    if constexpr (sizeof(T) == 2) {
        typedef typename Mma16<T>::vec vec;
        const int col = lane & 15, kg = lane >> 4;                 // activation row of this lane's results; its k-group / its 4 head rows of a tile
        const int target = r0 + col < M ? nll_target(a, r0 + col) : -1;
        const vec* frag = reinterpret_cast<const vec*>(nll_smem) + lane;
        for (int t = t0 + wave; t < t1; t += kNllWaves) {
            const int n0 = 16 * t;
            const f32x4_t acc = nll_tile16<T>(W, frag, n0, col, kg, K, V);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 4 * kg + r;
                if (n < V) nll_add(st, acc[r], n, target);         // (pad columns of the last tile never enter)
            }
        }
        st = nll_merge(st, nll_shfl_xor(st, 16));                  // the 4 k-groups of a row: (0 + 1) + (2 + 3)
        st = nll_merge(st, nll_shfl_xor(st, 32));
    } else {
        const int target = (lane < kNllRows && r0 + lane < M) ? nll_target(a, r0 + lane) : -1;   // lane r keeps row r
        const float* xs = reinterpret_cast<const float*>(nll_smem);
        const int c1 = min(V, 16 * t1);
        for (int g = 16 * t0 + 4 * wave; g < c1; g += 4 * kNllWaves) {      // 4 head rows per wave and pass, K over the lanes
            nll_cols4(W, xs, g, K, V, lane, [&](int c, float mine) {
                if (g + c < V && lane < kNllRows) nll_add(st, mine, g + c, target);
            });
        }
    }
    if (lane < kNllRows) s_st[wave][lane] = st;
    __syncthreads();
    if (tid < kNllRows && r0 + tid < M) {
        NllStat o = s_st[0][tid];
#pragma unroll
        for (int w = 1; w < kNllWaves; ++w) o = nll_merge(o, s_st[w][tid]);
        reinterpret_cast<float4*>(a.part)[(long)(r0 + tid) * gridDim.x + split] = make_float4(o.m, o.s, o.t, __int_as_float(o.arg));
    }
}

__global__ __launch_bounds__(256) void nll_combine_kernel(const float4* __restrict__ part, int M, int ns, float* logp, int* argmax, float* lse,
                                                          float* tlogit, float* rmax, float* sumexp) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    NllStat o = nll_init();
    for (int s = 0; s < ns; ++s) {
        const float4 p = part[(long)r * ns + s];
        o = nll_merge(o, NllStat{p.x, p.y, p.z, __float_as_int(p.w)});
    }
    nll_finish(o, r, logp, argmax, lse, tlogit, rmax, sumexp);
}

// one wave per row of given logits
__global__ __launch_bounds__(256) void logits_nll_kernel(const float* __restrict__ logits, long ld, int V, int M, const int* __restrict__ target,
                                                         int rows_per_group, long target_group_stride, float* logp, int* argmax, float* lse, float* tlogit) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const int tg = target[(long)(r / rows_per_group) * target_group_stride + r % rows_per_group];
    const float* lg = logits + (long)r * ld;
    NllStat st = nll_init();
    for (int n = lane; n < V; n += 64) nll_add(st, lg[n], n, tg);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) st = nll_merge(st, nll_shfl_xor(st, off));
    if (lane == 0) nll_finish(st, r, logp, argmax, lse, tlogit);
}


// ---- score diagnostics (umgen_score_detail): the second sweep, with the row's maximum m and target logit t known from the first ----
// Per row: the count of logits strictly above t; A = sum over those of exp((v - m) / tau); Z = the same sum over all; U = sum exp(v - m) (v - m);
// the kScoreTopK best (logit, index) pairs.  Nothing is rescaled (m is final), so every level folds by plain sums and list merges in a fixed order.
struct DetStat { int cnt; float A, Z, U; };
struct TopList { float v[kScoreTopK]; int i[kScoreTopK]; };      // descending; equal logits by ascending index; (-inf, INT_MAX): empty
constexpr int kTopEmpty = 0x7fffffff;

__device__ inline bool top_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
__device__ inline void top_init(TopList& L) {
#pragma unroll
    for (int k = 0; k < kScoreTopK; ++k) { L.v[k] = -INFINITY; L.i[k] = kTopEmpty; }
}
// an unrolled compare-and-select chain over registers: entry k takes its upper neighbour, the new pair or stays
__device__ inline void top_insert(TopList& L, float v, int n) {
    if (!top_before(v, n, L.v[kScoreTopK - 1], L.i[kScoreTopK - 1])) return;
#pragma unroll
    for (int k = kScoreTopK - 1; k > 0; --k) {
        const bool up = top_before(v, n, L.v[k - 1], L.i[k - 1]), here = top_before(v, n, L.v[k], L.i[k]);
        L.v[k] = up ? L.v[k - 1] : here ? v : L.v[k];
        L.i[k] = up ? L.i[k - 1] : here ? n : L.i[k];
    }
    if (top_before(v, n, L.v[0], L.i[0])) { L.v[0] = v; L.i[0] = n; }
}
__device__ inline void det_add(DetStat& d, TopList& L, float v, int n, float m, float t, float inv_tau) {
    const float c = v - m, e1 = expf(c), ez = expf(c * inv_tau);
    d.U += e1 > 0.f ? e1 * c : 0.f;
    d.Z += ez;
    if (v > t) { d.cnt += 1; d.A += ez; }
    top_insert(L, v, n);
}
// this lane's (d, L) with those of lane ^ mask; both lanes end with the same result (the pairs of two lanes differ in their indices)
__device__ inline void det_fold_xor(DetStat& d, TopList& L, int mask) {
    d.cnt += __shfl_xor(d.cnt, mask);
    d.A += __shfl_xor(d.A, mask);
    d.Z += __shfl_xor(d.Z, mask);
    d.U += __shfl_xor(d.U, mask);
    TopList o = L;                                                 // the partner's pairs arrive best first: take its head, shift, 16 times
#pragma unroll 1
    for (int k = 0; k < kScoreTopK; ++k) {
        top_insert(L, __shfl_xor(o.v[0], mask), __shfl_xor(o.i[0], mask));
#pragma unroll
        for (int j = 0; j + 1 < kScoreTopK; ++j) { o.v[j] = o.v[j + 1]; o.i[j] = o.i[j + 1]; }
    }
}
// l, s: the row's log-sum-exp and sum exp(v - m) of the first pass; a listed token's log-probability is formed like logp (nll_finish)
__device__ inline void det_finish(const DetStat& d, const TopList& L, float l, float s, long r, const ScoreDetailOut& o) {
    if (o.rank) o.rank[r] = d.cnt;
    if (o.mass_above) o.mass_above[r] = d.A / d.Z;
    if (o.entropy) o.entropy[r] = logf(s) - d.U / s;
#pragma unroll
    for (int k = 0; k < kScoreTopK; ++k)
        if (k < o.topk) {
            const bool empty = L.i[k] == kTopEmpty;
            if (o.topk_tok) o.topk_tok[r * o.topk + k] = empty ? -1 : L.i[k];
            if (o.topk_logp) o.topk_logp[r * o.topk + k] = empty ? -INFINITY : L.v[k] - l;
        }
}

// head_nll_kernel's geometry, prologue and tile products (so the logits are the first pass's bits); one record of kDetailRecFloats floats per (row, split)
template <typename T>
__global__ __launch_bounds__(kNllThreads) void head_detail_kernel(HeadDetailArgs da) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nll_smem[];
    __shared__ DetStat s_d[kNllWaves][kNllRows];
    __shared__ float s_v[kNllWaves][kScoreTopK][kNllRows];
    __shared__ int s_i[kNllWaves][kScoreTopK][kNllRows];
    const HeadNllArgs& a = da.h;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, V = a.V, M = a.M;
    const int split = blockIdx.x, r0 = blockIdx.y * kNllRows;
    const float inv_tau = da.out.inv_temperature;
    nll_ln_rows<T>(a, r0, nll_smem);
    __syncthreads();
    const int ntiles = (V + 15) / 16, tps = head_nll_tiles_per_split(V);
    const int t0 = split * tps, t1 = min(ntiles, t0 + tps);
    const T* W = reinterpret_cast<const T*>(a.W);
    DetStat d{0, 0.f, 0.f, 0.f};
    TopList L;
    top_init(L);
    if constexpr (sizeof(T) == 2) {
        typedef typename Mma16<T>::vec vec;
        const int col = lane & 15, kg = lane >> 4;
        const bool live = r0 + col < M;
        const float m = live ? a.rmax[r0 + col] : 0.f, t = live ? a.tlogit[r0 + col] : 0.f;
        const vec* frag = reinterpret_cast<const vec*>(nll_smem) + lane;
        for (int tl = t0 + wave; tl < t1; tl += kNllWaves) {
            const int n0 = 16 * tl;
            const f32x4_t acc = nll_tile16<T>(W, frag, n0, col, kg, K, V);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 4 * kg + r;
                if (n < V) det_add(d, L, acc[r], n, m, t, inv_tau);
            }
        }
        det_fold_xor(d, L, 16);                                    // the 4 k-groups of a row: (0 + 1) + (2 + 3)
        det_fold_xor(d, L, 32);
    } else {
        const bool live = lane < kNllRows && r0 + lane < M;        // lane r keeps row r
        const float m = live ? a.rmax[r0 + lane] : 0.f, t = live ? a.tlogit[r0 + lane] : 0.f;
        const float* xs = reinterpret_cast<const float*>(nll_smem);
        const int c1 = min(V, 16 * t1);
        for (int g = 16 * t0 + 4 * wave; g < c1; g += 4 * kNllWaves) {
            nll_cols4(W, xs, g, K, V, lane, [&](int c, float mine) {
                if (g + c < V && lane < kNllRows) det_add(d, L, mine, g + c, m, t, inv_tau);
            });
        }
    }
    if (lane < kNllRows) {
        s_d[wave][lane] = d;
#pragma unroll
        for (int k = 0; k < kScoreTopK; ++k) { s_v[wave][k][lane] = L.v[k]; s_i[wave][k][lane] = L.i[k]; }
    }
    __syncthreads();
    if (tid < kNllRows && r0 + tid < M) {                          // the 4 waves: 0, then 1, 2, 3
        d = s_d[0][tid];
#pragma unroll
        for (int k = 0; k < kScoreTopK; ++k) { L.v[k] = s_v[0][k][tid]; L.i[k] = s_i[0][k][tid]; }
#pragma unroll 1
        for (int w = 1; w < kNllWaves; ++w) {
            const DetStat o = s_d[w][tid];
            d.cnt += o.cnt; d.A += o.A; d.Z += o.Z; d.U += o.U;
#pragma unroll 1
            for (int k = 0; k < kScoreTopK; ++k) top_insert(L, s_v[w][k][tid], s_i[w][k][tid]);
        }
        float4* rec = reinterpret_cast<float4*>(da.part) + ((long)(r0 + tid) * gridDim.x + split) * (kDetailRecFloats / 4);
        rec[0] = make_float4(__int_as_float(d.cnt), d.A, d.Z, d.U);
#pragma unroll
        for (int q = 0; q < kScoreTopK / 4; ++q) {
            rec[1 + q] = make_float4(L.v[4 * q], L.v[4 * q + 1], L.v[4 * q + 2], L.v[4 * q + 3]);
            rec[1 + kScoreTopK / 4 + q] = make_float4(__int_as_float(L.i[4 * q]), __int_as_float(L.i[4 * q + 1]), __int_as_float(L.i[4 * q + 2]),
                                                      __int_as_float(L.i[4 * q + 3]));
        }
    }
}

// the splits of a row, in order
__global__ __launch_bounds__(256) void detail_combine_kernel(const float4* __restrict__ part, int M, int ns, const float* __restrict__ lse,
                                                             const float* __restrict__ sumexp, ScoreDetailOut o) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    DetStat d{0, 0.f, 0.f, 0.f};
    TopList L;
    top_init(L);
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
        const float4* rec = part + ((long)r * ns + s) * (kDetailRecFloats / 4);
        const float4 h = rec[0];
        d.cnt += __float_as_int(h.x); d.A += h.y; d.Z += h.z; d.U += h.w;
        const float* rv = reinterpret_cast<const float*>(rec + 1);
        const int* ri = reinterpret_cast<const int*>(rec + 1 + kScoreTopK / 4);
#pragma unroll 1
        for (int k = 0; k < kScoreTopK; ++k) top_insert(L, rv[k], ri[k]);
    }
    det_finish(d, L, lse[r], sumexp[r], r, o);
}

// one wave per row of given logits: logits_nll_kernel's sweep for (m, s, t), then the detail sweep
__global__ __launch_bounds__(256) void logits_detail_kernel(const float* __restrict__ logits, long ld, int V, int M, const int* __restrict__ target,
                                                            int rows_per_group, long target_group_stride, ScoreDetailOut o) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const int tg = target[(long)(r / rows_per_group) * target_group_stride + r % rows_per_group];
    const float* lg = logits + (long)r * ld;
    NllStat st = nll_init();
    for (int n = lane; n < V; n += 64) nll_add(st, lg[n], n, tg);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) st = nll_merge(st, nll_shfl_xor(st, off));
    DetStat d{0, 0.f, 0.f, 0.f};
    TopList L;
    top_init(L);
    for (int n = lane; n < V; n += 64) det_add(d, L, lg[n], n, st.m, st.t, o.inv_temperature);
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) det_fold_xor(d, L, off);
    if (lane == 0) det_finish(d, L, st.m + logf(st.s), st.s, r, o);
}

}  // namespace

template <typename T>
hipError_t launch_head_nll(hipStream_t s, const HeadNllArgs& a) {
    if (!head_nll_supported(a.K) || a.M < 1 || a.V < 1) return hipErrorInvalidValue;
    const int lds = 64 * a.K;
    if (lds > (48 << 10)) {
        const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void*>(head_nll_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (rc != hipSuccess) return rc;
    }
    const int ns = head_nll_nsplit(a.V);
    hipLaunchKernelGGL(head_nll_kernel<T>, dim3(ns, (a.M + kNllRows - 1) / kNllRows), dim3(kNllThreads), lds, s, a);
    hipLaunchKernelGGL(nll_combine_kernel, dim3((a.M + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float4*>(a.part), a.M, ns, a.logp, a.argmax,
                       a.lse, a.tlogit, a.rmax, a.sumexp);
    return hipSuccess;
}
template hipError_t launch_head_nll<float>(hipStream_t, const HeadNllArgs&);
template hipError_t launch_head_nll<bf16_t>(hipStream_t, const HeadNllArgs&);
template hipError_t launch_head_nll<f16_t>(hipStream_t, const HeadNllArgs&);

void launch_logits_nll(hipStream_t s, const float* logits, long ld, int V, int M, const int* target, int rows_per_group, long target_group_stride,
                       float* logp, int* argmax, float* lse, float* tlogit) {
    hipLaunchKernelGGL(logits_nll_kernel, dim3((M + 3) / 4), dim3(256), 0, s, logits, ld, V, M, target, rows_per_group, target_group_stride, logp, argmax,
                       lse, tlogit);
}

template <typename T>
hipError_t launch_head_detail(hipStream_t s, const HeadDetailArgs& da) {
    const HeadNllArgs& a = da.h;
    if (!head_nll_supported(a.K) || a.M < 1 || a.V < 1 || da.out.topk < 0 || da.out.topk > kScoreTopK || !(da.out.inv_temperature > 0.f) || !da.part ||
        !a.lse || !a.tlogit || !a.rmax || !a.sumexp)
        return hipErrorInvalidValue;
    const int lds = 64 * a.K;
    if (lds > (48 << 10)) {
        const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void*>(head_detail_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (rc != hipSuccess) return rc;
    }
    const int ns = head_nll_nsplit(a.V);
    hipLaunchKernelGGL(head_detail_kernel<T>, dim3(ns, (a.M + kNllRows - 1) / kNllRows), dim3(kNllThreads), lds, s, da);
    hipLaunchKernelGGL(detail_combine_kernel, dim3((a.M + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float4*>(da.part), a.M, ns, a.lse, a.sumexp,
                       da.out);
    return hipSuccess;
}
template hipError_t launch_head_detail<float>(hipStream_t, const HeadDetailArgs&);
template hipError_t launch_head_detail<bf16_t>(hipStream_t, const HeadDetailArgs&);
template hipError_t launch_head_detail<f16_t>(hipStream_t, const HeadDetailArgs&);

hipError_t launch_logits_detail(hipStream_t s, const float* logits, long ld, int V, int M, const int* target, int rows_per_group, long target_group_stride,
                                const ScoreDetailOut& out) {
    if (M < 1 || V < 1 || out.topk < 0 || out.topk > kScoreTopK || !(out.inv_temperature > 0.f)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(logits_detail_kernel, dim3((M + 3) / 4), dim3(256), 0, s, logits, ld, V, M, target, rows_per_group, target_group_stride, out);
    return hipSuccess;
}

}  // namespace umgen
