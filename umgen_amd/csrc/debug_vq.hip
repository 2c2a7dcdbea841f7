// Kernel-level test hooks of the VQ decoder / encoder kernels (vq_common.h): one launch each, through the launcher the handles use, on
// device scratch with guard bands (debug_util.h).  Never part of the product path.
//
// Outputs are in / out: the caller's WHOLE buffer (`*_n` floats, at least what the launch writes) is uploaded as it is (NaN bits), the
// launch runs on it, and it is downloaded whole, so a location the kernel leaves out comes back as NaN and one it should not touch
// comes back unchanged; the guard band behind it catches a write past its end (UMGEN_E_STATE).
#include "vq_common.h"
#include "debug_util.h"

namespace {
bool mult4(int c) { return c >= 4 && c % 4 == 0; }
}  // namespace

extern "C" {

// launch_code_norms + launch_quantize, as umgen_vqenc_finalize / umgen_vqenc_encode run them: h [n_pos][ldh] (columns D .. ldh - 1 are
// never read), emb [N][D] -> codes [n_pos], zn [n_pos][D].  codes and zn are in / out and hold n_pos + 4 entries ([n_pos + 4] and
// [n_pos + 4][D]): the entries behind n_pos are the ones the dead waves of the last workgroup would write.
int umgen_dbg_vq_quantize(const float* h, int ldh, const float* emb, int N, int D, long n_pos, int64_t* codes, float* zn) {
    if (!h || !emb || !codes || !zn || N < 1 || !mult4(D) || D > kQuantMaxD || ldh < D || n_pos < 1) return UMGEN_E_INVALID;
    const size_t cn = (size_t)(n_pos + 4) * sizeof(long long), zb = (size_t)(n_pos + 4) * D * 4;
    Scratch s;
    const float *dH = s.in(h, (size_t)n_pos * ldh * 4), *dE = s.in(emb, (size_t)N * D * 4);
    float* dE2 = s.out((size_t)N * 4);
    long long* dC = s.inout(codes, cn);
    float* dZ = s.inout(zn, zb);
    if (s.rc) return s.rc;
    launch_code_norms(nullptr, dE, N, D, dE2);
    launch_quantize(nullptr, dH, ldh, dE, dE2, N, D, n_pos, dC, dZ);
    if (int rc = s.finish()) return rc;
    if (down(codes, dC, cn)) return UMGEN_E_HIP;
    return down(zn, dZ, zb);
}

// the codebook tile of launch_quantize for embed_dim D (the tests place rows at its seams)
int umgen_dbg_vq_quant_tile(int D) { return mult4(D) && D <= kQuantMaxD ? quant_tile(D) : UMGEN_E_INVALID; }

// launch_im2col: x [H][W][C] -> col [H * W][KS * KS * C]
int umgen_dbg_vq_im2col(const float* x, int H, int W, int C, int KS, int pad, float* col, long col_n) {
    if (!x || !col || H < 1 || W < 1 || !mult4(C) || KS < 1 || KS > 7 || pad < 0 || pad > KS || col_n < (long)H * W * KS * KS * C) return UMGEN_E_INVALID;
    Scratch s;
    const float* dX = s.in(x, (size_t)H * W * C * 4);
    float* dO = s.inout(col, (size_t)col_n * 4);
    if (s.rc) return s.rc;
    launch_im2col(nullptr, dX, H, W, C, KS, pad, dO);
    if (int rc = s.finish()) return rc;
    return down(col, dO, (size_t)col_n * 4);
}

// launch_im2col_s2 (Downsample): x [H][W][C], H and W even -> col [H / 2 * W / 2][9 C]
int umgen_dbg_vq_im2col_s2(const float* x, int H, int W, int C, float* col, long col_n) {
    if (!x || !col || H < 2 || W < 2 || H % 2 || W % 2 || !mult4(C) || col_n < (long)(H / 2) * (W / 2) * 9 * C) return UMGEN_E_INVALID;
    Scratch s;
    const float* dX = s.in(x, (size_t)H * W * C * 4);
    float* dO = s.inout(col, (size_t)col_n * 4);
    if (s.rc) return s.rc;
    launch_im2col_s2(nullptr, dX, H, W, C, dO);
    if (int rc = s.finish()) return rc;
    return down(col, dO, (size_t)col_n * 4);
}

// launch_upsample: x [H][W][C] -> y [2 H][2 W][C]
int umgen_dbg_vq_upsample(const float* x, int H, int W, int C, float* y, long y_n) {
    if (!x || !y || H < 1 || W < 1 || !mult4(C) || y_n < (long)4 * H * W * C) return UMGEN_E_INVALID;
    Scratch s;
    const float* dX = s.in(x, (size_t)H * W * C * 4);
    float* dO = s.inout(y, (size_t)y_n * 4);
    if (s.rc) return s.rc;
    launch_upsample(nullptr, dX, H, W, C, dO);
    if (int rc = s.finish()) return rc;
    return down(y, dO, (size_t)y_n * 4);
}

// launch_from_nchw: x [C_in][n_px] -> y [n_px][C], C >= C_in a multiple of 4
int umgen_dbg_vq_from_nchw(const float* x, long n_px, int C_in, int C, float* y, long y_n) {
    if (!x || !y || n_px < 1 || C_in < 1 || !mult4(C) || C < C_in || y_n < n_px * C) return UMGEN_E_INVALID;
    Scratch s;
    const float* dX = s.in(x, (size_t)n_px * C_in * 4);
    float* dO = s.inout(y, (size_t)y_n * 4);
    if (s.rc) return s.rc;
    launch_from_nchw(nullptr, dX, n_px, C_in, C, dO);
    if (int rc = s.finish()) return rc;
    return down(y, dO, (size_t)y_n * 4);
}

// launch_to_nchw: x [n_px][ldx] (columns C .. ldx - 1 are never read) -> out [C][n_px]
int umgen_dbg_vq_to_nchw(const float* x, long n_px, int C, int ldx, float* out, long out_n) {
    if (!x || !out || n_px < 1 || C < 1 || ldx < C || out_n < n_px * C) return UMGEN_E_INVALID;
    Scratch s;
    const float* dX = s.in(x, (size_t)n_px * ldx * 4);
    float* dO = s.inout(out, (size_t)out_n * 4);
    if (s.rc) return s.rc;
    launch_to_nchw(nullptr, dX, n_px, C, ldx, dO);
    if (int rc = s.finish()) return rc;
    return down(out, dO, (size_t)out_n * 4);
}

// group_norm (statistics + apply): x [n_px][C], gamma, beta [C], C a multiple of 32 -> y [n_px][C]
int umgen_dbg_vq_group_norm(const float* x, long n_px, int C, const float* gamma, const float* beta, int swish, float* y, long y_n) {
    if (!x || !gamma || !beta || !y || n_px < 1 || C < 32 || C % 32 || y_n < n_px * C) return UMGEN_E_INVALID;
    Scratch s;
    Ctx e;
    Norm n;
    const float* dX = s.in(x, (size_t)n_px * C * 4);
    n.g = s.in(gamma, (size_t)C * 4); n.b = s.in(beta, (size_t)C * 4); n.c = C;
    e.stats = s.out(64 * 4);
    float* dO = s.inout(y, (size_t)y_n * 4);
    if (s.rc) return s.rc;
    group_norm(&e, n, dX, n_px, swish != 0, dO);
    if (int rc = s.finish()) return rc;
    return down(y, dO, (size_t)y_n * 4);
}

// launch_softmax, in place: sc holds n rows of n scores, ld >= n floats apart; C: the attention width (scale C^-0.5)
int umgen_dbg_vq_softmax(float* sc, int n, int ld, int C, long sc_n) {
    if (!sc || n < 1 || ld < n || C < 1 || sc_n < (long)(n - 1) * ld + n) return UMGEN_E_INVALID;
    Scratch s;
    float* dS = s.inout(sc, (size_t)sc_n * 4);
    if (s.rc) return s.rc;
    launch_softmax(nullptr, dS, n, ld, C);
    if (int rc = s.finish()) return rc;
    return down(sc, dS, (size_t)sc_n * 4);
}

}  // extern "C"
