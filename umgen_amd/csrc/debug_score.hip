// Kernel-level test hook of the scoring head (score.hip), in debug_util.h's idiom: host pointers in, host pointers out, through the product's
// launcher.  Every output carries a guard band and holds NaN at the launch.  Used only by tests/; never called by the product path.
#include "debug_util.h"

extern "C" {

// columns of one vocabulary split of launch_head_nll at vocabulary V (the tests plant a maximum on a split's first column)
int umgen_dbg_head_nll_split(int V) { return V < 1 ? UMGEN_E_INVALID : 16 * head_nll_tiles_per_split(V); }

// launch_head_nll on x [M] rows of K (row stride ldx, fp32), ln_w [K], W [V][K] (prec 0: fp32, 1: bf16 bits, 2: fp16 bits), target [M]:
// logp, argmax, lse, target_logit [M] each
int umgen_dbg_head_nll(int prec, int M, int K, int V, const float* x, long ldx, const float* ln_w, const void* W, const int32_t* target, float* logp,
                       int32_t* argmax, float* lse, float* target_logit) {
    if (prec < 0 || prec > 2 || M < 1 || V < 1 || K < 1 || ldx < K || !x || !ln_w || !W || !target || !logp || !argmax || !lse || !target_logit)
        return UMGEN_E_INVALID;
    if (!head_nll_supported(K)) return UMGEN_E_UNSUPPORTED;
    if (!in_range(target, (size_t)M, V)) return UMGEN_E_INVALID;
    const size_t wsz = (size_t)V * K * (prec ? 2 : 4);
    Scratch s;
    HeadNllArgs a{};
    a.x = s.in(x, ((size_t)(M - 1) * ldx + K) * 4); a.ldx = ldx; a.rows_per_group = M; a.group_stride = 0;
    a.ln_w = s.in(ln_w, (size_t)K * 4); a.W = s.in(W, wsz); a.V = V; a.K = K; a.M = M;
    a.target = s.in(target, (size_t)M * 4); a.target_group_stride = 0;
    a.part = s.out((size_t)M * head_nll_nsplit(V) * 16);
    a.logp = s.out((size_t)M * 4); a.argmax = s.out((size_t)M * 4); a.lse = s.out((size_t)M * 4); a.tlogit = s.out((size_t)M * 4);
    if (s.rc) return s.rc;
    if (fill_nan(a.logp, M, 0) || fill_nan(a.argmax, M, 0) || fill_nan(a.lse, M, 0) || fill_nan(a.tlogit, M, 0)) return UMGEN_E_HIP;
    hipError_t le = hipSuccess;
    by_prec(prec, [&](auto t) { le = launch_head_nll<decltype(t)>(nullptr, a); });
    if (le != hipSuccess) return UMGEN_E_HIP;
    if (int rc = s.finish()) return rc;
    if (down(logp, a.logp, (size_t)M * 4) || down(argmax, a.argmax, (size_t)M * 4) || down(lse, a.lse, (size_t)M * 4) ||
        down(target_logit, a.tlogit, (size_t)M * 4))
        return UMGEN_E_HIP;
    return UMGEN_OK;
}

}  // extern "C"
