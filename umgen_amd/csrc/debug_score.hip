// Kernel-level test hooks of the scoring head (score.hip), in debug_util.h's idiom: host pointers in, host pointers out, through the product's
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

namespace {
// the detail outputs of M rows on the device (guard bands, NaN / -1 at the launch) and their way back; a NULL host pointer asks for nothing
struct DetailBufs {
    ScoreDetailOut o{};
    int M, topk;
    DetailBufs(Scratch& s, int M_, int topk_, float temperature, const int32_t* rank, const float* mass, const float* ent, const int32_t* tok, const float* tlp)
        : M(M_), topk(topk_) {
        o.topk = topk; o.inv_temperature = 1.0f / temperature;
        if (rank) o.rank = s.out((size_t)M * 4);
        if (mass) o.mass_above = s.out((size_t)M * 4);
        if (ent) o.entropy = s.out((size_t)M * 4);
        if (tok) o.topk_tok = s.out((size_t)M * topk * 4);
        if (tlp) o.topk_logp = s.out((size_t)M * topk * 4);
    }
    int fill() const {
        return (o.rank && fill_nan(o.rank, M, 0)) || (o.mass_above && fill_nan(o.mass_above, M, 0)) || (o.entropy && fill_nan(o.entropy, M, 0)) ||
               (o.topk_tok && fill_nan(o.topk_tok, (size_t)M * topk, 0)) || (o.topk_logp && fill_nan(o.topk_logp, (size_t)M * topk, 0));
    }
    int get(int32_t* rank, float* mass, float* ent, int32_t* tok, float* tlp) const {
        return (rank && down(rank, o.rank, (size_t)M * 4)) || (mass && down(mass, o.mass_above, (size_t)M * 4)) || (ent && down(ent, o.entropy, (size_t)M * 4)) ||
               (tok && down(tok, o.topk_tok, (size_t)M * topk * 4)) || (tlp && down(tlp, o.topk_logp, (size_t)M * topk * 4));
    }
};
bool detail_args_ok(int topk, float temperature, const int32_t* tok, const float* tlp) {
    return topk >= 0 && topk <= kScoreTopK && temperature > 0.f && temperature <= 3.0e38f && (topk > 0 || (!tok && !tlp));
}
}  // namespace

extern "C" {

// launch_head_nll, then launch_head_detail on the same arguments (umgen_dbg_head_nll's operands): rank, mass_above, entropy [M] and
// topk_tok, topk_logp [M][topk]; any output may be NULL
int umgen_dbg_head_detail(int prec, int M, int K, int V, const float* x, long ldx, const float* ln_w, const void* W, const int32_t* target, int topk,
                          float temperature, int32_t* rank, float* mass_above, float* entropy, int32_t* topk_tok, float* topk_logp) {
    if (prec < 0 || prec > 2 || M < 1 || V < 1 || K < 1 || ldx < K || !x || !ln_w || !W || !target || !detail_args_ok(topk, temperature, topk_tok, topk_logp))
        return UMGEN_E_INVALID;
    if (!head_nll_supported(K)) return UMGEN_E_UNSUPPORTED;
    if (!in_range(target, (size_t)M, V)) return UMGEN_E_INVALID;
    const size_t wsz = (size_t)V * K * (prec ? 2 : 4);
    Scratch s;
    HeadDetailArgs d{};
    HeadNllArgs& a = d.h;
    a.x = s.in(x, ((size_t)(M - 1) * ldx + K) * 4); a.ldx = ldx; a.rows_per_group = M; a.group_stride = 0;
    a.ln_w = s.in(ln_w, (size_t)K * 4); a.W = s.in(W, wsz); a.V = V; a.K = K; a.M = M;
    a.target = s.in(target, (size_t)M * 4); a.target_group_stride = 0;
    a.part = s.out((size_t)M * head_nll_nsplit(V) * 16);
    a.lse = s.out((size_t)M * 4); a.tlogit = s.out((size_t)M * 4); a.rmax = s.out((size_t)M * 4); a.sumexp = s.out((size_t)M * 4);
    d.part = s.out((size_t)M * head_nll_nsplit(V) * kDetailRecFloats * 4);
    const DetailBufs b(s, M, topk, temperature, rank, mass_above, entropy, topk_tok, topk_logp);
    d.out = b.o;
    if (s.rc) return s.rc;
    if (b.fill()) return UMGEN_E_HIP;
    hipError_t le = hipSuccess;
    by_prec(prec, [&](auto t) {
        le = launch_head_nll<decltype(t)>(nullptr, a);
        if (le == hipSuccess) le = launch_head_detail<decltype(t)>(nullptr, d);
    });
    if (le != hipSuccess) return UMGEN_E_HIP;
    if (int rc = s.finish()) return rc;
    return b.get(rank, mass_above, entropy, topk_tok, topk_logp) ? UMGEN_E_HIP : UMGEN_OK;
}

// launch_logits_detail on logits [M] rows of V columns (row stride ld, fp32), target [M]: the same outputs
int umgen_dbg_logits_detail(int M, int V, const float* logits, long ld, const int32_t* target, int topk, float temperature, int32_t* rank,
                            float* mass_above, float* entropy, int32_t* topk_tok, float* topk_logp) {
    if (M < 1 || V < 1 || ld < V || !logits || !target || !detail_args_ok(topk, temperature, topk_tok, topk_logp)) return UMGEN_E_INVALID;
    if (!in_range(target, (size_t)M, V)) return UMGEN_E_INVALID;
    Scratch s;
    const float* dl = s.in(logits, ((size_t)(M - 1) * ld + V) * 4);
    const int* dt = s.in(target, (size_t)M * 4);
    const DetailBufs b(s, M, topk, temperature, rank, mass_above, entropy, topk_tok, topk_logp);
    if (s.rc) return s.rc;
    if (b.fill()) return UMGEN_E_HIP;
    if (launch_logits_detail(nullptr, dl, ld, V, M, dt, M, 0, b.o) != hipSuccess) return UMGEN_E_HIP;
    if (int rc = s.finish()) return rc;
    return b.get(rank, mass_above, entropy, topk_tok, topk_logp) ? UMGEN_E_HIP : UMGEN_OK;
}

}  // extern "C"
