// The C ABI of include/umgen.h that drives frames: version and error text, profiling and timings, the argument checks at the ABI boundary,
// umgen_frame(_logp, _detail), umgen_score(_detail), umgen_score_candidates, umgen_score_futures, umgen_score_clip and the rollout driver umgen_rollout(_logp) / umgen_rollout_fan / umgen_rollout_detail (UMGen.inference).  Creation, weights, the compute path, the frame itself and the scoring passes are in
// engine_setup.hip, engine_weights.hip, engine_stacks.hip, engine_decode.hip, engine_frame.hip and engine_score.hip.
#include "engine_state.h"

// host arithmetic stays unfused in every engine file, as it was while they were one file behind the numpy-faithful helpers (engine_weights.hip)
#pragma clang fp contract(off)

namespace umgen { thread_local BgRecorder* g_bg_rec = nullptr; }      // bg_queue.h: installed around the recording of a background pass

// =============================================================================================================
// C ABI
// =============================================================================================================
extern "C" {

#ifndef UMGEN_SRC_HASH
#define UMGEN_SRC_HASH "unknown"
#endif
const char* umgen_version(void) { return "umgen_hip 0.2 (gfx950) src " UMGEN_SRC_HASH; }
const char* umgen_last_error(const umgen_engine* e) { return e ? e->err.c_str() : "null engine"; }

int umgen_set_profiling(umgen_engine* e, int32_t enable) {
    if (!e) return UMGEN_E_INVALID;
    e->profiling = enable != 0;
    return UMGEN_OK;
}
int umgen_get_timings(umgen_engine* e, umgen_timings* out) {
    if (!e || !out) return UMGEN_E_INVALID;
    *out = e->tm;
    return UMGEN_OK;
}

static int check_sampling(umgen_engine* e, const umgen_sampling* s) {
    if (!s) return e->fail(UMGEN_E_INVALID, "sampling is null");
    if (s->method != UMGEN_SAMPLE_TOPK && s->method != UMGEN_SAMPLE_TOPP) return e->fail(UMGEN_E_INVALID, "sample method %d", s->method);
    if (s->method == UMGEN_SAMPLE_TOPP && !(s->p > 0.f && s->p_map > 0.f)) return e->fail(UMGEN_E_INVALID, "top-p mass must be > 0");
    if (s->top_k < 1 || s->top_k > 16 || s->top_k_map < 1 || s->top_k_map > 16 || s->topk_image < 1 || s->topk_image > 16)
        return e->fail(UMGEN_E_INVALID, "top-k values must be in [1, 16] (reference: 5 / 5 / 16)");
    if (!(s->temperature > 0.f)) return e->fail(UMGEN_E_INVALID, "temperature must be > 0");
    return 0;
}

// Every token that becomes a gather index is checked at the ABI boundary (history: embed_stack_kernel's table rows; control
// pose: the fouier_pe rows and decode_pose_value; control bbox3d: -1 = "free", anything else a be / posi row).
static int check_tokens(umgen_engine* e, const char* what, const int64_t* p, size_t n, int64_t vocab, bool allow_free) {
    for (size_t i = 0; i < n; ++i) {
        const int64_t v = p[i];
        if (v >= 0 && v < vocab) continue;
        if (allow_free && v == -1) continue;
        return e->fail(UMGEN_E_INVALID, "%s token %lld at flat index %zu is outside [0, %lld)%s", what, (long long)v, i, (long long)vocab,
                       allow_free ? " (and is not -1 = free)" : "");
    }
    return 0;
}
static int check_scene_tokens(umgen_engine* e, size_t frames, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image) {
    if (int rc = check_tokens(e, "pose", pose, frames * kNPose, e->cfg.pose_vocab, false)) return rc;
    if (int rc = check_tokens(e, "map", map, frames * kNMap, e->cfg.map_vocab, false)) return rc;
    if (int rc = check_tokens(e, "bbox3d", bbox3d, frames * kNBox, e->cfg.bbox3d_vocab, false)) return rc;
    if (int rc = check_tokens(e, "image", image, frames * kNImg, e->cfg.img_vocab, false)) return rc;
    // the x / y attribute tokens of a slot index the 1030-row spatial table; attribute tokens are bins (< 1024) or pad
    return 0;
}

static bool wants_logp(const umgen_logp_out* lp) { return lp && (lp->logp_pose || lp->logp_map || lp->logp_bbox3d || lp->logp_image); }

// umgen_gen_detail_out behind its checks: a frame's host buffers in the device layout (FrameDetail) and their way into the caller's arrays
struct GenDetail {
    int topk = 0;
    int* rank[4] = {}; float *mass_above[4] = {}, *entropy[4] = {};
    int* topk_tok[4] = {}; float* topk_logp[4] = {};
    bool on = false;
    std::vector<int> f_rank, f_tok;
    std::vector<float> f_mass, f_ent, f_tlp;
    FrameDetail fd{};

    // refuses what umgen_score_detail refuses; a NULL or all-NULL struct asks for nothing and is not checked further
    int init(umgen_engine* e, const umgen_gen_detail_out* d, int32_t k, const umgen_sampling* s, size_t B) {
        if (!d) return 0;
        int* const r[4] = {d->rank_pose, d->rank_map, d->rank_bbox3d, d->rank_image};
        float* const ma[4] = {d->mass_above_pose, d->mass_above_map, d->mass_above_bbox3d, d->mass_above_image};
        float* const en[4] = {d->entropy_pose, d->entropy_map, d->entropy_bbox3d, d->entropy_image};
        int* const tt[4] = {d->topk_tok_pose, d->topk_tok_map, d->topk_tok_bbox3d, d->topk_tok_image};
        float* const tl[4] = {d->topk_logp_pose, d->topk_logp_map, d->topk_logp_bbox3d, d->topk_logp_image};
        bool lists = false;
        for (int m = 0; m < 4; ++m) {
            rank[m] = r[m]; mass_above[m] = ma[m]; entropy[m] = en[m]; topk_tok[m] = tt[m]; topk_logp[m] = tl[m];
            lists = lists || tt[m] || tl[m];
            on = on || r[m] || ma[m] || en[m] || tt[m] || tl[m];
        }
        if (!on) return 0;
        if (k < 0 || k > UMGEN_SCORE_TOPK_MAX) return e->fail(UMGEN_E_INVALID, "topk=%d out of range [0,%d]", k, UMGEN_SCORE_TOPK_MAX);
        if (lists && k == 0) return e->fail(UMGEN_E_INVALID, "top-K outputs requested with topk = 0");
        if (!(s->temperature <= 3.0e38f)) return e->fail(UMGEN_E_INVALID, "temperature must be > 0 and finite");
        topk = lists ? k : 0;      // (lists nobody receives are not formed)
        const size_t n = B * kTokPerFrame;
        f_rank.resize(n); f_mass.resize(n); f_ent.resize(n);
        f_tok.resize(topk ? n * kDetailTopK : 0); f_tlp.resize(topk ? n * kDetailTopK : 0);
        fd = FrameDetail{topk, f_rank.data(), f_mass.data(), f_ent.data(), f_tok.data(), f_tlp.data()};
        return 0;
    }
    const FrameDetail* frame() const { return on ? &fd : nullptr; }
    // scene b of the frame just generated -> item `item` of the caller's arrays ([items][S_mod], the lists [items][S_mod][topk])
    void deliver(size_t b, size_t item) const {
        for (int m = 0; on && m < 4; ++m) {
            const size_t src = b * kTokPerFrame + kModOff[m], dst = item * kModLen[m], len = (size_t)kModLen[m];
            if (rank[m]) memcpy(rank[m] + dst, &f_rank[src], len * sizeof(int));
            if (mass_above[m]) memcpy(mass_above[m] + dst, &f_mass[src], len * sizeof(float));
            if (entropy[m]) memcpy(entropy[m] + dst, &f_ent[src], len * sizeof(float));
            for (size_t i = 0; i < len && topk; ++i) {
                if (topk_tok[m]) memcpy(topk_tok[m] + (dst + i) * topk, &f_tok[(src + i) * kDetailTopK], (size_t)topk * sizeof(int));
                if (topk_logp[m]) memcpy(topk_logp[m] + (dst + i) * topk, &f_tlp[(src + i) * kDetailTopK], (size_t)topk * sizeof(float));
            }
        }
    }
};

int umgen_frame_detail(umgen_engine* e, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                     const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test, const umgen_sampling* sampling,
                       int32_t frame_idx, const umgen_trace* trace, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                       const umgen_logp_out* lp, int32_t topk, const umgen_gen_detail_out* detail) {
    if (!e) return UMGEN_E_INVALID;
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_finalize_weights has not been called");
    if (T < 1 || T > e->cfg.max_cond_frames) return e->fail(UMGEN_E_INVALID, "T=%d out of range [1,%d]", T, e->cfg.max_cond_frames);
    if (int rc = check_sampling(e, sampling)) return rc;
    GenDetail gd;
    if (int rc = gd.init(e, detail, topk, sampling, 1)) return rc;
    if (!pose || !map || !bbox3d || !image || !out_pose || !out_map || !out_bbox3d || !out_image) return e->fail(UMGEN_E_INVALID, "null token buffer");
    if (int rc = check_scene_tokens(e, (size_t)T, pose, map, bbox3d, image)) return rc;
    if (ctrl_pose) { if (int rc = check_tokens(e, "control pose", ctrl_pose, 3, e->cfg.pose_vocab, false)) return rc; }
    if (ctrl_bbox3d) { if (int rc = check_tokens(e, "control bbox3d", ctrl_bbox3d, kNBox, e->cfg.bbox3d_vocab, true)) return rc; }
    if (ctrl_bbox3d && !control_test) return e->fail(UMGEN_E_UNSUPPORTED, "init_tokens['bbox3d'] without control_test is not a supported reference path");
    std::vector<int> p((size_t)T * 3), m((size_t)T * kNMap), bx((size_t)T * kNBox), im((size_t)T * kNImg);
    for (size_t i = 0; i < p.size(); ++i) p[i] = (int)pose[i];
    for (size_t i = 0; i < m.size(); ++i) m[i] = (int)map[i];
    for (size_t i = 0; i < bx.size(); ++i) bx[i] = (int)bbox3d[i];
    for (size_t i = 0; i < im.size(); ++i) im[i] = (int)image[i];
    std::vector<int> cp;
    std::vector<unsigned char> cs;
    if (ctrl_pose) { cp.resize(3); for (int i = 0; i < 3; ++i) cp[i] = (int)ctrl_pose[i]; }
    if (ctrl_bbox3d && control_test) {   // UMGen.py:1458-1473
        cs.assign(kSlots, 0);
        for (int i = 0; i < kNBox; ++i)
            if (ctrl_bbox3d[i] != -1) { bx[(size_t)(T - 1) * kNBox + i] = (int)ctrl_bbox3d[i]; cs[i / kSlotLen] = 1; }
    }
    std::vector<int> out(kTokPerFrame);
    FrameIO io{1, T, p.data(), m.data(), bx.data(), im.data(), ctrl_pose ? cp.data() : nullptr, cs.empty() ? nullptr : cs.data(),
               frame_idx, sampling, trace, out.data()};
    // the frame's GIVEN tokens (umgen_rollout's given_* for one frame: the predefined-token prefix of infer_oar_net, UMGen.py:1184-1201)
    std::vector<int> gm, gb;
    if (trace && trace->given_bbox3d && !trace->given_map)
        return e->fail(UMGEN_E_UNSUPPORTED, "given bbox3d tokens without a given map: the reference would put them on the map's positions (UMGen.py:1190-1201)");
    if (trace && trace->given_map) {
        if (control_test) return e->fail(UMGEN_E_UNSUPPORTED, "given tokens and control_test exclude each other");
        if (int rc = check_tokens(e, "given map", trace->given_map, kNMap, e->cfg.map_vocab, false)) return rc;
        gm.resize(kNMap);
        for (int i = 0; i < kNMap; ++i) gm[i] = (int)trace->given_map[i];
        io.given_map = gm.data();
        if (trace->given_bbox3d) {
            if (int rc = check_tokens(e, "given bbox3d", trace->given_bbox3d, kNBox, e->cfg.bbox3d_vocab, false)) return rc;
            gb.resize(kNBox);
            for (int i = 0; i < kNBox; ++i) gb[i] = (int)trace->given_bbox3d[i];
            io.given_box = gb.data();
        }
    }
    std::vector<float> flp(wants_logp(lp) ? (size_t)kTokPerFrame : 0);
    if (!flp.empty()) io.out_logp = flp.data();
    io.out_detail = gd.frame();
    if (int rc = run_frame_any(e, io)) return rc;
    gd.deliver(0, 0);
    for (int i = 0; i < kNPose; ++i) out_pose[i] = out[i];
    for (int i = 0; i < kNMap; ++i) out_map[i] = out[kOffMap + i];
    for (int i = 0; i < kNBox; ++i) out_bbox3d[i] = out[kOffBox + i];
    for (int i = 0; i < kNImg; ++i) out_image[i] = out[kOffImg + i];
    if (!flp.empty()) {
        if (lp->logp_pose) memcpy(lp->logp_pose, &flp[0], kNPose * sizeof(float));
        if (lp->logp_map) memcpy(lp->logp_map, &flp[kOffMap], kNMap * sizeof(float));
        if (lp->logp_bbox3d) memcpy(lp->logp_bbox3d, &flp[kOffBox], kNBox * sizeof(float));
        if (lp->logp_image) memcpy(lp->logp_image, &flp[kOffImg], kNImg * sizeof(float));
    }
    return UMGEN_OK;
}

int umgen_frame_logp(umgen_engine* e, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                     const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test, const umgen_sampling* sampling,
                     int32_t frame_idx, const umgen_trace* trace, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                     const umgen_logp_out* lp) {
    return umgen_frame_detail(e, T, pose, map, bbox3d, image, ctrl_pose, ctrl_bbox3d, control_test, sampling, frame_idx, trace, out_pose, out_map,
                              out_bbox3d, out_image, lp, 0, nullptr);
}

int umgen_frame(umgen_engine* e, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test, const umgen_sampling* sampling,
                int32_t frame_idx, const umgen_trace* trace, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image) {
    return umgen_frame_logp(e, T, pose, map, bbox3d, image, ctrl_pose, ctrl_bbox3d, control_test, sampling, frame_idx, trace, out_pose, out_map,
                            out_bbox3d, out_image, nullptr);
}

// ---- umgen_score(_detail), umgen_score_candidates, umgen_score_futures, umgen_score_clip: the passes of engine_score.hip behind the argument checks ----

// What these calls check alike, in their common order: the engine and B first; then, behind what only the call itself takes, the output struct,
// the token buffers -- a history of `frames` frames and, with next, n_next frames to score that an error names next_what -- the head, and every token
static int check_score_engine(umgen_engine* e, int32_t B) {
    if (!e) return UMGEN_E_INVALID;
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_finalize_weights has not been called");
    if (B < 1 || B > e->cfg.max_batch) return e->fail(UMGEN_E_INVALID, "B=%d out of range [1,%d]", B, e->cfg.max_batch);
    return 0;
}
static int check_score_common(umgen_engine* e, bool have_out, const int64_t* const win[4], size_t frames, const int64_t* const* next, size_t n_next,
                              const char* next_what) {
    if (!have_out) return e->fail(UMGEN_E_INVALID, "null output struct");
    for (int m = 0; m < 4; ++m)
        if (!win[m] || (next && !next[m])) return e->fail(UMGEN_E_INVALID, "null token buffer");
    if (!head_nll_supported(e->E)) return e->fail(UMGEN_E_UNSUPPORTED, "the scoring head is built for n_embd 96 / 768 / 1536, not %d", e->E);
    if (int rc = check_scene_tokens(e, frames, win[0], win[1], win[2], win[3])) return rc;
    if (!next) return 0;
    const int rc = check_scene_tokens(e, n_next, next[0], next[1], next[2], next[3]);
    if (rc) e->err = std::string(next_what) + ": " + e->err;
    return rc;
}
static int check_window_length(umgen_engine* e, int32_t T) {
    return T < 1 || T > e->cfg.max_cond_frames ? e->fail(UMGEN_E_INVALID, "T=%d out of range [1,%d]", T, e->cfg.max_cond_frames) : 0;
}

// int64 tokens [frames][S_mod] of every modality as int32
static void narrow_tokens(const int64_t* const in[4], size_t frames, std::vector<int> out[4]) {
    for (int m = 0; m < 4; ++m) {
        out[m].resize(frames * kModLen[m]);
        for (size_t i = 0; i < out[m].size(); ++i) out[m][i] = (int)in[m][i];
    }
}
// n frames, [n][S_mod] per modality, as int32 rows [n][2199] pose | map | bbox3d | image
static std::vector<int> frame_rows(const int64_t* const in[4], size_t n) {
    std::vector<int> rows(n * kTokPerFrame);
    for (int m = 0; m < 4; ++m)
        for (size_t it = 0; it < n; ++it)
            for (int i = 0; i < kModLen[m]; ++i) rows[it * kTokPerFrame + kModOff[m] + i] = (int)in[m][it * kModLen[m] + i];
    return rows;
}
static ScoreDst score_dst(const umgen_score_out* o) {
    if (!o) return ScoreDst{};
    return ScoreDst{{o->logp_pose, o->logp_map, o->logp_bbox3d, o->logp_image}, {o->argmax_pose, o->argmax_map, o->argmax_bbox3d, o->argmax_image}};
}

// umgen_score and umgen_score_detail: log p of a given next frame per content position (the reference's loss terms, UMGen.py:539-582) for B scenes, and
// with `detail` the diagnostics of the same rows: engine_score.hip run_score
static int score_call(umgen_engine* e, int32_t B, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                      const int64_t* next_pose, const int64_t* next_map, const int64_t* next_bbox3d, const int64_t* next_image, umgen_score_out* out,
                      const umgen_score_detail_out* d, int32_t topk, float temperature) {
    const int64_t *in[4] = {pose, map, bbox3d, image}, *nx[4] = {next_pose, next_map, next_bbox3d, next_image};
    if (int rc = check_score_engine(e, B)) return rc;
    if (int rc = check_window_length(e, T)) return rc;
    if (d) {
        if (topk < 0 || topk > UMGEN_SCORE_TOPK_MAX) return e->fail(UMGEN_E_INVALID, "topk=%d out of range [0,%d]", topk, UMGEN_SCORE_TOPK_MAX);
        if (!(temperature > 0.f) || !(temperature <= 3.0e38f)) return e->fail(UMGEN_E_INVALID, "temperature must be > 0 and finite");
        const bool lists = d->topk_tok_pose || d->topk_tok_map || d->topk_tok_bbox3d || d->topk_tok_image || d->topk_logp_pose || d->topk_logp_map ||
                           d->topk_logp_bbox3d || d->topk_logp_image;
        if (lists && topk == 0) return e->fail(UMGEN_E_INVALID, "top-K outputs requested with topk = 0");
    }
    if (int rc = check_score_common(e, out || d, in, (size_t)B * T, nx, (size_t)B, "next frame")) return rc;
    std::vector<int> win[4];
    narrow_tokens(in, (size_t)B * T, win);
    const std::vector<int> next = frame_rows(nx, (size_t)B);
    ScoreIO sc{B, T, win[0].data(), win[1].data(), win[2].data(), win[3].data(), next.data(), score_dst(out)};
    const ScoreDetailIO dio = !d ? ScoreDetailIO{}
                                 : ScoreDetailIO{topk, temperature, {d->rank_pose, d->rank_map, d->rank_bbox3d, d->rank_image},
                                                 {d->mass_above_pose, d->mass_above_map, d->mass_above_bbox3d, d->mass_above_image},
                                                 {d->entropy_pose, d->entropy_map, d->entropy_bbox3d, d->entropy_image},
                                                 {d->topk_tok_pose, d->topk_tok_map, d->topk_tok_bbox3d, d->topk_tok_image},
                                                 {d->topk_logp_pose, d->topk_logp_map, d->topk_logp_bbox3d, d->topk_logp_image}};
    if (d) sc.detail = &dio;
    return run_score_any(e, sc);
}

int umgen_score(umgen_engine* e, int32_t B, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                const int64_t* next_pose, const int64_t* next_map, const int64_t* next_bbox3d, const int64_t* next_image, umgen_score_out* out) {
    if (e && !out) return e->fail(UMGEN_E_INVALID, "null output struct");
    return score_call(e, B, T, pose, map, bbox3d, image, next_pose, next_map, next_bbox3d, next_image, out, nullptr, 0, 1.f);
}

int umgen_score_detail(umgen_engine* e, int32_t B, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                       const int64_t* next_pose, const int64_t* next_map, const int64_t* next_bbox3d, const int64_t* next_image, int32_t topk,
                       float temperature, umgen_score_out* out, umgen_score_detail_out* detail) {
    if (e && !detail) return e->fail(UMGEN_E_INVALID, "null detail struct");
    return score_call(e, B, T, pose, map, bbox3d, image, next_pose, next_map, next_bbox3d, next_image, out, detail, topk, temperature);
}

// umgen_score_candidates: C given next frames per scene against one history (engine_score.hip run_score_candidates)
int umgen_score_candidates(umgen_engine* e, int32_t B, int32_t T, int32_t C, const int64_t* pose, const int64_t* map, const int64_t* bbox3d,
                           const int64_t* image, const int64_t* next_pose, const int64_t* next_map, const int64_t* next_bbox3d, const int64_t* next_image,
                           umgen_score_out* out, int32_t* shared_slots) {
    const int64_t *in[4] = {pose, map, bbox3d, image}, *nx[4] = {next_pose, next_map, next_bbox3d, next_image};
    if (int rc = check_score_engine(e, B)) return rc;
    if (int rc = check_window_length(e, T)) return rc;
    if (C < 1) return e->fail(UMGEN_E_INVALID, "C=%d: at least one candidate per scene", C);
    if (int rc = check_score_common(e, out, in, (size_t)B * T, nx, (size_t)B * C, "candidate frames")) return rc;
    std::vector<int> win[4];
    narrow_tokens(in, (size_t)B * T, win);
    const std::vector<int> next = frame_rows(nx, (size_t)B * C);
    ScoreCandIO sc{B, T, C, win[0].data(), win[1].data(), win[2].data(), win[3].data(), next.data(), score_dst(out), 0};
    if (int rc = run_score_candidates_any(e, sc)) return rc;
    if (shared_slots) *shared_slots = sc.shared_slots;
    return UMGEN_OK;
}

// umgen_score_futures: C candidate futures of K frames per scene against one history, frame by frame under the rollout's window rule (engine_score.hip
// run_score_futures)
int umgen_score_futures(umgen_engine* e, int32_t B, int32_t T, int32_t C, int32_t K, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                        const int64_t* bbox3d, const int64_t* image, const int64_t* fut_pose, const int64_t* fut_map, const int64_t* fut_bbox3d,
                        const int64_t* fut_image, umgen_score_out* out, int32_t* shared_slots) {
    const int64_t *in[4] = {pose, map, bbox3d, image}, *nx[4] = {fut_pose, fut_map, fut_bbox3d, fut_image};
    if (int rc = check_score_engine(e, B)) return rc;
    if (T < 1) return e->fail(UMGEN_E_INVALID, "T=%d: at least one history frame", T);
    if (cond_frames < 1 || cond_frames > e->cfg.max_cond_frames)
        return e->fail(UMGEN_E_INVALID, "cond_frames=%d out of range [1,%d]", cond_frames, e->cfg.max_cond_frames);
    if (C < 1) return e->fail(UMGEN_E_INVALID, "C=%d: at least one candidate per scene", C);
    if (K < 1) return e->fail(UMGEN_E_INVALID, "K=%d: at least one future frame per candidate", K);
    if (int rc = check_score_common(e, out, in, (size_t)B * T, nx, (size_t)B * C * K, "future frames")) return rc;
    std::vector<int> win[4], fut[4];
    narrow_tokens(in, (size_t)B * T, win);
    narrow_tokens(nx, (size_t)B * C * K, fut);
    const ScoreFutIO sc{B, T, C, K, cond_frames, win[0].data(), win[1].data(), win[2].data(), win[3].data(),
                        {fut[0].data(), fut[1].data(), fut[2].data(), fut[3].data()}, score_dst(out), shared_slots};
    return run_score_futures_any(e, sc);
}

// umgen_score_clip: every frame of B recorded clips against the frames before it, the growing windows off one pass (engine_score.hip run_score_clip)
int umgen_score_clip(umgen_engine* e, int32_t B, int32_t L, int32_t T_in, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                     const int64_t* bbox3d, const int64_t* image, umgen_score_out* out, int32_t* shared_frames) {
    const int64_t* in[4] = {pose, map, bbox3d, image};
    if (int rc = check_score_engine(e, B)) return rc;
    if (L < 2) return e->fail(UMGEN_E_INVALID, "L=%d: a clip has at least two frames", L);
    if (T_in < 1 || T_in >= L) return e->fail(UMGEN_E_INVALID, "T_in=%d out of range [1,%d) (L=%d)", T_in, L, L);
    if (cond_frames < 1 || cond_frames > e->cfg.max_cond_frames)
        return e->fail(UMGEN_E_INVALID, "cond_frames=%d out of range [1,%d]", cond_frames, e->cfg.max_cond_frames);
    if (int rc = check_score_common(e, out, in, (size_t)B * L, nullptr, 0, nullptr)) return rc;
    std::vector<int> clip[4];
    narrow_tokens(in, (size_t)B * L, clip);
    ScoreClipIO sc{B, L, T_in, cond_frames, clip[0].data(), clip[1].data(), clip[2].data(), clip[3].data(), score_dst(out), 0};
    if (int rc = run_score_clip_any(e, sc)) return rc;
    if (shared_frames) *shared_frames = sc.shared_frames;
    return UMGEN_OK;
}

// UMGen.inference (UMGen.py:1542-1671).  fan_N >= 2 (umgen_rollout_fan): the B scenes are B / fan_N recorded scenes of fan_N branches each, branch (b, s) at
// b*fan_N + s with scene b's arrays replicated -- the first frame then runs its history once per scene (run_frame_fan) when its window has at least two slots,
// the slot caches fit and UMGEN_FAN_SHARE is not 0, and *shared_slots reports the slots that were shared.
static int rollout_driver(umgen_engine* e, int32_t B, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose,
                          const int64_t* map, const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose,
                          const int64_t* ctrl_bbox3d, int32_t control_test, const int64_t* given_map, const int64_t* given_bbox3d,
                          const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                          const umgen_logp_out* lp, int32_t fan_N, int32_t* shared_slots, int32_t topk, const umgen_gen_detail_out* detail) {
    if (!e) return UMGEN_E_INVALID;
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_finalize_weights has not been called");
    if (B < 1 || B > e->cfg.max_batch) return e->fail(UMGEN_E_INVALID, "B=%d out of range [1,%d]", B, e->cfg.max_batch);
    if (T_in < 1 || new_frames < 0 || cond_frames < 1 || cond_frames > e->cfg.max_cond_frames)
        return e->fail(UMGEN_E_INVALID, "T_in=%d new_frames=%d cond_frames=%d (max %d)", T_in, new_frames, cond_frames, e->cfg.max_cond_frames);
    if (int rc = check_sampling(e, sampling)) return rc;
    GenDetail gd;      // the frame's diagnostics, scattered to [B][new_frames][S_mod] below
    if (int rc = gd.init(e, detail, topk, sampling, (size_t)B)) return rc;
    if (!pose || !map || !bbox3d || !image || !out_pose || !out_map || !out_bbox3d || !out_image) return e->fail(UMGEN_E_INVALID, "null token buffer");
    if (int rc = check_scene_tokens(e, (size_t)B * T_in, pose, map, bbox3d, image)) return rc;
    if ((ctrl_pose || ctrl_bbox3d) && T_ctl < 1) return e->fail(UMGEN_E_INVALID, "control tokens given with T_ctl=%d", T_ctl);
    if (ctrl_pose) { if (int rc = check_tokens(e, "control pose", ctrl_pose, (size_t)B * T_ctl * 3, e->cfg.pose_vocab, false)) return rc; }
    if (ctrl_bbox3d) { if (int rc = check_tokens(e, "control bbox3d", ctrl_bbox3d, (size_t)B * T_ctl * kNBox, e->cfg.bbox3d_vocab, true)) return rc; }
    // given (not generated) modalities of the new frames: infer_oar_net's predefined-token prefix (UMGen.py:1184-1201)
    if ((given_map || given_bbox3d) && T_ctl < 1) return e->fail(UMGEN_E_INVALID, "given tokens with T_ctl=%d", T_ctl);
    if (given_bbox3d && !given_map)
        return e->fail(UMGEN_E_UNSUPPORTED, "init_tokens['bbox3d'] without init_tokens['map'] (and without control_test): the reference concatenates the given "
                                            "modalities back to back behind the pose, so the boxes would sit on the map's positions -- not a meaningful path");
    if (given_bbox3d && (ctrl_bbox3d || control_test)) return e->fail(UMGEN_E_INVALID, "given bbox3d tokens and bbox3d control exclude each other");
    if (given_map) { if (int rc = check_tokens(e, "given map", given_map, (size_t)B * T_ctl * kNMap, e->cfg.map_vocab, false)) return rc; }
    if (given_bbox3d) { if (int rc = check_tokens(e, "given bbox3d", given_bbox3d, (size_t)B * T_ctl * kNBox, e->cfg.bbox3d_vocab, false)) return rc; }
    e->tm = umgen_timings{};
    e->overlap_suspended = false;
    const int T_out = T_in + new_frames;
    const int64_t* in[4] = {pose, map, bbox3d, image};
    int64_t* out[4] = {out_pose, out_map, out_bbox3d, out_image};
    // history: out_tokens and cond_tokens both start as the first T_in frames (UMGen.py:1581-1595)
    std::vector<int> hist[4];   // [B][T_cur][S] "cond_tokens" window (control mode mutates its last bbox3d frame in place)
    for (int m = 0; m < 4; ++m) {
        hist[m].resize((size_t)B * T_in * kModLen[m]);
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < T_in; ++t)
                for (int i = 0; i < kModLen[m]; ++i) {
                    const int64_t v = in[m][((size_t)b * T_in + t) * kModLen[m] + i];
                    hist[m][((size_t)b * T_in + t) * kModLen[m] + i] = (int)v;
                    out[m][((size_t)b * T_out + t) * kModLen[m] + i] = v;
                }
    }
    int T_cur = T_in;
    // Control tokens (UMGen.py:1605-1619, 1438-1473).  With pose tokens the rollout leaves control mode for good once they are used
    // up (init_tokens = None, control_test = False); bbox3d tokens alone (agents controlled, ego inferred by the ego net) simply stop
    // applying after their last frame (get_mod_tokens returns None past the end).
    bool have_ctl = (ctrl_pose != nullptr) && T_ctl > 0;
    bool have_box = (ctrl_bbox3d != nullptr) && T_ctl > 0;
    bool have_given = (given_map != nullptr) && T_ctl > 0;   // like every init_tokens entry: None past its last frame (get_mod_tokens), and gone
                                                              // for good with the pose tokens (UMGen.py:1613-1619)
    std::vector<int> frame_out((size_t)B * kTokPerFrame);
    std::vector<float> frame_logp(wants_logp(lp) ? (size_t)B * kTokPerFrame : 0);      // the frame's log-likelihoods, scattered to [B][new_frames][S_mod] below
    float* const lp_out[4] = {lp ? lp->logp_pose : nullptr, lp ? lp->logp_map : nullptr, lp ? lp->logp_bbox3d : nullptr, lp ? lp->logp_image : nullptr};
    for (int idx = 0; idx < new_frames; ++idx) {
        if (T_cur > cond_frames) {   // sliding window (UMGen.py:1600-1603)
            for (int m = 0; m < 4; ++m) {
                std::vector<int> nw((size_t)B * cond_frames * kModLen[m]);
                for (int b = 0; b < B; ++b)
                    memcpy(&nw[(size_t)b * cond_frames * kModLen[m]], &hist[m][((size_t)b * T_cur + (T_cur - cond_frames)) * kModLen[m]],
                           (size_t)cond_frames * kModLen[m] * sizeof(int));
                hist[m].swap(nw);
            }
            T_cur = cond_frames;
        }
        if (have_ctl && idx >= T_ctl) { have_ctl = false; have_box = false; have_given = false; control_test = 0; }   // control tokens exhausted (UMGen.py:1613-1619)
        if (have_box && idx >= T_ctl) have_box = false;
        if (have_given && idx >= T_ctl) have_given = false;
        std::vector<int> gm, gb;
        if (have_given) {
            gm.resize((size_t)B * kNMap);
            for (int b = 0; b < B; ++b)
                for (int i = 0; i < kNMap; ++i) gm[(size_t)b * kNMap + i] = (int)given_map[((size_t)b * T_ctl + idx) * kNMap + i];
            if (given_bbox3d) {
                gb.resize((size_t)B * kNBox);
                for (int b = 0; b < B; ++b)
                    for (int i = 0; i < kNBox; ++i) gb[(size_t)b * kNBox + i] = (int)given_bbox3d[((size_t)b * T_ctl + idx) * kNBox + i];
            }
        }
        std::vector<int> cp;
        std::vector<unsigned char> cs;
        if (have_ctl) {
            cp.resize((size_t)B * 3);
            for (int b = 0; b < B; ++b)
                for (int a = 0; a < 3; ++a) cp[b * 3 + a] = (int)ctrl_pose[((size_t)b * T_ctl + idx) * 3 + a];
        }
        if (have_box) {
            if (control_test) {
                cs.assign((size_t)B * kSlots, 0);
                for (int b = 0; b < B; ++b)
                    for (int i = 0; i < kNBox; ++i) {
                        const int64_t v = ctrl_bbox3d[((size_t)b * T_ctl + idx) * kNBox + i];
                        if (v != -1) { hist[2][((size_t)b * T_cur + (T_cur - 1)) * kNBox + i] = (int)v; cs[(size_t)b * kSlots + i / kSlotLen] = 1; }
                    }
            } else {
                return e->fail(UMGEN_E_UNSUPPORTED, "init_tokens['bbox3d'] without control_test is not a supported reference path");
            }
        }
        FrameIO io{B, T_cur, hist[0].data(), hist[1].data(), hist[2].data(), hist[3].data(), have_ctl ? cp.data() : nullptr,
                   cs.empty() ? nullptr : cs.data(), idx, sampling, nullptr, frame_out.data()};
        io.cond_cap = cond_frames;
        io.next_follows = idx + 1 < new_frames;
        io.next_has_ctrl_pose = have_ctl && idx + 1 < T_ctl;
        io.given_map = gm.empty() ? nullptr : gm.data();
        io.given_box = gb.empty() ? nullptr : gb.data();
        io.out_logp = frame_logp.empty() ? nullptr : frame_logp.data();
        io.out_detail = gd.frame();
        const char* fse = getenv("UMGEN_FAN_SHARE");      // (read per call: the tests compare both forms in one process)
        const bool fan = idx == 0 && fan_N >= 2 && T_cur >= 2 && !(fse && fse[0] == '0') && ensure_tcache(e);
        if (fan && shared_slots) *shared_slots = T_cur - 1;
        if (int rc = fan ? run_frame_fan_any(e, io, fan_N) : run_frame_any(e, io)) return rc;
        // append (UMGen.py:1636-1666): control pose tokens are copied verbatim; everything else is what was generated
        for (int m = 0; m < 4; ++m) {
            std::vector<int> nw((size_t)B * (T_cur + 1) * kModLen[m]);
            for (int b = 0; b < B; ++b) {
                memcpy(&nw[(size_t)b * (T_cur + 1) * kModLen[m]], &hist[m][(size_t)b * T_cur * kModLen[m]], (size_t)T_cur * kModLen[m] * sizeof(int));
                for (int i = 0; i < kModLen[m]; ++i) {
                    const int v = frame_out[(size_t)b * kTokPerFrame + kModOff[m] + i];
                    nw[((size_t)b * (T_cur + 1) + T_cur) * kModLen[m] + i] = v;
                    out[m][((size_t)b * T_out + T_in + idx) * kModLen[m] + i] = v;
                }
            }
            hist[m].swap(nw);
            if (lp_out[m] && !frame_logp.empty())
                for (int b = 0; b < B; ++b)
                    memcpy(lp_out[m] + ((size_t)b * new_frames + idx) * kModLen[m], &frame_logp[(size_t)b * kTokPerFrame + kModOff[m]], (size_t)kModLen[m] * sizeof(float));
        }
        for (int b = 0; b < B; ++b) gd.deliver((size_t)b, (size_t)b * new_frames + idx);
        T_cur += 1;
    }
    return UMGEN_OK;
}

int umgen_rollout_logp(umgen_engine* e, int32_t B, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose,
                       const int64_t* map, const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose,
                       const int64_t* ctrl_bbox3d, int32_t control_test, const int64_t* given_map, const int64_t* given_bbox3d,
                       const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                       const umgen_logp_out* lp) {
    return rollout_driver(e, B, T_in, new_frames, cond_frames, pose, map, bbox3d, image, T_ctl, ctrl_pose, ctrl_bbox3d, control_test, given_map, given_bbox3d,
                          sampling, out_pose, out_map, out_bbox3d, out_image, lp, 0, nullptr, 0, nullptr);
}

// umgen_rollout_fan: N sampled futures per scene.  The branches are the scenes of an ordinary rollout of B * N scenes on replicated inputs -- the driver above,
// whose first frame shares the history between a scene's branches (engine_frame.hip run_frame_fan); outputs [B][N][..] are that rollout's [B * N][..].
// umgen_rollout_detail: the same with the diagnostics of every generated token ([B][N][..] likewise)
int umgen_rollout_detail(umgen_engine* e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                         const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test,
                         const int64_t* given_map, const int64_t* given_bbox3d, const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map,
                         int64_t* out_bbox3d, int64_t* out_image, const umgen_logp_out* lp, int32_t* shared_slots, int32_t topk,
                         const umgen_gen_detail_out* detail) {
    if (!e) return UMGEN_E_INVALID;
    if (shared_slots) *shared_slots = 0;
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_finalize_weights has not been called");
    if (B < 1) return e->fail(UMGEN_E_INVALID, "B=%d: at least one scene", B);
    if (N < 1) return e->fail(UMGEN_E_INVALID, "N=%d: at least one sample per scene", N);
    if ((int64_t)B * N > e->cfg.max_batch) return e->fail(UMGEN_E_INVALID, "B*N=%lld (B=%d, N=%d) exceeds max_batch=%d", (long long)B * N, B, N, e->cfg.max_batch);
    if (N == 1)
        return rollout_driver(e, B, T_in, new_frames, cond_frames, pose, map, bbox3d, image, T_ctl, ctrl_pose, ctrl_bbox3d, control_test, given_map, given_bbox3d,
                              sampling, out_pose, out_map, out_bbox3d, out_image, lp, 0, nullptr, topk, detail);
    // what the replication below reads; the driver checks everything again, and everything else, on the replicated arrays
    if (T_in < 1 || new_frames < 0 || cond_frames < 1 || cond_frames > e->cfg.max_cond_frames)
        return e->fail(UMGEN_E_INVALID, "T_in=%d new_frames=%d cond_frames=%d (max %d)", T_in, new_frames, cond_frames, e->cfg.max_cond_frames);
    if (!pose || !map || !bbox3d || !image || !out_pose || !out_map || !out_bbox3d || !out_image) return e->fail(UMGEN_E_INVALID, "null token buffer");
    if ((ctrl_pose || ctrl_bbox3d) && T_ctl < 1) return e->fail(UMGEN_E_INVALID, "control tokens given with T_ctl=%d", T_ctl);
    if ((given_map || given_bbox3d) && T_ctl < 1) return e->fail(UMGEN_E_INVALID, "given tokens with T_ctl=%d", T_ctl);
    auto replicate = [&](const int64_t* a, size_t per_scene) {      // [B][per_scene] -> [B][N][per_scene]
        std::vector<int64_t> r;
        if (!a) return r;
        r.resize((size_t)B * N * per_scene);
        for (int b = 0; b < B; ++b)
            for (int s = 0; s < N; ++s) memcpy(&r[((size_t)b * N + s) * per_scene], a + (size_t)b * per_scene, per_scene * sizeof(int64_t));
        return r;
    };
    const std::vector<int64_t> rp = replicate(pose, (size_t)T_in * kNPose), rm = replicate(map, (size_t)T_in * kNMap), rb = replicate(bbox3d, (size_t)T_in * kNBox),
                               ri = replicate(image, (size_t)T_in * kNImg), cp = replicate(ctrl_pose, (size_t)T_ctl * kNPose),
                               cb = replicate(ctrl_bbox3d, (size_t)T_ctl * kNBox), gm = replicate(given_map, (size_t)T_ctl * kNMap),
                               gb = replicate(given_bbox3d, (size_t)T_ctl * kNBox);
    return rollout_driver(e, B * N, T_in, new_frames, cond_frames, rp.data(), rm.data(), rb.data(), ri.data(), T_ctl, ctrl_pose ? cp.data() : nullptr,
                          ctrl_bbox3d ? cb.data() : nullptr, control_test, given_map ? gm.data() : nullptr, given_bbox3d ? gb.data() : nullptr, sampling, out_pose,
                          out_map, out_bbox3d, out_image, lp, N, shared_slots, topk, detail);
}

int umgen_rollout_fan(umgen_engine* e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                      const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test,
                      const int64_t* given_map, const int64_t* given_bbox3d, const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map,
                      int64_t* out_bbox3d, int64_t* out_image, const umgen_logp_out* lp, int32_t* shared_slots) {
    return umgen_rollout_detail(e, B, N, T_in, new_frames, cond_frames, pose, map, bbox3d, image, T_ctl, ctrl_pose, ctrl_bbox3d, control_test, given_map,
                                given_bbox3d, sampling, out_pose, out_map, out_bbox3d, out_image, lp, shared_slots, 0, nullptr);
}

int umgen_rollout(umgen_engine* e, int32_t B, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose,
                  const int64_t* map, const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose,
                  const int64_t* ctrl_bbox3d, int32_t control_test, const int64_t* given_map, const int64_t* given_bbox3d,
                  const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image) {
    return umgen_rollout_logp(e, B, T_in, new_frames, cond_frames, pose, map, bbox3d, image, T_ctl, ctrl_pose, ctrl_bbox3d, control_test, given_map,
                              given_bbox3d, sampling, out_pose, out_map, out_bbox3d, out_image, nullptr);
}

}  // extern "C"
