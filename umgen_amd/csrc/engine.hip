// The C ABI of include/umgen.h that drives frames: version and error text, profiling and timings, the argument checks at the ABI boundary,
// umgen_frame(_logp, _detail, _biased), umgen_score(_detail), umgen_score_candidates, umgen_score_futures, umgen_score_clip and the rollout driver
// umgen_rollout(_logp) / umgen_rollout_fan / umgen_rollout_detail / umgen_rollout_biased / umgen_rollout_planned (UMGen.inference).  Every call narrows its int64 tokens once (narrow_tokens) and
// hands them on as a TokenView (token_windows.h); the output structs become [4] arrays through MOD4; the driver keeps one conditioning sequence and
// gathers a frame's window from it, and a frame's control / given tokens are one plan_frame, for the driver and for umgen_frame alike.  Whatever a
// generation call returns beside its tokens -- logp, logz, diagnostics -- is one GenSide (gen_side.h): checked and sized by gen_side_request, handed to
// the frame as FrameIO::side, scattered to the caller's arrays by deliver.  Creation,
// weights, the compute path, the frame itself and the scoring passes are in engine_setup.hip, engine_weights.hip, engine_stacks.hip,
// engine_decode.hip, engine_frame.hip and engine_score.hip.
#include "engine_state.h"

// host arithmetic stays unfused in every engine file, as it was while they were one file behind the numpy-faithful helpers (engine_weights.hip)
#pragma clang fp contract(off)

namespace umgen { thread_local BgRecorder* g_bg_rec = nullptr; }      // bg_queue.h: installed around the recording of a background pass

// ---- helpers of the C ABI below that are templates (or hold one): they need C++ linkage ----

// One group `f` of an output struct of include/umgen.h -- umgen_logp_out, umgen_score_out, umgen_score_detail_out, umgen_gen_detail_out: every group is
// f_pose | f_map | f_bbox3d | f_image -- as a [4] array in the modality order; a null struct gives null pointers
#define MOD4(s, f) {(s) ? (s)->f##_pose : nullptr, (s) ? (s)->f##_map : nullptr, (s) ? (s)->f##_bbox3d : nullptr, (s) ? (s)->f##_image : nullptr}

template <typename D>      // umgen_score_detail_out or umgen_gen_detail_out: one layout
static ScoreDetailIO detail_io(const D* d, int topk, float temperature) {
    return ScoreDetailIO{topk, temperature, MOD4(d, rank), MOD4(d, mass_above), MOD4(d, entropy), MOD4(d, topk_tok), MOD4(d, topk_logp)};
}

// What one frame takes from the control arrays (ctrl_*) and the given arrays (given_*), each NULL or [scenes][T_ctl][S_mod], at their frame idx, for `items`
// branches of N per scene (item i reads scene i / N): the controlled pose cp [items][3], the given map gm and boxes gb [items][S_mod], and with control boxes
// the mask cs [items][60] of the controlled slots -- their tokens, all but -1 = free, overwrite item i's last conditioning frame at box_last + i * box_stride
// (UMGen.py:1458-1473).  Empty where the frame takes nothing.  The frame's asynchronous uploads read these until its synchronisation
struct FramePlan {
    std::vector<int> cp, gm, gb;
    std::vector<unsigned char> cs;
    template <typename V> static const V* ptr(const std::vector<V>& v) { return v.empty() ? nullptr : v.data(); }
};
static void plan_frame(int items, int N, int T_ctl, int idx, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, const int64_t* given_map,
                       const int64_t* given_bbox3d, int* box_last, size_t box_stride, FramePlan& p) {
    const auto at = [&](const int64_t* a, int i, int len) { return a + ((size_t)(i / N) * T_ctl + idx) * len; };
    const auto take = [&](const int64_t* a, int len, std::vector<int>& out) {
        out.resize(a ? (size_t)items * len : 0);
        for (int i = 0; a && i < items; ++i)
            for (int k = 0; k < len; ++k) out[(size_t)i * len + k] = (int)at(a, i, len)[k];
    };
    take(ctrl_pose, kNPose, p.cp);
    take(given_map, kNMap, p.gm);
    take(given_bbox3d, kNBox, p.gb);
    p.cs.assign(ctrl_bbox3d ? (size_t)items * kSlots : 0, 0);
    for (int i = 0; ctrl_bbox3d && i < items; ++i)
        for (int k = 0; k < kNBox; ++k) {
            const int64_t v = at(ctrl_bbox3d, i, kNBox)[k];
            if (v != -1) { box_last[i * box_stride + k] = (int)v; p.cs[(size_t)i * kSlots + k / kSlotLen] = 1; }
        }
}

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
    const std::string m = sampling_error(*s);      // (sample_plan.h: the same check serves every per_scene entry of a planned call)
    return m.empty() ? 0 : e->fail(UMGEN_E_INVALID, "%s", m.c_str());
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

static ScoreDst score_dst(const umgen_score_out* o) { return ScoreDst{MOD4(o, logp), MOD4(o, argmax)}; }
static bool wants_lists(const ScoreDetailIO& d) {
    bool lists = false;
    for (int m = 0; m < 4; ++m) lists = lists || d.topk_tok[m] || d.topk_logp[m];
    return lists;
}
// what umgen_score_detail and the generation calls refuse of a detail request
static int check_detail_request(umgen_engine* e, const ScoreDetailIO& d) {
    if (d.topk < 0 || d.topk > UMGEN_SCORE_TOPK_MAX) return e->fail(UMGEN_E_INVALID, "topk=%d out of range [0,%d]", d.topk, UMGEN_SCORE_TOPK_MAX);
    if (!(d.temperature > 0.f) || !(d.temperature <= 3.0e38f)) return e->fail(UMGEN_E_INVALID, "temperature must be > 0 and finite");
    if (wants_lists(d) && d.topk == 0) return e->fail(UMGEN_E_INVALID, "top-K outputs requested with topk = 0");
    return 0;
}

// The side outputs of a generation call over `items` scenes: refuses of the diagnostics what umgen_score_detail refuses (a NULL or all-NULL struct asks for
// nothing and is not checked further), then sizes gs from what the caller's structs ask for
static int gen_side_request(umgen_engine* e, const umgen_logp_out* lp, const umgen_logz_out* lz, const umgen_gen_detail_out* d, int32_t k,
                            const umgen_sampling* s, size_t items, GenSide& gs) {
    const SideDst dst{MOD4(lp, logp), MOD4(lz, logz), MOD4(d, rank), MOD4(d, mass_above), MOD4(d, entropy), MOD4(d, topk_tok), MOD4(d, topk_logp), k};
    if (dst.wants_detail()) { if (int rc = check_detail_request(e, detail_io(d, k, s->temperature))) return rc; }
    gs.init(dst, items);
    return 0;
}

// The logit-bias tables of a call (umgen_logit_bias) behind their checks, before anything reaches the device: entries are finite or -inf (a ban), every
// row keeps an allowed entry, and with control slots a bbox3d row must allow more than vocab - 1 (the control resample masks that index).  -> the bit
// per class with a table (OarState::bias_classes); host receives the tables in d_bias' layout (absent classes stay 0 and are never read)
static int check_bias(umgen_engine* e, const umgen_logit_bias* bias, bool control_slots, std::vector<float>& host, int* classes) {
    *classes = 0;
    if (!bias) return 0;
    const float* const tab[4] = {bias->pose, bias->map, bias->bbox3d, bias->image};
    const int vocab[4] = {e->cfg.pose_vocab, e->cfg.map_vocab, e->cfg.bbox3d_vocab, e->cfg.img_vocab};
    const std::string m = bias_tables_error(tab, vocab, kBiasRowLen, control_slots, classes);      // (sample_plan.h)
    if (!m.empty()) return e->fail(UMGEN_E_INVALID, "%s", m.c_str());
    if (!*classes) return 0;
    host.assign(e->bias_floats(), 0.f);
    for (int c = 0; c < 4; ++c)
        if (tab[c]) memcpy(host.data() + e->bias_offset(c), tab[c], (size_t)kPlanTableRows[c] * vocab[c] * sizeof(float));
    return 0;
}
// ... and onto the device, on the engine's stream and finished before the call's first frame starts (a frame may run on another stream of the engine)
static int upload_bias(umgen_engine* e, const std::vector<float>& host) {
    if (host.empty()) return 0;
    HIPCHK(e, hipMemcpyAsync(e->d_bias, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return 0;
}

// What a planned call (umgen_sample_plan) brings, behind its checks and before anything reaches the device.  plan == NULL, or a plan without per_scene
// entries and without an index array, resolves to the unplanned call: bits 0, its one set (if any) in set 0 of the pool.
struct PlanHost {
    int bits = 0;                      // OarState::plan
    int classes0 = 0;                  // the class bits of set 0 (OarState::bias_classes of the unplanned form)
    std::vector<SamplerParams> sp;     // [items] with kPlanSettings
    PlanIndex idx;                     // [items][new_frames] with kPlanSets
    std::vector<float> pool;           // [n_sets][bias_floats()], absent classes 0 (never read)
    int set_classes[kBiasSetsMax] = {};
};
static SamplerParams sampler_params(const umgen_sampling& s) {
    return SamplerParams{s.method, s.top_k, s.top_k_map, s.topk_image, s.p, s.p_map, s.temperature, s.rule_constrain, s.merge_ar_tar, s.only_ar};
}
static int check_plan(umgen_engine* e, const umgen_sample_plan* plan, const umgen_sampling* sampling, int items, int new_frames, bool control_slots,
                      bool wants_detail, PlanHost& ph) {
    if (!plan) return 0;
    if (plan->per_scene) {
        const std::string m = plan_settings_error(*sampling, plan->per_scene, items);
        if (!m.empty()) return e->fail(UMGEN_E_INVALID, "%s", m.c_str());
        for (int i = 0; wants_detail && i < items; ++i)      // (check_detail_request's bar on the call's temperature, per scene)
            if (!(plan->per_scene[i].temperature <= 3.0e38f)) return e->fail(UMGEN_E_INVALID, "sample plan: per_scene[%d]: temperature must be > 0 and finite", i);
        ph.sp.resize((size_t)items);
        for (int i = 0; i < items; ++i) ph.sp[(size_t)i] = sampler_params(plan->per_scene[i]);
        ph.bits |= kPlanSettings;
    }
    {
        const std::string m = plan_index_error(items, new_frames, plan->n_bias_sets, plan->bias_of, ph.idx);
        if (!m.empty()) return e->fail(UMGEN_E_INVALID, "%s", m.c_str());
    }
    if (plan->n_bias_sets > 0 && !plan->bias_sets) return e->fail(UMGEN_E_INVALID, "sample plan: n_bias_sets=%d with bias_sets = NULL", plan->n_bias_sets);
    // every set is validated, used or not; the control-slot rule holds for the sets some scene uses
    const bool named = plan->bias_of != nullptr || plan->n_bias_sets > 1;      // (umgen_rollout_biased's one set keeps its messages)
    ph.pool.assign((size_t)plan->n_bias_sets * e->bias_floats(), 0.f);
    for (int s = 0; s < plan->n_bias_sets; ++s) {
        std::vector<float> host;
        if (int rc = check_bias(e, &plan->bias_sets[s], control_slots && ph.idx.uses(s), host, &ph.set_classes[s])) {
            if (named) e->err = "sample plan: bias set " + std::to_string(s) + ": " + e->err;
            return rc;
        }
        if (!host.empty()) memcpy(ph.pool.data() + (size_t)s * e->bias_floats(), host.data(), host.size() * sizeof(float));
    }
    ph.classes0 = ph.set_classes[0];
    if (plan->bias_of) ph.bits |= kPlanSets;
    return 0;
}
// ... and onto the device like upload_bias: the pool, the sets' class bits and the per-scene settings, once per call
static int upload_plan(umgen_engine* e, const PlanHost& ph) {
    if (ph.bits == 0 && ph.classes0 == 0) return 0;      // nothing a sampler of this call reads
    if (!ph.pool.empty()) HIPCHK(e, hipMemcpyAsync(e->d_bias, ph.pool.data(), ph.pool.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (ph.bits & kPlanSets) HIPCHK(e, hipMemcpyAsync(e->d_set_classes, ph.set_classes, sizeof(ph.set_classes), hipMemcpyHostToDevice, e->stream));
    if (ph.bits & kPlanSettings) HIPCHK(e, hipMemcpyAsync(e->dv.d_sp_of, ph.sp.data(), ph.sp.size() * sizeof(SamplerParams), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return 0;
}

int umgen_frame_biased(umgen_engine* e, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                       const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test, const umgen_sampling* sampling,
                       int32_t frame_idx, const umgen_trace* trace, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                       const umgen_logp_out* lp, int32_t topk, const umgen_gen_detail_out* detail, const umgen_logit_bias* bias, const umgen_logz_out* lz) {
    if (!e) return UMGEN_E_INVALID;
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_finalize_weights has not been called");
    if (T < 1 || T > e->cfg.max_cond_frames) return e->fail(UMGEN_E_INVALID, "T=%d out of range [1,%d]", T, e->cfg.max_cond_frames);
    if (int rc = check_sampling(e, sampling)) return rc;
    GenSide gs;
    if (int rc = gen_side_request(e, lp, lz, detail, topk, sampling, 1, gs)) return rc;
    if (!pose || !map || !bbox3d || !image || !out_pose || !out_map || !out_bbox3d || !out_image) return e->fail(UMGEN_E_INVALID, "null token buffer");
    if (int rc = check_scene_tokens(e, (size_t)T, pose, map, bbox3d, image)) return rc;
    if (ctrl_pose) { if (int rc = check_tokens(e, "control pose", ctrl_pose, 3, e->cfg.pose_vocab, false)) return rc; }
    if (ctrl_bbox3d) { if (int rc = check_tokens(e, "control bbox3d", ctrl_bbox3d, kNBox, e->cfg.bbox3d_vocab, true)) return rc; }
    if (ctrl_bbox3d && !control_test) return e->fail(UMGEN_E_UNSUPPORTED, "init_tokens['bbox3d'] without control_test is not a supported reference path");
    // the frame's GIVEN tokens (umgen_rollout's given_* for one frame: the predefined-token prefix of infer_oar_net, UMGen.py:1184-1201)
    const int64_t* const given_map = trace ? trace->given_map : nullptr;
    const int64_t* const given_bbox3d = trace ? trace->given_bbox3d : nullptr;
    if (given_bbox3d && !given_map)
        return e->fail(UMGEN_E_UNSUPPORTED, "given bbox3d tokens without a given map: the reference would put them on the map's positions (UMGen.py:1190-1201)");
    if (given_map) {
        if (control_test) return e->fail(UMGEN_E_UNSUPPORTED, "given tokens and control_test exclude each other");
        if (int rc = check_tokens(e, "given map", given_map, kNMap, e->cfg.map_vocab, false)) return rc;
        if (given_bbox3d) { if (int rc = check_tokens(e, "given bbox3d", given_bbox3d, kNBox, e->cfg.bbox3d_vocab, false)) return rc; }
    }
    std::vector<float> bias_host;
    int bias_classes = 0;
    if (int rc = check_bias(e, bias, ctrl_bbox3d && control_test, bias_host, &bias_classes)) return rc;
    if (int rc = upload_bias(e, bias_host)) return rc;
    const int64_t* const in[4] = {pose, map, bbox3d, image};
    int64_t* const outp[4] = {out_pose, out_map, out_bbox3d, out_image};
    TokenSeqs win;
    narrow_tokens(in, 1, T, win);
    FramePlan plan;      // the rollout's plan for one scene and one frame of control / given tokens (the boxes overwrite window slot T - 1)
    plan_frame(1, 1, 1, 0, ctrl_pose, ctrl_bbox3d, given_map, given_bbox3d, win.at(2, 0, T - 1), 0, plan);
    std::vector<int> out(kTokPerFrame);
    FrameIO io{1, T, win.view(), FramePlan::ptr(plan.cp), FramePlan::ptr(plan.cs), frame_idx, sampling, trace, out.data()};
    io.given_map = FramePlan::ptr(plan.gm);
    io.given_box = FramePlan::ptr(plan.gb);
    io.side = gs.frame();
    io.bias_classes = bias_classes;
    if (int rc = run_frame_any(e, io)) return rc;
    gs.deliver(0, 0);
    for (int m = 0; m < 4; ++m)
        for (int i = 0; i < kModLen[m]; ++i) outp[m][i] = out[kModOff[m] + i];
    return UMGEN_OK;
}

int umgen_frame_detail(umgen_engine* e, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                       const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test, const umgen_sampling* sampling,
                       int32_t frame_idx, const umgen_trace* trace, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                       const umgen_logp_out* lp, int32_t topk, const umgen_gen_detail_out* detail) {
    return umgen_frame_biased(e, T, pose, map, bbox3d, image, ctrl_pose, ctrl_bbox3d, control_test, sampling, frame_idx, trace, out_pose, out_map,
                              out_bbox3d, out_image, lp, topk, detail, nullptr, nullptr);
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

// n frames, int64 [n][S_mod] per modality, as int32 rows [n][2199] pose | map | bbox3d | image
static std::vector<int> narrow_frame_rows(const int64_t* const in[4], size_t n) {
    TokenSeqs t;
    narrow_tokens(in, n, 1, t);
    std::vector<int> rows(n * kTokPerFrame);
    frame_rows(t.view(), n, [](size_t i) { return i; }, [](size_t) { return 0; }, rows.data());
    return rows;
}

// umgen_score and umgen_score_detail: log p of a given next frame per content position (the reference's loss terms, UMGen.py:539-582) for B scenes, and
// with `detail` the diagnostics of the same rows: engine_score.hip run_score
static int score_call(umgen_engine* e, int32_t B, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                      const int64_t* next_pose, const int64_t* next_map, const int64_t* next_bbox3d, const int64_t* next_image, umgen_score_out* out,
                      const umgen_score_detail_out* d, int32_t topk, float temperature) {
    const int64_t *in[4] = {pose, map, bbox3d, image}, *nx[4] = {next_pose, next_map, next_bbox3d, next_image};
    if (int rc = check_score_engine(e, B)) return rc;
    if (int rc = check_window_length(e, T)) return rc;
    const ScoreDetailIO dio = detail_io(d, topk, temperature);
    if (d) { if (int rc = check_detail_request(e, dio)) return rc; }
    if (int rc = check_score_common(e, out || d, in, (size_t)B * T, nx, (size_t)B, "next frame")) return rc;
    TokenSeqs win;
    narrow_tokens(in, B, T, win);
    const std::vector<int> next = narrow_frame_rows(nx, (size_t)B);
    ScoreIO sc{B, T, win.view(), next.data(), score_dst(out)};
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
    TokenSeqs win;
    narrow_tokens(in, B, T, win);
    const std::vector<int> next = narrow_frame_rows(nx, (size_t)B * C);
    ScoreCandIO sc{B, T, C, win.view(), next.data(), score_dst(out), 0};
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
    TokenSeqs win, fut;
    narrow_tokens(in, B, T, win);
    narrow_tokens(nx, (size_t)B * C, K, fut);
    const ScoreFutIO sc{B, T, C, K, cond_frames, win.view(), fut.view(), score_dst(out), shared_slots};
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
    TokenSeqs clip;
    narrow_tokens(in, B, L, clip);
    ScoreClipIO sc{B, L, T_in, cond_frames, clip.view(), score_dst(out), 0};
    if (int rc = run_score_clip_any(e, sc)) return rc;
    if (shared_frames) *shared_frames = sc.shared_frames;
    return UMGEN_OK;
}

// What every rollout call refuses, in this order, on the caller's arrays: B scenes, whatever the number of branches
static int check_rollout(umgen_engine* e, int32_t B, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* const in[4], int32_t T_ctl,
                         const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test, const int64_t* given_map, const int64_t* given_bbox3d,
                         const umgen_sampling* sampling, int64_t* const out[4], GenSide& gs, size_t branches, const umgen_logp_out* lp, const umgen_logz_out* lz, int32_t topk,
                         const umgen_gen_detail_out* detail) {
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_finalize_weights has not been called");
    if (B < 1 || B > e->cfg.max_batch) return e->fail(UMGEN_E_INVALID, "B=%d out of range [1,%d]", B, e->cfg.max_batch);
    if (T_in < 1 || new_frames < 0 || cond_frames < 1 || cond_frames > e->cfg.max_cond_frames)
        return e->fail(UMGEN_E_INVALID, "T_in=%d new_frames=%d cond_frames=%d (max %d)", T_in, new_frames, cond_frames, e->cfg.max_cond_frames);
    if (int rc = check_sampling(e, sampling)) return rc;
    if (int rc = gen_side_request(e, lp, lz, detail, topk, sampling, branches, gs)) return rc;
    for (int m = 0; m < 4; ++m)
        if (!in[m] || !out[m]) return e->fail(UMGEN_E_INVALID, "null token buffer");
    if (int rc = check_scene_tokens(e, (size_t)B * T_in, in[0], in[1], in[2], in[3])) return rc;
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
    return 0;
}

// UMGen.inference (UMGen.py:1542-1671) for B scenes of N branches each: branch i = (b, s) at b*N + s reads scene i / N of the caller's arrays and has its own
// seed, so every output is [B][N][..] = [B * N][..].  The driver keeps ONE int32 conditioning sequence per modality, seq [B * N][T_in + new_frames][S_mod]: filled
// from the input once, every new frame written behind it, and frame f = T_in + idx conditioned on the window cond_window(f, cond_frames) of it.  Control boxes
// overwrite frame f - 1 of seq in place, so the overwrite stays in later windows ("cond_tokens", UMGen.py:1465-1467); out_* receive the inputs and what was
// generated, never the overwrite.  Control and given tokens apply while idx < T_ctl (get_mod_tokens returns None past the end, and the pose tokens take
// control mode with them, UMGen.py:1605-1619).  N >= 2 (umgen_rollout_fan): the first frame runs its history once per scene (run_frame_fan) when its window has
// at least two slots, the slot caches fit and UMGEN_FAN_SHARE is not 0, and *shared_slots reports the slots that were shared.
static int rollout_driver(umgen_engine* e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                          const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test,
                          const int64_t* given_map, const int64_t* given_bbox3d, const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map,
                          int64_t* out_bbox3d, int64_t* out_image, const umgen_logp_out* lp, int32_t* shared_slots, int32_t topk,
                          const umgen_gen_detail_out* detail, const umgen_sample_plan* splan, const umgen_logz_out* lz) {
    if (!e) return UMGEN_E_INVALID;
    const int64_t* const in[4] = {pose, map, bbox3d, image};
    int64_t* const out[4] = {out_pose, out_map, out_bbox3d, out_image};
    const int BN = B * N, T_out = T_in + new_frames;
    GenSide gs;      // a frame's side outputs are scattered to [B * N][new_frames][S_mod] below
    if (int rc = check_rollout(e, B, T_in, new_frames, cond_frames, in, T_ctl, ctrl_pose, ctrl_bbox3d, control_test, given_map, given_bbox3d, sampling, out, gs,
                               (size_t)BN, lp, lz, topk, detail))
        return rc;
    // the call's plan: per-scene settings, the pool of table sets and which set scene i draws under in new frame f.  An unplanned call (one set of tables, or
    // none, for every scene, branch and frame) leaves ph.bits 0 and takes the path it always took
    PlanHost ph;
    const SideDst want{MOD4(lp, logp), MOD4(lz, logz), MOD4(detail, rank), MOD4(detail, mass_above), MOD4(detail, entropy), MOD4(detail, topk_tok), MOD4(detail, topk_logp), topk};
    if (int rc = check_plan(e, splan, sampling, BN, new_frames, ctrl_bbox3d && control_test, want.wants_detail(), ph)) return rc;
    if (int rc = upload_plan(e, ph)) return rc;
    std::vector<int> set_of((size_t)BN, -1);      // column idx of the plan's index (the frame's upload reads it until the frame's synchronisation)
    e->tm = umgen_timings{};
    e->overlap_suspended = false;
    TokenSeqs seq, win;      // (win: the frame's asynchronous uploads read it until the frame's synchronisation)
    seq.resize(BN, T_out);
    for (int m = 0; m < 4; ++m)      // out_tokens and cond_tokens both start as the first T_in frames (UMGen.py:1581-1595)
        for (int i = 0; i < BN; ++i) {
            const size_t len = (size_t)T_in * kModLen[m];
            const int64_t* src = in[m] + (size_t)(i / N) * len;
            for (size_t k = 0; k < len; ++k) { out[m][(size_t)i * T_out * kModLen[m] + k] = src[k]; seq.at(m, i, 0)[k] = (int)src[k]; }
        }
    std::vector<int> frame_out((size_t)BN * kTokPerFrame);
    for (int idx = 0; idx < new_frames; ++idx) {
        const int f = T_in + idx;
        const CondWindow w = cond_window(f, cond_frames);
        const bool ctl = idx < T_ctl;
        if (ctl && ctrl_bbox3d && !control_test) return e->fail(UMGEN_E_UNSUPPORTED, "init_tokens['bbox3d'] without control_test is not a supported reference path");
        FramePlan plan;
        plan_frame(BN, N, T_ctl, idx, ctl ? ctrl_pose : nullptr, ctl ? ctrl_bbox3d : nullptr, ctl ? given_map : nullptr, ctl && given_map ? given_bbox3d : nullptr,
                   seq.at(2, 0, f - 1), (size_t)T_out * kNBox, plan);
        gather_windows(seq.view(), BN, w.start, w.n, win);
        FrameIO io{BN, w.n, win.view(), FramePlan::ptr(plan.cp), FramePlan::ptr(plan.cs), idx, sampling, nullptr, frame_out.data()};
        io.cond_cap = cond_frames;
        io.next_follows = idx + 1 < new_frames;
        io.next_has_ctrl_pose = ctrl_pose && idx + 1 < T_ctl;
        io.given_map = FramePlan::ptr(plan.gm);
        io.given_box = FramePlan::ptr(plan.gb);
        io.side = gs.frame();
        io.plan = ph.bits;
        if (ph.bits & kPlanSets) {
            ph.idx.column(idx, set_of.data());
            io.bias_set_of = set_of.data();
        } else {
            io.bias_classes = ph.classes0;
        }
        const char* fse = getenv("UMGEN_FAN_SHARE");      // (read per call: the tests compare both forms in one process)
        const bool fan = idx == 0 && N >= 2 && w.n >= 2 && !(fse && fse[0] == '0') && ensure_tcache(e);
        if (fan && shared_slots) *shared_slots = w.n - 1;
        if (int rc = fan ? run_frame_fan_any(e, io, N) : run_frame_any(e, io)) return rc;
        // the new frame (UMGen.py:1636-1666): control pose tokens are copied verbatim; everything else is what was generated
        for (int m = 0; m < 4; ++m)
            for (int i = 0; i < BN; ++i) {
                const size_t src = (size_t)i * kTokPerFrame + kModOff[m], len = (size_t)kModLen[m];
                memcpy(seq.at(m, i, f), &frame_out[src], len * sizeof(int));
                for (size_t k = 0; k < len; ++k) out[m][((size_t)i * T_out + f) * len + k] = frame_out[src + k];
            }
        for (int i = 0; i < BN; ++i) gs.deliver((size_t)i, (size_t)i * new_frames + idx);
    }
    return UMGEN_OK;
}

int umgen_rollout_logp(umgen_engine* e, int32_t B, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose,
                       const int64_t* map, const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose,
                       const int64_t* ctrl_bbox3d, int32_t control_test, const int64_t* given_map, const int64_t* given_bbox3d,
                       const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                       const umgen_logp_out* lp) {
    return rollout_driver(e, B, 1, T_in, new_frames, cond_frames, pose, map, bbox3d, image, T_ctl, ctrl_pose, ctrl_bbox3d, control_test, given_map, given_bbox3d,
                          sampling, out_pose, out_map, out_bbox3d, out_image, lp, nullptr, 0, nullptr, nullptr, nullptr);
}

// umgen_rollout_fan: N sampled futures per scene, the driver above with N branches per scene, whose first frame shares the history between a scene's branches
// (engine_frame.hip run_frame_fan).  Every argument is checked once, on the caller's arrays: an error that names a flat index names it there.
// umgen_rollout_detail: the same with the diagnostics of every generated token ([B][N][..] likewise)
// umgen_rollout_planned: the same with the call's sampling plan (per-scene settings, per-scene and per-frame table sets) and logz of every sampled position
int umgen_rollout_planned(umgen_engine* e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                          const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test,
                          const int64_t* given_map, const int64_t* given_bbox3d, const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map,
                          int64_t* out_bbox3d, int64_t* out_image, const umgen_logp_out* lp, int32_t* shared_slots, int32_t topk,
                          const umgen_gen_detail_out* detail, const umgen_sample_plan* plan, const umgen_logz_out* lz) {
    if (!e) return UMGEN_E_INVALID;
    if (shared_slots) *shared_slots = 0;
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_finalize_weights has not been called");
    if (B < 1) return e->fail(UMGEN_E_INVALID, "B=%d: at least one scene", B);
    if (N < 1) return e->fail(UMGEN_E_INVALID, "N=%d: at least one sample per scene", N);
    if ((int64_t)B * N > e->cfg.max_batch) return e->fail(UMGEN_E_INVALID, "B*N=%lld (B=%d, N=%d) exceeds max_batch=%d", (long long)B * N, B, N, e->cfg.max_batch);
    return rollout_driver(e, B, N, T_in, new_frames, cond_frames, pose, map, bbox3d, image, T_ctl, ctrl_pose, ctrl_bbox3d, control_test, given_map, given_bbox3d,
                          sampling, out_pose, out_map, out_bbox3d, out_image, lp, shared_slots, topk, detail, plan, lz);
}

// umgen_rollout_biased: the plan of one set for every scene, branch and frame (none without a bias)
int umgen_rollout_biased(umgen_engine* e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                         const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test,
                         const int64_t* given_map, const int64_t* given_bbox3d, const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map,
                         int64_t* out_bbox3d, int64_t* out_image, const umgen_logp_out* lp, int32_t* shared_slots, int32_t topk,
                         const umgen_gen_detail_out* detail, const umgen_logit_bias* bias, const umgen_logz_out* lz) {
    const umgen_sample_plan one{nullptr, 1, bias, nullptr};
    return umgen_rollout_planned(e, B, N, T_in, new_frames, cond_frames, pose, map, bbox3d, image, T_ctl, ctrl_pose, ctrl_bbox3d, control_test, given_map,
                                 given_bbox3d, sampling, out_pose, out_map, out_bbox3d, out_image, lp, shared_slots, topk, detail, bias ? &one : nullptr, lz);
}

int umgen_rollout_detail(umgen_engine* e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                         const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test,
                         const int64_t* given_map, const int64_t* given_bbox3d, const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map,
                         int64_t* out_bbox3d, int64_t* out_image, const umgen_logp_out* lp, int32_t* shared_slots, int32_t topk,
                         const umgen_gen_detail_out* detail) {
    return umgen_rollout_biased(e, B, N, T_in, new_frames, cond_frames, pose, map, bbox3d, image, T_ctl, ctrl_pose, ctrl_bbox3d, control_test, given_map,
                                given_bbox3d, sampling, out_pose, out_map, out_bbox3d, out_image, lp, shared_slots, topk, detail, nullptr, nullptr);
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
