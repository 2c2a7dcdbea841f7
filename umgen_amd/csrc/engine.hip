// The C ABI of include/umgen.h that drives frames: version and error text, profiling and timings, umgen_frame(_logp, _detail, _biased), umgen_score(_detail),
// umgen_score_candidates, umgen_score_futures, umgen_score_clip and umgen_rollout(_logp) / umgen_rollout_fan / umgen_rollout_detail / umgen_rollout_biased /
// umgen_rollout_planned (UMGen.inference).  Each of the ten generation entry points fills one GenCall (gen_call.h) -- no rung calls another -- and hands it
// to rollout_call or frame_call.  Both admit the call the same way (admit_call): the argument checks of gen_call.h against the engine's GenLimits; the
// side outputs the caller asked for -- logp, logz, diagnostics: one SideDst per call (side_dst), sized into one GenSide (gen_side.h), handed to the frame
// as FrameIO::side, scattered to the caller's arrays by deliver; and the call's plan behind check_plan / upload_plan: the tables of umgen_rollout_biased /
// umgen_frame_biased are the plan of one set that every scene draws under in every frame, and run as that plan (OarState::plan, DrawPlan).  The driver keeps one conditioning sequence and gathers a frame's window from it; a frame's control / given
// tokens are one plan_frame and its FrameIO one frame_io, for the driver and for the frame call alike.  The scoring calls narrow their int64 tokens once
// (narrow_tokens) and hand them on as a TokenView (token_windows.h).  Creation, weights, the compute path, the frame itself and the scoring passes are in
// engine_setup.hip, engine_weights.hip, engine_stacks.hip, engine_decode.hip, engine_frame.hip and engine_score.hip.
#include "engine_state.h"
#include "gen_call.h"

// host arithmetic stays unfused in every engine file, as it was while they were one file behind the numpy-faithful helpers (engine_weights.hip)
#pragma clang fp contract(off)

namespace umgen { thread_local BgRecorder* g_bg_rec = nullptr; }      // bg_queue.h: installed around the recording of a background pass

// One group `f` of an output struct of include/umgen.h -- umgen_logp_out, umgen_score_out, umgen_score_detail_out, umgen_gen_detail_out: every group is
// f_pose | f_map | f_bbox3d | f_image -- as a [4] array in the modality order; a null struct gives null pointers
#define MOD4(s, f) {(s) ? (s)->f##_pose : nullptr, (s) ? (s)->f##_map : nullptr, (s) ? (s)->f##_bbox3d : nullptr, (s) ? (s)->f##_image : nullptr}

static ScoreDetailIO detail_io(const umgen_score_detail_out* d, int topk, float temperature) {
    return ScoreDetailIO{topk, temperature, MOD4(d, rank), MOD4(d, mass_above), MOD4(d, entropy), MOD4(d, topk_tok), MOD4(d, topk_logp)};
}
static ScoreDst score_dst(const umgen_score_out* o) { return ScoreDst{MOD4(o, logp), MOD4(o, argmax)}; }
static bool wants_lists(const ScoreDetailIO& d) { return SideDst::any(d.topk_tok) || SideDst::any(d.topk_logp); }
// the side request of a generation call, once per call: what the caller's structs ask for (a NULL or all-NULL struct asks for nothing)
static SideDst side_dst(const umgen_logp_out* lp, const umgen_logz_out* lz, const umgen_gen_detail_out* d, int32_t topk) {
    return SideDst{MOD4(lp, logp), MOD4(lz, logz), MOD4(d, rank), MOD4(d, mass_above), MOD4(d, entropy), MOD4(d, topk_tok), MOD4(d, topk_logp), topk};
}

// what the checks of gen_call.h read of the engine, and their refusal as the engine's error
static GenLimits limits_of(const umgen_engine* e) {
    return GenLimits{e->finalized, e->cfg.max_batch, e->cfg.max_cond_frames, {e->cfg.pose_vocab, e->cfg.map_vocab, e->cfg.bbox3d_vocab, e->cfg.img_vocab}};
}
static int refuse(umgen_engine* e, const Refusal& r) { return r.code ? e->fail(r.code, "%s", r.msg.c_str()) : 0; }

// ---- a generation call (GenCall, gen_call.h) from its checks to its frames ----

// What one frame takes from the control arrays (ctrl_*) and the given arrays (given_*) of its call, each NULL or [scenes][T_ctl][S_mod], at their frame idx
// -- nothing from T_ctl on: get_mod_tokens returns None past the end, and the pose tokens take control mode with them (UMGen.py:1605-1619) -- for the
// call's items, branches of N per scene (item i reads scene i / N): the controlled pose cp [items][3], the given map gm and boxes gb [items][S_mod], and
// with control boxes the mask cs [items][60] of the controlled slots -- their tokens, all but -1 = free, overwrite item i's last conditioning frame at
// box_last + i * box_stride (UMGen.py:1458-1473).  Empty where the frame takes nothing.  The frame's asynchronous uploads read these until its synchronisation
struct FramePlan {
    std::vector<int> cp, gm, gb;
    std::vector<unsigned char> cs;
    template <typename V> static const V* ptr(const std::vector<V>& v) { return v.empty() ? nullptr : v.data(); }
};
static void plan_frame(const GenCall& c, int idx, int* box_last, size_t box_stride, FramePlan& p) {
    const int items = c.items();
    const bool ctl = idx < c.T_ctl;
    const int64_t* const ctrl_bbox3d = ctl ? c.ctrl_bbox3d : nullptr;
    const auto at = [&](const int64_t* a, int i, int len) { return a + ((size_t)(i / c.N) * c.T_ctl + idx) * len; };
    const auto take = [&](const int64_t* a, int len, std::vector<int>& out) {
        out.resize(a ? (size_t)items * len : 0);
        for (int i = 0; a && i < items; ++i)
            for (int k = 0; k < len; ++k) out[(size_t)i * len + k] = (int)at(a, i, len)[k];
    };
    take(ctl ? c.ctrl_pose : nullptr, kNPose, p.cp);
    take(ctl ? c.given_map : nullptr, kNMap, p.gm);
    take(ctl && c.given_map ? c.given_bbox3d : nullptr, kNBox, p.gb);
    p.cs.assign(ctrl_bbox3d ? (size_t)items * kSlots : 0, 0);
    for (int i = 0; ctrl_bbox3d && i < items; ++i)
        for (int k = 0; k < kNBox; ++k) {
            const int64_t v = at(ctrl_bbox3d, i, kNBox)[k];
            if (v != -1) { box_last[i * box_stride + k] = (int)v; p.cs[(size_t)i * kSlots + k / kSlotLen] = 1; }
        }
}

// What a call's plan (umgen_sample_plan) brings, behind its checks and before anything reaches the device.  plan == NULL, or a plan without per_scene
// entries and without sets, resolves to bits 0.  One set without an index array (umgen_rollout_biased / umgen_frame_biased) is the plan whose index is 0
// everywhere: its set lands in set 0 of the pool.
struct PlanHost {
    int bits = 0;                      // OarState::plan
    std::vector<SamplerParams> sp;     // [items] with kPlanSettings
    PlanIndex idx;                     // [items][new_frames] with kPlanSets
    std::vector<float> pool;           // [n_sets][DrawPlan::stride], absent classes 0 (never read)
    int set_classes[kBiasSetsMax] = {};
};
static SamplerParams sampler_params(const umgen_sampling& s) {
    return SamplerParams{s.method, s.top_k, s.top_k_map, s.topk_image, s.p, s.p_map, s.temperature, s.rule_constrain, s.merge_ar_tar, s.only_ar};
}
// One set of logit-bias tables (umgen_logit_bias) behind its checks: entries are finite or -inf (a ban), every row keeps an allowed entry, and with control
// slots a bbox3d row must allow more than vocab - 1 (the control resample masks that index).  -> the bit per class with a table (DrawPlan::set_classes);
// dst, a zeroed set of the pool, receives the tables in the pool's layout (absent classes stay 0 and are never read)
static int check_bias(umgen_engine* e, const umgen_logit_bias& bias, bool control_slots, float* dst, int* classes) {
    const float* const tab[4] = {bias.pose, bias.map, bias.bbox3d, bias.image};
    const GenLimits lim = limits_of(e);
    const std::string m = bias_tables_error(tab, lim.vocab, kBiasRowLen, control_slots, classes);      // (sample_plan.h)
    if (!m.empty()) return e->fail(UMGEN_E_INVALID, "%s", m.c_str());
    for (int c = 0; c < 4; ++c)
        if (tab[c]) memcpy(dst + e->dv.d_plan.class_off[c], tab[c], (size_t)kPlanTableRows[c] * lim.vocab[c] * sizeof(float));
    return 0;
}
static int check_plan(umgen_engine* e, const GenCall& c, PlanHost& ph) {
    const umgen_sample_plan* const plan = c.plan;
    const int items = c.items();
    if (!plan) return 0;
    if (plan->per_scene) {
        const std::string m = plan_settings_error(*c.sampling, plan->per_scene, items);
        if (!m.empty()) return e->fail(UMGEN_E_INVALID, "%s", m.c_str());
        for (int i = 0; c.side.wants_detail() && i < items; ++i)      // (check_detail_request's bar on the call's temperature, per scene)
            if (!(plan->per_scene[i].temperature <= 3.0e38f)) return e->fail(UMGEN_E_INVALID, "sample plan: per_scene[%d]: temperature must be > 0 and finite", i);
        ph.sp.resize((size_t)items);
        for (int i = 0; i < items; ++i) ph.sp[(size_t)i] = sampler_params(plan->per_scene[i]);
        ph.bits |= kPlanSettings;
    }
    {
        const std::string m = plan_index_error(items, c.new_frames, plan->n_bias_sets, plan->bias_of, ph.idx);
        if (!m.empty()) return e->fail(UMGEN_E_INVALID, "%s", m.c_str());
    }
    if (plan->n_bias_sets > 0 && !plan->bias_sets) return e->fail(UMGEN_E_INVALID, "sample plan: n_bias_sets=%d with bias_sets = NULL", plan->n_bias_sets);
    // every set is validated, used or not; the control-slot rule holds for the sets some scene uses
    const bool named = plan->bias_of != nullptr || plan->n_bias_sets > 1;      // (the one set of umgen_rollout_biased / umgen_frame_biased keeps its messages)
    const size_t set_len = (size_t)e->dv.d_plan.stride;
    ph.pool.assign((size_t)plan->n_bias_sets * set_len, 0.f);
    for (int s = 0; s < plan->n_bias_sets; ++s)
        if (int rc = check_bias(e, plan->bias_sets[s], c.control_slots() && ph.idx.uses(s), ph.pool.data() + (size_t)s * set_len, &ph.set_classes[s])) {
            if (named) e->err = "sample plan: bias set " + std::to_string(s) + ": " + e->err;
            return rc;
        }
    if (plan->n_bias_sets >= 1) ph.bits |= kPlanSets;
    return 0;
}
// ... and onto the device, on the engine's stream and finished before the call's first frame starts (a frame may run on another stream of the engine): the
// pool, the sets' class bits and the per-scene settings, once per call
static int upload_plan(umgen_engine* e, const PlanHost& ph) {
    if (ph.bits == 0) return 0;      // nothing a sampler of this call reads
    const DrawPlan& dp = e->dv.d_plan;
    if (ph.bits & kPlanSets) {
        HIPCHK(e, hipMemcpyAsync(dp.pool, ph.pool.data(), ph.pool.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipMemcpyAsync(dp.set_classes, ph.set_classes, sizeof(ph.set_classes), hipMemcpyHostToDevice, e->stream));
    }
    if (ph.bits & kPlanSettings) HIPCHK(e, hipMemcpyAsync(dp.sp_of, ph.sp.data(), ph.sp.size() * sizeof(SamplerParams), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return 0;
}

// What a generation call keeps on the host for its frames; a frame's asynchronous uploads read fp, win and set_of until the frame's synchronisation
struct CallHost {
    GenSide gs;                  // a frame's side outputs, scattered to the caller's arrays by deliver
    PlanHost ph;
    FramePlan fp;
    TokenSeqs win;               // the frame's window [items][T][S_mod]
    std::vector<int> set_of;     // [items]: the frame's column of the plan's index
    std::vector<int> out;        // [items][2199]: the frame's tokens
};
// Everything a generation call is refused for -- the checks of gen_call.h, then the plan -- and what it uploads once: the plan.  A call without a
// plan leaves ph.bits 0: its samplers read nothing of it
static int admit_call(umgen_engine* e, const GenCall& c, CallHost& h) {
    if (int rc = refuse(e, check_gen_call(limits_of(e), c))) return rc;
    if (int rc = check_plan(e, c, h.ph)) return rc;
    h.gs.init(c.side, (size_t)c.items());
    h.set_of.assign((size_t)c.items(), -1);
    h.out.resize((size_t)c.items() * kTokPerFrame);
    return upload_plan(e, h.ph);
}
// new frame idx of the call, on the window of T frames in h.win and behind plan_frame: what the frame takes of its call
static FrameIO frame_io(const GenCall& c, CallHost& h, int idx, int T) {
    FrameIO io{c.items(), T, h.win.view(), FramePlan::ptr(h.fp.cp), FramePlan::ptr(h.fp.cs), c.frame_idx + idx, c.sampling, c.trace, h.out.data()};
    io.given_map = FramePlan::ptr(h.fp.gm);
    io.given_box = FramePlan::ptr(h.fp.gb);
    io.side = h.gs.frame();
    io.plan = h.ph.bits;
    h.ph.idx.column(idx, h.set_of.data());
    io.set_of = h.set_of.data();
    return io;
}

// umgen_frame(_logp, _detail, _biased): one frame of one scene on its window -- the rollout's plan_frame for one scene and one frame of control / given
// tokens (the boxes overwrite window slot T - 1; the GIVEN tokens are those of the trace: the predefined-token prefix of infer_oar_net, UMGen.py:1184-1201)
static int frame_call(umgen_engine* e, const GenCall& c) {
    if (!e) return UMGEN_E_INVALID;
    CallHost h;
    if (int rc = admit_call(e, c, h)) return rc;
    narrow_tokens(c.in, 1, c.T_in, h.win);
    plan_frame(c, 0, h.win.at(2, 0, c.T_in - 1), 0, h.fp);
    if (int rc = run_frame_any(e, frame_io(c, h, 0, c.T_in))) return rc;
    h.gs.deliver(0, 0);
    for (int m = 0; m < 4; ++m)
        for (int i = 0; i < kModLen[m]; ++i) c.out[m][i] = h.out[kModOff[m] + i];
    return UMGEN_OK;
}

// UMGen.inference (UMGen.py:1542-1671) for B scenes of N branches each: branch i = (b, s) at b*N + s reads scene i / N of the caller's arrays and has its own
// seed, so every output is [B][N][..] = [B * N][..].  The driver keeps ONE int32 conditioning sequence per modality, seq [B * N][T_in + new_frames][S_mod]: filled
// from the input once, every new frame written behind it, and frame f = T_in + idx conditioned on the window cond_window(f, cond_frames) of it.  Control boxes
// overwrite frame f - 1 of seq in place, so the overwrite stays in later windows ("cond_tokens", UMGen.py:1465-1467); out_* receive the inputs and what was
// generated, never the overwrite.  Control and given tokens apply while idx < T_ctl (plan_frame).  N >= 2 (umgen_rollout_fan): the first frame runs its history
// once per scene (run_frame_fan) when its window has at least two slots, the slot caches fit and UMGEN_FAN_SHARE is not 0, and *shared_slots reports the slots
// that were shared.  Every argument is checked once, on the caller's arrays: an error that names a flat index names it there.
static int rollout_call(umgen_engine* e, const GenCall& c) {
    if (!e) return UMGEN_E_INVALID;
    if (c.shared_slots) *c.shared_slots = 0;
    CallHost h;      // (a frame's side outputs are scattered to [B * N][new_frames][S_mod] below)
    if (int rc = admit_call(e, c, h)) return rc;
    const int N = c.N, BN = c.items(), T_in = c.T_in, T_out = T_in + c.new_frames;
    e->tm = umgen_timings{};
    e->overlap_suspended = false;
    TokenSeqs seq;
    seq.resize(BN, T_out);
    for (int m = 0; m < 4; ++m)      // out_tokens and cond_tokens both start as the first T_in frames (UMGen.py:1581-1595)
        for (int i = 0; i < BN; ++i) {
            const size_t len = (size_t)T_in * kModLen[m];
            const int64_t* src = c.in[m] + (size_t)(i / N) * len;
            for (size_t k = 0; k < len; ++k) { c.out[m][(size_t)i * T_out * kModLen[m] + k] = src[k]; seq.at(m, i, 0)[k] = (int)src[k]; }
        }
    for (int idx = 0; idx < c.new_frames; ++idx) {
        const int f = T_in + idx;
        const CondWindow w = cond_window(f, c.cond_frames);
        if (idx < c.T_ctl && c.ctrl_bbox3d && !c.control_test)
            return e->fail(UMGEN_E_UNSUPPORTED, "init_tokens['bbox3d'] without control_test is not a supported reference path");
        plan_frame(c, idx, seq.at(2, 0, f - 1), (size_t)T_out * kNBox, h.fp);
        gather_windows(seq.view(), BN, w.start, w.n, h.win);
        FrameIO io = frame_io(c, h, idx, w.n);
        io.cond_cap = c.cond_frames;
        io.next_follows = idx + 1 < c.new_frames;
        io.next_has_ctrl_pose = c.ctrl_pose && idx + 1 < c.T_ctl;
        const char* fse = getenv("UMGEN_FAN_SHARE");      // (read per call: the tests compare both forms in one process)
        const bool fan = idx == 0 && N >= 2 && w.n >= 2 && !(fse && fse[0] == '0') && ensure_tcache(e);
        if (fan && c.shared_slots) *c.shared_slots = w.n - 1;
        if (int rc = fan ? run_frame_fan_any(e, io, N) : run_frame_any(e, io)) return rc;
        // the new frame (UMGen.py:1636-1666): control pose tokens are copied verbatim; everything else is what was generated
        for (int m = 0; m < 4; ++m)
            for (int i = 0; i < BN; ++i) {
                const size_t src = (size_t)i * kTokPerFrame + kModOff[m], len = (size_t)kModLen[m];
                memcpy(seq.at(m, i, f), &h.out[src], len * sizeof(int));
                for (size_t k = 0; k < len; ++k) c.out[m][((size_t)i * T_out + f) * len + k] = h.out[src + k];
            }
        for (int i = 0; i < BN; ++i) h.gs.deliver((size_t)i, (size_t)i * c.new_frames + idx);
    }
    return UMGEN_OK;
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
    if (int rc = refuse(e, check_scene_tokens(limits_of(e), frames, win))) return rc;
    if (!next) return 0;
    const int rc = refuse(e, check_scene_tokens(limits_of(e), n_next, next));
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
    if (d) { if (int rc = refuse(e, check_detail_request(dio.topk, dio.temperature, wants_lists(dio)))) return rc; }
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

// ---- the ten generation entry points: each fills a GenCall from its arguments, under the names include/umgen.h gives them ----

// the arguments every rung of a ladder shares, as the leading members of GenCall (N: the branches per scene).  A frame call is B = N = 1, T_in = T,
// new_frames = 1 (cond_frames unused), T_ctl = 1, and takes its given tokens from the trace
#define ROLLOUT_ARGS(N) B, N, T_in, new_frames, cond_frames, {pose, map, bbox3d, image}, {out_pose, out_map, out_bbox3d, out_image}, T_ctl, ctrl_pose, \
                        ctrl_bbox3d, control_test, given_map, given_bbox3d, sampling
#define FRAME_ARGS 1, 1, T, 1, T, {pose, map, bbox3d, image}, {out_pose, out_map, out_bbox3d, out_image}, 1, ctrl_pose, ctrl_bbox3d, control_test, \
                   trace ? trace->given_map : nullptr, trace ? trace->given_bbox3d : nullptr, sampling

int umgen_frame(umgen_engine* e, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test, const umgen_sampling* sampling,
                int32_t frame_idx, const umgen_trace* trace, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image) {
    return frame_call(e, GenCall{FRAME_ARGS, side_dst(nullptr, nullptr, nullptr, 0), kFrameCall, nullptr, nullptr, frame_idx, trace});
}

int umgen_frame_logp(umgen_engine* e, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                     const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test, const umgen_sampling* sampling,
                     int32_t frame_idx, const umgen_trace* trace, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                     const umgen_logp_out* lp) {
    return frame_call(e, GenCall{FRAME_ARGS, side_dst(lp, nullptr, nullptr, 0), kFrameCall, nullptr, nullptr, frame_idx, trace});
}

int umgen_frame_detail(umgen_engine* e, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                       const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test, const umgen_sampling* sampling,
                       int32_t frame_idx, const umgen_trace* trace, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                       const umgen_logp_out* lp, int32_t topk, const umgen_gen_detail_out* detail) {
    return frame_call(e, GenCall{FRAME_ARGS, side_dst(lp, nullptr, detail, topk), kFrameCall, nullptr, nullptr, frame_idx, trace});
}

int umgen_frame_biased(umgen_engine* e, int32_t T, const int64_t* pose, const int64_t* map, const int64_t* bbox3d, const int64_t* image,
                       const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test, const umgen_sampling* sampling,
                       int32_t frame_idx, const umgen_trace* trace, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                       const umgen_logp_out* lp, int32_t topk, const umgen_gen_detail_out* detail, const umgen_logit_bias* bias, const umgen_logz_out* lz) {
    const umgen_sample_plan one{nullptr, 1, bias, nullptr};      // umgen_rollout_biased's plan, for one frame
    return frame_call(e, GenCall{FRAME_ARGS, side_dst(lp, lz, detail, topk), kFrameCall, nullptr, bias ? &one : nullptr, frame_idx, trace});
}

int umgen_rollout(umgen_engine* e, int32_t B, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose,
                  const int64_t* map, const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose,
                  const int64_t* ctrl_bbox3d, int32_t control_test, const int64_t* given_map, const int64_t* given_bbox3d,
                  const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image) {
    return rollout_call(e, GenCall{ROLLOUT_ARGS(1), side_dst(nullptr, nullptr, nullptr, 0)});
}

int umgen_rollout_logp(umgen_engine* e, int32_t B, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose,
                       const int64_t* map, const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose,
                       const int64_t* ctrl_bbox3d, int32_t control_test, const int64_t* given_map, const int64_t* given_bbox3d,
                       const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map, int64_t* out_bbox3d, int64_t* out_image,
                       const umgen_logp_out* lp) {
    return rollout_call(e, GenCall{ROLLOUT_ARGS(1), side_dst(lp, nullptr, nullptr, 0)});
}

// umgen_rollout_fan: N sampled futures per scene, whose first frame shares the history between a scene's branches (engine_frame.hip run_frame_fan)
// umgen_rollout_detail: the same with the diagnostics of every generated token ([B][N][..] likewise)
// umgen_rollout_biased: the same under one set of logit-bias tables, with logz of every sampled position
// umgen_rollout_planned: the same with the call's sampling plan (per-scene settings, per-scene and per-frame table sets)
int umgen_rollout_fan(umgen_engine* e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                      const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test,
                      const int64_t* given_map, const int64_t* given_bbox3d, const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map,
                      int64_t* out_bbox3d, int64_t* out_image, const umgen_logp_out* lp, int32_t* shared_slots) {
    return rollout_call(e, GenCall{ROLLOUT_ARGS(N), side_dst(lp, nullptr, nullptr, 0), kFanCall, shared_slots});
}

int umgen_rollout_detail(umgen_engine* e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                         const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test,
                         const int64_t* given_map, const int64_t* given_bbox3d, const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map,
                         int64_t* out_bbox3d, int64_t* out_image, const umgen_logp_out* lp, int32_t* shared_slots, int32_t topk,
                         const umgen_gen_detail_out* detail) {
    return rollout_call(e, GenCall{ROLLOUT_ARGS(N), side_dst(lp, nullptr, detail, topk), kFanCall, shared_slots});
}

int umgen_rollout_biased(umgen_engine* e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                         const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test,
                         const int64_t* given_map, const int64_t* given_bbox3d, const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map,
                         int64_t* out_bbox3d, int64_t* out_image, const umgen_logp_out* lp, int32_t* shared_slots, int32_t topk,
                         const umgen_gen_detail_out* detail, const umgen_logit_bias* bias, const umgen_logz_out* lz) {
    const umgen_sample_plan one{nullptr, 1, bias, nullptr};      // the plan of one set for every scene, branch and frame (none without a bias)
    return rollout_call(e, GenCall{ROLLOUT_ARGS(N), side_dst(lp, lz, detail, topk), kFanCall, shared_slots, bias ? &one : nullptr});
}

int umgen_rollout_planned(umgen_engine* e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames, const int64_t* pose, const int64_t* map,
                          const int64_t* bbox3d, const int64_t* image, int32_t T_ctl, const int64_t* ctrl_pose, const int64_t* ctrl_bbox3d, int32_t control_test,
                          const int64_t* given_map, const int64_t* given_bbox3d, const umgen_sampling* sampling, int64_t* out_pose, int64_t* out_map,
                          int64_t* out_bbox3d, int64_t* out_image, const umgen_logp_out* lp, int32_t* shared_slots, int32_t topk,
                          const umgen_gen_detail_out* detail, const umgen_sample_plan* plan, const umgen_logz_out* lz) {
    return rollout_call(e, GenCall{ROLLOUT_ARGS(N), side_dst(lp, lz, detail, topk), kFanCall, shared_slots, plan});
}

}  // extern "C"
