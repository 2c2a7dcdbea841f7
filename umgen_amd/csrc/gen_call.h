// One generation call as a record, and what it is refused for.  Plain C++ (no HIP, no engine types): the ten generation entry points of include/umgen.h
// -- umgen_rollout(_logp, _fan, _detail, _biased, _planned), umgen_frame(_logp, _detail, _biased) -- each fill one GenCall (engine.hip) and hand it to
// rollout_call / frame_call; the checks below read it and the GenLimits of the engine and return {code, message}, code 0 = accepted, which engine.hip
// turns into umgen_engine::fail before anything reaches the device.  Codes, texts and order are part of the ABI's contract.
//
// The order of the checks (check_gen_call), for both forms -- a frame call is the record with B = N = 1, T_in = T, new_frames = 1, T_ctl = 1 and the
// given arrays of its trace:
//   1. the engine's weights are finalized
//   2. the counts.  kRolloutCall: B in [1, max_batch]; kFanCall: B >= 1, N >= 1, B * N <= max_batch; both: T_in >= 1, new_frames >= 0, cond_frames in
//      [1, max_cond_frames] (one message).  kFrameCall: T in [1, max_cond_frames]
//   3. the sampler settings (sample_plan.h sampling_error)
//   4. the diagnostics request, when a diagnostics array is asked for: topk, a finite temperature, lists only with topk > 0
//   5. no NULL among the eight token buffers
//   6. the history tokens, pose | map | bbox3d | image, each inside its vocabulary
//   7. control tokens: T_ctl >= 1; the pose tokens; the bbox3d tokens (-1 = free); kFrameCall: control boxes only with control_test (the rollout
//      driver refuses the same when it reaches a controlled frame)
//   8. given tokens: T_ctl >= 1; boxes only behind a map; what they exclude (kFrameCall: control_test; rollouts: bbox3d control beside given boxes);
//      the map tokens; the bbox3d tokens
// The call's plan and its logit-bias tables follow in engine.hip (check_plan).  A message that names a flat index names it in the caller's array,
// whatever N is.  tests/host/gen_call_test.cpp holds every refusal, and the order, to the texts of the ABI.
#pragma once

#include <cstdint>
#include <string>
#include <utility>

#include "../../include/umgen.h"
#include "gen_side.h"
#include "sample_plan.h"

namespace umgen {

enum GenForm { kRolloutCall, kFanCall, kFrameCall };      // umgen_rollout(_logp) | umgen_rollout_fan .. _planned | umgen_frame ..

// What every generation entry point hands on.  Members follow the ABI's argument order, so that an entry point fills the record in one initializer
struct GenCall {
    int B, N, T_in, new_frames, cond_frames;      // (kFrameCall: 1, 1, T, 1, unused)
    const int64_t* in[4];                         // pose | map | bbox3d | image, [B][T_in][S_mod]
    int64_t* out[4];                              // [B * N][T_in + new_frames][S_mod]; kFrameCall: [S_mod]
    int T_ctl;
    const int64_t *ctrl_pose, *ctrl_bbox3d;       // NULL or [B][T_ctl][S_mod]
    int control_test;
    const int64_t *given_map, *given_bbox3d;      // likewise
    const umgen_sampling* sampling;
    SideDst side;                                 // the caller's logp / logz / diagnostics arrays and topk, built once per call
    GenForm form = kRolloutCall;
    int32_t* shared_slots = nullptr;
    const umgen_sample_plan* plan = nullptr;      // umgen_rollout_biased and umgen_frame_biased: their one set, for everyone
    int frame_idx = 0;                            // kFrameCall (a rollout numbers its frames from 0)
    const umgen_trace* trace = nullptr;           // kFrameCall
    int items() const { return B * N; }
    bool control_slots() const { return ctrl_bbox3d && control_test; }
};

// what the checks read of the engine (vocab: pose | map | bbox3d | image), and what they return: code 0 = accepted
struct GenLimits { bool finalized; int max_batch, max_cond_frames; int vocab[4]; };
struct Refusal { int code = 0; std::string msg; explicit operator bool() const { return code != 0; } };
inline Refusal invalid(std::string msg) { return Refusal{UMGEN_E_INVALID, std::move(msg)}; }

// Every token that becomes a gather index is checked at the ABI boundary (history: embed_stack_kernel's table rows; control
// pose: the fouier_pe rows and decode_pose_value; control bbox3d: -1 = "free", anything else a be / posi row).
inline Refusal check_tokens(const char* what, const int64_t* p, size_t n, int64_t vocab, bool allow_free) {
    for (size_t i = 0; i < n; ++i) {
        const int64_t v = p[i];
        if ((v >= 0 && v < vocab) || (allow_free && v == -1)) continue;
        return invalid(plan_msg("%s token %lld at flat index %zu is outside [0, %lld)%s", what, (long long)v, i, (long long)vocab,
                                allow_free ? " (and is not -1 = free)" : ""));
    }
    return {};
}
// `frames` frames of every modality (the x / y attribute tokens of a slot index the 1030-row spatial table; attribute tokens are bins (< 1024) or pad)
inline Refusal check_scene_tokens(const GenLimits& lim, size_t frames, const int64_t* const tok[4]) {
    static const char* const name[4] = {"pose", "map", "bbox3d", "image"};
    for (int m = 0; m < 4; ++m)
        if (Refusal r = check_tokens(name[m], tok[m], frames * kModLen[m], lim.vocab[m], false)) return r;
    return {};
}

inline Refusal check_sampling(const umgen_sampling* s) {
    if (!s) return invalid("sampling is null");
    std::string m = sampling_error(*s);      // (sample_plan.h: the same check serves every per_scene entry of a planned call)
    return m.empty() ? Refusal{} : invalid(std::move(m));
}
// what umgen_score_detail and the generation calls refuse of a detail request
inline Refusal check_detail_request(int topk, float temperature, bool wants_lists) {
    if (topk < 0 || topk > UMGEN_SCORE_TOPK_MAX) return invalid(plan_msg("topk=%d out of range [0,%d]", topk, UMGEN_SCORE_TOPK_MAX));
    if (!(temperature > 0.f) || !(temperature <= 3.0e38f)) return invalid("temperature must be > 0 and finite");
    if (wants_lists && topk == 0) return invalid("top-K outputs requested with topk = 0");
    return {};
}

inline Refusal check_counts(const GenLimits& lim, const GenCall& c) {
    if (c.form == kFrameCall)
        return c.T_in < 1 || c.T_in > lim.max_cond_frames ? invalid(plan_msg("T=%d out of range [1,%d]", c.T_in, lim.max_cond_frames)) : Refusal{};
    if (c.form == kRolloutCall && (c.B < 1 || c.B > lim.max_batch)) return invalid(plan_msg("B=%d out of range [1,%d]", c.B, lim.max_batch));
    if (c.form == kFanCall) {
        if (c.B < 1) return invalid(plan_msg("B=%d: at least one scene", c.B));
        if (c.N < 1) return invalid(plan_msg("N=%d: at least one sample per scene", c.N));
        if ((int64_t)c.B * c.N > lim.max_batch)
            return invalid(plan_msg("B*N=%lld (B=%d, N=%d) exceeds max_batch=%d", (long long)c.B * c.N, c.B, c.N, lim.max_batch));
    }
    if (c.T_in < 1 || c.new_frames < 0 || c.cond_frames < 1 || c.cond_frames > lim.max_cond_frames)
        return invalid(plan_msg("T_in=%d new_frames=%d cond_frames=%d (max %d)", c.T_in, c.new_frames, c.cond_frames, lim.max_cond_frames));
    return {};
}

// steps 7 and 8: the control and given arrays, [B][T_ctl][S_mod] on the caller's side (a frame call: B = T_ctl = 1)
inline Refusal check_control_and_given(const GenLimits& lim, const GenCall& c) {
    const bool frame = c.form == kFrameCall;
    const size_t n = (size_t)c.B * (size_t)(c.T_ctl > 0 ? c.T_ctl : 0);
    if ((c.ctrl_pose || c.ctrl_bbox3d) && c.T_ctl < 1) return invalid(plan_msg("control tokens given with T_ctl=%d", c.T_ctl));
    if (c.ctrl_pose) { if (Refusal r = check_tokens("control pose", c.ctrl_pose, n * kModLen[0], lim.vocab[0], false)) return r; }
    if (c.ctrl_bbox3d) { if (Refusal r = check_tokens("control bbox3d", c.ctrl_bbox3d, n * kModLen[2], lim.vocab[2], true)) return r; }
    if (frame && c.ctrl_bbox3d && !c.control_test)
        return Refusal{UMGEN_E_UNSUPPORTED, "init_tokens['bbox3d'] without control_test is not a supported reference path"};
    // given (not generated) modalities of the new frames: infer_oar_net's predefined-token prefix (UMGen.py:1184-1201)
    if ((c.given_map || c.given_bbox3d) && c.T_ctl < 1) return invalid(plan_msg("given tokens with T_ctl=%d", c.T_ctl));
    if (c.given_bbox3d && !c.given_map)
        return Refusal{UMGEN_E_UNSUPPORTED,
                       frame ? "given bbox3d tokens without a given map: the reference would put them on the map's positions (UMGen.py:1190-1201)"
                             : "init_tokens['bbox3d'] without init_tokens['map'] (and without control_test): the reference concatenates the given "
                               "modalities back to back behind the pose, so the boxes would sit on the map's positions -- not a meaningful path"};
    if (frame && c.given_map && c.control_test) return Refusal{UMGEN_E_UNSUPPORTED, "given tokens and control_test exclude each other"};
    if (!frame && c.given_bbox3d && (c.ctrl_bbox3d || c.control_test)) return invalid("given bbox3d tokens and bbox3d control exclude each other");
    if (c.given_map) { if (Refusal r = check_tokens("given map", c.given_map, n * kModLen[1], lim.vocab[1], false)) return r; }
    if (c.given_bbox3d) { if (Refusal r = check_tokens("given bbox3d", c.given_bbox3d, n * kModLen[2], lim.vocab[2], false)) return r; }
    return {};
}

// everything a generation call is refused for ahead of its plan, in the order of the comment at the top
inline Refusal check_gen_call(const GenLimits& lim, const GenCall& c) {
    if (!lim.finalized) return Refusal{UMGEN_E_STATE, "umgen_finalize_weights has not been called"};
    if (Refusal r = check_counts(lim, c)) return r;
    if (Refusal r = check_sampling(c.sampling)) return r;
    if (c.side.wants_detail()) { if (Refusal r = check_detail_request(c.side.topk, c.sampling->temperature, c.side.wants_lists())) return r; }
    for (int m = 0; m < 4; ++m)
        if (!c.in[m] || !c.out[m]) return invalid("null token buffer");
    if (Refusal r = check_scene_tokens(lim, (size_t)c.B * c.T_in, c.in)) return r;
    return check_control_and_given(lim, c);
}

}  // namespace umgen
