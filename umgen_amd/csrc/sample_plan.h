// Host side of a sampling plan (umgen_rollout_planned, include/umgen.h), plain C++ (no HIP, no engine types): what a call's sampler settings and
// logit-bias tables must satisfy -- for the one `sampling` / `bias` of an unplanned call and for every per_scene entry / table set of a planned one --
// and the resolved index of a plan: which table set scene i draws under in new frame f (PlanIndex: the broadcast of a NULL bias_of, the range check,
// column f for the frame).  Every check returns its message ("" = accepted); engine.hip turns a message into UMGEN_E_INVALID before anything reaches the
// device.  tests/host/sample_plan_test.cpp holds all of it to element-by-element restatements.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace umgen {

constexpr int kPlanSetsMax = 16;                      // == UMGEN_BIAS_SETS_MAX (kBiasSetsMax, frame.h)
constexpr int kPlanTableRows[4] = {3, 1, 11, 1};      // rows of a class's table: pose component, bbox3d attribute

inline std::string plan_msg(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}

// what a call refuses of ONE set of sampler settings (S: umgen_sampling or any struct with its members)
template <typename S>
std::string sampling_error(const S& s) {
    if (s.method != 0 && s.method != 1) return plan_msg("sample method %d", s.method);
    if (s.method == 1 && !(s.p > 0.f && s.p_map > 0.f)) return "top-p mass must be > 0";
    if (s.top_k < 1 || s.top_k > 16 || s.top_k_map < 1 || s.top_k_map > 16 || s.topk_image < 1 || s.topk_image > 16)
        return "top-k values must be in [1, 16] (reference: 5 / 5 / 16)";
    if (!(s.temperature > 0.f)) return "temperature must be > 0";
    return "";
}

// per_scene [items] of a plan: every entry passes sampling_error, and rule_constrain / merge_ar_tar / only_ar agree with `call` (the call's `sampling`):
// the host decides per call whether head_tar_bbox3d runs, so these three stay per call.  The message names the scene
template <typename S>
std::string plan_settings_error(const S& call, const S* per_scene, int items) {
    for (int i = 0; per_scene && i < items; ++i) {
        const S& s = per_scene[i];
        const std::string m = sampling_error(s);
        if (!m.empty()) return plan_msg("sample plan: per_scene[%d]: %s", i, m.c_str());
        if (s.rule_constrain != call.rule_constrain || s.merge_ar_tar != call.merge_ar_tar || s.only_ar != call.only_ar)
            return plan_msg("sample plan: per_scene[%d] has rule_constrain / merge_ar_tar / only_ar = %d / %d / %d, the call's sampling %d / %d / %d (these are per call)", i,
                            s.rule_constrain, s.merge_ar_tar, s.only_ar, call.rule_constrain, call.merge_ar_tar, call.only_ar);
    }
    return "";
}

// One set of logit-bias tables tab[class] ([rows][vocab[class]], null: no table): entries are finite or -inf (a ban), every row keeps an allowed entry,
// a vocabulary fits the samplers' scratch row, and with control_rule a bbox3d row must allow more than vocab - 1 (the control resample masks that
// index).  -> *classes: the bit per class with a table
inline std::string bias_tables_error(const float* const tab[4], const int vocab[4], int row_len, bool control_rule, int* classes) {
    static const char* const name[4] = {"pose", "map", "bbox3d", "image"};
    *classes = 0;
    for (int c = 0; c < 4; ++c) {
        if (!tab[c]) continue;
        if (vocab[c] > row_len) return plan_msg("logit bias: class %s has a vocabulary of %d, the samplers' scratch row holds %d", name[c], vocab[c], row_len);
        for (int r = 0; r < kPlanTableRows[c]; ++r) {
            const float* row = tab[c] + (size_t)r * vocab[c];
            int allowed = 0, last = -1;
            for (int n = 0; n < vocab[c]; ++n) {
                const float v = row[n];
                if (v != v || v == __builtin_inff())
                    return plan_msg("logit bias: class %s row %d index %d is %s (entries are finite or -inf)", name[c], r, n, v != v ? "NaN" : "+inf");
                if (v != -__builtin_inff()) { ++allowed; last = n; }
            }
            if (!allowed) return plan_msg("logit bias: class %s row %d bans every token (index 0 .. %d are all -inf)", name[c], r, vocab[c] - 1);
            if (c == 2 && control_rule && allowed == 1 && last == vocab[c] - 1)
                return plan_msg("logit bias: class %s row %d allows only index %d, which the control resample of a controlled slot masks", name[c], r, last);
        }
        *classes |= 1 << c;
    }
    return "";
}

// The resolved index of a plan over `items` scenes / branches and `frames` new frames: of[i][f] = the table set of scene i in new frame f, -1 = unbiased
struct PlanIndex {
    int items = 0, frames = 0, n_sets = 0;
    std::vector<int> of;
    int at(int i, int f) const { return of[(size_t)i * frames + f]; }
    bool uses(int set) const {
        for (int v : of)
            if (v == set) return true;
        return false;
    }
    bool constant() const {      // one value everywhere (an empty index counts)
        for (int v : of)
            if (v != of[0]) return false;
        return true;
    }
    // column f: the [items] set ids the samplers of new frame f read
    void column(int f, int* out) const {
        for (int i = 0; i < items; ++i) out[i] = at(i, f);
    }
};

// bias_of of a plan ([items][frames], or null: every scene and frame uses set 0 when n_sets >= 1, nothing when n_sets == 0) -> idx.  Refused: n_sets
// outside [0, kPlanSetsMax], an index array without sets, an entry outside [-1, n_sets); the message names the scene and the frame
inline std::string plan_index_error(int items, int frames, int n_sets, const int32_t* bias_of, PlanIndex& idx) {
    if (n_sets < 0 || n_sets > kPlanSetsMax) return plan_msg("sample plan: n_bias_sets=%d out of range [0,%d]", n_sets, kPlanSetsMax);
    if (bias_of && n_sets == 0) return "sample plan: bias_of given with n_bias_sets = 0";
    idx.items = items; idx.frames = frames; idx.n_sets = n_sets;
    idx.of.assign((size_t)items * frames, n_sets >= 1 ? 0 : -1);
    if (!bias_of) return "";
    for (int i = 0; i < items; ++i)
        for (int f = 0; f < frames; ++f) {
            const int32_t v = bias_of[(size_t)i * frames + f];
            if (v < -1 || v >= n_sets) return plan_msg("sample plan: bias_of of scene %d in new frame %d is %d, outside [-1, %d)", i, f, v, n_sets);
            idx.of[(size_t)i * frames + f] = v;
        }
    return "";
}

}  // namespace umgen
