// umgen_amd/csrc/sample_plan.h against element-by-element restatements: the broadcast of a NULL bias_of, column f of the index for every frame, every
// refusal of a plan's settings, index and tables, 16 sets accepted and 17 refused, a set no scene uses still validated.  Plain host C++ with its own
// main; tests/test_sample_plan_host.py compiles it with -fsanitize=address,undefined and runs it once.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sample_plan.h"

using namespace umgen;

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static bool has(const std::string& msg, const char* part) { return msg.find(part) != std::string::npos; }

struct Sampling {      // umgen_sampling's members
    int method, top_k, top_k_map, topk_image;
    float p, p_map, temperature;
    int rule_constrain, merge_ar_tar, only_ar;
    const unsigned long long* seeds;
};
static Sampling good() { return Sampling{0, 5, 5, 16, 0.4f, 0.4f, 1.0f, 1, 1, 0, nullptr}; }

static void test_sampling() {
    EXPECT(sampling_error(good()).empty());
    Sampling s = good(); s.method = 2;
    EXPECT(has(sampling_error(s), "sample method 2"));
    s = good(); s.method = 1; s.p_map = 0.f;
    EXPECT(has(sampling_error(s), "top-p mass"));
    for (int which = 0; which < 3; ++which)
        for (int bad : {0, 17}) {
            s = good();
            (which == 0 ? s.top_k : which == 1 ? s.top_k_map : s.topk_image) = bad;
            EXPECT(has(sampling_error(s), "top-k values"));
        }
    s = good(); s.temperature = 0.f;
    EXPECT(has(sampling_error(s), "temperature"));
    s = good(); s.temperature = std::nanf("");
    EXPECT(has(sampling_error(s), "temperature"));

    // per_scene: every entry checked, the message names the scene; the three per-call flags must agree with the call's
    std::vector<Sampling> per(5, good());
    per[1].temperature = 0.5f; per[2].top_k = 16; per[3].method = 1;
    EXPECT(plan_settings_error(good(), per.data(), 5).empty());
    EXPECT(plan_settings_error(good(), (const Sampling*)nullptr, 5).empty());
    per[4].temperature = -1.f;
    EXPECT(has(plan_settings_error(good(), per.data(), 5), "per_scene[4]") && has(plan_settings_error(good(), per.data(), 5), "temperature"));
    EXPECT(plan_settings_error(good(), per.data(), 4).empty());      // (entries past `items` are not read)
    per[4] = good();
    for (int which = 0; which < 3; ++which) {
        std::vector<Sampling> q(per);
        (which == 0 ? q[2].rule_constrain : which == 1 ? q[2].merge_ar_tar : q[2].only_ar) ^= 1;
        const std::string m = plan_settings_error(good(), q.data(), 5);
        EXPECT(has(m, "per_scene[2]") && has(m, "per call"));
    }
}

static void test_index() {
    const int items = 5, frames = 3;
    PlanIndex idx;
    // NULL bias_of: everyone on set 0 with sets, nobody without
    EXPECT(plan_index_error(items, frames, 2, nullptr, idx).empty());
    EXPECT(idx.items == items && idx.frames == frames && idx.n_sets == 2 && idx.of.size() == (size_t)items * frames);
    for (int v : idx.of) EXPECT(v == 0);
    EXPECT(idx.uses(0) && !idx.uses(1) && idx.constant());
    EXPECT(plan_index_error(items, frames, 0, nullptr, idx).empty());
    for (int v : idx.of) EXPECT(v == -1);
    EXPECT(!idx.uses(0) && idx.constant());
    // a full index: every column of every frame, element by element
    std::vector<int32_t> of((size_t)items * frames);
    for (int i = 0; i < items; ++i)
        for (int f = 0; f < frames; ++f) of[(size_t)i * frames + f] = (i * 7 + f * 3) % 4 - 1;      // -1 .. 2
    EXPECT(plan_index_error(items, frames, 3, of.data(), idx).empty());
    for (int f = 0; f < frames; ++f) {
        std::vector<int> col((size_t)items + 1, 12345);
        idx.column(f, col.data());
        for (int i = 0; i < items; ++i) EXPECT(col[i] == of[(size_t)i * frames + f] && idx.at(i, f) == col[i]);
        EXPECT(col[items] == 12345);
    }
    EXPECT(idx.uses(0) && idx.uses(1) && idx.uses(2) && !idx.uses(3) && !idx.constant());
    // refusals
    EXPECT(has(plan_index_error(items, frames, -1, nullptr, idx), "n_bias_sets=-1"));
    EXPECT(plan_index_error(items, frames, kPlanSetsMax, nullptr, idx).empty());
    EXPECT(has(plan_index_error(items, frames, kPlanSetsMax + 1, nullptr, idx), "n_bias_sets=17"));
    EXPECT(has(plan_index_error(items, frames, 0, of.data(), idx), "n_bias_sets = 0"));
    of[(size_t)3 * frames + 2] = 3;
    std::string m = plan_index_error(items, frames, 3, of.data(), idx);
    EXPECT(has(m, "scene 3") && has(m, "frame 2") && has(m, "is 3"));
    of[(size_t)3 * frames + 2] = -2;
    m = plan_index_error(items, frames, 3, of.data(), idx);
    EXPECT(has(m, "scene 3") && has(m, "frame 2") && has(m, "is -2"));
    // no new frames: an empty index
    EXPECT(plan_index_error(items, 0, 1, nullptr, idx).empty() && idx.of.empty() && idx.constant() && !idx.uses(0));
}

static void test_tables() {
    const int vocab[4] = {8, 6, 12, 5};
    const float NEG = -INFINITY;
    std::vector<float> pose(3 * 8, 0.f), map(6, 0.5f), box(11 * 12, -1.f), img(5, 2.f);
    const float* tab[4] = {pose.data(), map.data(), box.data(), img.data()};
    int classes = -1;
    EXPECT(bias_tables_error(tab, vocab, 8192, true, &classes).empty() && classes == 15);
    const float* some[4] = {nullptr, map.data(), nullptr, img.data()};
    EXPECT(bias_tables_error(some, vocab, 8192, true, &classes).empty() && classes == ((1 << 1) | (1 << 3)));
    const float* none[4] = {nullptr, nullptr, nullptr, nullptr};
    EXPECT(bias_tables_error(none, vocab, 8192, true, &classes).empty() && classes == 0);
    // NaN / +inf: class, row and index are named
    box[4 * 12 + 7] = std::nanf("");
    std::string m = bias_tables_error(tab, vocab, 8192, false, &classes);
    EXPECT(has(m, "class bbox3d row 4 index 7 is NaN"));
    box[4 * 12 + 7] = INFINITY;
    m = bias_tables_error(tab, vocab, 8192, false, &classes);
    EXPECT(has(m, "class bbox3d row 4 index 7 is +inf"));
    box[4 * 12 + 7] = -1.f;
    // a row without an allowed entry
    for (int n = 0; n < 8; ++n) pose[2 * 8 + n] = NEG;
    m = bias_tables_error(tab, vocab, 8192, false, &classes);
    EXPECT(has(m, "class pose row 2 bans every token"));
    pose[2 * 8 + 3] = 0.f;
    EXPECT(bias_tables_error(tab, vocab, 8192, false, &classes).empty());
    // the control resample's masked index: refused under the control rule only
    for (int n = 0; n < 11; ++n) box[9 * 12 + n] = NEG;
    EXPECT(bias_tables_error(tab, vocab, 8192, false, &classes).empty());
    m = bias_tables_error(tab, vocab, 8192, true, &classes);
    EXPECT(has(m, "class bbox3d row 9 allows only index 11"));
    box[9 * 12 + 0] = 0.f;
    EXPECT(bias_tables_error(tab, vocab, 8192, true, &classes).empty());
    // a vocabulary the scratch row does not hold
    m = bias_tables_error(tab, vocab, 7, false, &classes);
    EXPECT(has(m, "class pose has a vocabulary of 8"));
}

// A plan's sets the way check_plan (engine.hip) walks them: every set validated, the control rule for the sets some scene uses
static std::string check_sets(const std::vector<const float* const*>& sets, const int vocab[4], const PlanIndex& idx, bool control) {
    for (size_t s = 0; s < sets.size(); ++s) {
        int classes = 0;
        const std::string m = bias_tables_error(sets[s], vocab, 8192, control && idx.uses((int)s), &classes);
        if (!m.empty()) return "bias set " + std::to_string(s) + ": " + m;
    }
    return "";
}
static void test_unused_set_is_validated() {
    const int vocab[4] = {8, 6, 12, 5};
    std::vector<float> ok(6, 0.f), bad(6, 0.f), onlylast(11 * 12, -INFINITY);
    bad[2] = std::nanf("");
    for (int r = 0; r < 11; ++r) onlylast[r * 12 + 11] = 0.f;
    const float* set_ok[4] = {nullptr, ok.data(), nullptr, nullptr};
    const float* set_bad[4] = {nullptr, bad.data(), nullptr, nullptr};
    const float* set_last[4] = {nullptr, nullptr, onlylast.data(), nullptr};
    PlanIndex idx;
    const int32_t of[4] = {0, 0, -1, 0};      // 2 scenes, 2 frames: nobody uses set 1 or 2
    EXPECT(plan_index_error(2, 2, 3, of, idx).empty());
    std::string m = check_sets({set_ok, set_bad, set_ok}, vocab, idx, true);
    EXPECT(has(m, "bias set 1") && has(m, "class map row 0 index 2 is NaN"));
    EXPECT(check_sets({set_ok, set_ok, set_last}, vocab, idx, true).empty());      // the control rule: used sets only
    const int32_t of2[4] = {0, 0, -1, 2};
    EXPECT(plan_index_error(2, 2, 3, of2, idx).empty());
    m = check_sets({set_ok, set_ok, set_last}, vocab, idx, true);
    EXPECT(has(m, "bias set 2") && has(m, "allows only index 11"));
    EXPECT(check_sets({set_ok, set_ok, set_last}, vocab, idx, false).empty());
}

int main() {
    test_sampling();
    test_index();
    test_tables();
    test_unused_set_is_validated();
    if (failures) { printf("sample_plan_test: %d failure(s)\n", failures); return 1; }
    printf("sample_plan_test: ok\n");
    return 0;
}
