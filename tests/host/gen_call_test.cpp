// umgen_amd/csrc/gen_call.h: every refusal of a generation call -- both rollout forms and the frame form -- with its code and its whole message, the texts
// being those of the ABI (include/umgen.h: "refused before anything reaches the device, the message naming ..."); the order of consecutive refusals; and
// that a token-range message indexes the caller's array whatever N is.  Plain host C++ with its own main; tests/test_gen_call_host.py compiles it with
// -fsanitize=address,undefined and runs it once.
#include <cmath>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "gen_call.h"

using namespace umgen;

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const GenLimits kLim{true, 4, 4, {32, 48, 40, 64}};
static const int B = 2, N = 2, T_IN = 2, NF = 2, T_CTL = 1;
static const umgen_sampling kSampling{0, 5, 5, 16, 0.4f, 0.4f, 1.0f, 1, 1, 0, nullptr};

// the arrays of a call: [B][T_in][S_mod] inputs, [B][T_ctl][S_mod] control / given tokens, outputs (never read or written by a check)
struct Arrays {
    std::vector<int64_t> in[4], out[4], cp, cb, gm, gb;
    Arrays() : cp((size_t)B * T_CTL * 3, 1), cb((size_t)B * T_CTL * 660, -1), gm((size_t)B * T_CTL * 1024, 2), gb((size_t)B * T_CTL * 660, 3) {
        for (int m = 0; m < 4; ++m) { in[m].assign((size_t)B * T_IN * kModLen[m], 1); out[m].assign(1, 0); }
    }
};
static float side_f[4];      // whatever a side output points at: a check never follows the pointer
static int side_i[4];
static SideDst side(bool detail, bool lists, int topk) {
    SideDst d{};
    d.logp[0] = d.logz[3] = side_f;
    if (detail) d.rank[1] = side_i;
    if (lists) d.topk_logp[2] = side_f;
    d.topk = topk;
    return d;
}
static GenCall rollout(Arrays& a, GenForm form) {
    return GenCall{B, form == kFanCall ? N : 1, T_IN, NF, 4, {a.in[0].data(), a.in[1].data(), a.in[2].data(), a.in[3].data()},
                   {a.out[0].data(), a.out[1].data(), a.out[2].data(), a.out[3].data()}, T_CTL, nullptr, nullptr, 0, nullptr, nullptr, &kSampling,
                   side(true, true, 4), form};
}
static GenCall frame(Arrays& a) {      // scene 0's window
    GenCall c = rollout(a, kFrameCall);
    c.B = c.N = c.new_frames = c.T_ctl = 1;
    c.cond_frames = c.T_in;
    return c;
}

typedef std::function<void(GenCall&, Arrays&, umgen_sampling&)> Fault;
// the call of `form` with the faults injected in turn: code and the whole message
static void expect(GenForm form, int code, const std::string& msg, const Fault& f1, const Fault& f2 = nullptr, const GenLimits& lim = kLim) {
    Arrays a;
    umgen_sampling s = kSampling;
    GenCall c = form == kFrameCall ? frame(a) : rollout(a, form);
    c.sampling = &s;
    f1(c, a, s);
    if (f2) f2(c, a, s);
    const Refusal r = check_gen_call(lim, c);
    if (r.code != code || r.msg != msg) { printf("FAILED: form %d: got %d \"%s\", expected %d \"%s\"\n", (int)form, r.code, r.msg.c_str(), code, msg.c_str()); ++failures; }
}

static const GenForm kAll[3] = {kRolloutCall, kFanCall, kFrameCall}, kRollouts[2] = {kRolloutCall, kFanCall};
static const char* const kBoxesWithoutMapRollout =
    "init_tokens['bbox3d'] without init_tokens['map'] (and without control_test): the reference concatenates the given "
    "modalities back to back behind the pose, so the boxes would sit on the map's positions -- not a meaningful path";
static const char* const kBoxesWithoutMapFrame = "given bbox3d tokens without a given map: the reference would put them on the map's positions (UMGen.py:1190-1201)";

// the faults of the documented order, one per step, each valid for every form; `msg` where the forms word it alike
struct Step { const char* name; Fault fault; int code; const char* msg; };
static std::vector<Step> ladder() {
    return {
        {"state", nullptr, UMGEN_E_STATE, "umgen_finalize_weights has not been called"},      // (through the limits: see test_order)
        {"counts", [](GenCall& c, Arrays&, umgen_sampling&) { c.T_in = 0; }, UMGEN_E_INVALID, nullptr},
        {"sampling", [](GenCall&, Arrays&, umgen_sampling& s) { s.method = 2; }, UMGEN_E_INVALID, "sample method 2"},
        {"side", [](GenCall& c, Arrays&, umgen_sampling&) { c.side.topk = 17; }, UMGEN_E_INVALID, "topk=17 out of range [0,16]"},
        {"null", [](GenCall& c, Arrays&, umgen_sampling&) { c.out[2] = nullptr; }, UMGEN_E_INVALID, "null token buffer"},
        {"history", [](GenCall&, Arrays& a, umgen_sampling&) { a.in[3][700] = 64; }, UMGEN_E_INVALID, "image token 64 at flat index 700 is outside [0, 64)"},
        {"control", [](GenCall& c, Arrays& a, umgen_sampling&) { c.ctrl_pose = a.cp.data(); c.control_test = 1; a.cp[2] = -1; }, UMGEN_E_INVALID,
         "control pose token -1 at flat index 2 is outside [0, 32)"},
        {"given", [](GenCall& c, Arrays& a, umgen_sampling&) { c.given_bbox3d = a.gb.data(); }, UMGEN_E_UNSUPPORTED, nullptr},
    };
}

static void test_valid() {
    for (GenForm form : kAll)
        expect(form, 0, "", [](GenCall&, Arrays&, umgen_sampling&) {});
    // everything a call may bring at once: control pose and boxes under control_test, a given map (rollouts: beside the control), nothing asked of the side
    for (GenForm form : kRollouts)
        expect(form, 0, "", [](GenCall& c, Arrays& a, umgen_sampling&) {
            c.ctrl_pose = a.cp.data(); c.ctrl_bbox3d = a.cb.data(); c.control_test = 1; c.given_map = a.gm.data(); c.side = SideDst{};
        });
    expect(kFrameCall, 0, "", [](GenCall& c, Arrays& a, umgen_sampling&) { c.given_map = a.gm.data(); c.given_bbox3d = a.gb.data(); c.T_in = 4; });
    expect(kRolloutCall, 0, "", [](GenCall& c, Arrays&, umgen_sampling&) { c.new_frames = 0; c.cond_frames = 1; });
    // top-K lists nobody asked for: topk is not looked at without a diagnostics array
    expect(kFanCall, 0, "", [](GenCall& c, Arrays&, umgen_sampling&) { c.side = side(false, false, 99); });
}

static void test_counts() {
    const auto set = [](int GenCall::*field, int v) { return [=](GenCall& c, Arrays&, umgen_sampling&) { c.*field = v; }; };
    expect(kRolloutCall, UMGEN_E_INVALID, "B=0 out of range [1,4]", set(&GenCall::B, 0));
    expect(kRolloutCall, UMGEN_E_INVALID, "B=5 out of range [1,4]", set(&GenCall::B, 5));
    expect(kFanCall, UMGEN_E_INVALID, "B=0: at least one scene", set(&GenCall::B, 0), set(&GenCall::N, 0));
    expect(kFanCall, UMGEN_E_INVALID, "B=-3: at least one scene", set(&GenCall::B, -3));
    expect(kFanCall, UMGEN_E_INVALID, "N=0: at least one sample per scene", set(&GenCall::N, 0));
    expect(kFanCall, UMGEN_E_INVALID, "B*N=6 (B=2, N=3) exceeds max_batch=4", set(&GenCall::N, 3));
    expect(kFanCall, UMGEN_E_INVALID, "B*N=4294967296 (B=65536, N=65536) exceeds max_batch=4", set(&GenCall::B, 65536), set(&GenCall::N, 65536));
    expect(kFanCall, UMGEN_E_INVALID, "B*N=5 (B=5, N=1) exceeds max_batch=4", set(&GenCall::B, 5), set(&GenCall::N, 1));
    for (GenForm form : kRollouts) {
        expect(form, UMGEN_E_INVALID, "T_in=0 new_frames=2 cond_frames=4 (max 4)", set(&GenCall::T_in, 0));
        expect(form, UMGEN_E_INVALID, "T_in=2 new_frames=-1 cond_frames=4 (max 4)", set(&GenCall::new_frames, -1));
        expect(form, UMGEN_E_INVALID, "T_in=2 new_frames=2 cond_frames=0 (max 4)", set(&GenCall::cond_frames, 0));
        expect(form, UMGEN_E_INVALID, "T_in=2 new_frames=2 cond_frames=5 (max 4)", set(&GenCall::cond_frames, 5));
    }
    expect(kFrameCall, UMGEN_E_INVALID, "T=0 out of range [1,4]", set(&GenCall::T_in, 0));
    expect(kFrameCall, UMGEN_E_INVALID, "T=5 out of range [1,4]", set(&GenCall::T_in, 5));
}

static void test_sampling_and_side() {
    for (GenForm form : kAll) {
        expect(form, UMGEN_E_INVALID, "sampling is null", [](GenCall& c, Arrays&, umgen_sampling&) { c.sampling = nullptr; });
        expect(form, UMGEN_E_INVALID, "sample method 2", [](GenCall&, Arrays&, umgen_sampling& s) { s.method = 2; });
        expect(form, UMGEN_E_INVALID, "top-p mass must be > 0", [](GenCall&, Arrays&, umgen_sampling& s) { s.method = 1; s.p_map = 0.f; });
        expect(form, UMGEN_E_INVALID, "top-k values must be in [1, 16] (reference: 5 / 5 / 16)", [](GenCall&, Arrays&, umgen_sampling& s) { s.topk_image = 17; });
        expect(form, UMGEN_E_INVALID, "temperature must be > 0", [](GenCall&, Arrays&, umgen_sampling& s) { s.temperature = std::nanf(""); });
        expect(form, UMGEN_E_INVALID, "topk=-1 out of range [0,16]", [](GenCall& c, Arrays&, umgen_sampling&) { c.side.topk = -1; });
        expect(form, UMGEN_E_INVALID, "topk=17 out of range [0,16]", [](GenCall& c, Arrays&, umgen_sampling&) { c.side = side(true, false, 17); });
        expect(form, UMGEN_E_INVALID, "temperature must be > 0 and finite", [](GenCall&, Arrays&, umgen_sampling& s) { s.temperature = INFINITY; });
        expect(form, UMGEN_E_INVALID, "top-K outputs requested with topk = 0", [](GenCall& c, Arrays&, umgen_sampling&) { c.side = side(false, true, 0); });
        // an infinite temperature is the diagnostics' bar alone
        expect(form, 0, "", [](GenCall& c, Arrays&, umgen_sampling& s) { s.temperature = INFINITY; c.side = side(false, false, 0); });
    }
}

static void test_buffers_and_tokens() {
    static const char* const name[4] = {"pose", "map", "bbox3d", "image"};
    for (GenForm form : kAll)
        for (int m = 0; m < 4; ++m) {
            expect(form, UMGEN_E_INVALID, "null token buffer", [m](GenCall& c, Arrays&, umgen_sampling&) { c.in[m] = nullptr; });
            expect(form, UMGEN_E_INVALID, "null token buffer", [m](GenCall& c, Arrays&, umgen_sampling&) { c.out[m] = nullptr; });
            // the last token the form reads: scene 0's window for a frame call, scene B - 1's for a rollout, N > 1 or not -- the caller's index
            const size_t last = (size_t)(form == kFrameCall ? 1 : B) * T_IN * kModLen[m] - 1;
            for (long long v : {-1ll, (long long)kLim.vocab[m], 1ll << 40})
                expect(form, UMGEN_E_INVALID, plan_msg("%s token %lld at flat index %zu is outside [0, %d)", name[m], v, last, kLim.vocab[m]),
                       [m, v, last](GenCall&, Arrays& a, umgen_sampling&) { a.in[m][last] = v; });
            if (form == kFrameCall)      // scene 1 is not a frame call's
                expect(form, 0, "", [m, last](GenCall&, Arrays& a, umgen_sampling&) { a.in[m][last + 1] = -1; });
        }
}

static void test_control_and_given() {
    const Fault pose = [](GenCall& c, Arrays& a, umgen_sampling&) { c.ctrl_pose = a.cp.data(); }, boxes = [](GenCall& c, Arrays& a, umgen_sampling&) { c.ctrl_bbox3d = a.cb.data(); };
    const Fault test = [](GenCall& c, Arrays&, umgen_sampling&) { c.control_test = 1; };
    const Fault map = [](GenCall& c, Arrays& a, umgen_sampling&) { c.given_map = a.gm.data(); }, gboxes = [](GenCall& c, Arrays& a, umgen_sampling&) { c.given_bbox3d = a.gb.data(); };
    const auto both = [](const Fault& f, const Fault& g) { return [=](GenCall& c, Arrays& a, umgen_sampling& s) { f(c, a, s); g(c, a, s); }; };
    const auto zero_ctl = [](GenCall& c, Arrays&, umgen_sampling&) { c.T_ctl = 0; };
    for (GenForm form : kRollouts) {
        const size_t last = (size_t)B * T_CTL;      // (times S_mod, minus one: scene B - 1 of the caller's array)
        expect(form, UMGEN_E_INVALID, "control tokens given with T_ctl=0", pose, zero_ctl);
        expect(form, UMGEN_E_INVALID, "control tokens given with T_ctl=0", boxes, zero_ctl);
        expect(form, UMGEN_E_INVALID, "control pose token 32 at flat index 5 is outside [0, 32)", pose, [=](GenCall&, Arrays& a, umgen_sampling&) { a.cp[last * 3 - 1] = 32; });
        expect(form, UMGEN_E_INVALID, "control bbox3d token 40 at flat index 1319 is outside [0, 40) (and is not -1 = free)", both(boxes, test),
               [=](GenCall&, Arrays& a, umgen_sampling&) { a.cb[last * 660 - 1] = 40; });
        expect(form, UMGEN_E_INVALID, "control bbox3d token -2 at flat index 0 is outside [0, 40) (and is not -1 = free)", boxes, [](GenCall&, Arrays& a, umgen_sampling&) { a.cb[0] = -2; });
        expect(form, 0, "", boxes);      // (without control_test: the driver refuses it at the first controlled frame, behind the plan)
        expect(form, UMGEN_E_INVALID, "given tokens with T_ctl=-1", map, [](GenCall& c, Arrays&, umgen_sampling&) { c.T_ctl = -1; });
        expect(form, UMGEN_E_INVALID, "given tokens with T_ctl=0", gboxes, zero_ctl);
        expect(form, UMGEN_E_UNSUPPORTED, kBoxesWithoutMapRollout, gboxes);
        expect(form, UMGEN_E_INVALID, "given bbox3d tokens and bbox3d control exclude each other", both(map, gboxes), test);
        expect(form, UMGEN_E_INVALID, "given bbox3d tokens and bbox3d control exclude each other", both(map, gboxes), boxes);
        expect(form, 0, "", map, test);      // a given map alone stands beside control
        expect(form, UMGEN_E_INVALID, "given map token 48 at flat index 2047 is outside [0, 48)", map, [=](GenCall&, Arrays& a, umgen_sampling&) { a.gm[last * 1024 - 1] = 48; });
        expect(form, UMGEN_E_INVALID, "given bbox3d token -1 at flat index 1319 is outside [0, 40)", both(map, gboxes), [=](GenCall&, Arrays& a, umgen_sampling&) { a.gb[last * 660 - 1] = -1; });
    }
    // the frame form: one scene, one frame of each array; its own words and codes for what the given tokens exclude
    expect(kFrameCall, UMGEN_E_INVALID, "control pose token 32 at flat index 2 is outside [0, 32)", pose, [](GenCall&, Arrays& a, umgen_sampling&) { a.cp[2] = 32; });
    expect(kFrameCall, 0, "", pose, [](GenCall&, Arrays& a, umgen_sampling&) { a.cp[3] = 32; });
    expect(kFrameCall, UMGEN_E_INVALID, "control bbox3d token 40 at flat index 659 is outside [0, 40) (and is not -1 = free)", boxes, [](GenCall&, Arrays& a, umgen_sampling&) { a.cb[659] = 40; });
    expect(kFrameCall, UMGEN_E_UNSUPPORTED, "init_tokens['bbox3d'] without control_test is not a supported reference path", boxes);
    expect(kFrameCall, 0, "", both(boxes, test));
    expect(kFrameCall, UMGEN_E_UNSUPPORTED, kBoxesWithoutMapFrame, gboxes);
    expect(kFrameCall, UMGEN_E_UNSUPPORTED, "given tokens and control_test exclude each other", map, test);
    expect(kFrameCall, UMGEN_E_UNSUPPORTED, "given tokens and control_test exclude each other", both(map, gboxes), both(boxes, test));
    expect(kFrameCall, UMGEN_E_INVALID, "given map token 48 at flat index 1023 is outside [0, 48)", map, [](GenCall&, Arrays& a, umgen_sampling&) { a.gm[1023] = 48; });
    expect(kFrameCall, UMGEN_E_INVALID, "given bbox3d token 40 at flat index 0 is outside [0, 40)", both(map, gboxes), [](GenCall&, Arrays& a, umgen_sampling&) { a.gb[0] = 40; });
    expect(kFrameCall, 0, "", both(map, gboxes), pose);
}

// consecutive steps of the documented order, both faults injected: the earlier one is reported
static void test_order() {
    const std::vector<Step> steps = ladder();
    GenLimits raw = kLim;
    raw.finalized = false;
    for (GenForm form : kAll) {
        const auto text = [form](const Step& s) -> std::string {
            if (s.msg) return s.msg;
            if (std::string(s.name) == "counts") return form == kFrameCall ? "T=0 out of range [1,4]" : "T_in=0 new_frames=2 cond_frames=4 (max 4)";
            return form == kFrameCall ? kBoxesWithoutMapFrame : kBoxesWithoutMapRollout;
        };
        expect(form, UMGEN_E_STATE, steps[0].msg, steps[1].fault, nullptr, raw);
        for (size_t i = 1; i + 1 < steps.size(); ++i) {
            expect(form, steps[i].code, text(steps[i]), steps[i].fault, steps[i + 1].fault);
            expect(form, steps[i].code, text(steps[i]), steps[i + 1].fault, steps[i].fault);      // (whichever is injected first)
        }
        expect(form, steps.back().code, text(steps.back()), steps.back().fault);
    }
    // inside a step.  counts: B, N, B * N, then the frames; side: topk, temperature, lists; control before given; the pose before the boxes
    expect(kFanCall, UMGEN_E_INVALID, "N=0: at least one sample per scene", [](GenCall& c, Arrays&, umgen_sampling&) { c.N = 0; c.T_in = 0; });
    expect(kFanCall, UMGEN_E_INVALID, "B*N=8 (B=2, N=4) exceeds max_batch=4", [](GenCall& c, Arrays&, umgen_sampling&) { c.N = 4; c.cond_frames = 9; });
    expect(kRolloutCall, UMGEN_E_INVALID, "B=9 out of range [1,4]", [](GenCall& c, Arrays&, umgen_sampling&) { c.B = 9; c.new_frames = -1; });
    expect(kFrameCall, UMGEN_E_INVALID, "topk=17 out of range [0,16]", [](GenCall& c, Arrays&, umgen_sampling& s) { c.side.topk = 17; s.temperature = INFINITY; });
    expect(kFanCall, UMGEN_E_INVALID, "temperature must be > 0 and finite", [](GenCall& c, Arrays&, umgen_sampling& s) { c.side.topk = 0; s.temperature = INFINITY; });
    expect(kRolloutCall, UMGEN_E_INVALID, "pose token 99 at flat index 0 is outside [0, 32)", [](GenCall&, Arrays& a, umgen_sampling&) { a.in[0][0] = 99; a.in[1][0] = 99; });
    expect(kFanCall, UMGEN_E_INVALID, "control pose token 40 at flat index 0 is outside [0, 32)",
           [](GenCall& c, Arrays& a, umgen_sampling&) { c.ctrl_pose = a.cp.data(); c.ctrl_bbox3d = a.cb.data(); a.cp[0] = a.cb[0] = 40; });
    expect(kFrameCall, UMGEN_E_INVALID, "control bbox3d token 40 at flat index 0 is outside [0, 40) (and is not -1 = free)",
           [](GenCall& c, Arrays& a, umgen_sampling&) { c.ctrl_bbox3d = a.cb.data(); a.cb[0] = 40; });      // (before the bar on control_test)
    expect(kFrameCall, UMGEN_E_UNSUPPORTED, "init_tokens['bbox3d'] without control_test is not a supported reference path",
           [](GenCall& c, Arrays& a, umgen_sampling&) { c.ctrl_bbox3d = a.cb.data(); c.given_bbox3d = a.gb.data(); });
    expect(kFrameCall, UMGEN_E_UNSUPPORTED, "given tokens and control_test exclude each other",
           [](GenCall& c, Arrays& a, umgen_sampling&) { c.given_map = a.gm.data(); c.control_test = 1; a.gm[0] = -1; });
    expect(kFanCall, UMGEN_E_INVALID, "given bbox3d tokens and bbox3d control exclude each other",
           [](GenCall& c, Arrays& a, umgen_sampling&) { c.given_map = a.gm.data(); c.given_bbox3d = a.gb.data(); c.control_test = 1; a.gm[0] = -1; });
    expect(kFanCall, UMGEN_E_INVALID, "given map token -1 at flat index 0 is outside [0, 48)",
           [](GenCall& c, Arrays& a, umgen_sampling&) { c.given_map = a.gm.data(); c.given_bbox3d = a.gb.data(); a.gm[0] = a.gb[0] = -1; });
}

// the pieces the scoring calls take: a count of tokens, a count of frames
static void test_token_helpers() {
    const int64_t t[5] = {0, 7, -1, 8, 3};
    EXPECT(!check_tokens("x", t, 2, 8, false) && !check_tokens("x", t, 3, 8, true) && !check_tokens("x", t, 0, 1, false));
    EXPECT(check_tokens("x", t, 5, 8, false).msg == "x token -1 at flat index 2 is outside [0, 8)");
    EXPECT(check_tokens("x", t, 5, 8, true).msg == "x token 8 at flat index 3 is outside [0, 8) (and is not -1 = free)");
    Arrays a;
    const int64_t* const tok[4] = {a.in[0].data(), a.in[1].data(), a.in[2].data(), a.in[3].data()};
    EXPECT(!check_scene_tokens(kLim, (size_t)B * T_IN, tok));
    a.in[2][660 * 3] = 40;
    EXPECT(!check_scene_tokens(kLim, 3, tok));
    const Refusal r = check_scene_tokens(kLim, 4, tok);
    EXPECT(r.code == UMGEN_E_INVALID && r.msg == "bbox3d token 40 at flat index 1980 is outside [0, 40)");
    EXPECT(!check_detail_request(16, 1.f, true) && !check_detail_request(0, 3.0e38f, false));
}

int main() {
    test_valid();
    test_counts();
    test_sampling_and_side();
    test_buffers_and_tokens();
    test_control_and_given();
    test_order();
    test_token_helpers();
    if (failures) { printf("gen_call_test: %d FAILED\n", failures); return 1; }
    printf("gen_call_test: ok\n");
    return 0;
}
