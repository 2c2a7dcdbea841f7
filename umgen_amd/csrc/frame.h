// Per-frame data layout shared by the host engine (engine.hip) and the frame kernels (frame.hip): scene positions, embedding tables, window tokens, the
// device-resident decode state (OarState), and what a sampler touches (SampleArgs).  Whatever a sampler writes beside its token -- log-likelihood, logz,
// diagnostics -- is ONE bundle, TokenSide: SampleArgs carries it, the ego sampler takes it inside EgoSide, the engine owns one (umgen_engine::d_side) and
// decode lanes slice it with side_at.  Its host counterpart is FrameSide / GenSide (gen_side.h).  Whatever constrains a draw -- per-scene settings, logit-bias
// table sets -- is one bundle too, DrawPlan, behind the one switch OarState::plan: SampleArgs and EgoSide carry it, lanes slice it with plan_at.
#pragma once
#include <cstddef>

#include "common.h"
#include "sample_plan.h"

namespace umgen {

// scene-sequence positions (0-based) -- infer_fun.py:112-118, UMGen.py:976-992
constexpr int kPoseBos = 0, kPoseEos = 4, kMapBos = 5, kMapC0 = 6, kMapEos = 1030, kBoxBos = 1031, kBoxC0 = 1032, kBoxEos = 1692,
              kImgBos = 1693, kImgC0 = 1694, kImgEos = 2206;
constexpr int kNMap = 1024, kNBox = 660, kNImg = 512, kNPose = 3;
constexpr int kSlots = 60, kSlotLen = 11, kBoxPad = 1027;
constexpr int kTokPerFrame = kNPose + kNMap + kNBox + kNImg;   // 2199 content tokens, stored pose|map|bbox3d|image
constexpr int kOffMap = kNPose, kOffBox = kNPose + kNMap, kOffImg = kNPose + kNMap + kNBox;

enum Stack { STACK_EGO = 0, STACK_MAP = 1, STACK_BOX = 2, STACK_TAR = 3 };
__host__ __device__ inline int stack_len(int st) { return st == STACK_MAP ? 1031 : (st == STACK_BOX ? 1693 : 2207); }

// embedding tables (device pointers); fp32 unless noted
struct EmbedTables {
    const float *egoe, *axe, *be, *tpe, *spe, *tske;
    const bf16_t *fouier_pe, *posi, *grid_posi;   // bf16 sinusoid tables (UMGen.py:137-153)
    const float *gmap, *gimg;                     // GMLP(codebook) rows [vocab][E] (module.py:710-743 applied to every code once)
    int E;
};

// window tokens of the B scenes on the device: int32 [B][T][...]
struct WindowTokens {
    const int *pose;   // [B][T][3]   (already shifted one frame ahead for the TAR stacks, UMGen.py:1445-1452)
    const int *map;    // [B][T][1024]
    const int *box;    // [B][T][660]
    const int *img;    // [B][T][512]
    int B, T;          // scenes, history slots covered by this pass (rows of X are (b, t_local, s))
    int Tfull = 0;     // slots per scene in the token arrays / pose_diff (0: = T)
    int t0 = 0;        // first slot of the pass: tokens and tpe are indexed with t0 + t_local
};

constexpr unsigned kEpochPerStep = 16384;  // hand-off tags one decode step may use: (round or scene <= 32) x (layer <= 64) x (edge <= 8)
constexpr int kEngMaxSystolic = 32;        // scenes one systolic engine launch can carry (tag budget)

struct SamplerParams {
    int method, top_k, top_k_map, topk_image;
    float p, p_map, temperature;
    int rule_constrain, merge_ar_tar, only_ar;
};

// state of the OAR decode loop: device resident, so that one decode step is a fixed kernel sequence with fixed
// arguments and can be replayed from a hipGraph (everything that changes between steps / frames / calls lives here)
struct OarState {
    int step;        // input position j of the current step == KV length before the step
    int frame_idx;
    int use_forced;  // teacher forcing: take tokens from SampleArgs::forced
    int use_control; // control_test: SampleArgs::control_slot is valid
    int done;        // blocks of the step's last kernel that have finished (the last one advances `step`)
    unsigned epoch;  // base of the decode engine's hand-off tags for this step (advanced with `step`, oar_engine.hip)
    SamplerParams sp;
    // What the samplers write beside the token, into SampleArgs::side: every switch is per call and lives here, at the end of the struct (the decode engines
    // read step and epoch at the offsets they know; an older initialiser leaves the switches it does not name 0), so one captured step graph serves every kind
    // of call.  want_logp: the token's log-likelihood; want_detail: its diagnostics, the detail_topk <= kDetailTopK most likely tokens among them
    int want_logp;
    int want_detail;
    int detail_topk;
    int want_logz;   // the samplers also write logz (constrained sampling)
    // The one switch of constrained sampling, the last word: what the samplers read of SampleArgs::plan (DrawPlan).  Bit 0 (kPlanSettings) -- scene b draws
    // under plan.sp_of[b] instead of sp (umgen_rollout_planned); bit 1 (kPlanSets) -- the call has table sets, one (umgen_rollout_biased /
    // umgen_frame_biased) or several, and scene b's tables are set plan.set_of[b] of the pool (-1: none).  0: neither sampler executes anything beyond
    // testing the word
    int plan;
};
static_assert(offsetof(OarState, step) == 0 && offsetof(OarState, epoch) == 20, "the decode engines read step and epoch in front of the per-call switches");
enum { kPlanSettings = 1, kPlanSets = 2 };
constexpr int kBiasSetsMax = 16;    // == UMGEN_BIAS_SETS_MAX: table sets of the pool

// Logit-bias classes: the bit of a token class in a set's class word (DrawPlan::set_classes) is 1 << class; map / bbox3d / image are SampleArgs::mod.  The
// tables of a set lie back to back on the device: pose [3][pose_vocab] | map [map_vocab] | bbox3d [11][bbox3d_vocab] | image [img_vocab]
enum { kBiasPose = 0, kBiasMap = 1, kBiasBox = 2, kBiasImg = 3 };
constexpr int kBiasRowLen = 8192;   // a scratch row holds the largest vocabulary the samplers take
constexpr int kBiasRows = 3;        // scratch rows per scene: the biased AR and TAR rows of the token sampler (0, 1), the three pose rows of the ego sampler

// Diagnostics of a generated token (umgen_rollout_detail / umgen_frame_detail, block_detail in frame.hip), device buffers: rank, mass_above, entropy
// [B][2199]; topk_tok, topk_logp [B][2199][kDetailTopK] -- a call that lists K < kDetailTopK tokens writes the first K entries of a position.
constexpr int kDetailTopK = 16;   // == UMGEN_SCORE_TOPK_MAX
struct DetailOut {
    int* rank;
    float *mass_above, *entropy;
    int* topk_tok;
    float* topk_logp;
};
// The side outputs of a generated token, device buffers [B][2199] that the samplers write beside the token at the token's entry (block_token_side, frame.hip):
// logp = log softmax(AR row over [0, vocab))[token the step settled on]; logz = lse(w) - lse(v) of the AR row (+0.0 for a class without a table); the same
// token's diagnostics on the same row.  In SampleArgs every pointer is set and OarState's switches say what a step writes; in EgoSide a null member is
// not asked for (detail: a null rank)
struct TokenSide {
    float* logp;
    float* logz;
    DetailOut detail;
};
inline TokenSide side_at(const TokenSide& s, long scene) {   // the buffers of scene `scene` on (decode lanes, like d_tokens)
    const long o = scene * kTokPerFrame;
    const auto at = [o](auto* p, long per_token) { return p ? p + o * per_token : p; };
    const DetailOut& d = s.detail;
    return TokenSide{at(s.logp, 1), at(s.logz, 1), DetailOut{at(d.rank, 1), at(d.mass_above, 1), at(d.entropy, 1), at(d.topk_tok, kDetailTopK), at(d.topk_logp, kDetailTopK)}};
}

// What constrains a draw, ONE bundle like TokenSide: device pointers fixed at engine creation, read by the samplers under OarState::plan's bits (the ego
// sampler: EgoSide::plan_bits) and never otherwise.  SampleArgs and EgoSide carry it, the engine owns one (DecView::d_plan) and uploads through it, and
// decode lanes slice it with plan_at.  A call with one set of tables for every scene is the plan whose set_of is 0 everywhere.
struct DrawPlan {
    SamplerParams* sp_of;    // [B] per-scene settings (kPlanSettings)
    int* set_of;             // [B] the scene's table set in the frame being generated, -1 = none (kPlanSets)
    int* set_classes;        // [kBiasSetsMax] the class bits of every set
    float* pool;             // set 0 of the table pool; set s lies s * stride floats behind it
    long stride;             // floats per set
    long class_off[4];       // where pose / map / bbox3d / image start inside a set
    float* rows;             // [B][kBiasRows][kBiasRowLen] scratch of the scene's block: w = v + r of the AR / TAR row (token sampler: rows 0 / 1), of pose row jq (ego sampler)
};
// stride and class_off for the classes' vocabularies: the tables of a set back to back, pose [3][V] | map [V] | bbox3d [11][V] | image [V]
inline void lay_out_sets(DrawPlan& p, const int (&vocab)[4]) {
    p.stride = 0;
    for (int c = 0; c < 4; ++c) { p.class_off[c] = p.stride; p.stride += (long)kPlanTableRows[c] * vocab[c]; }
}
inline DrawPlan plan_at(const DrawPlan& p, long scene) {   // the plan of scene `scene` on (decode lanes)
    DrawPlan q = p;
    q.sp_of += scene; q.set_of += scene; q.rows += scene * kBiasRows * kBiasRowLen;
    return q;
}

// everything the per-token sampler kernel touches
struct SampleArgs {
    OarState* st;
    EmbedTables tb;
    const float* logits;       // [B][ld_logits] current AR head
    const float* logits_tar;   // [B][660][ld_tar] head_tar_bbox3d on the conditioning rows of the 660 bbox3d positions (one GEMM per frame)
    int ld_logits;
    int ld_tar;
    int vocab;                 // vocab of the current AR head
    int mod;                   // 1 map, 2 bbox3d, 3 image
    const float* cond;         // [B][2207][E]
    float* x_next;             // [B][E] input of the next step
    int* tokens;               // [B][2199] tokens of the frame being generated
    const int* prev_box;       // [B][660] bbox3d tokens of the last history frame (after control overwrite)
    const unsigned char* control_slot;   // [B][60] (valid when st->use_control)
    double* boxes;             // [B][64][10] decoded boxes of this frame (rule constraint), boxes[b][0] = ego
    int* n_boxes;              // [B]
    const unsigned long long* seeds;   // [B]
    const int* forced;         // [B][2199] teacher forcing (valid when st->use_forced)
    int* counters;             // [8] per-frame event counters (pad_avoid, control, rule_checked, rule_collision, rule_blanked, sampled != forced,
                               //     -, 7: unused since round 5 -- more than 64 ties at the k-th logit are sampled by an exhaustive walk, frame.hip)
    TokenSide side;            // [B][2199] side outputs of the token at its entry: what a step writes of them is st->want_logp / want_detail / want_logz
    DrawPlan plan;             // the scenes' own settings and table sets: what a step reads of them is st->plan
};

// what the ego sampler writes beside its three pose tokens, entries [b][jq] of `out`, and what constrains its draws (plan_bits 0: the plain call)
struct EgoSide {
    TokenSide out{};       // a null member is not asked for
    int detail_topk = 0;   // entries of the diagnostics' lists
    int plan_bits = 0;     // OarState::plan of the call
    DrawPlan plan{};       // the pose class of the scene's set, rows jq of scene b
};

void launch_embed_stack(hipStream_t s, int stack, const EmbedTables& tb, const WindowTokens& w, float* X, float* mapfeat);
// warp the map features by the ego motion and finish the map rows of X (UMGen.py:321-354, 729-736, 799-802, 836-840)
void launch_warp_map(hipStream_t s, int stack, const EmbedTables& tb, int B, int T, const float* mapfeat, const float* pose_diff,
                     float* X, float* warped_last, int Tfull = 0, int t0 = 0, float* warped_all = nullptr);   // warped_all: [B][T][1024][E], every slot's warped map
// conditioning rows: LayerNorm of the last history frame of a stack (+ warped-map prior) -> cond[b][s] (UMGen.py:1496-1511)
void launch_cond_rows(hipStream_t s, int stack, int B, int T, int E, const float* X, const float* ln_w, const float* warped_last,
                      float* cond);
// the same rows of (scene, slot) items of a pass over T slots: items [n_items][2], warped_all [B][T][1024][E] (STACK_MAP) -> cond_all [n_items][2207][E]
void launch_cond_rows_slots(hipStream_t s, int stack, int T, int E, const float* X, const float* ln_w, const float* warped_all, const int* items,
                            int n_items, float* cond_all);
// x[b] = row (+ cond[b][pos])
void launch_first_input(hipStream_t s, int B, int E, const float* tske_row, const float* cond, float* x);
void launch_fixed_token(hipStream_t s, const SampleArgs& a, int B);             // bos/eos/pose prefix steps
// given-token prefix as one pass (engine.hip run_prefix_prefill): decode inputs of positions 0 .. P - 1, and a pass's k | V^T rows -> the decode cache
void launch_prefix_rows(hipStream_t s, const EmbedTables& tb, const float* tske_row, const float* cond, const int* tokens, int B, int P, float* X,
                        float* x_last);
template <typename T>
void launch_prefix_kv_to_cache(hipStream_t s, const T* qk, const T* vt, int B, int S, int S_pad, int H, int Lmax, T* cache, long scene_stride);
void launch_sample_token(hipStream_t s, const SampleArgs& a, int B);            // sampled steps
// ego head: sample 3 pose tokens per scene from logits [B*3][vocab]
void launch_sample_rows(hipStream_t s, const float* logits, int V, int k, float temp, const float* u, int* out, int* overflow, int n);   // test hook
// test hooks: block_sample (top-k or top-p by sp.method) with a masked index; check_collision_dev on sets of <= 64 boxes [n_sets][max_n][10]
void launch_sample_dbg(hipStream_t s, const float* logits, int V, const SamplerParams& sp, int k, float p, const float* u, int mask_idx, int* out,
                       int* overflow, int n);
void launch_collision_rows(hipStream_t s, const double* boxes, const int* counts, int max_n, int* out, int n_sets);
void launch_sample_ego(hipStream_t s, const float* logits, int vocab, SamplerParams sp, const unsigned long long* seeds, int frame_idx,
                       const int* forced, int* out_tokens, int B, int* overflow, const EgoSide& es = EgoSide{});
// test hook: block_sample on n rows w = logits + bias (their own bias rows [n][V], scratch rows [n][kBiasRowLen]) with given uniforms and one masked index
void launch_sample_dbg_biased(hipStream_t s, const float* logits, const float* bias, float* rows, int V, const SamplerParams& sp, int k, float p, const float* u,
                              int mask_idx, int* out, int* overflow, int n);
// ego query rows: egoe[j] + spe[j] + tpe[T-1]; item_T [B] on the device (or nullptr): item i's own window length instead of T
void launch_ego_queries(hipStream_t s, const EmbedTables& tb, int B, int T, float* x, const int* item_T = nullptr);

}  // namespace umgen
