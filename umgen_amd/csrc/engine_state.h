// State of the host engine, shared by the engine_*.hip files: the weight table and struct umgen_engine (one block of members per mechanism),
// the per-frame call arguments (FrameIO) and the scoring calls' (ScoreIO ...), which carry their host tokens as a TokenView (token_windows.h),
// where a stack pass runs (Place: stream and workspaces, an argument of every pass) and what a decode step reads and writes per scene (DecView: the engine
// holds the whole batch's as `dv`, a decode lane gets its sub-batch's from lane_view; both are arguments, nothing is swapped into the engine around a
// call), the path a decode step takes (DecodePath), and the declarations of the functions that cross files.  A generated token's side outputs
// (log-likelihood, logz, diagnostics) take one path: FrameIO::side (FrameSide, gen_side.h) says what a frame's call asked for, dv.d_side (TokenSide,
// frame.h) holds the device buffers, and side_buffers pairs the two for the 0xFF fill and the copy back.  What constrains a draw takes one path too:
// FrameIO::plan / set_of say what a frame's call brought, dv.d_plan (DrawPlan, frame.h) holds the device side -- per-scene settings, the pool of table
// sets, the scenes' sets of the frame, the scratch rows -- whether the call came with one set of tables or with a plan.
// No code that launches or decides anything lives here.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdarg>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/umgen.h"
#include "bg_queue.h"
#include "frame.h"
#include "gen_side.h"
#include "kernels.h"
#include "sample_plan.h"
#include "token_windows.h"

static_assert(umgen::kBiasSetsMax == UMGEN_BIAS_SETS_MAX && umgen::kPlanSetsMax == UMGEN_BIAS_SETS_MAX, "one limit on the table sets of a sampling plan");

using namespace umgen;

#define HIPCHK(e, call)                                                                              \
    do {                                                                                             \
        hipError_t _err = (call);                                                                    \
        if (_err != hipSuccess) return (e)->fail(UMGEN_E_HIP, "%s -> %s", #call, hipGetErrorString(_err)); \
    } while (0)

namespace umgen {

struct AttnW { void* Wqkv; float* bqkv; void* Wo; float* bo; };
struct MlpW { void* Wfc; void* Wproj; };
struct SubW { float* ln_a; AttnW attn; float* ln_b; MlpW mlp; };
struct TarW { SubW sub[3]; };
struct DecW { float* ln1; AttnW self; float *ln2, *ln3; void* Wq; float* bq; void* Wkv; float* bkv; void* Wco; float* bco; float* ln4; MlpW mlp; };

struct Slot {            // destination of one state-dict entry
    void* dst;
    std::vector<int64_t> shape;
    int kind;            // 0: fp32 param, 1: T (precision dtype) weight, 2: bf16 table
    bool loaded;
    bool optional;
};

// What a decode step reads and writes per scene, and how it is enqueued: the only home of these buffers.  umgen_engine::dv is the whole batch's
// (engine_setup.hip allocates into it; its stream and flags stay unset); a step takes a copy with the call's stream and flags, a decode lane the view
// of its sub-batch (lane_view: scenes b0 .. b0 + nb - 1 of every per-scene array, its own stream / step state / fragment buffers).
struct DecView {
    hipStream_t stream;      // the step's launches go here
    bool lane;               // a lane's sub-batch of a batch that took the batched layer: so does the lane (use_batched); timed around its graph launches
    bool capture;            // the step is being captured into a graph: no per-step events, no hipGetLastError
    float *xdec, *qdec, *logits, *logits_tar, *cond, *xfrag, *afrag, *hfrag;   // (xfrag / afrag / hfrag: fragment-major x / attention output [64 E], gelu(c_fc) [64 x 4E] of the batched layer)
    void* kvcache;
    int *d_tokens, *d_prev_box, *d_nboxes;
    unsigned char* d_control;
    double* d_boxes;
    unsigned long long* d_seeds;
    OarState* d_state;
    // [max_batch][2199] (the lists x kDetailTopK) side outputs of the frame being generated (SampleArgs::side), allocated with the engine -- like d_plan
    // -- so that every captured step graph holds the final pointers
    TokenSide d_side;
    // Constrained sampling (SampleArgs::plan; umgen_rollout_biased / umgen_frame_biased / umgen_rollout_planned), read under OarState::plan only: sp_of
    // [max_batch] per-scene settings and set_classes, uploaded once per call with the pool [kBiasSetsMax] sets of pose [3][pose_vocab] | map [map_vocab] |
    // bbox3d [11][bbox3d_vocab] | image [img_vocab] (a call's one set is set 0); set_of [max_batch], the scenes' table sets in the frame being generated
    // (-1 = none), uploaded per frame; rows [max_batch][kBiasRows][kBiasRowLen], the samplers' scratch
    DrawPlan d_plan;
};

}  // namespace umgen

struct umgen_engine {
    umgen_config cfg{};
    int E = 0, H = 0;
    size_t tsz = 4;                      // sizeof(T)
    hipStream_t stream = nullptr;        // the foreground stream (the decode stream of overlapped rollouts); assigned in engine_setup.hip only
    std::string err = "";
    std::map<std::string, Slot> slots;
    std::vector<void*> allocs;
    bool finalized = false;
    // weights
    std::vector<TarW> stk[4];            // STACK_EGO, STACK_MAP, STACK_BOX, STACK_TAR
    std::vector<SubW> oar;
    std::vector<DecW> dec;
    float *ln_ego_tar = nullptr, *ln_ego = nullptr, *ln_tar = nullptr, *ln_oar = nullptr, *ln_map_tar = nullptr, *ln_box_tar = nullptr;
    void *head_ego = nullptr, *head_ar_map = nullptr, *head_ar_box = nullptr, *head_tar_box = nullptr, *head_ar_img = nullptr;
    void *map_fc = nullptr, *map_proj = nullptr, *img_fc = nullptr, *img_proj = nullptr;
    float *map_cb = nullptr, *img_cb = nullptr;
    EmbedTables tb{};
    // workspace
    float *warped_last = nullptr, *pose_diff = nullptr, *pego = nullptr;
    float *part = nullptr, *hdec = nullptr, *qkv3 = nullptr;
    DecView dv{};                        // the per-scene decode buffers of the whole batch
    long kv_layer_stride = 0, kv_scene_stride = 0;
    int Lmax = kAttnSplit * kAttnChunk, S_pad = 2240;   // cache rows per head: every split's fixed key range is addressable
    int *d_pose = nullptr, *d_pose_shift = nullptr, *d_map = nullptr, *d_box = nullptr, *d_img = nullptr;
    int *d_forced = nullptr, *d_counters = nullptr, *d_ego_tok = nullptr;
    // umgen_score (engine_score.hip run_score): per (row, vocabulary split) records of the scoring head, and its results pose | map | bbox3d | image,
    // each block [max_batch][S_mod]
    float *score_part = nullptr, *score_logp = nullptr;
    int* score_arg = nullptr;
    // umgen_score_candidates (engine_score.hip run_score_candidates): the scene of every item (b, c) of the chunk in flight, [max_batch], and the number of
    // scenes whose slot caches the chunk's last-slot pass reads travels with the pass (run_stack's fan_scenes; CACHE_SHARED_ITEMS); umgen_rollout_fan's first
    // frame (run_frame_fan) uses both the same way for its B * N branches (CACHE_SHARED_ITEMS / CACHE_SHARED_ITEMS_APPEND), umgen_score_futures for its B * C
    // items (CACHE_SHARED_ITEMS_TAIL)
    int* d_item_scene = nullptr;
    // umgen_score_futures (engine_score.hip run_score_futures): per-scene history passes of the last call (read by the test hook umgen_dbg_score_futures_passes)
    int fut_history_passes = 0;
    // umgen_score_clip (engine_score.hip run_score_clip): allocated by its first call (ensure_score_clip), for max_batch * max_cond_frames items (b, slot) of one
    // window pass.  clip_items [n][2] (scene, slot) and clip_item_T [n] (window length slot + 1); clip_warped [max_batch][max_cond_frames][1024][E], the map
    // stack's warped map of every slot; clip_cond [n][2207][E]; clip_tokens [n][2199], each item's scored frame; clip_xlast [n][E] (the prefix rows' unused
    // last position); clip_part / clip_logp / clip_arg: score_part / score_logp / score_arg for n items.  clip_state: 0 not tried, 1 allocated, -1 no room
    int *clip_items = nullptr, *clip_item_T = nullptr, *clip_tokens = nullptr, *clip_arg = nullptr;
    float *clip_warped = nullptr, *clip_cond = nullptr, *clip_xlast = nullptr, *clip_part = nullptr, *clip_logp = nullptr;
    int clip_state = 0;
    // umgen_score_detail: allocated by its first call (engine_score.hip ensure_score_detail).  det_part: the detail sweep's (row, split) records; det_row:
    // lse | target logit | row maximum | sum-exp of one modality's rows, [4][max_batch * 1024]; the results in score_logp's block layout, the lists with room for 16 per row (a call packs its topk)
    float *det_part = nullptr, *det_row = nullptr, *det_mass = nullptr, *det_ent = nullptr, *det_tlp = nullptr;
    int *det_rank = nullptr, *det_tok = nullptr;
    // Overlapped TAR pass.  Causal temporal attention + frame-local spatial attention make every history
    // slot but the last one of the NEXT frame's window independent of the frame being decoded, so those slots are pushed through
    // the ego / map / box / TAR stacks on `bg_stream` (a CU-masked stream) while the latency-bound decode loop runs on the
    // other CUs; their temporal k | v rows are kept per layer in `tcache`.  The next frame then only computes its last slot.
    bool overlap = false, overlap_suspended = false;
    bool conc_stacks = false;            // plain path: the map / box stacks on side streams beside the TAR stack (UMGEN_CONCURRENT_STACKS, default on)
    int last_B = 0;
    float last_full_pre_ms = 0.f, last_oar_ms = 0.f;   // ego + TAR phase of the last whole-window frame / decode loop of the last frame
    int overlap_mode = 1;                // UMGEN_OVERLAP: 0 off, 1 on for one scene per GPU (default), 2 always
    hipStream_t bg_stream = nullptr;
    // the stacks' workspaces: w_main, and w_side for the last-slot passes of the map / box stacks, which run beside the TAR stack's on their own streams
    struct Work { float* X; void *A, *QKV, *VT, *Hb; float* mapfeat; };
    Work w_main{}, w_side[2] = {};
    hipStream_t side_stream[2] = {nullptr, nullptr};
    hipEvent_t ev_side_in = nullptr, ev_side_done[2] = {nullptr, nullptr};
    hipStream_t full_stream = nullptr;   // unmasked: whole-window passes, profiling frames and rollouts that do not overlap use all CUs
    hipEvent_t ev_pre_done = nullptr;
    hipEvent_t ev_tar_done = nullptr, ev_bg_done = nullptr, ev_bg0 = nullptr;
    bool bg_pending = false;
    // The overlapped pass ON THE DECODE ENGINE'S IDLE XCDs (round 6; bg_worker.h): one scene per GPU runs the engine on 4 of the 8 XCD groups (same step
    // time) and the engine workgroups of the other four execute the pass as an op list, recorded from the very launchers of the stand-alone kernels
    // (BgRecorder).  No second stream, no CU masks: the pass advances inside the decode steps' launches and is drained behind the frame's last step.
    bool bg_engine = false;
    BgQueue* d_bgq = nullptr;
    struct BgHead { unsigned w[4]; EmbedTables tb; } bg_head{};      // staging of the queue's header (must outlive the asynchronous upload)
    BgRecorder bg_rec;                   // host copy of the op list in flight (kept: the asynchronous uploads read it, and the next pass is compared with it)
    std::vector<unsigned> bg_state_host; // worker states read back behind the drain
    hipEvent_t ev_drain0 = nullptr, ev_drain1 = nullptr;
    std::vector<void*> tcache[4];        // per stack, per BlockTAR: [max_batch][max_cond_frames][S_stack][2E] of T
    // Growing window in the FOREGROUND (control mode starts with 13 history frames and grows to the cap,
    // infer_fun.py:64-71, UMGen.py:1600-1603): while the window grows, slot t of frame n + 1's window is slot t of frame n's window --
    // same tokens (the control overwrite of the last bbox3d frame persists, UMGen.py:1465-1467), same tpe row, and every later block
    // sees it through frame-local spatial sub-blocks and a CAUSAL temporal sub-block (module.py:332-359) -- so a frame that is followed
    // by a longer window leaves the temporal k | v rows of all its slots in the slot caches (allocated on first use), and the next
    // frame pushes only its new last slot through the stacks.  No second stream: this is the production path with the decode engine.
    bool grow_cache = true;              // UMGEN_GROW_CACHE=0: recompute the whole window every frame, like the reference
    int tcache_state = 0;                // 0 not tried, 1 allocated, -1 does not fit (plain path)
    struct Prefix {
        bool valid = false, has_ego = false;
        int B = 0, P = 0, Tfull = 0;
        TokenSeqs win;                          // slots 0..P-1 of the window the pass was computed for, [B][P][S_mod]
        std::vector<int> pose_next;             // [B][3] pose tokens the new frame must carry (they sit in shifted slot P-1)
    } px;
    TokenSeqs px_up;                        // host staging of the background pass's uploads (must outlive the async copies)
    std::vector<int> px_pshift;
    std::vector<float> px_pdiff;
    // timing
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    umgen_timings tm{};
    bool profiling = false;
    int rows_per_block = -1;              // few-row launches: rows per workgroup; -1 = by row count (1 up to 6 rows, else 2), 0 = row loop
    bool dbg_same_layer = false;          // UMGEN_DEBUG_SAME_LAYER=1: timing experiment, every decode layer reads layer 0's weights
    // decode step graphs per (kind: fixed / map / bbox3d / image, number of attention key splits 1..8)
    hipGraphExec_t step_graph[4][kAttnSplit + 1] = {};
    int step_graph_B = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> gemm_ev, attn_ev, layer_ev;
    size_t gemm_ev_used = 0, attn_ev_used = 0, layer_ev_used = 0;
    // XCD-resident decode engine (oar_engine.hip): one launch per decode step instead of five per layer
    struct EngStream { bool ok = false; int NG = 0; unsigned char map[16]; };
    bool eng_enabled = false, eng_fallback = false;   // eng_fallback: wanted, but the census failed (umgen_timings::engine_fallback)
    EngStream eng_fg, eng_full;          // census of the decode stream (CU-masked when the overlap exists) and of the unmasked stream
    OarLayerDev* d_layers = nullptr;
    unsigned long long *eng_gx = nullptr, *eng_gloc = nullptr;
    unsigned int *eng_ticket = nullptr, *eng_err = nullptr;
    std::vector<void*> eng_wp2;             // per BlockOAR: mlp c_proj repacked for the engine's hidden-unit split (repack_mlp_proj)
    std::vector<void*> eng_wf2;             // per BlockOAR: c_fc as matrix-core fragments (repack_mlp_proj)
    unsigned long long* eng_stamps = nullptr;   // UMGEN_DEBUG_TIMING: per-phase ticks of the engine (printed at destroy)
    size_t eng_gloc_bytes = 0;
    // Chip-wide decode engine for wide layers (oar_engine_wide.hip; n_embd 1536; one launch per scene and step).  Default: engines created for ONE scene per
    // call (two scenes as two launches: step 1696 us against 1523 on five launches per layer, four: 3382 against 2217 -- profiles/r05_wide2x_engine.txt);
    // UMGEN_DECODE_WIDE=n (1..4): engines of up to n scenes per call; =0: five launches per layer
    bool wide_enabled = false;
    OarLayerDev* d_layers_wide = nullptr;
    std::vector<void*> wide_wp2;            // per BlockOAR: mlp c_proj repacked [256 ranks][E rows][24 hidden units of the rank]
    unsigned long long* wide_gran = nullptr;
    unsigned int *wide_ticket = nullptr, *wide_err = nullptr;
    unsigned long long* wide_stamps = nullptr;
    bool use_wide(int B) const { return wide_enabled && tsz == 2 && B <= 4; }
    void* burn_buf = nullptr;             // UMGEN_DEBUG_BURN (measurement builds): the synthetic load's stream buffer
    int fg_xcds = 8;
    unsigned eng_epoch = 16u;             // first hand-off tag of the next frame (see run_frame)
    int step_graph_NG = -1;
    const EngStream* eng_for(hipStream_t s) const {
        if (!eng_enabled) return nullptr;
        const EngStream* es = (full_stream && s == full_stream) ? &eng_full : &eng_fg;
        return es->ok ? es : nullptr;
    }
    double gemm_flops_pending = 0, attn_flops_pending = 0;
    // Batched decode layer (decode_batched.hip) from `batched_min` scenes per launch on (UMGEN_DECODE_BATCHED=n; 0 = never): the weights
    // once per step for the whole batch, the scenes as the matrix-core instruction's B-columns
    int batched_min = 24;               // measured crossover with the engine (profiles/r04_lanes_sweep.txt): 20 scenes 1546 (engine) vs 1674 us per step, 24: 1843 vs 1708, 28: 2104 vs 1775
    bool use_batched(int B, bool lane = false) const {      // (lane: a lane's sub-batch of a batch that qualified, DecView::lane)
        return tsz == 2 && (lane || (batched_min > 0 && B >= batched_min)) && B <= kRowsMaxM && E % 32 == 0 && E <= 768;
    }
    // Decode LANES: the scenes of a batch are independent until the frame is complete (own K/V rows, own sampler state, own RNG
    // stream), and a batched layer launch for <= 16 scenes is latency-bound (5 dependent launches per layer, 48 - 96 workgroups each,
    // 34 us per layer whatever the batch is) while its attention launch is the only part at the HBM roof.  The batch is therefore cut
    // into `lanes` sub-batches, each with its own stream, OarState, fragment buffers and step graphs, forked once behind the TAR stacks
    // and joined once before the token download: one lane's weight GEMMs run in the shadow of another lane's K/V stream.  Tokens are
    // those of the single-lane batched layer bit for bit (a scene's column never mixes with another's, decode_batched.hip).
    static constexpr int kMaxLanes = 8;
    struct DecLane {
        hipStream_t s = nullptr;
        hipEvent_t done = nullptr;
        OarState* st = nullptr;
        float *xfrag = nullptr, *afrag = nullptr, *hfrag = nullptr;
        hipGraphExec_t graph[4][3] = {};
    };
    DecLane lane[kMaxLanes];
    hipEvent_t ev_lane_fork = nullptr;
    int lanes_env = -1;                  // UMGEN_DECODE_LANES=n: n lanes whenever the batched layer runs (1 = off); -1: by batch size
    int lane_graph_B = 0, lane_graph_n = 0;
    int lane_count(int B) const {
        if (!use_batched(B) || !lane[0].s) return 1;
        // measured (profiles/r04_lanes_sweep.txt): lanes of 16 scenes (one full column block of the matrix-core instruction) are best --
        // 32 scenes 2132 / 1829 / 2040 us per step on 1 / 2 / 4 lanes, 64 scenes 3284 / 2689 / 2532 on 1 / 2 / 4; the device runs four
        // streams' kernels at a time (8 lanes: two rounds, 3784 / 4063 us)
        // ; from the threshold of 24 scenes on at least two lanes (24 scenes: 1978 us on one lane, 1708 on two)
        // ; lanes of at most 16 scenes: 40 scenes 2285 / 2020 / 2136 us on 2 / 3 / 4 lanes, 48: 2182 / 2231 on 3 / 4, 56: 2570 / 2369 on 3 / 4
        int n = lanes_env > 0 ? lanes_env : std::min(4, std::max(B >= 24 ? 2 : 1, (B + 15) / 16));
        return std::max(1, std::min(std::min(n, kMaxLanes), B));
    }
    hipError_t launch_status = hipSuccess;   // first refused kernel launch of the frame (hipGetLastError behind the GEMM launches): fails the frame

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

namespace umgen {

// ---- engine_setup.hip: device allocations owned by the engine, the slot caches --------------------------------------
int dev_alloc(umgen_engine* e, void** p, size_t bytes);
template <typename P>
int dalloc(umgen_engine* e, P** p, size_t n) { return dev_alloc(e, reinterpret_cast<void**>(p), n * sizeof(P)); }
bool ensure_tcache(umgen_engine* e);

// Few-row launches with several rows (scenes, ego queries): one row per workgroup keeps the single-row dependency chain (4 scenes:
// 2.58 vs 3.12 s of decode per frame) but re-reads the weights from L2 once per row; from 7 rows on, 2 rows per workgroup win
// (8 scenes: 3.53 vs 3.77 s).  UMGEN_ROWS_PER_BLOCK overrides (0 = every workgroup loops over all rows).
inline int rows_per_block_for(const umgen_engine* e, int M) { return e->rows_per_block >= 0 ? e->rows_per_block : (M <= 6 ? 1 : 2); }

static_assert(kModLen[0] == kNPose && kModLen[1] == kNMap && kModLen[2] == kNBox && kModLen[3] == kNImg && kModOff[1] == kOffMap && kModOff[2] == kOffBox &&
                  kModOff[3] == kOffImg && kFrameRowLen == kTokPerFrame, "token_windows.h states the frame layout of frame.h");
static_assert(kSideTopK == kDetailTopK, "gen_side.h states the list length of frame.h");

// f(T{}) for the engine's precision T: templates on T do not cross files, so every file dispatches its own through this
template <typename F>
auto with_precision(const umgen_engine* e, F&& f) {
    return e->cfg.precision == UMGEN_PREC_BF16 ? f(bf16_t{}) : e->cfg.precision == UMGEN_PREC_FP16 ? f(f16_t{}) : f(float{});
}

// What a pass through a stack (run_stack, w its WindowTokens) does with the per-layer slot caches of temporal k | v rows.  The values are fixed.
enum CacheMode {
    CACHE_NONE = 0,                // one pass over the whole window, no slot caches
    CACHE_FILL_PREFIX = 1,         // prefix pass: slots [0, w.T), their k | v rows appended to the slot caches
    CACHE_LAST_SLOT = 2,           // last-slot pass: slots [w.t0, w.t0 + w.T) against the caches
    CACHE_WINDOW_KEEP = 3,         // whole window like CACHE_NONE, and its k | v rows are left in the slot caches for a longer window that follows
    CACHE_LAST_SLOT_APPEND = 4,    // last-slot pass like CACHE_LAST_SLOT that appends its own k | v rows (the window keeps growing)
    // last-slot pass of w.B ITEMS (w.T == 1, w.t0 = P) that share the caches of fan_scenes scenes (run_stack's argument): item i reads the slots [0, P) of scene
    // e->d_item_scene[i] (umgen_score_candidates; the token arrays and pose_diff hold every item's own window)
    CACHE_SHARED_ITEMS = 5,
    // ... and item i appends its own k | v rows to block i of the caches (umgen_rollout_fan ahead of a longer window: spread_tcaches then hands every
    // item its scene's slots [0, P))
    CACHE_SHARED_ITEMS_APPEND = 6,
    // tail pass of w.B ITEMS that share the caches of fan_scenes scenes like CACHE_SHARED_ITEMS, with w.T >= 1 slots [w.t0, w.t0 + w.T) of their own each
    // (umgen_score_futures: future frame k of a candidate brings k + 1 slots); nothing is written to the caches.  The final block's last-frame shortcut
    // applies to the tail (w.T > 1), as it does to a whole window
    CACHE_SHARED_ITEMS_TAIL = 7,
};
constexpr bool cache_writes(CacheMode m) { return m == CACHE_FILL_PREFIX || m == CACHE_WINDOW_KEEP || m == CACHE_LAST_SLOT_APPEND; }   // launch_attn_temporal appends
constexpr bool cache_whole_window(CacheMode m) { return m == CACHE_NONE || m == CACHE_WINDOW_KEEP; }
constexpr bool cache_last_frame_shortcut(CacheMode m) { return cache_whole_window(m) || m == CACHE_SHARED_ITEMS_TAIL; }                // run_stack's `last`
constexpr int cache_fan_form(CacheMode m) {                                                                                             // tar_sub's `fan`
    return m == CACHE_SHARED_ITEMS ? 1 : (m == CACHE_SHARED_ITEMS_APPEND ? 2 : (m == CACHE_SHARED_ITEMS_TAIL ? 3 : 0));
}

struct FrameIO {
    int B, T;
    TokenView win;                               // host window tokens [B][T][S_mod] (box already control-overwritten)
    const int* ctrl_pose;                        // host [B][3] or nullptr: pose given (init_tokens["pose"])
    const unsigned char* control_slot;           // host [B][60] or nullptr
    int frame_idx;
    const umgen_sampling* smp;
    const umgen_trace* trace;                    // B == 1 only
    int* out_tokens;                             // host [B][2199]
    const FrameSide* side = nullptr;             // or nullptr: the side outputs the call asked for of every content token of the new frame (NaN / -1 where no head ran)
    int plan = 0;                                // OarState::plan of the call: kPlanSettings (dv.d_plan.sp_of is uploaded), kPlanSets (the pool is, and set_of below)
    const int* set_of = nullptr;                 // host [B] with kPlanSets: the scenes' table sets in this frame, -1 = none (column f of the plan's index)
    int cond_cap = 0;                            // window cap (cond_frames) of the rollout; 0 = single frame, nothing follows
    bool next_follows = false;                   // another frame of the same rollout follows: run its prefix pass beside the decode
    bool next_has_ctrl_pose = false;             // ... and its pose is given, so the ego net's prefix is not needed
    const int* given_map = nullptr;              // host [B][1024] or nullptr: the new frame's map is given (predefined-token prefix)
    const int* given_box = nullptr;              // host [B][660] or nullptr: ... and its boxes (only behind a given map)
};

// Where a scoring call leaves its results: per modality [N][S_mod] for the call's N items in its own order (umgen_score_out's layout); any pointer may be null
struct ScoreDst { float* logp[4]; int* argmax[4]; };
// what umgen_score_detail computes beside the scores: ScoreDst's layout, the lists with topk entries per position (unused when topk == 0)
struct ScoreDetailIO {
    int topk; float temperature;
    int* rank[4]; float *mass_above[4], *entropy[4];
    int* topk_tok[4]; float* topk_logp[4];
};
// umgen_score's arguments: B scenes' history windows and the frame to score, as host int32 arrays
struct ScoreIO {
    int B, T;
    TokenView win;                               // [B][T][S_mod]
    const int* next;                             // [B][2199]: the scored frame, pose | map | bbox3d | image
    ScoreDst out;
    long row0 = 0;                               // scene b's results go to row row0 + b of `out` ...
    const long* rows = nullptr;                  // ... or, when given, to row rows[b]
    const ScoreDetailIO* detail = nullptr;       // umgen_score_detail: what else to compute (rows row0 + b)
};

// umgen_score_candidates' arguments: B scenes' history windows and C candidate next frames of every scene
struct ScoreCandIO {
    int B, T, C;
    TokenView win;                               // [B][T][S_mod]
    const int* next;                             // [B][C][2199]: the candidates, pose | map | bbox3d | image
    ScoreDst out;                                // candidate (b, c) at row b*C + c
    int shared_slots;                            // out: T - 1 when the history slots ran once per scene, 0 on the replicated path
};

// umgen_score_futures' arguments: B scenes' histories of T frames and C candidate futures of K frames per scene; future frame k of candidate (b, c) is scored
// against the last min(T + k, cond) frames of history[b] ++ future[b][c]
struct ScoreFutIO {
    int B, T, C, K, cond;
    TokenView win;                               // [B][T][S_mod]
    TokenView fut;                               // [B * C][K][S_mod]
    ScoreDst out;                                // frame k of candidate (b, c) at row (b*C + c)*K + k
    int* shared_slots;                           // out, [K]: per future frame the history slots that ran once per scene, 0 on the replicated path
};

// umgen_score_clip's arguments: B recorded clips of L frames; every frame f in [T_in, L) is scored against the min(f, cond) frames before it
struct ScoreClipIO {
    int B, L, T_in, cond;
    TokenView clip;                              // [B][L][S_mod]
    ScoreDst out;                                // frame f of clip b at row b*(L - T_in) + f - T_in
    int shared_frames;                           // out: frames per clip that were read off one window pass, 0 on the per-frame path
};

// what run_prefix_prefill reads and writes instead of the engine's per-scene buffers (umgen_score_clip: more items than max_batch)
struct PrefillSrc {
    const float* cond;                           // [B][2207][E]
    const int* tokens;                           // [B][2199]
    float* x_last;                               // [B][E]
    bool skip_cache;                             // leave the decode cache alone (it holds max_batch scenes; a scoring pass never reads it)
};
// run_stack's `tail`
enum { TAIL_AUTO = -1, TAIL_NONE = 0 };

// ---- engine_weights.hip ---------------------------------------------------------------------------------------------
void decode_pose_shift(const int* pose, const int* ego, int B, int Tn, std::vector<int>& pshift, std::vector<float>& pdiff);

// Where a stack pass runs: its stream and the workspaces it owns (umgen_engine::w_main, or a side stream's w_side[i]).  An argument of every pass:
// the engine keeps no "current" stream or workspace.  capture: the launches are being captured into a graph (gemm_timed then leaves hipGetLastError alone)
struct Place { hipStream_t stream; const umgen_engine::Work* work; bool capture = false; };

// ---- engine_stacks.hip: by-precision entry points of the templated compute path ------------------------------------
// fan_scenes (the CACHE_SHARED_ITEMS modes): the scenes whose slot caches the pass's items share through e->d_item_scene
void run_stack_any(umgen_engine* e, const Place& pl, int stack, const WindowTokens& w, CacheMode cache_mode, int tail = TAIL_AUTO, float* warped_all = nullptr,
                   int fan_scenes = 0);
void ego_decoder_any(umgen_engine* e, const Place& pl, int n, const long* frame_of, int Tq, const int* d_item_T);
void run_ego_any(umgen_engine* e, const Place& pl, const WindowTokens& w, const SamplerParams& sp, int frame_idx, bool forced, float* trace_logits,
                 CacheMode cache_mode, const EgoSide& es = EgoSide{});
void run_ego_fan_any(umgen_engine* e, const Place& pl, const WindowTokens& w, int N, const SamplerParams& sp, int frame_idx, CacheMode cache_mode, const EgoSide& es);
int run_prefix_prefill_any(umgen_engine* e, const Place& pl, int B, int P, const PrefillSrc* src = nullptr);
// what the test hooks of debug_bg.hip change about a background pass (launch_prefix)
struct BgPassDebug {
    int foreground;                              // 1: the pass as stand-alone launches on the caller's stream, synchronised; 0: recorded and uploaded, nothing runs
    int chunk;                                   // > 0: BgOpHead::chunk of every uploaded op
    int margin_ticks;                            // >= 0: BgQueue::margin_ticks
};
// fg: the frame's decode stream and the main workspaces
int launch_prefix_any(umgen_engine* e, const Place& fg, const FrameIO& io, const std::vector<int>& ego, const BgPassDebug* dbg = nullptr);
void gemv_any(umgen_engine* e, const Place& pl, const float* x, long ldx, const float* ln_w, const void* W, const float* bias, int N, int K, int M, int mode, float* out,
              long ldo);
int build_tables_any(umgen_engine* e, const Place& pl);

// ---- engine_decode.hip ----------------------------------------------------------------------------------------------
// The path that takes a decode step of B scenes (umgen_dbg_oar_step's numbering)
enum DecodePath { PATH_LAUNCHES = 0, PATH_ENGINE = 1, PATH_BATCHED = 2, PATH_WIDE = 3 };   // five launches per layer, XCD-resident engine, batched layer, chip-wide engine
DecodePath decode_path(const umgen_engine* e, int B, hipStream_t st, bool lane);
DecView lane_view(const umgen_engine* e, const umgen_engine::DecLane& ln, int b0);
int enqueue_step_any(umgen_engine* e, const DecView& v, int B, int mod, int ns, const umgen_trace* tr, int j);
int launch_bg_drain(umgen_engine* e, hipStream_t st);   // the launch without an engine part that runs what is left of the background workers' op list

// ---- engine_frame.hip -----------------------------------------------------------------------------------------------
int run_frame_any(umgen_engine* e, const FrameIO& io);
// umgen_rollout_fan's first frame: io.B = B * N branches as scenes (branch (b, s) at b*N + s, scene b's window replicated), io.T >= 2, slot caches allocated
int run_frame_fan_any(umgen_engine* e, const FrameIO& io, int N);
// ---- engine_score.hip -----------------------------------------------------------------------------------------------
int run_score_any(umgen_engine* e, const ScoreIO& sc);
int run_score_candidates_any(umgen_engine* e, ScoreCandIO& sc);
int run_score_clip_any(umgen_engine* e, ScoreClipIO& sc);
int run_score_futures_any(umgen_engine* e, const ScoreFutIO& sc);

}  // namespace umgen
