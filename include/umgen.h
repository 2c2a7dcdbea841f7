/*
 * umgen.h -- C ABI of libumgen_hip.so, the MI355X (gfx950) next-scene rollout engine for UMGen.
 *
 * This is the drop-in boundary for ONE hot path of the reference (YanhaoWu/UMGen):
 *     UMGen.inference(...)                       projects/models/UMGen.py:1542-1671
 * reached through the model registry             projects/registry.py:1-3, UMGen.py:51-52
 * from                                           projects/tools/model_pl.py:173-175, 237-239.
 * The reference has no FFI of its own (it is pure PyTorch); a maintainer binds these entry points
 * with ctypes from a `UMGen(nn.Module)` shim -- see INTEGRATION.md and umgen_amd/model.py.
 *
 * Conventions: plain C, no exceptions across the boundary.  Every function returns 0 on success
 * or a negative UMGEN_E_* code; umgen_last_error() gives the message.  All pointer arguments are
 * HOST pointers to contiguous arrays owned by the caller (the library copies); a handle owns one
 * HIP stream and is not thread-safe.  Token arrays are int64 like the reference's LongTensors.
 */
#ifndef UMGEN_H_
#define UMGEN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UMGEN_ABI_VERSION 4   /* 2: umgen_rollout takes given_map / given_bbox3d; umgen_timings::decode_batched.  3: umgen_timings::prefix_passes; decode_engine values 1 / 3 (2 retired).
                               * 4: umgen_trace::given_map / given_bbox3d (umgen_frame with a given-token prefix: traced logits behind a prefix pass) */

enum {
    UMGEN_OK = 0,
    UMGEN_E_INVALID = -1,   /* bad argument / shape / key          */
    UMGEN_E_STATE = -2,     /* call order (e.g. rollout before finalize) */
    UMGEN_E_HIP = -3,       /* HIP runtime error                   */
    UMGEN_E_NOMEM = -4,
    UMGEN_E_UNSUPPORTED = -5
};

/* FP32: exact-fp32 parity mode.  BF16: bf16 weights / operands / KV cache (the bench mode, BASELINE.json configs[1]).
 * FP16: the same kernels with IEEE-half operands -- the reference's own arithmetic (torch.cuda.amp.autocast fp16, UMGen.py:1604-1605);
 *       umgen_load_tensor refuses (UMGEN_E_INVALID) a matrix weight whose magnitude exceeds 65504 instead of storing inf */
enum { UMGEN_PREC_FP32 = 0, UMGEN_PREC_BF16 = 1, UMGEN_PREC_FP16 = 2 };
enum { UMGEN_DT_F32 = 0, UMGEN_DT_BF16 = 1, UMGEN_DT_F16 = 2, UMGEN_DT_F64 = 3 };
enum { UMGEN_SAMPLE_TOPK = 0, UMGEN_SAMPLE_TOPP = 1 };

/* scene-sequence constants (infer_fun.py:112-118): content tokens per frame */
#define UMGEN_S_POSE 3
#define UMGEN_S_MAP 1024
#define UMGEN_S_BBOX3D 660
#define UMGEN_S_IMAGE 512
#define UMGEN_SEQ_LEN 2207

typedef struct umgen_engine umgen_engine; /* opaque */

/* Mirrors the resolved `config` Namespace read in UMGen.__init__ (UMGen.py:53-172). */
typedef struct umgen_config {
    int32_t abi_version; /* = UMGEN_ABI_VERSION */
    int32_t n_embd, n_head;
    int32_t n_ego_tar_layer, n_ego_ca_layer, n_map_tar_layer, n_box_tar_layer, n_tar_layer, n_oar_layer;
    int32_t pose_vocab, map_vocab, bbox3d_vocab, img_vocab, aux_vocab;
    int32_t n_map_embd, n_img_embd;
    int32_t max_frame_len; /* rows of tpe */
    int32_t task_num, task_id;
    int32_t precision;       /* UMGEN_PREC_* */
    int32_t max_batch;       /* scenes rolled out together on this GPU */
    int32_t max_cond_frames; /* history window T (reference: 20) */
    int32_t device;          /* HIP device ordinal */
    int32_t use_graphs;      /* 1 = replay the decode step from a hipGraph */
} umgen_config;

/* Sampler parameters (UMGen.py:99-126; infer_task_config, config.py:442-463). */
typedef struct umgen_sampling {
    int32_t method;                     /* UMGEN_SAMPLE_* */
    int32_t top_k, top_k_map, topk_image;
    float p, p_map, temperature;
    int32_t rule_constrain;             /* evaluate.py:59-63, UMGen.py:1116-1123 */
    int32_t merge_ar_tar, only_ar;      /* UMGen.py:1092-1104 */
    const uint64_t *seeds;              /* [B] per-scene RNG seed (counter-based) */
} umgen_sampling;

/* Optional per-frame trace of one scene (teacher-forced logit parity; replaces SURVEY's umgen_step_logits).
 * Any pointer may be NULL.  Sizes use the engine's n_embd / vocab sizes. */
typedef struct umgen_trace {
    float *cond;            /* [2207][n_embd]  conditioning rows fed to the OAR (UMGen.py:1227-1231) */
    float *ego_logits;      /* [3][pose_vocab]                                  (UMGen.py:1001-1002) */
    float *logits_map;      /* [1024][map_vocab]                                 (UMGen.py:1062)      */
    float *logits_bbox3d;   /* [660][bbox3d_vocab]                               (UMGen.py:1072)      */
    float *logits_image;    /* [512][img_vocab]                                  (UMGen.py:1132)      */
    const int64_t *forced_pose, *forced_map, *forced_bbox3d, *forced_image; /* teacher forcing, [S_mod] */
    int32_t *counters;      /* [8] events of the frame: 0 pad-avoid resamples, 1 control resamples, 2 rule checks,
                               3 rule collisions, 4 slots blanked, 5 sampled != forced token (teacher forcing only) */
    const int64_t *given_map, *given_bbox3d; /* NULL, or the frame's GIVEN map [1024] (and boxes [660], only behind a given map): umgen_rollout's
                               given_* for one frame (UMGen.py:1184-1201), so that the logits behind a given-token prefix can be traced */
} umgen_trace;

/* Event-timed phases of the last umgen_rollout call (milliseconds, HIP events on the engine stream). */
typedef struct umgen_timings {
    double total_ms, ego_ms, tar_ms, oar_ms;   /* foreground stream: ego net, TAR stacks (or their last slot), decode loop */
    int64_t frames, oar_steps, oar_kernels;
    double gemm_ms;         /* sum over launches of the TAR/ego GEMM kernel (when profiling enabled) */
    int64_t gemm_launches;
    double gemm_flops;      /* algorithmic FLOPs of those launches */
    double oar_bytes;       /* algorithmic HBM bytes of the decode steps */
    double attn_ms;         /* sum over launches of the spatial attention kernel (when profiling enabled) */
    int64_t attn_launches;
    double attn_flops;
    double bg_ms;           // busy time of the background stream (next frame's history slots run beside the decode loop)
    int64_t overlapped_frames; /* frames whose TAR stacks only had to compute their last history slot */
    double layers_ms;       /* sum over launches of the decode step's layer kernel(s): the decode engine's one launch per step, or the
                             * 5 x n_oar_layer launches of the five-launch form (when profiling enabled; HIP events on the decode stream) */
    int64_t layers_launches; /* decode steps timed that way */
    int32_t decode_engine;  /* which persistent decode engine ran the last frame's decode steps: 0 none (five launches per layer, or the batched layer:
                             * see decode_batched), 1 the XCD-resident engine (csrc/oar_engine.hip; n_embd 768, up to 23 scenes), 3 the chip-wide engine
                             * of the 2x-width layers (csrc/oar_engine_wide.hip; n_embd 1536).  2 was round 5's multi-scene engine: measured behind the
                             * other paths and removed in round 6 -- the value is not reused */
    int32_t engine_fallback; /* 1 when this configuration would use the decode engine (16-bit mode, n_embd 768) but its census failed at
                              * umgen_create: the five-launch decode layer runs instead (a warning is printed at create) */
    int32_t decode_batched; /* 1 when the last frame's decode steps ran on the batched decode layer (24 and more scenes per call: the scenes
                              * as the matrix-core instruction's columns, csrc/decode_batched.hip) */
    int32_t decode_lanes;   /* ... and on how many decode lanes (sub-batches on their own streams, forked behind the TAR stacks and joined at the
                              * end of the frame; 0 when the batched layer did not run) */
    int64_t prefix_passes;  /* frames whose GIVEN map / bbox3d positions went through the BlockOAR layers as one forward pass (UMGen.py:1184-1201)
                             * instead of one decode step per position */
} umgen_timings;

/* UMGen(config)  -- UMGen.py:53 */
int umgen_create(const umgen_config *cfg, umgen_engine **out);

/* model.load_state_dict(ckpt["module"], strict=False) -- infer_fun.py:43-50.  One call per state-dict entry;
 * unknown keys are ignored (returns 1), known keys are shape-checked and repacked to the kernel layouts. */
int umgen_load_tensor(umgen_engine *e, const char *key, const void *data, int32_t dtype,
                      const int64_t *shape, int32_t ndim);

/* Builds derived tables (GMLP(codebook) rows, sinusoid tables if not loaded) and checks that every
 * tensor the rollout reads has been loaded.  Corresponds to model.eval() readiness. */
int umgen_finalize_weights(umgen_engine *e);

/* UMGen.inference(new_frames, cond_frames, input_cond_frames=T_in, input_cond_tokens, init_tokens, control_test)
 * for B independent scenes (the reference is B = 1; scenes never interact).
 *   pose/map/bbox3d/image : [B][T_in][S_mod] int64 history tokens (first T_in frames are used)
 *   ctrl_pose/ctrl_bbox3d : NULL, or [B][T_ctl][3] / [B][T_ctl][660] control tokens (init_tokens; -1 = free).  Either may be given
 *                           alone: pose only (ego controlled), bbox3d only with control_test (agents controlled, the ego net
 *                           infers the pose; UMGen.py:1438-1473), or both (the reference's control pickles)
 *   given_map / given_bbox3d : NULL, or [B][T_ctl][1024] / [B][T_ctl][660] tokens of the new frames that are GIVEN, not generated
 *                           (init_tokens["map"], init_tokens["bbox3d"] without control_test: infer_oar_net's predefined-token prefix,
 *                           UMGen.py:1184-1201 -- "use the predefined tokens and don't infer these tokens any more").  They must continue
 *                           the pose prefix in scene order: the map, or the map and the boxes (the reference concatenates whatever is
 *                           given back to back, so boxes without the map would sit on the map's positions: refused).  The given
 *                           positions go through the BlockOAR layers as ONE forward pass like the reference's first iteration (no head, no
 *                           sampler; engines created with the overlapped background pass, UMGEN_OVERLAP=1, replay them as decode steps instead
 *                           -- a property of the engine, the same for every frame), sampling starts behind them; the given tokens are
 *                           returned verbatim (UMGen.py:1640-1651).  given_bbox3d and control_test exclude each other.
 *   out_*                 : [B][T_in + new_frames][S_mod], caller-allocated
 */
int umgen_rollout(umgen_engine *e, int32_t B, int32_t T_in, int32_t new_frames, int32_t cond_frames,
                  const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image,
                  int32_t T_ctl, const int64_t *ctrl_pose, const int64_t *ctrl_bbox3d, int32_t control_test,
                  const int64_t *given_map, const int64_t *given_bbox3d,
                  const umgen_sampling *sampling,
                  int64_t *out_pose, int64_t *out_map, int64_t *out_bbox3d, int64_t *out_image);

/* One frame of one scene (UMGen._inference, UMGen.py:1406-1540) with optional trace / teacher forcing.
 * Window tokens are [T][S_mod]; ctrl_* are NULL or the [S_mod] control tokens of this frame.
 * out_* receive the new frame's tokens [S_mod]. */
int umgen_frame(umgen_engine *e, int32_t T, const int64_t *pose, const int64_t *map, const int64_t *bbox3d,
                const int64_t *image, const int64_t *ctrl_pose, const int64_t *ctrl_bbox3d, int32_t control_test,
                const umgen_sampling *sampling, int32_t frame_idx, const umgen_trace *trace,
                int64_t *out_pose, int64_t *out_map, int64_t *out_bbox3d, int64_t *out_image);

/* ---- log-likelihoods of GENERATED frames: the counterpart of umgen_score on the generating side --------------------------------------
 * umgen_rollout / umgen_frame with one more argument; lp == NULL or all-NULL members behave exactly like those (which are calls of these
 * with lp = NULL), and the tokens are the same bits either way.  For every content token of every NEW frame a float32 natural-log value in
 * umgen_score's measure -- the plain AR heads head_ar_map / head_ar_bbox3d / head_ar_img (head_ego for the pose) at temperature 1 over the
 * whole vocabulary, not the sampler's truncated / tempered distribution, and never head_tar_bbox3d:
 *     logp[k] = (row[t] - max row) - log sum exp(row - max row)
 * with `row` the fp32 logit row the sampler of that decode step read (fixed summation order: the bits depend on the row and the token only,
 * not on B) and t
 *   - the token the step settled on BEFORE the rule constraint: the main draw, or the control / pad-avoid resample where the step took one
 *     (drawn from the TAR head, scored under the AR row like everything else);
 *   - under teacher forcing (umgen_trace::forced_*) the forced token: a forced frame is a step-by-step umgen_score;
 *   - for the pose, the ego sampler's token on its head_ego row.
 * NaN where no head was evaluated: the pose when ctrl_pose is given, every given map / bbox3d position (one-pass prefix or replayed steps).
 * bos / eos carry nothing; history frames are not part of the output.
 * Rule constraint: a slot the constraint blanks returns pad tokens, but its 11 entries keep the log-probabilities of the tokens that were
 * DRAWN -- those are what the KV cache holds, what every later step of the frame was conditioned on, and the density of the sampled path.
 * Consequence: these values and umgen_score of the RETURNED frame agree only for frames without a blanked slot (scoring conditions on the
 * pads).  Without a blanked slot they agree the way the decode steps agree with the one-pass arithmetic (see umgen_score below). */
typedef struct umgen_logp_out {
    float *logp_pose, *logp_map, *logp_bbox3d, *logp_image; /* rollout: [B][new_frames][S_mod]; frame: [S_mod]; any may be NULL */
} umgen_logp_out;
int umgen_rollout_logp(umgen_engine *e, int32_t B, int32_t T_in, int32_t new_frames, int32_t cond_frames,
                       const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image,
                       int32_t T_ctl, const int64_t *ctrl_pose, const int64_t *ctrl_bbox3d, int32_t control_test,
                       const int64_t *given_map, const int64_t *given_bbox3d,
                       const umgen_sampling *sampling,
                       int64_t *out_pose, int64_t *out_map, int64_t *out_bbox3d, int64_t *out_image, const umgen_logp_out *lp);
int umgen_frame_logp(umgen_engine *e, int32_t T, const int64_t *pose, const int64_t *map, const int64_t *bbox3d,
                     const int64_t *image, const int64_t *ctrl_pose, const int64_t *ctrl_bbox3d, int32_t control_test,
                     const umgen_sampling *sampling, int32_t frame_idx, const umgen_trace *trace,
                     int64_t *out_pose, int64_t *out_map, int64_t *out_bbox3d, int64_t *out_image, const umgen_logp_out *lp);

/* ---- fan-out rollout: N sampled futures of every scene off one pass over its history --------------------------------------------------
 * Contract: branch (b, s) of every output is bit for bit what umgen_rollout_logp returns for scene b*N + s on the same engine when it is called with
 * B*N scenes, history b replicated N times, the control / given arrays replicated likewise, and the same seeds[b*N + s] -- in every precision, tokens
 * and log-likelihoods.  (The sampler's RNG is a function of seed, frame, position and draw kind; the scene index does not enter.)
 *   - pose/map/bbox3d/image [B][T_in][S_mod]; ctrl_* / given_* NULL or [B][T_ctl][S_mod]: a scene's branches share them; sampling->seeds [B*N] (NULL: 0),
 *     branch (b, s) at b*N + s; out_* [B][N][T_in + new_frames][S_mod]; lp NULL or arrays [B][N][new_frames][S_mod].
 *   - B >= 1, N >= 1, B*N <= max_batch; everything else is checked like umgen_rollout's arguments.  N == 1 is umgen_rollout_logp itself.
 *     Every argument is checked once, on the arrays as the caller passed them: an error message that names a token "at flat index i" indexes the caller's
 *     [B][T_in][S_mod] (or [B][T_ctl][S_mod]) array, for every N.
 *   - What is saved: in the FIRST frame, with n0 = min(T_in, cond_frames) window slots, the ego net and slots 0 .. n0-2 of the map / box / TAR stacks run
 *     once per scene, and only slot n0-1 -- the one the pose shift hands the branch's own new pose -- runs per branch, against the scene's slot caches.
 *     When the window then grows (n0 + 1 <= cond_frames) every branch's slot caches are completed from its scene's, so later frames push one slot per
 *     branch as in umgen_rollout.  From the decode loop of the first frame on, the call is umgen_rollout_logp on B*N scenes.
 *   - *shared_slots (NULL allowed): n0 - 1 when the first frame ran that way; 0 when the call took the replicated path with the same bits: N == 1, n0 == 1,
 *     slot caches that do not fit, UMGEN_FAN_SHARE=0 in the environment (read per call), or new_frames == 0. */
int umgen_rollout_fan(umgen_engine *e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames,
                      const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image,
                      int32_t T_ctl, const int64_t *ctrl_pose, const int64_t *ctrl_bbox3d, int32_t control_test,
                      const int64_t *given_map, const int64_t *given_bbox3d,
                      const umgen_sampling *sampling,
                      int64_t *out_pose, int64_t *out_map, int64_t *out_bbox3d, int64_t *out_image,
                      const umgen_logp_out *lp, int32_t *shared_slots);

/* Per-token log-likelihoods of a GIVEN next frame: the reference's teacher-forced loss terms (get_targets, d_loss, F.cross_entropy per modality,
 * UMGen.py:539-582) as one forward pass.  For B scenes with history windows pose/map/bbox3d/image [B][T][S_mod] and their next frames next_* [B][S_mod]:
 *     logp_m[b][k]   = log_softmax(logits_m[k])[next_m[b][k]]   (natural log)
 *     argmax_m[b][k] = the most likely token at that position (lowest index among equal maxima)
 * where logits_m are the rows umgen_frame traces for the same window with forced_* = next_* (pose: its ego_logits): the plain AR heads head_ar_map /
 * head_ar_bbox3d / head_ar_img and head_ego at temperature 1 -- not the sampler's distribution (no top-k / top-p, no resampling through head_tar_bbox3d, no
 * rule constraint).  bos / eos positions carry no score; no RNG is involved.  All 2206 positions go through the BlockOAR layers as ONE pass with the
 * arithmetic of the given-token prefix pass (umgen_rollout's given_*), not as 2206 decode steps: fp32 engines agree with the traced logits up to summation
 * order, 16-bit engines the way the one-pass prefix agrees with its step-by-step replay.  B <= max_batch, T <= max_cond_frames; tokens are range-checked
 * like umgen_rollout's.  Any pointer of `out` may be NULL. */
typedef struct umgen_score_out {
    float *logp_pose, *logp_map, *logp_bbox3d, *logp_image;           /* [B][3], [B][1024], [B][660], [B][512] */
    int32_t *argmax_pose, *argmax_map, *argmax_bbox3d, *argmax_image; /* the same shapes */
} umgen_score_out;
int umgen_score(umgen_engine *e, int32_t B, int32_t T, const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image,
                const int64_t *next_pose, const int64_t *next_map, const int64_t *next_bbox3d, const int64_t *next_image, umgen_score_out *out);

/* Score diagnostics: what else the distribution behind every logp said.  umgen_score's arguments and rows; per content position, with v the fp32
 * logit row, t = v[target] and lse as umgen_score forms them:
 *     rank        number of n with v[n] > t, strictly (ties are not counted, like the sampler's "ties kept" threshold): rank < top_k means inside
 *                 the top-k support, rank == 0 that the target's logit is the row maximum
 *     mass_above  sum over v[n] > t of softmax(v / temperature)[n]; mass_above <= p is the reference's nucleus rule for "kept"
 *                 ((cumsum - p_sorted) > p removes, UMGen.py:944-953).  The only output that depends on `temperature` (> 0, finite)
 *     entropy     -sum p log p of softmax(v) in nats, at temperature 1
 *     topk_tok    the `topk` (0 .. UMGEN_SCORE_TOPK_MAX) most likely tokens in descending order of logit, equal logits by ascending index;
 *     topk_logp   v[topk_tok[i]] - lse, the bits of logp where the target is listed; -1 / -inf past a vocabulary smaller than topk.  topk_tok[0] is argmax
 * `out` may be NULL; when given it is filled exactly as umgen_score fills it.  Any pointer of `detail` may be NULL (top-K pointers with topk == 0
 * are refused).  The call costs one more sweep of the heads behind umgen_score's; its device buffers are allocated by the first call (UMGEN_E_NOMEM). */
#define UMGEN_SCORE_TOPK_MAX 16
typedef struct umgen_score_detail_out {
    int32_t *rank_pose, *rank_map, *rank_bbox3d, *rank_image;                                 /* [B][S_mod] */
    float *mass_above_pose, *mass_above_map, *mass_above_bbox3d, *mass_above_image;
    float *entropy_pose, *entropy_map, *entropy_bbox3d, *entropy_image;
    int32_t *topk_tok_pose, *topk_tok_map, *topk_tok_bbox3d, *topk_tok_image;                 /* [B][S_mod][topk] */
    float *topk_logp_pose, *topk_logp_map, *topk_logp_bbox3d, *topk_logp_image;
} umgen_score_detail_out;
int umgen_score_detail(umgen_engine *e, int32_t B, int32_t T, const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image,
                       const int64_t *next_pose, const int64_t *next_map, const int64_t *next_bbox3d, const int64_t *next_image, int32_t topk,
                       float temperature, umgen_score_out *out, umgen_score_detail_out *detail);

/* ---- rollout diagnostics: umgen_score_detail's quantities for every GENERATED token, from the decode step that sampled it ------------------
 * umgen_rollout_detail is umgen_rollout_fan, umgen_frame_detail is umgen_frame_logp, plus `topk` and `detail`; with detail == NULL or all its
 * pointers NULL they are exactly those calls (which are these with detail = NULL), and tokens and lp are the same bits whether or not detail is
 * asked.  N == 1 is the plain rollout.  Per content token of every NEW frame, with v the fp32 logit row [0, vocab) the sampler of that decode
 * step read -- the plain AR head's row (head_ego for the pose), never head_tar_bbox3d -- m its maximum, S = sum exp(v - m), and t = v[tok] for
 * the token umgen_rollout_logp scores (the token the step settled on BEFORE the rule constraint; the forced token under teacher forcing):
 *     rank        number of n with v[n] > t, strictly.  For a token of the main draw rank < top_k (top-k sampler) holds exactly: it is the row the
 *                 sampler drew from.  A token resampled from the TAR head (control / pad-avoid) is ranked on the AR row and may lie outside
 *     mass_above  A / Z, A = sum over v[n] > t of exp((v[n] - m) / tau), Z = the same sum over all n, tau = sampling->temperature (finite)
 *     entropy     log S - U / S, U = sum exp(v - m)(v - m): the entropy of softmax(v) in nats at temperature 1
 *     topk_tok    the `topk` (0 .. UMGEN_SCORE_TOPK_MAX) largest logits' tokens, descending, equal logits by ascending index
 *     topk_logp   (v[topk_tok[i]] - m) - log S, formed like lp's value: where the scored token is listed its entry has the bits of lp's.
 *                 -1 / -inf past a vocabulary smaller than topk
 * Every sum runs in lp's fixed order, so a position's outputs are a function of (row, vocab, topk, tau, token) alone: not of B, the scene's place
 * in the batch or the decode path.  Where no head ran -- exactly where lp is NaN: the pose under ctrl_pose, every given map / bbox3d position --
 * rank and topk_tok are -1 and the floats NaN.  Rule constraint: like lp, a blanked slot returns pad tokens and keeps the diagnostics of the
 * tokens that were DRAWN; scoring the returned frame with umgen_score_detail conditions on the pads and is a different quantity there.
 * Shapes: rollout [B][N][new_frames][S_mod] (lists [..][S_mod][topk]), frame [S_mod] (lists [S_mod][topk]).  Any pointer may be NULL; top-K
 * pointers with topk == 0, topk outside [0, UMGEN_SCORE_TOPK_MAX] and a non-finite temperature are refused (UMGEN_E_INVALID) when detail is asked.
 * Cost: no extra pass over the model and no extra launch; the sampler kernel of a step sweeps its row twice more and runs topk arg-max rounds. */
typedef struct umgen_gen_detail_out {
    int32_t *rank_pose, *rank_map, *rank_bbox3d, *rank_image;
    float *mass_above_pose, *mass_above_map, *mass_above_bbox3d, *mass_above_image;
    float *entropy_pose, *entropy_map, *entropy_bbox3d, *entropy_image;
    int32_t *topk_tok_pose, *topk_tok_map, *topk_tok_bbox3d, *topk_tok_image;
    float *topk_logp_pose, *topk_logp_map, *topk_logp_bbox3d, *topk_logp_image;
} umgen_gen_detail_out;
int umgen_rollout_detail(umgen_engine *e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames,
                         const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image,
                         int32_t T_ctl, const int64_t *ctrl_pose, const int64_t *ctrl_bbox3d, int32_t control_test,
                         const int64_t *given_map, const int64_t *given_bbox3d,
                         const umgen_sampling *sampling,
                         int64_t *out_pose, int64_t *out_map, int64_t *out_bbox3d, int64_t *out_image,
                         const umgen_logp_out *lp, int32_t *shared_slots, int32_t topk, const umgen_gen_detail_out *detail);
int umgen_frame_detail(umgen_engine *e, int32_t T, const int64_t *pose, const int64_t *map, const int64_t *bbox3d,
                       const int64_t *image, const int64_t *ctrl_pose, const int64_t *ctrl_bbox3d, int32_t control_test,
                       const umgen_sampling *sampling, int32_t frame_idx, const umgen_trace *trace,
                       int64_t *out_pose, int64_t *out_map, int64_t *out_bbox3d, int64_t *out_image, const umgen_logp_out *lp,
                       int32_t topk, const umgen_gen_detail_out *detail);

/* ---- constrained sampling: per-class logit bias and token bans inside the samplers of every decode step -----------------------------------
 * umgen_rollout_biased is umgen_rollout_detail, umgen_frame_biased is umgen_frame_detail, plus `bias` and `lz`; with bias NULL or all its tables
 * NULL, and lz NULL, they are exactly those calls (which are these with bias = lz = NULL): no existing call changes its bits.
 * A bias table belongs to a token class (host float32; entries finite, or -inf = a ban):
 *     pose    [3][pose_vocab]       row of component jq
 *     map     [map_vocab]           the one row
 *     bbox3d  [11][bbox3d_vocab]    row of attribute a = k % 11, k the position in the 660; a == 10 is the category token
 *     image   [img_vocab]           the one row
 * Wherever a sampler would read a logit row v of such a position -- the AR head's row (head_ego's for the pose), or the head_tar_bbox3d row of a
 * control or pad-avoid resample -- it reads w[n] = v[n] + r[n] instead: one fp32 add, round to nearest, -inf where r[n] is -inf; r the class row
 * of the position.  Everything else is unchanged and runs on w: the top-k threshold with ties kept, temperature, the nucleus, the control
 * resample's masked index vocab - 1, the RNG draw kinds, the pad-avoid trigger, the rule constraint, teacher forcing.  A biased call returns, bit
 * for bit, what the unbiased samplers return on the rows w.  Consequences:
 *   - Bans hold for draws: a banned token is never the result of a draw, for any uniform (an inverse-CDF walk that finds no prefix sum above its
 *     target ends on its last ALLOWED entry).
 *   - Bans do not hold for non-draws: the rule constraint blanks a slot to pad whatever the tables say; forced, controlled and given tokens are
 *     written as given.
 *   - lp (umgen_logp_out) and the diagnostics (umgen_gen_detail_out) stay in the model's measure: computed on v, never on w, for the token the step
 *     settled on.  lp is finite for every drawn token (r > -inf there and v is finite).  rank < top_k for a token of the main draw is guaranteed
 *     only WITHOUT a bias on its class: under a bias the top-k support is that of w.
 *   - logz (umgen_logz_out, float32, the shapes of umgen_logp_out): per sampled position logz = lse(w) - lse(v) over [0, vocab) of the AR row -- the
 *     log of sum_n softmax(v)[n] exp(r[n]); for a table of bans the log of the model's mass on the allowed set, <= 0.  Each lse is max + log sum
 *     exp(row - max) in lp's fixed order, so the bits are a function of (row, class row, vocab) alone; an all-zero table gives exactly +0.0.  +0.0 at
 *     sampled positions of a class without a table; NaN exactly where lp is NaN; for a TAR-resampled token still the AR row's value, like lp.
 *     What it is for: under an UNTRUNCATED sampler at temperature 1 (top-k >= vocab / nucleus keeping everything) the proposal's log-density of a
 *     drawn token is lp + r[tok] - logz, so logz - r[tok], summed over a frame, is the log importance weight of a constrained sample against the
 *     model.  The renormalisation of a truncated sampler and the composite density of the resample flow are not part of it.
 *   - Refused with UMGEN_E_INVALID before anything reaches the device, the message naming class, row and index: a NaN or +inf entry; a row without an
 *     allowed entry; a bbox3d row whose only allowed entry is vocab - 1 when the call has control slots (control_test with ctrl_bbox3d: the control
 *     resample masks that index); a table of a class whose vocabulary exceeds 8192.
 *   - One set of tables per call: scenes, fan-out branches and frames share it (umgen_rollout_planned below lifts this).  lz without a bias is
 *     allowed (+0.0 / NaN).
 * The scoring entry points take no bias: they describe the model, not a sampler. */
typedef struct umgen_logit_bias { const float *pose, *map, *bbox3d, *image; } umgen_logit_bias;   /* host; any may be NULL = no bias for that class */
typedef struct umgen_logz_out   { float *logz_pose, *logz_map, *logz_bbox3d, *logz_image; } umgen_logz_out; /* shapes of umgen_logp_out */
int umgen_rollout_biased(umgen_engine *e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames,
                         const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image,
                         int32_t T_ctl, const int64_t *ctrl_pose, const int64_t *ctrl_bbox3d, int32_t control_test,
                         const int64_t *given_map, const int64_t *given_bbox3d,
                         const umgen_sampling *sampling,
                         int64_t *out_pose, int64_t *out_map, int64_t *out_bbox3d, int64_t *out_image,
                         const umgen_logp_out *lp, int32_t *shared_slots, int32_t topk, const umgen_gen_detail_out *detail,
                         const umgen_logit_bias *bias, const umgen_logz_out *lz);
int umgen_frame_biased(umgen_engine *e, int32_t T, const int64_t *pose, const int64_t *map, const int64_t *bbox3d,
                       const int64_t *image, const int64_t *ctrl_pose, const int64_t *ctrl_bbox3d, int32_t control_test,
                       const umgen_sampling *sampling, int32_t frame_idx, const umgen_trace *trace,
                       int64_t *out_pose, int64_t *out_map, int64_t *out_bbox3d, int64_t *out_image, const umgen_logp_out *lp,
                       int32_t topk, const umgen_gen_detail_out *detail, const umgen_logit_bias *bias, const umgen_logz_out *lz);

/* ---- sampling plans: per-scene sampler settings, per-scene and per-frame table sets --------------------------------------------------------
 * umgen_rollout_planned is umgen_rollout_biased with a plan in the place of `bias`: every scene / fan-out branch i = b*N + s of the call may draw
 * under its own sampler settings, per_scene[i], and, in every NEW frame f, under its own set of logit-bias tables, bias_sets[bias_of[i][f]] (-1 = no
 * bias).  umgen_rollout_biased is this call with per_scene = NULL and, when it has a `bias`, one set with bias_of = NULL; plan = NULL is the unbiased
 * call.  There is no umgen_frame_planned: a frame call is one scene and one frame, so its caller has already resolved the plan.
 * Contract.  Take a planned call on B*N scenes.  The tokens, lp, lz and diagnostics of scene i in new frame f are, bit for bit, what scene i of
 * umgen_rollout_biased returns when that call has the same B, N, arrays and seeds, sampling = per_scene[i] (the call's `sampling` when per_scene is
 * NULL), bias = bias_sets[bias_of[i][f]] (no bias for -1), and a history up to frame f that is the same bits.  In particular:
 *   - a plan whose per_scene entries all equal `sampling`, and whose bias_of is constant, returns the bytes of the unplanned call;
 *   - the plan does not enter the RNG: draws stay a function of (seed, frame, position, draw kind); the `seeds` members of per_scene are ignored,
 *     the seeds are `sampling`'s;
 *   - mass_above of the diagnostics is taken at the scene's own temperature;
 *   - lp and the diagnostics stay on the model's row v; logz is formed against the scene's own table;
 *   - a class without a table in a scene's set is not biased and its logz is +0.0: the "class without a table" path, not a table of zeros.
 * rule_constrain, merge_ar_tar and only_ar stay PER CALL: the host decides per call whether head_tar_bbox3d runs, so every per_scene entry must
 * carry the values of `sampling`.
 * Refused with UMGEN_E_INVALID before anything reaches the device, the message naming scene, frame, set, class, row and index as applicable:
 *   - a per_scene[i] that the call would refuse as its `sampling`, or whose rule_constrain / merge_ar_tar / only_ar differ from `sampling`'s;
 *   - n_bias_sets outside [0, UMGEN_BIAS_SETS_MAX], or bias_of given with n_bias_sets == 0; a bias_of entry outside [-1, n_bias_sets);
 *   - in ANY set, used by a scene or not, a table that umgen_rollout_biased refuses; the "bbox3d row that allows only vocab - 1 under control slots"
 *     rule applies to every set that some scene uses.
 * A set whose tables are all NULL is an empty set: its scenes are unbiased. */
#define UMGEN_BIAS_SETS_MAX 16
typedef struct umgen_sample_plan {
    const umgen_sampling   *per_scene;   /* NULL, or [B*N]: the sampler settings of scene / branch b*N + s; their `seeds` members are ignored */
    int32_t                 n_bias_sets; /* 0 .. UMGEN_BIAS_SETS_MAX */
    const umgen_logit_bias *bias_sets;   /* [n_bias_sets]; every set is what umgen_rollout_biased takes as `bias` */
    const int32_t          *bias_of;     /* NULL (every scene and frame uses set 0 when n_bias_sets >= 1), or [B*N][new_frames]: the set of scene i
                                            in NEW frame f, -1 = unbiased */
} umgen_sample_plan;
int umgen_rollout_planned(umgen_engine *e, int32_t B, int32_t N, int32_t T_in, int32_t new_frames, int32_t cond_frames,
                          const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image,
                          int32_t T_ctl, const int64_t *ctrl_pose, const int64_t *ctrl_bbox3d, int32_t control_test,
                          const int64_t *given_map, const int64_t *given_bbox3d,
                          const umgen_sampling *sampling,
                          int64_t *out_pose, int64_t *out_map, int64_t *out_bbox3d, int64_t *out_image,
                          const umgen_logp_out *lp, int32_t *shared_slots, int32_t topk, const umgen_gen_detail_out *detail,
                          const umgen_sample_plan *plan, const umgen_logz_out *lz);

/* Ranking futures: C given next frames per scene against ONE history.  Entry (b, c) of every output is bit for bit what
 *     umgen_score(e, 1, T, window b, candidate (b, c))
 * returns on the same engine, in every precision, whichever path ran and however the B * C items were chunked.  Only the last history slot of the map /
 * bbox3d / TAR stacks sees a candidate (the pose shift hands slot T - 1 the candidate's pose), so for T >= 2 the ego net and slots 0 .. T - 2 are
 * evaluated once per scene and the items, in chunks of at most max_batch, run their last slot against the scene's slot caches, then the BlockOAR pass and
 * the heads: one history pass plus B * C small passes instead of B * C history passes.  T == 1, slot caches that do not fit in device memory, or
 * UMGEN_SCORE_SHARE=0 in the environment (read per call) evaluate umgen_score's own pass on replicated windows -- the same bits.
 * B <= max_batch, T <= max_cond_frames, C >= 1; B * C may exceed max_batch.  Tokens are range-checked like umgen_score's; `out` must not be NULL, any
 * pointer in it may be.  Like umgen_score, the call leaves nothing an overlapped rollout could reuse in the slot caches. */
int umgen_score_candidates(umgen_engine *e, int32_t B, int32_t T, int32_t C,
                           const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image,                     /* [B][T][S_mod] */
                           const int64_t *next_pose, const int64_t *next_map, const int64_t *next_bbox3d, const int64_t *next_image, /* [B][C][S_mod] */
                           umgen_score_out *out,   /* every array [B][C][S_mod]; any pointer may be NULL */
                           int32_t *shared_slots); /* NULL, or receives T - 1 when the history slots were evaluated once per scene, 0 on the replicated path */

/* Ranking futures of several frames: C candidate futures of K frames per scene against ONE history of T frames.  With seq(b, c) = history[b] ++
 * future[b][c], f = T + k and n_k = min(T + k, cond_frames), entry (b, c, k) of every output is bit for bit what
 *     umgen_score(e, 1, n_k, seq(b, c)[f - n_k : f], seq(b, c)[f])
 * returns on the same engine -- umgen_rollout's window rule with the given frames in place of generated ones -- in every precision, whichever path ran and
 * however the B * C items were chunked.  At frame k the window holds h_k = max(0, n_k - k) history frames; slots 0 .. h_k - 2 of the map / bbox3d / TAR
 * stacks (slot h_k - 1 carries the pose of future frame 0 through the pose shift) and slots 0 .. h_k - 1 of the ego stack are the same for every candidate
 * of a scene, and the causal temporal attention never lets them see one.  They are evaluated once per scene -- and only when the window's first frame
 * moved: while the window grows the slot caches already hold them -- and the items, in chunks of at most max_batch, run their tail of k + 1 slots (ego: k)
 * against the scene's caches, then the ego decoder, the BlockOAR pass and the heads.  A frame with no shared slot (h_k < 2), a tail longer than the tail
 * kernel holds (16 slots; 8 when it needs four heads per workgroup), slot caches that do not fit in device memory, or UMGEN_SCORE_FUTURES_SHARE=0 in the
 * environment (read per call) evaluate umgen_score's own pass on per-item windows -- the same bits; shared_slots[k] is then 0.
 * B <= max_batch, T >= 1, 1 <= cond_frames <= max_cond_frames, C >= 1, K >= 1; B * C may exceed max_batch and T may exceed cond_frames.  Tokens are
 * range-checked like umgen_score's; `out` must not be NULL, any pointer in it may be.  K == 1 with T <= cond_frames gives umgen_score_candidates' bytes.
 * Like umgen_score, the call settles a pending background pass and leaves nothing an overlapped rollout could reuse in the slot caches. */
int umgen_score_futures(umgen_engine *e, int32_t B, int32_t T, int32_t C, int32_t K, int32_t cond_frames,
                        const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image,                 /* [B][T][S_mod]    */
                        const int64_t *fut_pose, const int64_t *fut_map, const int64_t *fut_bbox3d, const int64_t *fut_image, /* [B][C][K][S_mod] */
                        umgen_score_out *out,    /* every array [B][C][K][S_mod]; any pointer may be NULL, out itself not */
                        int32_t *shared_slots);  /* NULL, or [K]: per future frame the history slots evaluated once per scene, 0 = replicated path */

/* Scoring a recorded clip: the teacher-forced counterpart of umgen_rollout.  For B clips of L frames, every frame f with T_in <= f < L is scored against
 * the n_f = min(f, cond_frames) frames before it -- umgen_rollout's window rule (UMGen.py:1597-1603) with the recorded frames in place of generated ones.
 * Entry (b, f - T_in) of every output is bit for bit what
 *     umgen_score(e, 1, n_f, clip[b][f - n_f : f], clip[b][f])
 * returns on the same engine, in every precision, whichever path ran.  While the window still starts at frame 0 (f <= cond_frames) slot t of every such
 * window is the same computation -- the same tokens, tpe[t], the pose of frame t + 1 from the pose shift, frame-local spatial sub-blocks and a causal
 * temporal attention -- so these G = min(L - 1, cond_frames) - T_in + 1 frames are read off ONE pass of the four stacks over frames [0, min(L - 1,
 * cond_frames)) with every block evaluated on every slot, then one BlockOAR pass and one sweep of the heads over the B * G items.  The frames behind them,
 * whose windows slide, are umgen_score's own pass in chunks of at most max_batch items.  G < 2, no device memory for the clip buffers (allocated by the
 * first call), or UMGEN_SCORE_CLIP_SHARE=0 in the environment (read per call) evaluate umgen_score's pass for every frame -- the same bits.
 * 1 <= T_in < L, 1 <= cond_frames <= max_cond_frames, B <= max_batch; L has no upper limit.  Tokens are range-checked like umgen_score's; `out` must not
 * be NULL, any pointer in it may be.  Like umgen_score, the call settles a pending background pass and leaves nothing an overlapped rollout could reuse. */
int umgen_score_clip(umgen_engine *e, int32_t B, int32_t L, int32_t T_in, int32_t cond_frames,
                     const int64_t *pose, const int64_t *map, const int64_t *bbox3d, const int64_t *image, /* [B][L][S_mod] */
                     umgen_score_out *out,      /* every array [B][L - T_in][S_mod]; any pointer may be NULL, out itself not */
                     int32_t *shared_frames);   /* NULL, or receives G when the growing windows shared one pass, 0 when nothing was shared */

int umgen_set_profiling(umgen_engine *e, int32_t enable); /* per-launch HIP-event timing of the GEMM / attention kernels and of the
                                                            * decode step's layer kernel(s); profiled frames launch eagerly */
int umgen_get_timings(umgen_engine *e, umgen_timings *out);

/* ---- scene formats either side of the rollout (host only, no engine needed) ------------------
 * DigitalBinsTokenizer.encode/.decode (tokenizer.py:316-354) + Normalize_Standard (normalize.py:7-76) for the ego motion and
 * Normalize min-max (normalize.py:79-137, 189-229) + the attribute / category tokens of BBox3DTokenizer (tokenizer.py:515-600)
 * for agent boxes.  Arrays are caller-owned; return 0 or UMGEN_E_INVALID. */
int umgen_tokenize_ego(const double *pose_diff /*[n][3] (dx, dy, dheading)*/, int64_t n, int64_t *tokens /*[n][3]*/);
int umgen_detokenize_ego(const int64_t *tokens /*[n][3]*/, int64_t n, float *pose_diff /*[n][3]*/);   /* == UMGen.decode_pose */
int umgen_tokenize_boxes(const float *boxes /*[n][stride], first 10 columns used*/, int64_t n, int32_t stride,
                         const int32_t *category_index /*[n], 0..2*/, int64_t *tokens /*[n][11]*/);
int umgen_detokenize_boxes(const int64_t *slot_tokens /*[n][11]*/, int64_t n, double *boxes /*[n][10]*/);

/* ---- VQ decoders: map / image tokens -> rasters, fp32 ---------------------------------------------
 * NormVQModel.decode_code (projects/tokenizer/vq_model.py:88-103,126-150) = quantize.embedding lookup -> post_quant_conv ->
 * Decoder.forward (projects/tokenizer/vq_modules.py:293-415), as called by Mapdecoder.decode_maps / Imagedecoder.decode_images
 * (projects/tools/decode_map.py:110-183).  The config mirrors the `ddconfig` dicts of vq_model.py:153-202. */
typedef struct umgen_vq umgen_vq; /* opaque */
typedef struct umgen_vq_config {
    int32_t n_embed, embed_dim;        /* codebook: 8192 x 16 */
    int32_t z_channels, ch, out_ch;    /* ddconfig */
    int32_t n_levels;                  /* len(ch_mult) */
    int32_t ch_mult[8];
    int32_t num_res_blocks;
    int32_t n_attn_res;
    int32_t attn_resolutions[4];
    int32_t resolution;                /* ddconfig["resolution"] (only used to place the attention blocks, like the reference) */
    int32_t post_quant_ks, post_quant_pad; /* NormVQModel(stride=..., padding=...): kernel size / padding of post_quant_conv */
    int32_t token_h, token_w;          /* token grid of one frame: 32 x 32 (map), 16 x 32 (image) */
    int32_t device;
} umgen_vq_config;
int umgen_vq_create(const umgen_vq_config *cfg, umgen_vq **out);
/* one call per state-dict entry of the VQ checkpoint (fp32, reference key names: "decoder.conv_in.weight", "post_quant_conv.bias",
 * "quantize.embedding.weight", ...); entries the decode path does not read (encoder.*, quant_conv.*, EMA buffers) return 1 */
int umgen_vq_load_tensor(umgen_vq *d, const char *key, const float *data, const int64_t *shape, int32_t ndim);
int umgen_vq_finalize(umgen_vq *d);
/* codes [n][token_h][token_w] -> out [n][out_ch][token_h * 2^(n_levels-1)][token_w * 2^(n_levels-1)] */
int umgen_vq_decode(umgen_vq *d, int32_t n, const int64_t *codes, float *out);
const char *umgen_vq_last_error(const umgen_vq *d);
int umgen_vq_destroy(umgen_vq *d);

/* ---- VQ encoders: map / image rasters -> tokens, fp32 ---------------------------------------------
 * NormVQModel.encode (projects/tokenizer/vq_model.py:80-85, the call behind NormVQModelTokenizer.encode, vq_tokenizer.py:25-47) =
 * Encoder.forward (projects/tokenizer/vq_modules.py:179-290) -> quant_conv -> the l2norm + nearest-code search of
 * NormEMAVectorQuantizer.forward (projects/tokenizer/quantize.py:414-429).  A handle of its own: a decoder handle does not read encoder.* keys. */
typedef struct umgen_vqenc umgen_vqenc; /* opaque */
/* cfg: the same ddconfig mirror the decoder takes (out_ch, post_quant_* are ignored); in_channels = ddconfig["in_channels"] */
int umgen_vqenc_create(const umgen_vq_config *cfg, int32_t in_channels, umgen_vqenc **out);
/* reference key names: "encoder.conv_in.weight", "encoder.down.1.downsample.conv.bias", "encoder.mid.attn_1.q.weight",
 * "quant_conv.weight", "quantize.embedding.weight", ...; entries the encode path does not read (decoder.*, post_quant_conv.*,
 * cluster_size / embed_avg / initted buffers) return 1; known keys are shape-checked */
int umgen_vqenc_load_tensor(umgen_vqenc *q, const char *key, const float *data, const int64_t *shape, int32_t ndim);
int umgen_vqenc_finalize(umgen_vqenc *q);
/* x [n][in_channels][H][W] fp32 (H = token_h * 2^(n_levels-1), W likewise; finite values, nominally in [-1, 1]) -> codes
 * [n][token_h][token_w];  z: NULL, or [n][token_h][token_w][embed_dim], the l2-normalised rows the nearest-code search ran on */
int umgen_vqenc_encode(umgen_vqenc *q, int32_t n, const float *x, int64_t *codes, float *z);
const char *umgen_vqenc_last_error(const umgen_vqenc *q);
int umgen_vqenc_destroy(umgen_vqenc *q);

const char *umgen_last_error(const umgen_engine *e); /* never NULL */
const char *umgen_version(void);
int umgen_destroy(umgen_engine *e);

#ifdef __cplusplus
}
#endif
#endif /* UMGEN_H_ */
