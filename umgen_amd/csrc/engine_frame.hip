// One frame, UMGen._inference: run_frame<T> as a sequence of stages -- background pass, uploads, ego net and pose shift, decode state, the
// stacks, first input and prefix pass, the lane loop or the single-stream step loop, drain, download, checks, bookkeeping -- run_frame_fan<T>,
// the first frame of umgen_rollout_fan with the history once per scene, and run_frame_any / run_frame_fan_any, which pick the precision and
// clean up behind a failed call.  The scoring passes (engine_score.hip) are built from the stages engine_frame.h declares.  A frame's host tokens
// are FrameIO::win, a TokenView (token_windows.h); every upload of the four token arrays is upload_tokens.
#include "engine_frame.h"

// host arithmetic stays unfused in every engine file, as it was while they were one file behind the numpy-faithful helpers (engine_weights.hip)
#pragma clang fp contract(off)

namespace {

// Does the prefix pass that ran beside the previous frame's decode cover exactly this window's slots 0..P-1 ?
bool prefix_matches(const umgen_engine* e, const FrameIO& io) {
    const umgen_engine::Prefix& px = e->px;
    if (!px.valid || io.trace || io.B != px.B || io.T != px.Tfull || px.P != io.T - 1 || px.P < 1) return false;
    if (!io.ctrl_pose && !px.has_ego) return false;
    const TokenView old = px.win.view();
    for (int m = 0; m < 4; ++m)
        for (int b = 0; b < io.B; ++b)
            if (memcmp(io.win.at(m, b, 0), old.at(m, b, 0), (size_t)px.P * kModLen[m] * sizeof(int))) return false;
    for (int b = 0; b < io.B; ++b)   // the last frame's pose tokens were already baked into shifted slot P-1
        if (memcmp(io.win.at(0, b, px.P), &px.pose_next[(size_t)b * 3], 3 * sizeof(int))) return false;
    return true;
}

// Foreground growing-window reuse (f-3): the next frame's window is this one plus one slot (it grows, it does not slide), so this frame's passes
// leave their temporal k | v rows in the slot caches
bool grows_into_cache(umgen_engine* e, const FrameIO& io) {
    return !e->overlap && e->grow_cache && io.next_follows && io.cond_cap > 0 && io.T + 1 <= io.cond_cap && io.T + 1 <= e->cfg.max_cond_frames && !io.trace &&
           ensure_tcache(e);
}

// the slot caches now hold slots 0 .. T-1 of this window: what the next frame must find unchanged (prefix_matches)
void remember_window(umgen_engine* e, const FrameIO& io, const std::vector<int>& ego) {
    umgen_engine::Prefix& px = e->px;
    px.B = io.B; px.P = io.T; px.Tfull = io.T + 1; px.has_ego = !io.ctrl_pose;
    gather_windows(io.win, io.B, 0, io.T, px.win);
    px.pose_next.assign(ego.begin(), ego.end());   // slot T-1 was evaluated with the new frame's pose (the shift of UMGen.py:1445-1452)
    px.valid = true;
}

}  // namespace

namespace umgen {

FrameCtx begin_call(umgen_engine* e, const umgen_sampling& smp) {
    e->launch_status = hipSuccess;
    (void)hipGetLastError();
    FrameCtx ctx{};
    ctx.fg = ctx.st = e->stream;
    ctx.sp = SamplerParams{smp.method, smp.top_k, smp.top_k_map, smp.topk_image, smp.p, smp.p_map, smp.temperature, smp.rule_constrain, smp.merge_ar_tar, smp.only_ar};
    return ctx;
}

int finish_call(umgen_engine* e, const char* what) {
    const hipError_t le = e->launch_status != hipSuccess ? e->launch_status : hipGetLastError();
    e->launch_status = hipSuccess;
    if (le != hipSuccess) return e->fail(UMGEN_E_HIP, "a kernel launch of this %s was refused: %s", what, hipGetErrorString(le));
    return 0;
}

int upload_tokens(umgen_engine* e, hipStream_t st, const TokenView& v, size_t rows, bool with_pose) {
    int* const dev[4] = {e->d_pose, e->d_map, e->d_box, e->d_img};
    for (int m = with_pose ? 0 : 1; m < 4; ++m) HIPCHK(e, hipMemcpyAsync(dev[m], v.mod[m], rows * kModLen[m] * 4, hipMemcpyHostToDevice, st));
    return 0;
}

int upload_pose_shift(umgen_engine* e, hipStream_t st, const int* pose, const int* ego, int B, int Tn, std::vector<int>& pshift, std::vector<float>& pdiff) {
    decode_pose_shift(pose, ego, B, Tn, pshift, pdiff);
    HIPCHK(e, hipMemcpyAsync(e->d_pose_shift, pshift.data(), pshift.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->pose_diff, pdiff.data(), pdiff.size() * 4, hipMemcpyHostToDevice, st));
    return 0;
}

void stacks_with_cond_rows(umgen_engine* e, const Place& pl, const WindowTokens& w, CacheMode mode, int fan_scenes) {
    const int stack[3] = {STACK_MAP, STACK_BOX, STACK_TAR};
    const float* const ln[3] = {e->ln_map_tar, e->ln_box_tar, e->ln_tar};
    for (int i = 0; i < 3; ++i) {
        run_stack_any(e, pl, stack[i], w, mode, TAIL_AUTO, nullptr, fan_scenes);
        launch_cond_rows(pl.stream, stack[i], w.B, w.T, e->E, pl.work->X, ln[i], stack[i] == STACK_MAP ? e->warped_last : nullptr, e->dv.cond);
    }
}

int history_slots_once(umgen_engine* e, const Place& pl, const int* pose, int B, int Tn, std::vector<int>& pshift, std::vector<float>& pdiff) {
    const std::vector<int> no_pose((size_t)B * 3, 0);
    if (int rc = upload_pose_shift(e, pl.stream, pose, no_pose.data(), B, Tn, pshift, pdiff)) return rc;
    const WindowTokens wh{e->d_pose_shift, e->d_map, e->d_box, e->d_img, B, Tn - 1, Tn, 0};
    for (int stack : {STACK_MAP, STACK_BOX, STACK_TAR}) run_stack_any(e, pl, stack, wh, CACHE_FILL_PREFIX);
    return 0;
}

// a pending background pass is waited for (second stream) or dropped (engine workers); does the previous pass cover this window, can the next
// one hide behind this frame's decode loop, and which streams do the two phases of the frame take
int settle_background_pass(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B;
    const umgen_trace* tr = io.trace;
    hipStream_t const fg = ctx.fg;
    if (e->bg_pending && e->bg_engine) {
        // a pass whose frame failed before its drain: whatever the workers have done of it is worthless -- empty the queue, the slot caches are not to be trusted
        HIPCHK(e, hipMemsetAsync(&e->d_bgq->n_ops, 0, 4, fg));
        e->bg_pending = false;
        e->px.valid = false;
    }
    if (e->bg_pending && !e->bg_engine) {   // the background pass reads the token arrays and owns the TAR scratch buffers until it is done
        const auto tw0 = std::chrono::steady_clock::now();
        HIPCHK(e, hipEventSynchronize(e->ev_bg_done));
        const double waited = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
        // the pass only pays while it hides behind the decode loop: if the foreground had to wait for it (many scenes per GPU,
        // a much wider model), later frames go back to the plain one-pass path
        if (waited > 25.0 && e->overlap_mode != 2) e->overlap_suspended = true;
        if (getenv("UMGEN_DEBUG_TIMING")) fprintf(stderr, "[umgen] waited %.1f ms for the background pass\n", waited);
        float bms = 0.f;
        hipEventElapsedTime(&bms, e->ev_bg0, e->ev_bg_done);
        e->tm.bg_ms += bms;
        e->bg_pending = false;
    }
    // overlapped TAR pass: when the previous frame's background pass covered slots 0..Tn-2 of this very window, only the last slot
    // is pushed through the stacks now (against the per-layer slot caches)
    ctx.use_px = prefix_matches(e, io);
    // the background pass runs on a quarter of the CUs (measured 3.1x the whole-window time of the same stacks on all CUs): only
    // worth launching when that is expected to hide behind the decode loop (numbers of the previous frames of this engine)
    if (e->last_B != B) { e->last_B = B; e->last_full_pre_ms = 0.f; }
    // (On the decode engine's idle XCDs the pass of a one-scene frame takes ~1800 of its 2206 decode steps, 3.3 x its foreground time (profiles/r06_bg_worker_trace.txt), and what
    //  the steps leave of it drains at 2.7 x: starting it pays as long as about two thirds of it hide -- 2.3 x the foreground time inside the decode loop.  A tighter rule (3.4 x, 5 %
    //  slack) switched the pass OFF on a box whose stacks ran 12 % slower: fp16 1737 instead of 2041 scene-tokens/s.)
    const bool hides = e->overlap_mode == 2 || e->last_full_pre_ms <= 0.f || (e->bg_engine ? 2.3f * e->last_full_pre_ms < e->last_oar_ms : 3.3f * e->last_full_pre_ms < 0.95f * e->last_oar_ms);
    ctx.ov_active = e->overlap && !e->overlap_suspended && hides && !e->profiling && !tr && (B == 1 || e->overlap_mode == 2);
    // the ego / TAR phase runs on all CUs; the decode loop leaves the background stream's XCDs alone only when a pass can follow
    ctx.pre = e->full_stream ? e->full_stream : fg;   // (the background stream is idle until this phase is over)
    ctx.dec = (e->full_stream && !ctx.ov_active) ? e->full_stream : fg;
    ctx.st = ctx.pre;
    return 0;
}

int upload_frame_inputs(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B, Tn = io.T;
    const umgen_trace* tr = io.trace;
    hipStream_t const st = ctx.st;
    if (int rc = upload_tokens(e, st, io.win, (size_t)B * Tn)) return rc;
    ctx.seeds.resize(B);
    for (int b = 0; b < B; ++b) ctx.seeds[b] = io.smp->seeds ? io.smp->seeds[b] : 0ull;
    HIPCHK(e, hipMemcpyAsync(e->dv.d_seeds, ctx.seeds.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
    // the scenes' table sets of this frame (a call with one set: 0 for every scene, so nothing an earlier call left is read), beside the seeds and like them read by the ego sampler and by every token sampler of the frame: both are
    // launched behind this copy in stream order (the ego sampler on this stream; the decode stream and the lanes wait for this stream's events), and the
    // previous frame's last sampler finished before that frame's token download returned
    if (io.plan & kPlanSets) HIPCHK(e, hipMemcpyAsync(e->dv.d_plan.set_of, io.set_of, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    if (ctx.forced) {
        ctx.forced_host.resize(kTokPerFrame);
        for (int i = 0; i < kNPose; ++i) ctx.forced_host[i] = (int)tr->forced_pose[i];
        for (int i = 0; i < kNMap; ++i) ctx.forced_host[kOffMap + i] = (int)tr->forced_map[i];
        for (int i = 0; i < kNBox; ++i) ctx.forced_host[kOffBox + i] = (int)tr->forced_bbox3d[i];
        for (int i = 0; i < kNImg; ++i) ctx.forced_host[kOffImg + i] = (int)tr->forced_image[i];
        HIPCHK(e, hipMemcpyAsync(e->d_forced, ctx.forced_host.data(), (size_t)kTokPerFrame * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(e, hipMemsetAsync(e->d_counters, 0, 8 * sizeof(int), st));
    HIPCHK(e, hipMemsetAsync(e->dv.d_nboxes, 0, (size_t)B * sizeof(int), st));
    // the side outputs of the new frame: all bits set -- NaN, -1 for rank and tokens -- wherever no head is evaluated: a given pose, given map / bbox3d positions
    if (io.side)
        for (const SideBuf& sb : side_buffers(e->dv.d_side, *io.side, (size_t)B)) HIPCHK(e, hipMemsetAsync(sb.dev, 0xFF, sb.bytes, st));
    return 0;
}

// what the ego sampler writes of the call's side outputs, and what constrains its draws
static EgoSide ego_side(const umgen_engine* e, const FrameIO& io) {
    EgoSide es{{}, 0, io.plan, e->dv.d_plan};
    if (const FrameSide* h = io.side) {
        es.out = TokenSide{h->logp ? e->dv.d_side.logp : nullptr, h->logz ? e->dv.d_side.logz : nullptr, h->rank ? e->dv.d_side.detail : DetailOut{}};
        es.detail_topk = h->topk;
    }
    return es;
}

int ego_and_pose_shift(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B, Tn = io.T;
    const umgen_trace* tr = io.trace;
    hipStream_t const st = ctx.st;
    ctx.fg_write = grows_into_cache(e, io);
    ctx.t0 = ctx.use_px ? Tn - 1 : 0; ctx.Tc = ctx.use_px ? 1 : Tn;
    ctx.cmode = ctx.use_px ? (ctx.fg_write ? CACHE_LAST_SLOT_APPEND : CACHE_LAST_SLOT) : (ctx.fg_write ? CACHE_WINDOW_KEEP : CACHE_NONE);
    e->px.valid = false;
    WindowTokens w{e->d_pose, e->d_map, e->d_box, e->d_img, B, ctx.Tc, Tn, ctx.t0};
    // Step 1: ego pose tokens (UMGen.py:1440-1455)
    ctx.ego.resize(B * 3);
    HIPCHK(e, hipEventRecord(e->ev[0], st));
    if (io.ctrl_pose) {
        for (int i = 0; i < B * 3; ++i) ctx.ego[i] = io.ctrl_pose[i];
    } else {
        run_ego_any(e, Place{st, &e->w_main}, w, ctx.sp, io.frame_idx, ctx.forced, tr ? tr->ego_logits : nullptr, ctx.cmode, ego_side(e, io));
        HIPCHK(e, hipMemcpyAsync(ctx.ego.data(), e->d_ego_tok, (size_t)B * 3 * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
    }
    HIPCHK(e, hipEventRecord(e->ev[1], st));
    return upload_pose_shift(e, st, io.win.pose(), ctx.ego.data(), B, Tn, ctx.pshift, ctx.pdiff);
}

int run_stacks(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int E = e->E, B = io.B, Tn = io.T;
    const umgen_trace* tr = io.trace;
    hipStream_t const st = ctx.st;
    // Step 2: the three TAR stacks (UMGen.py:1484-1494) and the conditioning rows (1496-1511)
    WindowTokens ws{e->d_pose_shift, e->d_map, e->d_box, e->d_img, B, ctx.Tc, Tn, ctx.t0};
    // (a profiled frame keeps the stacks one behind the other: its per-launch events are meant to time each kernel alone)
    if ((ctx.use_px || (e->conc_stacks && !e->profiling)) && e->side_stream[0]) {
        // the three stacks are independent -- map and box run on side streams (own workspaces: 1 slot for the last-slot passes of the
        // overlapped path, where 2207 rows per scene leave most CUs idle; the whole window otherwise) beside the TAR stack
        HIPCHK(e, hipEventRecord(e->ev_side_in, st));
        const int side_stack[2] = {STACK_MAP, STACK_BOX};
        for (int i = 0; i < 2; ++i) {
            const Place side{e->side_stream[i], &e->w_side[i]};
            HIPCHK(e, hipStreamWaitEvent(side.stream, e->ev_side_in, 0));
            run_stack_any(e, side, side_stack[i], ws, ctx.cmode);
            launch_cond_rows(side.stream, side_stack[i], B, ctx.Tc, E, side.work->X, i == 0 ? e->ln_map_tar : e->ln_box_tar, i == 0 ? e->warped_last : nullptr,
                             e->dv.cond);
            HIPCHK(e, hipEventRecord(e->ev_side_done[i], side.stream));
        }
        run_stack_any(e, Place{st, &e->w_main}, STACK_TAR, ws, ctx.cmode);
        launch_cond_rows(st, STACK_TAR, B, ctx.Tc, E, e->w_main.X, e->ln_tar, nullptr, e->dv.cond);
        for (int i = 0; i < 2; ++i) HIPCHK(e, hipStreamWaitEvent(st, e->ev_side_done[i], 0));
    } else {
        stacks_with_cond_rows(e, Place{st, &e->w_main}, ws, ctx.cmode);
    }
    if (tr && tr->cond) HIPCHK(e, hipMemcpyAsync(tr->cond, e->dv.cond, (size_t)kSeq * E * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipEventRecord(e->ev[2], st));
    if (ctx.fg_write) remember_window(e, io, ctx.ego);
    return 0;
}

// a profiled call's per-launch events (gemm_timed, tar_sub, the decode loops) into the timings
void fold_launch_events(umgen_engine* e) {
    float ms;
    for (size_t i = 0; i < e->gemm_ev_used; ++i) {
        hipEventElapsedTime(&ms, e->gemm_ev[i].first, e->gemm_ev[i].second);
        e->tm.gemm_ms += ms;
    }
    e->tm.gemm_launches += (int64_t)e->gemm_ev_used;
    e->tm.gemm_flops += e->gemm_flops_pending;
    e->gemm_ev_used = 0;
    e->gemm_flops_pending = 0;
    for (size_t i = 0; i < e->attn_ev_used; ++i) {
        hipEventElapsedTime(&ms, e->attn_ev[i].first, e->attn_ev[i].second);
        e->tm.attn_ms += ms;
    }
    for (size_t i = 0; i < e->layer_ev_used; ++i) {
        hipEventElapsedTime(&ms, e->layer_ev[i].first, e->layer_ev[i].second);
        e->tm.layers_ms += ms;
    }
    e->tm.layers_launches += (int64_t)e->layer_ev_used;
    e->layer_ev_used = 0;
    e->tm.attn_launches += (int64_t)e->attn_ev_used;
    e->tm.attn_flops += e->attn_flops_pending;
    e->attn_ev_used = 0;
    e->attn_flops_pending = 0;
}

// A failed frame may have left a stream capture open, async copies in flight that read this call's host buffers, and a
// background pass the next call would wait for: drain everything and forget the pass (the error message is kept).
void drain_failed_frame(umgen_engine* e) {
    const std::string msg = e->err;
    for (hipStream_t s : {e->stream, e->full_stream, e->bg_stream, e->side_stream[0], e->side_stream[1], e->lane[0].s, e->lane[1].s, e->lane[2].s,
                          e->lane[3].s, e->lane[4].s, e->lane[5].s, e->lane[6].s, e->lane[7].s}) {
        if (!s) continue;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
            hipGraph_t g = nullptr;
            (void)hipStreamEndCapture(s, &g);
            if (g) (void)hipGraphDestroy(g);
        }
    }
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    e->bg_pending = false;
    e->px.valid = false;
    e->err = msg;
}

}  // namespace umgen

namespace {

template <typename T>
int init_decode_state(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B, Tn = io.T;
    const umgen_trace* tr = io.trace;
    hipStream_t const st = ctx.st;
    // new-frame token buffer: pose = ego tokens; previous frame's bbox3d tokens; control mask
    ctx.tok0.assign((size_t)B * kTokPerFrame, 0);
    ctx.prevbox.resize((size_t)B * kNBox);
    for (int b = 0; b < B; ++b) {
        for (int a = 0; a < 3; ++a) ctx.tok0[(size_t)b * kTokPerFrame + a] = ctx.ego[b * 3 + a];
        memcpy(&ctx.prevbox[(size_t)b * kNBox], io.win.at(2, b, Tn - 1), kNBox * sizeof(int));
        if (io.given_map) memcpy(&ctx.tok0[(size_t)b * kTokPerFrame + kOffMap], io.given_map + (size_t)b * kNMap, kNMap * sizeof(int));
        if (io.given_box) memcpy(&ctx.tok0[(size_t)b * kTokPerFrame + kOffBox], io.given_box + (size_t)b * kNBox, kNBox * sizeof(int));
    }
    // scene positions whose tokens are GIVEN (UMGen.py:1184-1201): the pose prefix always; the map, or the map and the boxes, when the
    // caller provides them.  Their steps replay the token (fixed_token_kernel), the sampled steps start behind them.
    ctx.given_end = io.given_box ? kBoxEos + 1 : (io.given_map ? kMapEos + 1 : kPoseEos + 1);
    HIPCHK(e, hipMemcpyAsync(e->dv.d_tokens, ctx.tok0.data(), ctx.tok0.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->dv.d_prev_box, ctx.prevbox.data(), ctx.prevbox.size() * 4, hipMemcpyHostToDevice, st));
    if (io.control_slot) HIPCHK(e, hipMemcpyAsync(e->dv.d_control, io.control_slot, (size_t)B * kSlots, hipMemcpyHostToDevice, st));
    // measurement knob (never set in production): UMGEN_DEBUG_OAR_STEPS="a:b" runs only decode steps j in [a, b) so that
    // per-dispatch PMC collection (which serialises every kernel) stays bounded; results are meaningless then.
    ctx.j_begin = 0; ctx.j_end = kImgEos;
    if (const char* dbg = getenv("UMGEN_DEBUG_OAR_STEPS")) {
        int a0 = 0, b0 = kImgEos;
        if (sscanf(dbg, "%d:%d", &a0, &b0) == 2 && a0 >= 0 && b0 <= kImgEos && a0 < b0) { ctx.j_begin = a0; ctx.j_end = b0; }
    }
    // Hand-off tags of the decode engine never repeat while a copy of an old granule can survive anywhere (a group's L2 keeps its
    // plain-stored granules across launches): the epoch runs on monotonically over the engine's lifetime.  Before the 32-bit
    // counter would wrap (~100 frames at 16384 tags per step) everything is drained and the granule buffers are cleared.
    if (e->wide_enabled && e->eng_epoch > 0xE0000000u) {
        HIPCHK(e, hipDeviceSynchronize());
        HIPCHK(e, hipMemset(e->wide_gran, 0, oar_engine_wide_granules() * 8));
        e->eng_epoch = 16u;
    }
    if (e->eng_enabled && e->eng_epoch > 0xE0000000u) {
        HIPCHK(e, hipDeviceSynchronize());
        HIPCHK(e, hipMemset(e->eng_gx, 0, (size_t)e->cfg.max_batch * kEngE * 8));
        HIPCHK(e, hipMemset(e->eng_gloc, 0, e->eng_gloc_bytes));
        e->eng_epoch = 16u;
    }
    const FrameSide sd = io.side ? *io.side : FrameSide{};      // (topk is 0 without the diagnostics)
    ctx.s0 = OarState{ctx.j_begin, io.frame_idx, ctx.forced ? 1 : 0, io.control_slot ? 1 : 0, 0, e->eng_epoch, ctx.sp, sd.logp ? 1 : 0, sd.rank ? 1 : 0, sd.topk,
                      sd.logz ? 1 : 0, io.plan};
    e->eng_epoch += (unsigned)(kImgEos + 1) * kEpochPerStep;
    HIPCHK(e, hipMemcpyAsync(e->dv.d_state, &ctx.s0, sizeof(ctx.s0), hipMemcpyHostToDevice, st));
    ctx.n_lanes = (sizeof(T) == 2 && !tr) ? e->lane_count(B) : 1;      // decode lanes: every lane steps its own copy of the state
    for (int l = 0; l < ctx.n_lanes && ctx.n_lanes > 1; ++l) HIPCHK(e, hipMemcpyAsync(e->lane[l].st, &ctx.s0, sizeof(ctx.s0), hipMemcpyHostToDevice, st));
    return 0;
}

template <typename T>
int begin_decode(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int E = e->E, B = io.B;
    // Step 3: OAR decode loop (infer_oar_net, UMGen.py:1151-1273).  Step j consumes scene position j (KV length j) and
    // emits scene token j; j = 0..4 replays the given pose prefix, bos/eos are fixed, everything else is sampled.
    // A step is a fixed kernel sequence with fixed arguments (all per-step state is device resident), replayed from a
    // hipGraph per step kind; trace mode launches directly so the logits can be copied out between kernels.
    if (ctx.dec != ctx.pre) {
        HIPCHK(e, hipEventRecord(e->ev_pre_done, ctx.pre));
        HIPCHK(e, hipStreamWaitEvent(ctx.dec, e->ev_pre_done, 0));
    }
    ctx.st = ctx.dec;
    launch_first_input(ctx.st, B, E, e->tb.tske + (long)e->cfg.task_id * E, e->dv.cond, e->dv.xdec);
    {   // tar_head_logits: logits_tar[b][k][:] = head_tar_bbox3d . cond[b][kBoxC0 + k][:]  (exact fp32 FMA chain, bf16 or fp32 weights)
        GemmArgs g{};
        g.P = e->head_tar_box; g.Q = e->dv.cond + (long)kBoxC0 * E; g.Mi = e->cfg.bbox3d_vocab; g.Nj = kNBox; g.K = E; g.ldp = E; g.ldq = E;
        g.strideP = 0; g.strideQ = (long)kSeq * E; g.batch = B; g.mode = GEMM_STORE_F32; g.out = e->dv.logits_tar; g.ldo = e->cfg.bbox3d_vocab;
        g.strideO = (long)kNBox * e->cfg.bbox3d_vocab;
        launch_gemm_valu<T, float>(ctx.st, g);
    }
    if (ctx.ov_active && io.next_follows) {
        const auto tp0 = std::chrono::steady_clock::now();
        if (int rc = launch_prefix_any(e, Place{ctx.st, &e->w_main}, io, ctx.ego)) return rc;
        if (getenv("UMGEN_DEBUG_TIMING"))
            fprintf(stderr, "[umgen] host time to enqueue the background pass: %.1f ms\n",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count());
    }
    return 0;
}

int prefix_pass(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B;
    hipStream_t const st = ctx.st;
    // given map (/ boxes): positions 0 .. given_end - 2 as one pass, the step loop starts at given_end - 1 (UMGEN_PREFIX_PASS=0: replay every
    // given position as a decode step, rounds 1-4).  WHICH form runs is a property of the engine, never of the frame: the pass works in the stacks'
    // buffers, so an engine created with the overlapped background TAR pass ON A SECOND STREAM (UMGEN_OVERLAP=1) replays on every frame, and every
    // other engine -- the decode engine's background workers included: their pass starts with the first decode step, behind this one -- takes the
    // pass on every frame -- traced or not, followed by another frame or not -- so that rollout(n) stays a token prefix of rollout(n + 1) in the
    // 16-bit modes, whose two forms differ in arithmetic.
    const char* ppe = getenv("UMGEN_PREFIX_PASS");      // (read per frame: the tests compare both forms in one process)
    const bool prefix_pass_off = ppe && ppe[0] == '0';
    ctx.s1 = ctx.s0;                                   // (function scope: the asynchronous uploads below read it until the stream is drained)
    if (ctx.given_end > kPoseEos + 1 && !prefix_pass_off && (!e->overlap || e->bg_engine) && ctx.j_begin == 0) {
        if (int rc = run_prefix_prefill_any(e, Place{st, &e->w_main}, B, ctx.given_end)) return rc;
        ctx.j_begin = ctx.given_end - 1;
        ctx.s1.step = ctx.j_begin;
        HIPCHK(e, hipMemcpyAsync(e->dv.d_state, &ctx.s1, sizeof(ctx.s1), hipMemcpyHostToDevice, st));
        for (int l = 0; l < ctx.n_lanes && ctx.n_lanes > 1; ++l) HIPCHK(e, hipMemcpyAsync(e->lane[l].st, &ctx.s1, sizeof(ctx.s1), hipMemcpyHostToDevice, st));
        e->tm.prefix_passes += 1;
    }
    return 0;
}

void plan_decode_steps(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B;
    const umgen_trace* tr = io.trace;
    hipStream_t const st = ctx.st;
    ctx.steps_run = ctx.j_end - ctx.j_begin;             // decode steps of this frame (a prefix pass replaces the given positions' steps)
    ctx.graphs = e->cfg.use_graphs && !tr && !e->profiling;   // profiled frames time every decode step's layer kernel(s) with events
    const DecodePath path = decode_path(e, B, st, false);   // what oar_layers takes for the whole batch (a lane's sub-batch follows it: DecView::lane)
    ctx.batched = path == PATH_BATCHED;
    ctx.wide = path == PATH_WIDE;                            // the chip-wide engine of the wide layers: one launch per scene and step
    static const umgen_engine::EngStream wide_stream{true, 8, {}};
    ctx.eng = ctx.wide ? &wide_stream : (path == PATH_ENGINE ? e->eng_for(st) : nullptr);
    const int eng_ng = ctx.wide ? -3 : (ctx.eng ? ctx.eng->NG + (e->bg_engine && B == 1 ? 100 : 0) : (ctx.batched ? -2 : 0));     // the engine's grid depends on the stream's XCDs: graphs are per (B, NG)
    if (ctx.graphs && (e->step_graph_B != B || e->step_graph_NG != eng_ng)) {
        for (auto& row : e->step_graph)
            for (auto& g : row)
                if (g) { hipGraphExecDestroy(g); g = nullptr; }
        e->step_graph_B = B;
        e->step_graph_NG = eng_ng;
    }
}

// the kind of decode step j: 0 a fixed or given token, 1 map, 2 bbox3d, 3 image
int step_kind(int j, int given_end) {
    if (j < given_end) return 0;
    return (j >= kMapC0 && j < kMapEos) ? 1 : (j >= kBoxC0 && j < kBoxEos) ? 2 : (j >= kImgC0 && j < kImgEos) ? 3 : 0;
}

int run_lane_loop(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B, given_end = ctx.given_end, n_lanes = ctx.n_lanes, j_end = ctx.j_end;
    hipStream_t const st = ctx.st;
    // Decode lanes (umgen_engine::DecLane): fork behind the first input, every lane replays the step runs for its scenes on its own
    // stream, join before the token download.  Step runs are graphs in every mode but --no-graphs (a profiled frame times lane 0's
    // runs around the graph launches: eager launches of n lanes x 182 kernels per step would measure the host).
    const bool lane_graphs = e->cfg.use_graphs;
    if (e->lane_graph_B != B || e->lane_graph_n != n_lanes) {
        for (auto& ln : e->lane)
            for (auto& row : ln.graph)
                for (auto& g : row)
                    if (g) { hipGraphExecDestroy(g); g = nullptr; }
        e->lane_graph_B = B;
        e->lane_graph_n = n_lanes;
    }
    HIPCHK(e, hipEventRecord(e->ev_lane_fork, st));
    DecView view[umgen_engine::kMaxLanes];
    int nbs[umgen_engine::kMaxLanes];
    for (int l = 0, b0 = 0; l < n_lanes; ++l) {
        nbs[l] = B / n_lanes + (l < B % n_lanes ? 1 : 0);
        view[l] = lane_view(e, e->lane[l], b0);
        b0 += nbs[l];
        HIPCHK(e, hipStreamWaitEvent(e->lane[l].s, e->ev_lane_fork, 0));
    }
    for (int j = ctx.j_begin; j < j_end; ++j) {
        const int mod = step_kind(j, given_end);
        int same = 1;
        while (same < 16 && j + same < j_end && step_kind(j + same, given_end) == mod) ++same;
        const int run = !lane_graphs ? 1 : (same >= 16 ? 16 : (same >= 4 ? 4 : 1));
        const int ri = run == 16 ? 2 : (run == 4 ? 1 : 0);
        for (int l = 0; l < n_lanes; ++l) {
            umgen_engine::DecLane& ln = e->lane[l];
            const bool timed = e->profiling && l == 0;
            if (timed) {
                if (e->layer_ev_used == e->layer_ev.size()) {
                    hipEvent_t a0, a1;
                    hipEventCreate(&a0);
                    hipEventCreate(&a1);
                    e->layer_ev.emplace_back(a0, a1);
                }
                hipEventRecord(e->layer_ev[e->layer_ev_used].first, ln.s);
            }
            if (lane_graphs) {
                hipGraphExec_t& ge = ln.graph[mod][ri];
                if (!ge) {
                    hipGraph_t g;
                    HIPCHK(e, hipStreamBeginCapture(ln.s, hipStreamCaptureModeThreadLocal));
                    DecView cap = view[l];
                    cap.capture = true;
                    int crc = 0;
                    for (int r = 0; r < run && !crc; ++r) crc = enqueue_step_any(e, cap, nbs[l], mod, 1, nullptr, 0);
                    if (crc) return crc;   // (run_frame_any ends the open capture)
                    HIPCHK(e, hipStreamEndCapture(ln.s, &g));
                    HIPCHK(e, hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
                    HIPCHK(e, hipGraphDestroy(g));
                }
                HIPCHK(e, hipGraphLaunch(ge, ln.s));
            } else if (int rc = enqueue_step_any(e, view[l], nbs[l], mod, 1, nullptr, j)) {
                return rc;
            }
            if (timed) {
                hipEventRecord(e->layer_ev[e->layer_ev_used++].second, ln.s);
                e->tm.layers_launches += run - 1;      // (the frame's bookkeeping below adds one per event pair)
            }
            e->tm.oar_kernels += (int64_t)run * (5 * (int64_t)e->oar.size() + (mod == 0 ? 1 : (mod == 2 ? 3 : 2)));
        }
        j += run - 1;
    }
    for (int l = 0; l < n_lanes; ++l) {
        HIPCHK(e, hipEventRecord(e->lane[l].done, e->lane[l].s));
        HIPCHK(e, hipStreamWaitEvent(st, e->lane[l].done, 0));
    }
    ctx.j_begin = j_end;     // (the single-stream loop below has nothing left to do)
    return 0;
}

int run_step_loop(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B, given_end = ctx.given_end, j_begin = ctx.j_begin, j_end = ctx.j_end;
    const bool graphs = ctx.graphs, batched = ctx.batched, wide = ctx.wide;
    const umgen_engine::EngStream* eng = ctx.eng;
    const umgen_trace* tr = io.trace;
    hipStream_t const st = ctx.st;
    DecView view = e->dv;                      // the whole batch on the frame's decode stream
    view.stream = st;
    for (int j = j_begin; j < j_end; ++j) {   // the img-eos step (j = 2206) produces nothing that is consumed
        const int mod = step_kind(j, given_end);
        const int ns = attn_nsplit(j + 1);          // key splits over the j cached keys + the new one
        const int gkey = (eng || batched) ? 0 : ns;   // the engine / the batched layer derive their key geometry from the device-side step
        if (graphs) {
            // With the decode engine a step is 3 kernel nodes and ~600 us, and a graph launch costs ~7 us on the device (the gap between
            // the sampler of one replay and the engine of the next, rocprofv3 kernel trace): runs of steps of the same kind are replayed
            // 16 or 4 at a time (gkey 1 / 2; the engine derives everything else from the device-side step counter).
            int run = 1;
            if (eng || batched) {
                int same = 1;
                while (same < 16 && j + same < j_end) {
                    if (step_kind(j + same, given_end) != mod) break;
                    ++same;
                }
                run = same >= 16 ? 16 : (same >= 4 ? 4 : 1);
            }
            hipGraphExec_t& ge = e->step_graph[mod][(eng || batched) ? (run == 16 ? 2 : (run == 4 ? 1 : 0)) : gkey];
            if (!ge) {
                hipGraph_t g;
                HIPCHK(e, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
                DecView cap = view;
                cap.capture = true;
                int crc = 0;
                for (int r = 0; r < run && !crc; ++r) crc = enqueue_step_any(e, cap, B, mod, ns, nullptr, 0);
                if (crc) return crc;   // (run_frame_any ends the open capture)
                HIPCHK(e, hipStreamEndCapture(st, &g));
                HIPCHK(e, hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
                HIPCHK(e, hipGraphDestroy(g));
            }
            HIPCHK(e, hipGraphLaunch(ge, st));
            e->tm.oar_kernels += (int64_t)(run - 1) * ((eng ? (wide ? B : 1) : 5 * (int64_t)e->oar.size()) + (mod == 0 ? 1 : (mod == 2 ? 3 : 2)));
            j += run - 1;
        } else if (int rc = enqueue_step_any(e, view, B, mod, ns, tr, j)) {
            return rc;
        }
        e->tm.oar_kernels += (eng ? (wide ? B : 1) : 5 * (int64_t)e->oar.size()) + (mod == 0 ? 1 : (mod == 2 ? 3 : 2));
    }
    e->tm.oar_steps += ctx.steps_run;
    return 0;
}

template <typename T>
int drain_and_download(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B;
    const bool wide = ctx.wide;
    const umgen_engine::EngStream* eng = ctx.eng;
    hipStream_t const st = ctx.st;
    ctx.drained = e->bg_engine && e->bg_pending;
    if (ctx.drained) {      // what the decode steps' launches left of the background pass: one launch without an engine part runs it to the end
        HIPCHK(e, hipEventRecord(e->ev_drain0, st));
        if (int rc = launch_bg_drain(e, st)) return rc;
        HIPCHK(e, hipEventRecord(e->ev_drain1, st));
        e->bg_state_host.assign((size_t)kBgMaxWorkers * 4, 0u);
        HIPCHK(e, hipMemcpyAsync(e->bg_state_host.data(), &e->d_bgq->state[0][0], sizeof(e->d_bgq->state), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(e, hipEventRecord(e->ev[3], st));
    HIPCHK(e, hipMemcpyAsync(io.out_tokens, e->dv.d_tokens, (size_t)B * kTokPerFrame * 4, hipMemcpyDeviceToHost, st));
    if (io.side)
        for (const SideBuf& sb : side_buffers(e->dv.d_side, *io.side, (size_t)B)) HIPCHK(e, hipMemcpyAsync(sb.host, sb.dev, sb.bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(ctx.counters, e->d_counters, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (eng) HIPCHK(e, hipMemcpyAsync(&ctx.eng_err, wide ? e->wide_err : e->eng_err, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return finish_call(e, "frame");
}

int check_frame_results(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const umgen_trace* tr = io.trace;
    const bool wide = ctx.wide;
    if (ctx.drained) {
        e->bg_pending = false;
        float dms = 0.f;
        hipEventElapsedTime(&dms, e->ev_drain0, e->ev_drain1);
        e->tm.bg_ms += dms;
        for (int wk = 0; wk < kBgMaxWorkers; ++wk)
            if (e->bg_state_host[(size_t)wk * 4] < e->bg_rec.ops.size()) {
                e->px.valid = false;
                if (getenv("UMGEN_DEBUG_TIMING")) {
                    fprintf(stderr, "[umgen] worker states (op, units done | arrived):");
                    for (int k = 0; k < kBgMaxWorkers; ++k) fprintf(stderr, " %u:%x", e->bg_state_host[(size_t)k * 4], e->bg_state_host[(size_t)k * 4 + 1]);
                    const unsigned o0 = e->bg_state_host[(size_t)wk * 4];
                    unsigned arr[4] = {};
                    (void)hipMemcpy(arr, &e->d_bgq->arrive[o0 > 0 ? o0 - 1 : 0], sizeof(arr), hipMemcpyDeviceToHost);
                    const BgOpHead& h = e->bg_rec.ops[o0].h;
                    fprintf(stderr, "\n[umgen] arrivals from op %u on: %u %u %u %u; op %u: kind %d mode %d units %d chunk %d i0..3 %d %d %d %d\n", o0 > 0 ? o0 - 1 : 0, arr[0], arr[1], arr[2], arr[3], o0,
                            h.kind, h.mode, h.n_units, h.chunk, h.i0, h.i1, h.i2, h.i3);
                }
                return e->fail(UMGEN_E_HIP, "background pass incomplete: worker %d stopped at op %u of %zu", wk, e->bg_state_host[(size_t)wk * 4], e->bg_rec.ops.size());
            }
        e->px.valid = true;
        if (getenv("UMGEN_DEBUG_TIMING")) {
            fprintf(stderr, "[umgen] background pass: %zu ops, drain launch %.2f ms\n", e->bg_rec.ops.size(), dms);
            // where a worker's time goes, by kind: sum over the ops of (units per worker) x (the slowest batch's time per unit) -- an upper bound
            std::vector<unsigned> est(e->bg_rec.ops.size());
            if (hipMemcpy(est.data(), &e->d_bgq->est[0], est.size() * 4, hipMemcpyDeviceToHost) == hipSuccess) {
                double by_kind[8] = {}, gemm_by_mode[4] = {};
                for (size_t i = 0; i < est.size(); ++i) {
                    const BgOpHead& h = e->bg_rec.ops[i].h;
                    const double us = std::ceil((double)h.n_units / 128.0) * ((double)est[i] - 20.0) / 1.125 / 100.0;
                    by_kind[h.kind & 7] += us;
                    if (h.kind == BG_GEMM) gemm_by_mode[h.mode & 3] += us;
                }
                fprintf(stderr, "[umgen] per-worker time by kind (ms, upper bound): gemm %.1f (store %.1f, resid %.1f, vt %.1f) ln %.1f attn_s %.1f attn_t %.1f embed %.1f warp %.1f\n", by_kind[BG_GEMM] / 1e3,
                        gemm_by_mode[GEMM_STORE] / 1e3, gemm_by_mode[GEMM_RESID] / 1e3, gemm_by_mode[GEMM_VT] / 1e3, by_kind[BG_LN] / 1e3, by_kind[BG_ATTN_S] / 1e3, by_kind[BG_ATTN_T] / 1e3,
                        by_kind[BG_EMBED] / 1e3, by_kind[BG_WARP] / 1e3);
            }
        }
    }
    if (ctx.eng_err) {   // a hand-off of the decode engine timed out (e.g. two engines sharing one GPU): never return tokens from such a frame
        (void)hipMemset(wide ? e->wide_err : e->eng_err, 0, sizeof(unsigned));
        return e->fail(UMGEN_E_HIP, "decode engine gave up waiting for hand-off tag 0x%08x (is another persistent kernel using this GPU?)", ctx.eng_err);
    }
    if (tr && tr->counters) memcpy(tr->counters, ctx.counters, sizeof(ctx.counters));
    return 0;
}

void frame_bookkeeping(umgen_engine* e, const FrameIO& io, const FrameCtx& ctx) {
    const int E = e->E, B = io.B, n_lanes = ctx.n_lanes;
    const bool use_px = ctx.use_px, batched = ctx.batched, wide = ctx.wide;
    const umgen_engine::EngStream* eng = ctx.eng;
    float ms;
    hipEventElapsedTime(&ms, e->ev[0], e->ev[1]); e->tm.ego_ms += ms;
    hipEventElapsedTime(&ms, e->ev[1], e->ev[2]); e->tm.tar_ms += ms;
    hipEventElapsedTime(&ms, e->ev[2], e->ev[3]); e->tm.oar_ms += ms;
    e->last_oar_ms = ms;
    if (!use_px) {
        float pre = 0.f;
        hipEventElapsedTime(&pre, e->ev[0], e->ev[2]);
        e->last_full_pre_ms = pre;
    }
    hipEventElapsedTime(&ms, e->ev[0], e->ev[3]); e->tm.total_ms += ms;
    e->tm.frames += 1;
    e->tm.decode_engine = eng ? (wide ? 3 : 1) : 0;      // 1: the XCD-resident engine, 3: the chip-wide engine of the wide layers (2: the retired multi-scene engine of round 5)
    e->tm.decode_batched = batched ? 1 : 0;
    e->tm.decode_lanes = batched ? n_lanes : 0;
    e->tm.engine_fallback = e->eng_fallback ? 1 : 0;
    if (use_px) e->tm.overlapped_frames += 1;
    if (e->profiling) fold_launch_events(e);
    // algorithmic HBM bytes of this frame's decode steps: weights once per step + KV read + KV write
    {
        const double w_layer = (double)e->tsz * (12.0 * E * E) + 4.0 * (6.0 * E);   // 3E*E + E*E + 4E*E + 4E*E weights, biases/LN
        const double w_oar = w_layer * (double)e->oar.size();
        double bytes = 0;
        for (int j = 0; j < kImgEos; ++j) {
            bytes += w_oar + (double)B * (double)e->oar.size() * (double)e->tsz * 2.0 * E * (double)(j + 1);
            const int V = (j >= kMapC0 && j < kMapEos) ? e->cfg.map_vocab : (j >= kBoxC0 && j < kBoxEos) ? e->cfg.bbox3d_vocab
                        : (j >= kImgC0 && j < kImgEos) ? e->cfg.img_vocab : 0;
            bytes += (double)V * E * (double)e->tsz;
        }
        bytes += (double)e->cfg.bbox3d_vocab * E * (double)e->tsz;   // head_tar_bbox3d: one GEMM per frame (tar_head_logits), not one GEMV per bbox3d step
        e->tm.oar_bytes += bytes;
    }
}

// a frame from the first decode input on, behind the stacks and the conditioning rows: run_frame's and run_frame_fan's common end
template <typename T>
int decode_and_finish(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    if (int rc = begin_decode<T>(e, io, ctx)) return rc;
    if (int rc = prefix_pass(e, io, ctx)) return rc;
    plan_decode_steps(e, io, ctx);
    if (ctx.n_lanes > 1) {
        if (int rc = run_lane_loop(e, io, ctx)) return rc;
    }
    if (int rc = run_step_loop(e, io, ctx)) return rc;
    if (int rc = drain_and_download<T>(e, io, ctx)) return rc;
    if (int rc = check_frame_results(e, io, ctx)) return rc;
    frame_bookkeeping(e, io, ctx);
    return 0;
}

// UMGen._inference (UMGen.py:1406-1540) for B scenes
template <typename T>
int run_frame(umgen_engine* e, const FrameIO& io) {
    FrameCtx ctx = begin_call(e, *io.smp);
    ctx.forced = io.trace && io.trace->forced_map;
    if (int rc = settle_background_pass(e, io, ctx)) return rc;
    if (int rc = upload_frame_inputs(e, io, ctx)) return rc;
    if (int rc = ego_and_pose_shift(e, io, ctx)) return rc;
    if (int rc = init_decode_state<T>(e, io, ctx)) return rc;
    if (int rc = run_stacks(e, io, ctx)) return rc;
    return decode_and_finish<T>(e, io, ctx);
}

// every BlockTAR cache of one stack: slots [0, P) of the scene blocks b < B to the blocks b*N + s (launch_tcache_spread: scene by scene in descending b)
void spread_tcaches(umgen_engine* e, hipStream_t st, int stack, int B, int N, int P) {
    const size_t row_bytes = (size_t)stack_len(stack) * 2 * e->E * e->tsz;
    for (void* c : e->tcache[stack]) launch_tcache_spread(st, c, B, N, P, e->cfg.max_cond_frames, row_bytes);
}

// The first frame of umgen_rollout_fan: io holds the B * N branches as scenes -- branch (b, s) at b*N + s, every scene's window, control slots and given tokens
// replicated N times, the seeds per branch -- and everything that does not depend on the branch runs once per scene, as in run_score_candidates.  The ego net
// reads the unshifted window, so it runs on the B scenes and every branch draws its pose from its scene's head_ego rows (run_ego_fan).  The pose shift hands
// only slot T - 1 the new frame's pose, so slots [0, T - 1) of the map / box / TAR stacks run on the B scenes (history_slots_once) and the branches push their last
// slot against their scene's caches (CACHE_SHARED_ITEMS).  Every kernel's row arithmetic is that of run_frame, so the conditioning rows, and from begin_decode on the
// whole frame -- an ordinary frame of B * N scenes -- have the bits of run_frame on io.
// When the next frame's window is this one plus a slot (grows_into_cache) the slot caches must end up as run_frame's CACHE_WINDOW_KEEP leaves them for all B * N
// scenes: the ego stack fills the scenes' blocks in that mode, the last-slot passes append every branch's own slot T - 1 to its own block (CACHE_SHARED_ITEMS_APPEND),
// and then every cache is spread -- block b*N + s receives slots [0, T - 1) ([0, T) of the ego stack) of scene block b, behind ALL reads of the scene blocks and
// scene by scene in descending b (tcache_spread_kernel states why) -- and px is filled for B * N scenes like run_stacks fills it.
template <typename T>
int run_frame_fan(umgen_engine* e, const FrameIO& io, int N) {
    const int BN = io.B, B = io.B / N, Tn = io.T, P = io.T - 1;
    FrameCtx ctx = begin_call(e, *io.smp);
    e->px.valid = false;                 // the passes below overwrite the slot caches: nothing an earlier call left there covers this window
    if (int rc = settle_background_pass(e, io, ctx)) return rc;
    if (int rc = upload_frame_inputs(e, io, ctx)) return rc;      // seeds, counters and logp of the B * N branches; the token arrays follow below
    hipStream_t const st = ctx.st;
    // the scenes' windows [B][T][S_mod] (branch (b, 0) holds scene b's) for the passes that run once per scene
    TokenSeqs win;
    std::vector<int> item_scene(BN), hshift;
    std::vector<float> hdiff;
    gather_windows(io.win, B, [N](size_t b) { return b * N; }, [](size_t) { return 0; }, Tn, win);
    if (int rc = upload_tokens(e, st, win.view(), (size_t)B * Tn)) return rc;
    ctx.fg_write = grows_into_cache(e, io);      // (io.trace is null: a fan frame is a rollout's)
    ctx.t0 = 0; ctx.Tc = Tn; ctx.cmode = ctx.fg_write ? CACHE_WINDOW_KEEP : CACHE_NONE;
    // Step 1: the ego net once per scene, a pose per branch
    ctx.ego.resize((size_t)BN * 3);
    HIPCHK(e, hipEventRecord(e->ev[0], st));
    if (io.ctrl_pose) {
        for (int i = 0; i < BN * 3; ++i) ctx.ego[i] = io.ctrl_pose[i];
    } else {
        run_ego_fan_any(e, Place{st, &e->w_main}, WindowTokens{e->d_pose, e->d_map, e->d_box, e->d_img, B, Tn, Tn, 0}, N, ctx.sp, io.frame_idx, ctx.cmode, ego_side(e, io));
        HIPCHK(e, hipMemcpyAsync(ctx.ego.data(), e->d_ego_tok, (size_t)BN * 3 * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
    }
    HIPCHK(e, hipEventRecord(e->ev[1], st));
    if (int rc = init_decode_state<T>(e, io, ctx)) return rc;
    // Step 2a: slots [0, T - 1) of the three stacks once per scene, their temporal k | v rows into the scenes' blocks of the slot caches (slot T - 1 of the
    // shifted pose is not read)
    if (int rc = history_slots_once(e, Place{st, &e->w_main}, win.view().pose(), B, Tn, hshift, hdiff)) return rc;
    // Step 2b: slot T - 1 of every branch -- its own pose in the shift, its own window rows -- against its scene's caches, and the conditioning rows
    if (int rc = upload_pose_shift(e, st, io.win.pose(), ctx.ego.data(), BN, Tn, ctx.pshift, ctx.pdiff)) return rc;
    if (int rc = upload_tokens(e, st, io.win, (size_t)BN * Tn)) return rc;
    for (int i = 0; i < BN; ++i) item_scene[i] = i / N;
    HIPCHK(e, hipMemcpyAsync(e->d_item_scene, item_scene.data(), (size_t)BN * 4, hipMemcpyHostToDevice, st));
    stacks_with_cond_rows(e, Place{st, &e->w_main}, WindowTokens{e->d_pose_shift, e->d_map, e->d_box, e->d_img, BN, 1, Tn, P},
                          ctx.fg_write ? CACHE_SHARED_ITEMS_APPEND : CACHE_SHARED_ITEMS, B);
    if (ctx.fg_write) {   // behind every read of the scene blocks: each branch's block gets its scene's slots; then the caches hold slots 0 .. T-1 of all B * N windows
        spread_tcaches(e, st, STACK_MAP, B, N, P);
        spread_tcaches(e, st, STACK_BOX, B, N, P);
        spread_tcaches(e, st, STACK_TAR, B, N, P);
        if (!io.ctrl_pose) spread_tcaches(e, st, STACK_EGO, B, N, Tn);
        remember_window(e, io, ctx.ego);
    }
    HIPCHK(e, hipEventRecord(e->ev[2], st));
    return decode_and_finish<T>(e, io, ctx);      // Step 3 on: an ordinary frame of B * N scenes
}

}  // namespace

namespace umgen {

int run_frame_any(umgen_engine* e, const FrameIO& io) {
    const int rc = with_precision(e, [&](auto t) { return run_frame<decltype(t)>(e, io); });
    if (rc != UMGEN_OK) drain_failed_frame(e);
    return rc;
}

int run_frame_fan_any(umgen_engine* e, const FrameIO& io, int N) {
    const int rc = with_precision(e, [&](auto t) { return run_frame_fan<decltype(t)>(e, io, N); });
    if (rc != UMGEN_OK) drain_failed_frame(e);
    return rc;
}

}  // namespace umgen
