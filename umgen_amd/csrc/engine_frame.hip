// One frame, UMGen._inference: run_frame<T> as a sequence of stages -- background pass, uploads, ego net and pose shift, decode state, the
// stacks, first input and prefix pass, the lane loop or the single-stream step loop, drain, download, checks, bookkeeping -- run_score<T>,
// the scoring pass of umgen_score built from the same stages, run_score_candidates<T>, which scores several next frames per scene on one pass
// over the history, run_score_clip<T>, which scores every frame of a recorded clip, the growing windows off one pass, run_frame_fan<T>, the first frame of
// umgen_rollout_fan with the history once per scene, and run_frame_any / run_frame_fan_any / run_score_any / run_score_candidates_any / run_score_clip_any,
// which pick the precision and clean up behind a failed call.
#include "engine_state.h"

// host arithmetic stays unfused in every engine file, as it was while they were one file behind the numpy-faithful helpers (engine_weights.hip)
#pragma clang fp contract(off)

namespace {

// Does the prefix pass that ran beside the previous frame's decode cover exactly this window's slots 0..P-1 ?
bool prefix_matches(const umgen_engine* e, const FrameIO& io) {
    const umgen_engine::Prefix& px = e->px;
    if (!px.valid || io.trace || io.B != px.B || io.T != px.Tfull || px.P != io.T - 1 || px.P < 1) return false;
    if (!io.ctrl_pose && !px.has_ego) return false;
    const int S[4] = {kNPose, kNMap, kNBox, kNImg};
    const int* cur[4] = {io.pose, io.map, io.box, io.img};
    const std::vector<int>* old[4] = {&px.pose, &px.map, &px.box, &px.img};
    for (int m = 0; m < 4; ++m)
        for (int b = 0; b < io.B; ++b)
            if (memcmp(cur[m] + (size_t)b * io.T * S[m], old[m]->data() + (size_t)b * px.P * S[m], (size_t)px.P * S[m] * sizeof(int))) return false;
    for (int b = 0; b < io.B; ++b)   // the last frame's pose tokens were already baked into shifted slot P-1
        if (memcmp(io.pose + ((size_t)b * io.T + px.P) * kNPose, &px.pose_next[(size_t)b * 3], 3 * sizeof(int))) return false;
    return true;
}

// The locals of run_frame that more than one stage uses, or that the frame's asynchronous copies read until the stream is drained (so they
// live as long as the frame does).  Filled stage by stage, in run_frame's order; zero-initialised there.
struct FrameCtx {
    hipStream_t fg, st, pre, dec;       // the engine's stream at entry; the stream in use; the streams of the ego / TAR phase and of the decode loop
    SamplerParams sp;
    bool forced;                        // teacher-forced trace frame
    bool use_px, ov_active, fg_write;   // last slot only against the slot caches; a background pass may follow; this frame's passes fill the caches
    int t0, Tc, cmode;                  // first slot, slot count and cache_mode of this frame's passes through the stacks
    std::vector<unsigned long long> seeds;
    std::vector<int> forced_host, ego, pshift, tok0, prevbox;
    std::vector<float> pdiff;
    int given_end, j_begin, j_end, n_lanes, steps_run;
    OarState s0, s1;                    // step state at the start of the loop, and behind a prefix pass
    bool graphs, batched, wide, drained;
    const umgen_engine::EngStream* eng;
    int counters[8];
    unsigned eng_err;
};

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
    e->stream = ctx.pre;
    return 0;
}

int upload_frame_inputs(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B, Tn = io.T;
    const umgen_trace* tr = io.trace;
    hipStream_t const st = ctx.st;
    HIPCHK(e, hipMemcpyAsync(e->d_pose, io.pose, (size_t)B * Tn * 3 * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->d_map, io.map, (size_t)B * Tn * kNMap * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->d_box, io.box, (size_t)B * Tn * kNBox * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->d_img, io.img, (size_t)B * Tn * kNImg * 4, hipMemcpyHostToDevice, st));
    ctx.seeds.resize(B);
    for (int b = 0; b < B; ++b) ctx.seeds[b] = io.smp->seeds ? io.smp->seeds[b] : 0ull;
    HIPCHK(e, hipMemcpyAsync(e->d_seeds, ctx.seeds.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
    if (ctx.forced) {
        ctx.forced_host.resize(kTokPerFrame);
        for (int i = 0; i < kNPose; ++i) ctx.forced_host[i] = (int)tr->forced_pose[i];
        for (int i = 0; i < kNMap; ++i) ctx.forced_host[kOffMap + i] = (int)tr->forced_map[i];
        for (int i = 0; i < kNBox; ++i) ctx.forced_host[kOffBox + i] = (int)tr->forced_bbox3d[i];
        for (int i = 0; i < kNImg; ++i) ctx.forced_host[kOffImg + i] = (int)tr->forced_image[i];
        HIPCHK(e, hipMemcpyAsync(e->d_forced, ctx.forced_host.data(), (size_t)kTokPerFrame * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(e, hipMemsetAsync(e->d_counters, 0, 8 * sizeof(int), st));
    HIPCHK(e, hipMemsetAsync(e->d_nboxes, 0, (size_t)B * sizeof(int), st));
    // log-likelihoods of the new frame: NaN (all bits set) wherever no head is evaluated -- a given pose, given map / bbox3d positions
    if (io.out_logp) HIPCHK(e, hipMemsetAsync(e->d_logp, 0xFF, (size_t)B * kTokPerFrame * sizeof(float), st));
    return 0;
}

int ego_and_pose_shift(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B, Tn = io.T;
    const umgen_trace* tr = io.trace;
    hipStream_t const st = ctx.st;
    // foreground growing-window reuse (f-3): the next frame's window is this one plus one slot (it grows, it does not slide), so this
    // frame's passes leave their temporal k | v rows in the slot caches
    ctx.fg_write = !e->overlap && e->grow_cache && io.next_follows && io.cond_cap > 0 && Tn + 1 <= io.cond_cap &&
                          Tn + 1 <= e->cfg.max_cond_frames && !tr && ensure_tcache(e);
    ctx.t0 = ctx.use_px ? Tn - 1 : 0; ctx.Tc = ctx.use_px ? 1 : Tn; ctx.cmode = ctx.use_px ? (ctx.fg_write ? 4 : 2) : (ctx.fg_write ? 3 : 0);
    e->px.valid = false;
    WindowTokens w{e->d_pose, e->d_map, e->d_box, e->d_img, B, ctx.Tc, Tn, ctx.t0};
    // Step 1: ego pose tokens (UMGen.py:1440-1455)
    ctx.ego.resize(B * 3);
    HIPCHK(e, hipEventRecord(e->ev[0], st));
    if (io.ctrl_pose) {
        for (int i = 0; i < B * 3; ++i) ctx.ego[i] = io.ctrl_pose[i];
    } else {
        run_ego_any(e, w, ctx.sp, io.frame_idx, ctx.forced, tr ? tr->ego_logits : nullptr, ctx.cmode, io.out_logp ? e->d_logp : nullptr);
        HIPCHK(e, hipMemcpyAsync(ctx.ego.data(), e->d_ego_tok, (size_t)B * 3 * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
    }
    HIPCHK(e, hipEventRecord(e->ev[1], st));
    decode_pose_shift(io.pose, ctx.ego.data(), B, Tn, ctx.pshift, ctx.pdiff);
    HIPCHK(e, hipMemcpyAsync(e->d_pose_shift, ctx.pshift.data(), ctx.pshift.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->pose_diff, ctx.pdiff.data(), ctx.pdiff.size() * 4, hipMemcpyHostToDevice, st));
    return 0;
}

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
        memcpy(&ctx.prevbox[(size_t)b * kNBox], io.box + ((size_t)b * Tn + (Tn - 1)) * kNBox, kNBox * sizeof(int));
        if (io.given_map) memcpy(&ctx.tok0[(size_t)b * kTokPerFrame + kOffMap], io.given_map + (size_t)b * kNMap, kNMap * sizeof(int));
        if (io.given_box) memcpy(&ctx.tok0[(size_t)b * kTokPerFrame + kOffBox], io.given_box + (size_t)b * kNBox, kNBox * sizeof(int));
    }
    // scene positions whose tokens are GIVEN (UMGen.py:1184-1201): the pose prefix always; the map, or the map and the boxes, when the
    // caller provides them.  Their steps replay the token (fixed_token_kernel), the sampled steps start behind them.
    ctx.given_end = io.given_box ? kBoxEos + 1 : (io.given_map ? kMapEos + 1 : kPoseEos + 1);
    HIPCHK(e, hipMemcpyAsync(e->d_tokens, ctx.tok0.data(), ctx.tok0.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->d_prev_box, ctx.prevbox.data(), ctx.prevbox.size() * 4, hipMemcpyHostToDevice, st));
    if (io.control_slot) HIPCHK(e, hipMemcpyAsync(e->d_control, io.control_slot, (size_t)B * kSlots, hipMemcpyHostToDevice, st));
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
    ctx.s0 = OarState{ctx.j_begin, io.frame_idx, ctx.forced ? 1 : 0, io.control_slot ? 1 : 0, 0, e->eng_epoch, ctx.sp, io.out_logp ? 1 : 0};
    e->eng_epoch += (unsigned)(kImgEos + 1) * kEpochPerStep;
    HIPCHK(e, hipMemcpyAsync(e->d_state, &ctx.s0, sizeof(ctx.s0), hipMemcpyHostToDevice, st));
    ctx.n_lanes = (sizeof(T) == 2 && !tr) ? e->lane_count(B) : 1;      // decode lanes: every lane steps its own copy of the state
    for (int l = 0; l < ctx.n_lanes && ctx.n_lanes > 1; ++l) HIPCHK(e, hipMemcpyAsync(e->lane[l].st, &ctx.s0, sizeof(ctx.s0), hipMemcpyHostToDevice, st));
    return 0;
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
        struct Restore { umgen_engine* e; hipStream_t s; ~Restore() { e->stream = s; e->set_work(e->w_main); } } restore{e, st};
        HIPCHK(e, hipEventRecord(e->ev_side_in, st));
        const int side_stack[2] = {STACK_MAP, STACK_BOX};
        for (int i = 0; i < 2; ++i) {
            HIPCHK(e, hipStreamWaitEvent(e->side_stream[i], e->ev_side_in, 0));
            e->stream = e->side_stream[i];
            e->set_work(e->w_side[i]);
            run_stack_any(e, side_stack[i], ws, ctx.cmode);
            launch_cond_rows(e->stream, side_stack[i], B, ctx.Tc, E, e->X, i == 0 ? e->ln_map_tar : e->ln_box_tar, i == 0 ? e->warped_last : nullptr,
                             e->cond);
            HIPCHK(e, hipEventRecord(e->ev_side_done[i], e->side_stream[i]));
        }
        e->stream = st;
        e->set_work(e->w_main);
        run_stack_any(e, STACK_TAR, ws, ctx.cmode);
        launch_cond_rows(st, STACK_TAR, B, ctx.Tc, E, e->X, e->ln_tar, nullptr, e->cond);
        for (int i = 0; i < 2; ++i) HIPCHK(e, hipStreamWaitEvent(st, e->ev_side_done[i], 0));
    } else {
        run_stack_any(e, STACK_MAP, ws, ctx.cmode);
        launch_cond_rows(st, STACK_MAP, B, ctx.Tc, E, e->X, e->ln_map_tar, e->warped_last, e->cond);
        run_stack_any(e, STACK_BOX, ws, ctx.cmode);
        launch_cond_rows(st, STACK_BOX, B, ctx.Tc, E, e->X, e->ln_box_tar, nullptr, e->cond);
        run_stack_any(e, STACK_TAR, ws, ctx.cmode);
        launch_cond_rows(st, STACK_TAR, B, ctx.Tc, E, e->X, e->ln_tar, nullptr, e->cond);
    }
    if (tr && tr->cond) HIPCHK(e, hipMemcpyAsync(tr->cond, e->cond, (size_t)kSeq * E * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipEventRecord(e->ev[2], st));
    if (ctx.fg_write) {   // the slot caches now hold slots 0 .. Tn-1 of this window: what the next frame must find unchanged (prefix_matches)
        umgen_engine::Prefix& px = e->px;
        px.B = B; px.P = Tn; px.Tfull = Tn + 1; px.has_ego = !io.ctrl_pose;
        px.pose.assign(io.pose, io.pose + (size_t)B * Tn * kNPose);
        px.map.assign(io.map, io.map + (size_t)B * Tn * kNMap);
        px.box.assign(io.box, io.box + (size_t)B * Tn * kNBox);
        px.img.assign(io.img, io.img + (size_t)B * Tn * kNImg);
        px.pose_next.assign(ctx.ego.begin(), ctx.ego.end());   // slot Tn-1 was evaluated with the new frame's pose (the shift of UMGen.py:1445-1452)
        px.valid = true;
    }
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
    e->stream = ctx.dec;
    launch_first_input(ctx.st, B, E, e->tb.tske + (long)e->cfg.task_id * E, e->cond, e->xdec);
    {   // tar_head_logits: logits_tar[b][k][:] = head_tar_bbox3d . cond[b][kBoxC0 + k][:]  (exact fp32 FMA chain, bf16 or fp32 weights)
        GemmArgs g{};
        g.P = e->head_tar_box; g.Q = e->cond + (long)kBoxC0 * E; g.Mi = e->cfg.bbox3d_vocab; g.Nj = kNBox; g.K = E; g.ldp = E; g.ldq = E;
        g.strideP = 0; g.strideQ = (long)kSeq * E; g.batch = B; g.mode = GEMM_STORE_F32; g.out = e->logits_tar; g.ldo = e->cfg.bbox3d_vocab;
        g.strideO = (long)kNBox * e->cfg.bbox3d_vocab;
        launch_gemm_valu<T, float>(ctx.st, g);
    }
    if (ctx.ov_active && io.next_follows) {
        const auto tp0 = std::chrono::steady_clock::now();
        if (int rc = launch_prefix_any(e, io, ctx.ego)) return rc;
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
        if (int rc = run_prefix_prefill_any(e, B, ctx.given_end)) return rc;
        ctx.j_begin = ctx.given_end - 1;
        ctx.s1.step = ctx.j_begin;
        HIPCHK(e, hipMemcpyAsync(e->d_state, &ctx.s1, sizeof(ctx.s1), hipMemcpyHostToDevice, st));
        for (int l = 0; l < ctx.n_lanes && ctx.n_lanes > 1; ++l) HIPCHK(e, hipMemcpyAsync(e->lane[l].st, &ctx.s1, sizeof(ctx.s1), hipMemcpyHostToDevice, st));
        e->tm.prefix_passes += 1;
    }
    return 0;
}

template <typename T>
void plan_decode_steps(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B;
    const umgen_trace* tr = io.trace;
    hipStream_t const st = ctx.st;
    ctx.steps_run = ctx.j_end - ctx.j_begin;             // decode steps of this frame (a prefix pass replaces the given positions' steps)
    ctx.graphs = e->cfg.use_graphs && !tr && !e->profiling;   // profiled frames time every decode step's layer kernel(s) with events
    ctx.batched = sizeof(T) == 2 && e->use_batched(B);       // the batched decode layer takes the step (oar_layers)
    ctx.wide = sizeof(T) == 2 && e->use_wide(B);           // the chip-wide engine of the wide layers: one launch per scene and step
    static const umgen_engine::EngStream wide_stream{true, 8, {}};
    ctx.eng = ctx.wide ? &wide_stream : ((sizeof(T) == 2 && !ctx.batched) ? e->eng_for(st) : nullptr);
    const int eng_ng = ctx.wide ? -3 : (ctx.eng ? ctx.eng->NG + (e->bg_engine && B == 1 ? 100 : 0) : (ctx.batched ? -2 : 0));     // the engine's grid depends on the stream's XCDs: graphs are per (B, NG)
    if (ctx.graphs && (e->step_graph_B != B || e->step_graph_NG != eng_ng)) {
        for (auto& row : e->step_graph)
            for (auto& g : row)
                if (g) { hipGraphExecDestroy(g); g = nullptr; }
        e->step_graph_B = B;
        e->step_graph_NG = eng_ng;
    }
}

int run_lane_loop(umgen_engine* e, const FrameIO& io, FrameCtx& ctx) {
    const int B = io.B, given_end = ctx.given_end, n_lanes = ctx.n_lanes, j_end = ctx.j_end;
    hipStream_t const st = ctx.st;
    // Decode lanes (umgen_engine::DecLane): fork behind the first input, every lane replays the step runs for its scenes on its own
    // stream, join before the token download.  Step runs are graphs in every mode but --no-graphs (a profiled frame times lane 0's
    // runs around the graph launches: eager launches of n lanes x 182 kernels per step would measure the host).
    auto kind_of = [given_end](int jj) {
        if (jj < given_end) return 0;
        return (jj >= kMapC0 && jj < kMapEos) ? 1 : (jj >= kBoxC0 && jj < kBoxEos) ? 2 : (jj >= kImgC0 && jj < kImgEos) ? 3 : 0;
    };
    const bool lane_graphs = e->cfg.use_graphs;
    if (e->lane_graph_B != B || e->lane_graph_n != n_lanes) {
        for (auto& ln : e->lane)
            for (auto& row : ln.graph)
                for (auto& g : row)
                    if (g) { hipGraphExecDestroy(g); g = nullptr; }
        e->lane_graph_B = B;
        e->lane_graph_n = n_lanes;
    }
    const DecView all = current_view(e);
    struct RestoreView { umgen_engine* e; DecView v; ~RestoreView() { apply_view(e, v); e->in_lanes = false; e->in_capture = false; } } restore_view{e, all};
    e->in_lanes = true;
    HIPCHK(e, hipEventRecord(e->ev_lane_fork, st));
    int b0s[umgen_engine::kMaxLanes], nbs[umgen_engine::kMaxLanes];
    for (int l = 0, b0 = 0; l < n_lanes; ++l) {
        nbs[l] = B / n_lanes + (l < B % n_lanes ? 1 : 0);
        b0s[l] = b0;
        b0 += nbs[l];
        HIPCHK(e, hipStreamWaitEvent(e->lane[l].s, e->ev_lane_fork, 0));
    }
    for (int j = ctx.j_begin; j < j_end; ++j) {
        const int mod = kind_of(j);
        int same = 1;
        while (same < 16 && j + same < j_end && kind_of(j + same) == mod) ++same;
        const int run = !lane_graphs ? 1 : (same >= 16 ? 16 : (same >= 4 ? 4 : 1));
        const int ri = run == 16 ? 2 : (run == 4 ? 1 : 0);
        for (int l = 0; l < n_lanes; ++l) {
            umgen_engine::DecLane& ln = e->lane[l];
            apply_view(e, lane_view(e, all, ln, b0s[l]));
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
                    e->in_capture = true;
                    int crc = 0;
                    for (int r = 0; r < run && !crc; ++r) crc = enqueue_step_any(e, nbs[l], mod, 1, nullptr, 0);
                    e->in_capture = false;
                    if (crc) return crc;   // (run_frame_any ends the open capture)
                    HIPCHK(e, hipStreamEndCapture(ln.s, &g));
                    HIPCHK(e, hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
                    HIPCHK(e, hipGraphDestroy(g));
                }
                HIPCHK(e, hipGraphLaunch(ge, ln.s));
            } else if (int rc = enqueue_step_any(e, nbs[l], mod, 1, nullptr, j)) {
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
    for (int j = j_begin; j < j_end; ++j) {   // the img-eos step (j = 2206) produces nothing that is consumed
        auto kind_of = [given_end](int jj) {
            if (jj < given_end) return 0;
            return (jj >= kMapC0 && jj < kMapEos) ? 1 : (jj >= kBoxC0 && jj < kBoxEos) ? 2 : (jj >= kImgC0 && jj < kImgEos) ? 3 : 0;
        };
        const int mod = kind_of(j);
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
                    if (kind_of(j + same) != mod) break;
                    ++same;
                }
                run = same >= 16 ? 16 : (same >= 4 ? 4 : 1);
            }
            hipGraphExec_t& ge = e->step_graph[mod][(eng || batched) ? (run == 16 ? 2 : (run == 4 ? 1 : 0)) : gkey];
            if (!ge) {
                hipGraph_t g;
                HIPCHK(e, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
                e->in_capture = true;
                int crc = 0;
                for (int r = 0; r < run && !crc; ++r) crc = enqueue_step_any(e, B, mod, ns, nullptr, 0);
                e->in_capture = false;
                if (crc) return crc;   // (run_frame_any ends the open capture)
                HIPCHK(e, hipStreamEndCapture(st, &g));
                HIPCHK(e, hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
                HIPCHK(e, hipGraphDestroy(g));
            }
            HIPCHK(e, hipGraphLaunch(ge, st));
            e->tm.oar_kernels += (int64_t)(run - 1) * ((eng ? (wide ? B : 1) : 5 * (int64_t)e->oar.size()) + (mod == 0 ? 1 : (mod == 2 ? 3 : 2)));
            j += run - 1;
        } else if (int rc = enqueue_step_any(e, B, mod, ns, tr, j)) {
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
    HIPCHK(e, hipMemcpyAsync(io.out_tokens, e->d_tokens, (size_t)B * kTokPerFrame * 4, hipMemcpyDeviceToHost, st));
    if (io.out_logp) HIPCHK(e, hipMemcpyAsync(io.out_logp, e->d_logp, (size_t)B * kTokPerFrame * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(ctx.counters, e->d_counters, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (eng) HIPCHK(e, hipMemcpyAsync(&ctx.eng_err, wide ? e->wide_err : e->eng_err, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    {
        const hipError_t le = e->launch_status != hipSuccess ? e->launch_status : hipGetLastError();
        e->launch_status = hipSuccess;
        if (le != hipSuccess) return e->fail(UMGEN_E_HIP, "a kernel launch of this frame was refused: %s", hipGetErrorString(le));
    }
    return 0;
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
    plan_decode_steps<T>(e, io, ctx);
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
    hipStream_t const fg = e->stream;   // the decode stream of overlapped rollouts (6 of the 8 XCDs when the overlap exists)
    e->launch_status = hipSuccess;
    (void)hipGetLastError();            // a stale error another HIP user of this thread left behind (torch, RCCL) is not this frame's
    struct RestoreStream { umgen_engine* e; hipStream_t s; ~RestoreStream() { e->stream = s; e->set_work(e->w_main); } } restore{e, fg};
    FrameCtx ctx{};
    ctx.fg = fg;
    ctx.st = fg;
    ctx.sp = SamplerParams{io.smp->method, io.smp->top_k, io.smp->top_k_map, io.smp->topk_image, io.smp->p, io.smp->p_map, io.smp->temperature,
                           io.smp->rule_constrain, io.smp->merge_ar_tar, io.smp->only_ar};
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
// only slot T - 1 the new frame's pose, so slots [0, T - 1) of the map / box / TAR stacks run on the B scenes in cache mode 1 and the branches push their last
// slot against their scene's caches (cache mode 5).  Every kernel's row arithmetic is that of run_frame, so the conditioning rows, and from begin_decode on the
// whole frame -- an ordinary frame of B * N scenes -- have the bits of run_frame on io.
// When the next frame's window is this one plus a slot (run_frame's fg_write rule) the slot caches must end up as run_frame's cache mode 3 leaves them for all
// B * N scenes: the ego stack fills the scenes' blocks in mode 3, the last-slot passes append every branch's own slot T - 1 to its own block (cache mode 6),
// and then every cache is spread -- block b*N + s receives slots [0, T - 1) ([0, T) of the ego stack) of scene block b, behind ALL reads of the scene blocks and
// scene by scene in descending b (tcache_spread_kernel states why) -- and px is filled for B * N scenes like run_stacks fills it.
template <typename T>
int run_frame_fan(umgen_engine* e, const FrameIO& io, int N) {
    const int E = e->E, BN = io.B, B = io.B / N, Tn = io.T, P = io.T - 1;
    hipStream_t const fg = e->stream;
    e->launch_status = hipSuccess;
    (void)hipGetLastError();
    struct RestoreStream { umgen_engine* e; hipStream_t s; ~RestoreStream() { e->stream = s; e->set_work(e->w_main); } } restore{e, fg};
    FrameCtx ctx{};
    ctx.fg = fg;
    ctx.st = fg;
    ctx.sp = SamplerParams{io.smp->method, io.smp->top_k, io.smp->top_k_map, io.smp->topk_image, io.smp->p, io.smp->p_map, io.smp->temperature,
                           io.smp->rule_constrain, io.smp->merge_ar_tar, io.smp->only_ar};
    e->px.valid = false;                 // the passes below overwrite the slot caches: nothing an earlier call left there covers this window
    if (int rc = settle_background_pass(e, io, ctx)) return rc;
    if (int rc = upload_frame_inputs(e, io, ctx)) return rc;      // seeds, counters and logp of the B * N branches; the token arrays follow below
    hipStream_t const st = ctx.st;
    // the scenes' windows [B][T][S_mod] (branch (b, 0) holds scene b's) for the passes that run once per scene
    const int S[4] = {kNPose, kNMap, kNBox, kNImg};
    const int* src[4] = {io.pose, io.map, io.box, io.img};
    int* dev[4] = {e->d_pose, e->d_map, e->d_box, e->d_img};
    std::vector<int> win[4], item_scene(BN), hshift;
    std::vector<float> hdiff;
    for (int m = 0; m < 4; ++m) {
        win[m].resize((size_t)B * Tn * S[m]);
        for (int b = 0; b < B; ++b)
            memcpy(&win[m][(size_t)b * Tn * S[m]], src[m] + (size_t)b * N * Tn * S[m], (size_t)Tn * S[m] * sizeof(int));
        HIPCHK(e, hipMemcpyAsync(dev[m], win[m].data(), win[m].size() * 4, hipMemcpyHostToDevice, st));
    }
    ctx.fg_write = !e->overlap && e->grow_cache && io.next_follows && io.cond_cap > 0 && Tn + 1 <= io.cond_cap && Tn + 1 <= e->cfg.max_cond_frames && ensure_tcache(e);
    ctx.t0 = 0; ctx.Tc = Tn; ctx.cmode = ctx.fg_write ? 3 : 0;
    // Step 1: the ego net once per scene, a pose per branch
    ctx.ego.resize((size_t)BN * 3);
    HIPCHK(e, hipEventRecord(e->ev[0], st));
    if (io.ctrl_pose) {
        for (int i = 0; i < BN * 3; ++i) ctx.ego[i] = io.ctrl_pose[i];
    } else {
        run_ego_fan_any(e, WindowTokens{e->d_pose, e->d_map, e->d_box, e->d_img, B, Tn, Tn, 0}, N, ctx.sp, io.frame_idx, ctx.cmode, io.out_logp ? e->d_logp : nullptr);
        HIPCHK(e, hipMemcpyAsync(ctx.ego.data(), e->d_ego_tok, (size_t)BN * 3 * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
    }
    HIPCHK(e, hipEventRecord(e->ev[1], st));
    if (int rc = init_decode_state<T>(e, io, ctx)) return rc;
    // Step 2a: slots [0, T - 1) of the three stacks once per scene, their temporal k | v rows into the scenes' blocks of the slot caches (slot T - 1 of the
    // shifted pose is not read)
    const std::vector<int> no_pose((size_t)B * 3, 0);
    decode_pose_shift(win[0].data(), no_pose.data(), B, Tn, hshift, hdiff);
    HIPCHK(e, hipMemcpyAsync(e->d_pose_shift, hshift.data(), hshift.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->pose_diff, hdiff.data(), hdiff.size() * 4, hipMemcpyHostToDevice, st));
    const WindowTokens wh{e->d_pose_shift, e->d_map, e->d_box, e->d_img, B, P, Tn, 0};
    run_stack_any(e, STACK_MAP, wh, 1);
    run_stack_any(e, STACK_BOX, wh, 1);
    run_stack_any(e, STACK_TAR, wh, 1);
    // Step 2b: slot T - 1 of every branch -- its own pose in the shift, its own window rows -- against its scene's caches, and the conditioning rows
    decode_pose_shift(io.pose, ctx.ego.data(), BN, Tn, ctx.pshift, ctx.pdiff);
    HIPCHK(e, hipMemcpyAsync(e->d_pose_shift, ctx.pshift.data(), ctx.pshift.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->pose_diff, ctx.pdiff.data(), ctx.pdiff.size() * 4, hipMemcpyHostToDevice, st));
    for (int m = 0; m < 4; ++m) HIPCHK(e, hipMemcpyAsync(dev[m], src[m], (size_t)BN * Tn * S[m] * 4, hipMemcpyHostToDevice, st));
    for (int i = 0; i < BN; ++i) item_scene[i] = i / N;
    HIPCHK(e, hipMemcpyAsync(e->d_item_scene, item_scene.data(), (size_t)BN * 4, hipMemcpyHostToDevice, st));
    e->fan_scenes = B;
    const int lmode = ctx.fg_write ? 6 : 5;
    const WindowTokens wl{e->d_pose_shift, e->d_map, e->d_box, e->d_img, BN, 1, Tn, P};
    run_stack_any(e, STACK_MAP, wl, lmode);
    launch_cond_rows(st, STACK_MAP, BN, 1, E, e->X, e->ln_map_tar, e->warped_last, e->cond);
    run_stack_any(e, STACK_BOX, wl, lmode);
    launch_cond_rows(st, STACK_BOX, BN, 1, E, e->X, e->ln_box_tar, nullptr, e->cond);
    run_stack_any(e, STACK_TAR, wl, lmode);
    launch_cond_rows(st, STACK_TAR, BN, 1, E, e->X, e->ln_tar, nullptr, e->cond);
    if (ctx.fg_write) {   // behind every read of the scene blocks: each branch's block gets its scene's slots; then the caches hold slots 0 .. T-1 of all B * N windows
        spread_tcaches(e, st, STACK_MAP, B, N, P);
        spread_tcaches(e, st, STACK_BOX, B, N, P);
        spread_tcaches(e, st, STACK_TAR, B, N, P);
        if (!io.ctrl_pose) spread_tcaches(e, st, STACK_EGO, B, N, Tn);
        umgen_engine::Prefix& px = e->px;
        px.B = BN; px.P = Tn; px.Tfull = Tn + 1; px.has_ego = !io.ctrl_pose;
        px.pose.assign(io.pose, io.pose + (size_t)BN * Tn * kNPose);
        px.map.assign(io.map, io.map + (size_t)BN * Tn * kNMap);
        px.box.assign(io.box, io.box + (size_t)BN * Tn * kNBox);
        px.img.assign(io.img, io.img + (size_t)BN * Tn * kNImg);
        px.pose_next.assign(ctx.ego.begin(), ctx.ego.end());
        px.valid = true;
    }
    HIPCHK(e, hipEventRecord(e->ev[2], st));
    return decode_and_finish<T>(e, io, ctx);      // Step 3 on: an ordinary frame of B * N scenes
}

// umgen_score: log p of a GIVEN next frame for B scenes (the reference's teacher-forced loss, UMGen.py:539-582), from run_frame's own stages.  The
// window, pose shift, map warp and conditioning rows are those of a teacher-forced frame; then all 2206 decode inputs of the frame go through
// the BlockOAR layers as ONE pass (run_prefix_prefill: the stacks' arithmetic contract) and the scoring head (score.hip) reads ln_oar . head
// off the rows of X: no decode step, no sampler, no RNG, no logit buffer.  The pass works in the stacks' workspaces and the decode cache, so
// nothing an earlier rollout left in the slot caches is trusted afterwards (px.valid).
// device buffers of umgen_score_detail, on its first call: engines that never ask keep their footprint
int ensure_score_detail(umgen_engine* e) {
    if (e->det_part) return 0;
    const size_t Bm = e->cfg.max_batch;
    void* got[7] = {};
    const size_t bytes[7] = {Bm * kNMap * 8 * kDetailRecFloats * 4, 4 * Bm * kNMap * 4, Bm * kTokPerFrame * 4, Bm * kTokPerFrame * 4,
                             Bm * kTokPerFrame * kScoreTopK * 4, Bm * kTokPerFrame * 4, Bm * kTokPerFrame * kScoreTopK * 4};      // (head_nll_nsplit <= 8)
    for (int i = 0; i < 7; ++i)
        if (hipMalloc(&got[i], bytes[i]) != hipSuccess) {
            (void)hipGetLastError();
            for (int k = 0; k < i; ++k) (void)hipFree(got[k]);
            return e->fail(UMGEN_E_NOMEM, "no device memory for the score-detail buffers (%zu bytes)", bytes[i]);
        }
    for (void* p : got) e->allocs.push_back(p);
    e->det_row = (float*)got[1]; e->det_mass = (float*)got[2]; e->det_ent = (float*)got[3]; e->det_tlp = (float*)got[4];
    e->det_rank = (int*)got[5]; e->det_tok = (int*)got[6];
    e->det_part = (float*)got[0];
    return 0;
}

// block b0 of the detail results: topk per row in the lists
ScoreDetailOut score_detail_out(const umgen_engine* e, const ScoreDetailIO* dt, long b0) {
    return ScoreDetailOut{e->det_rank + b0, e->det_mass + b0, e->det_ent + b0, e->det_tok + b0 * dt->topk, e->det_tlp + b0 * dt->topk, dt->topk,
                          1.0f / dt->temperature};
}

// where score_heads finds its targets and leaves its results when B may exceed max_batch (umgen_score_clip): d_tokens, score_part, score_logp, score_arg for B items
struct ScoreBufs { const int* tokens; float *part, *logp; int* arg; };

// the scoring head on the rows run_prefix_prefill left in X for B scenes (row j predicts the token at position j, targets in d_tokens): the map,
// bbox3d and image blocks of score_logp / score_arg, each [B][S_mod]; with dt the detail sweep of the same rows
template <typename T>
int score_heads(umgen_engine* e, hipStream_t st, int B, const ScoreDetailIO* dt, const ScoreBufs* sb = nullptr) {
    const int E = e->E;
    const int c0[3] = {kMapC0, kBoxC0, kImgC0}, n[3] = {kNMap, kNBox, kNImg}, off[3] = {kOffMap, kOffBox, kOffImg};
    const int V[3] = {e->cfg.map_vocab, e->cfg.bbox3d_vocab, e->cfg.img_vocab};
    const void* head[3] = {e->head_ar_map, e->head_ar_box, e->head_ar_img};
    for (int m = 0; m < 3; ++m) {
        HeadNllArgs a{};
        a.x = e->X + (long)c0[m] * E; a.ldx = E; a.rows_per_group = n[m]; a.group_stride = (long)(kSeq - 1) * E;
        a.ln_w = e->ln_oar; a.W = head[m]; a.V = V[m]; a.K = E; a.M = B * n[m];
        a.target = (sb ? sb->tokens : e->d_tokens) + off[m]; a.target_group_stride = kTokPerFrame;
        a.part = sb ? sb->part : e->score_part; a.logp = (sb ? sb->logp : e->score_logp) + (long)B * off[m];
        a.argmax = (sb ? sb->arg : e->score_arg) + (long)B * off[m];
        if (dt) {
            const long nr = (long)e->cfg.max_batch * kNMap;
            a.lse = e->det_row; a.tlogit = e->det_row + nr; a.rmax = e->det_row + 2 * nr; a.sumexp = e->det_row + 3 * nr;
        }
        HIPCHK(e, launch_head_nll<T>(st, a));
        if (dt) HIPCHK(e, launch_head_detail<T>(st, HeadDetailArgs{a, e->det_part, score_detail_out(e, dt, (long)B * off[m])}));
    }
    return 0;
}

template <typename T>
int run_score(umgen_engine* e, const ScoreIO& sc) {
    hipStream_t const fg = e->stream;
    e->launch_status = hipSuccess;
    (void)hipGetLastError();
    struct RestoreStream { umgen_engine* e; hipStream_t s; ~RestoreStream() { e->stream = s; e->set_work(e->w_main); } } restore{e, fg};
    const int B = sc.B;
    const ScoreDetailIO* dt = sc.detail;
    if (dt) { if (int rc = ensure_score_detail(e)) return rc; }
    // the ego net's sampler runs and is overridden by the given pose (run_ego's forced form): any valid parameters do
    static const umgen_sampling smp{UMGEN_SAMPLE_TOPK, 1, 1, 1, 1.f, 1.f, 1.f, 0, 0, 0, nullptr};
    const FrameIO io{B, sc.T, sc.pose, sc.map, sc.box, sc.img, nullptr, nullptr, 0, &smp, nullptr, nullptr};
    FrameCtx ctx{};
    ctx.fg = fg;
    ctx.st = fg;
    ctx.sp = SamplerParams{smp.method, smp.top_k, smp.top_k_map, smp.topk_image, smp.p, smp.p_map, smp.temperature, 0, 0, 0};
    e->px.valid = false;                 // (before the stage below asks whether an earlier pass covers this window: the score is always a whole-window pass)
    if (int rc = settle_background_pass(e, io, ctx)) return rc;
    hipStream_t const st = ctx.st;
    if (int rc = upload_frame_inputs(e, io, ctx)) return rc;
    HIPCHK(e, hipMemcpyAsync(e->d_forced, sc.next, (size_t)B * kTokPerFrame * 4, hipMemcpyHostToDevice, st));
    ctx.forced = true;                   // the ego net with the next pose forced: its logits stay in e->logits [3 B][pose_vocab]
    if (int rc = ego_and_pose_shift(e, io, ctx)) return rc;
    float* lp = e->score_logp;
    int* am = e->score_arg;
    launch_logits_nll(st, e->logits, e->cfg.pose_vocab, e->cfg.pose_vocab, 3 * B, e->d_forced, kNPose, kTokPerFrame, lp, am, nullptr, nullptr);
    if (dt) HIPCHK(e, launch_logits_detail(st, e->logits, e->cfg.pose_vocab, e->cfg.pose_vocab, 3 * B, e->d_forced, kNPose, kTokPerFrame, score_detail_out(e, dt, 0)));
    HIPCHK(e, hipMemcpyAsync(e->d_tokens, sc.next, (size_t)B * kTokPerFrame * 4, hipMemcpyHostToDevice, st));
    if (int rc = run_stacks(e, io, ctx)) return rc;
    if (int rc = run_prefix_prefill_any(e, B, kSeq)) return rc;      // rows 0 .. 2205 of every scene in X; row j predicts the token at position j
    if (int rc = score_heads<T>(e, st, B, dt)) return rc;
    HIPCHK(e, hipMemcpyAsync(sc.logp, lp, (size_t)B * kTokPerFrame * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(sc.argmax, am, (size_t)B * kTokPerFrame * 4, hipMemcpyDeviceToHost, st));
    if (dt) {
        const size_t n = (size_t)B * kTokPerFrame * 4;
        HIPCHK(e, hipMemcpyAsync(dt->rank, e->det_rank, n, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipMemcpyAsync(dt->mass_above, e->det_mass, n, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipMemcpyAsync(dt->entropy, e->det_ent, n, hipMemcpyDeviceToHost, st));
        if (dt->topk) {
            HIPCHK(e, hipMemcpyAsync(dt->topk_tok, e->det_tok, n * dt->topk, hipMemcpyDeviceToHost, st));
            HIPCHK(e, hipMemcpyAsync(dt->topk_logp, e->det_tlp, n * dt->topk, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(e, hipStreamSynchronize(st));
    const hipError_t le = e->launch_status != hipSuccess ? e->launch_status : hipGetLastError();
    e->launch_status = hipSuccess;
    if (le != hipSuccess) return e->fail(UMGEN_E_HIP, "a kernel launch of this scoring pass was refused: %s", hipGetErrorString(le));
    return 0;
}

// umgen_score_candidates: C given next frames per scene against one history.  Of run_score's work only the last history slot of the map / box / TAR
// stacks (the pose shift hands slot t the pose of frame t + 1, so slot T - 1 carries the candidate's pose), the conditioning rows, the BlockOAR pass and
// the heads depend on the candidate: the ego net (it reads the unshifted window) and slots [0, T - 1) of the three stacks run once per scene, the
// latter in cache mode 1 -- the pass launch_prefix records for the background, as stand-alone launches -- and the items (b, c), in chunks of at most
// max_batch, run their last slot against the scenes' slot caches (run_stack cache mode 5).  Every kernel's row arithmetic is that of run_score, so
// entry (b, c) has the bits of umgen_score on window b and candidate (b, c).  T == 1, slot caches that do not fit and UMGEN_SCORE_SHARE=0 take
// run_score itself on replicated windows, chunk by chunk.
template <typename T>
int run_score_candidates(umgen_engine* e, ScoreCandIO& sc) {
    const int E = e->E, B = sc.B, Tn = sc.T, C = sc.C, P = sc.T - 1, Bm = e->cfg.max_batch;
    const long N = (long)B * C;
    const int S[4] = {kNPose, kNMap, kNBox, kNImg}, off[4] = {0, kOffMap, kOffBox, kOffImg};
    const int* win[4] = {sc.pose, sc.map, sc.box, sc.img};
    const char* she = getenv("UMGEN_SCORE_SHARE");      // (read per call: the tests compare both forms in one process)
    const bool share = Tn >= 2 && !(she && she[0] == '0') && ensure_tcache(e);
    sc.shared_slots = share ? P : 0;
    // host staging of a chunk (the asynchronous copies read it until the chunk's synchronisation)
    std::vector<int> rep[4], cand_pose, item_scene, pshift, am;
    std::vector<float> pdiff, lp;
    auto replicate = [&](long i0, int n) {               // the windows of items [i0, i0 + n): [n][T][S_mod]
        for (int m = 0; m < 4; ++m) {
            rep[m].resize((size_t)n * Tn * S[m]);
            for (int i = 0; i < n; ++i)
                memcpy(&rep[m][(size_t)i * Tn * S[m]], win[m] + (size_t)((i0 + i) / C) * Tn * S[m], (size_t)Tn * S[m] * sizeof(int));
        }
    };
    auto copy_out = [&](long i0, int n) {                // the chunk's blocks pose | map | bbox3d | image, each [n][S_mod] -> [b][c][2199]
        for (int m = 0; m < 4; ++m)
            for (int i = 0; i < n; ++i) {
                memcpy(sc.logp + (size_t)(i0 + i) * kTokPerFrame + off[m], &lp[(size_t)n * off[m] + (size_t)i * S[m]], (size_t)S[m] * sizeof(float));
                memcpy(sc.argmax + (size_t)(i0 + i) * kTokPerFrame + off[m], &am[(size_t)n * off[m] + (size_t)i * S[m]], (size_t)S[m] * sizeof(int));
            }
    };
    if (!share) {
        for (long i0 = 0; i0 < N; i0 += Bm) {
            const int n = (int)std::min<long>(Bm, N - i0);
            replicate(i0, n);
            lp.resize((size_t)n * kTokPerFrame);
            am.resize((size_t)n * kTokPerFrame);
            const ScoreIO one{n, Tn, rep[0].data(), rep[1].data(), rep[2].data(), rep[3].data(), sc.next + (size_t)i0 * kTokPerFrame, lp.data(), am.data()};
            if (int rc = run_score<T>(e, one)) return rc;
            copy_out(i0, n);
        }
        return 0;
    }
    hipStream_t const fg = e->stream;
    e->launch_status = hipSuccess;
    (void)hipGetLastError();
    struct RestoreStream { umgen_engine* e; hipStream_t s; ~RestoreStream() { e->stream = s; e->set_work(e->w_main); } } restore{e, fg};
    // the ego net's sampler runs and its tokens are not used: any valid parameters do
    static const umgen_sampling smp{UMGEN_SAMPLE_TOPK, 1, 1, 1, 1.f, 1.f, 1.f, 0, 0, 0, nullptr};
    const FrameIO io{B, Tn, sc.pose, sc.map, sc.box, sc.img, nullptr, nullptr, 0, &smp, nullptr, nullptr};
    FrameCtx ctx{};
    ctx.fg = fg;
    ctx.st = fg;
    ctx.sp = SamplerParams{smp.method, smp.top_k, smp.top_k_map, smp.topk_image, smp.p, smp.p_map, smp.temperature, 0, 0, 0};
    e->px.valid = false;                 // the passes below overwrite the slot caches and the stacks' workspaces
    if (int rc = settle_background_pass(e, io, ctx)) return rc;
    hipStream_t const st = ctx.st;
    if (int rc = upload_frame_inputs(e, io, ctx)) return rc;
    // a profiled call (umgen_set_profiling) drains the stream at every stage boundary and books host time: ego_ms the ego net, tar_ms the history pass and
    // the items' last-slot passes, oar_ms the BlockOAR pass and the heads
    auto t_last = std::chrono::steady_clock::now();
    auto stage = [&](double& acc) {
        if (!e->profiling) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - t_last).count();
        acc += ms;
        e->tm.total_ms += ms;
        t_last = now;
    };
    double uploads_ms = 0;               // (in total_ms only)
    stage(uploads_ms);
    // once per scene: the ego net on the whole window (its three head_ego rows stay in e->logits [3 B][pose_vocab]) ...
    run_ego_any(e, WindowTokens{e->d_pose, e->d_map, e->d_box, e->d_img, B, Tn, Tn, 0}, ctx.sp, 0, false, nullptr, 0);
    stage(e->tm.ego_ms);
    // ... and slots [0, T - 1) of the three stacks, their temporal k | v rows into the slot caches (slot T - 1 of the shifted pose is not read)
    const std::vector<int> no_pose((size_t)B * 3, 0);
    decode_pose_shift(sc.pose, no_pose.data(), B, Tn, ctx.pshift, ctx.pdiff);
    HIPCHK(e, hipMemcpyAsync(e->d_pose_shift, ctx.pshift.data(), ctx.pshift.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->pose_diff, ctx.pdiff.data(), ctx.pdiff.size() * 4, hipMemcpyHostToDevice, st));
    const WindowTokens wh{e->d_pose_shift, e->d_map, e->d_box, e->d_img, B, P, Tn, 0};
    run_stack_any(e, STACK_MAP, wh, 1);
    run_stack_any(e, STACK_BOX, wh, 1);
    run_stack_any(e, STACK_TAR, wh, 1);
    stage(e->tm.tar_ms);
    e->fan_scenes = B;
    for (long i0 = 0; i0 < N; i0 += Bm) {
        const int n = (int)std::min<long>(Bm, N - i0);
        const int* next = sc.next + (size_t)i0 * kTokPerFrame;
        replicate(i0, n);
        cand_pose.resize((size_t)n * 3);
        item_scene.resize(n);
        for (int i = 0; i < n; ++i) {
            item_scene[i] = (int)((i0 + i) / C);
            for (int a = 0; a < 3; ++a) cand_pose[(size_t)i * 3 + a] = next[(size_t)i * kTokPerFrame + a];
        }
        decode_pose_shift(rep[0].data(), cand_pose.data(), n, Tn, pshift, pdiff);      // slot T - 1 of item (b, c): the candidate's pose
        HIPCHK(e, hipMemcpyAsync(e->d_pose_shift, pshift.data(), pshift.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(e->pose_diff, pdiff.data(), pdiff.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(e->d_map, rep[1].data(), rep[1].size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(e->d_box, rep[2].data(), rep[2].size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(e->d_img, rep[3].data(), rep[3].size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(e->d_item_scene, item_scene.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(e->d_tokens, next, (size_t)n * kTokPerFrame * 4, hipMemcpyHostToDevice, st));
        // a candidate's pose: a lookup in its scene's rows (the bits depend on the row and the target only)
        for (int i = 0; i < n; ++i)
            launch_logits_nll(st, e->logits + (long)item_scene[i] * 3 * e->cfg.pose_vocab, e->cfg.pose_vocab, e->cfg.pose_vocab, 3, e->d_tokens + (long)i * kTokPerFrame,
                              kNPose, kTokPerFrame, e->score_logp + (long)i * 3, e->score_arg + (long)i * 3, nullptr, nullptr);
        const WindowTokens wl{e->d_pose_shift, e->d_map, e->d_box, e->d_img, n, 1, Tn, P};
        run_stack_any(e, STACK_MAP, wl, 5);
        launch_cond_rows(st, STACK_MAP, n, 1, E, e->X, e->ln_map_tar, e->warped_last, e->cond);
        run_stack_any(e, STACK_BOX, wl, 5);
        launch_cond_rows(st, STACK_BOX, n, 1, E, e->X, e->ln_box_tar, nullptr, e->cond);
        run_stack_any(e, STACK_TAR, wl, 5);
        launch_cond_rows(st, STACK_TAR, n, 1, E, e->X, e->ln_tar, nullptr, e->cond);
        stage(e->tm.tar_ms);
        if (int rc = run_prefix_prefill_any(e, n, kSeq)) return rc;
        if (int rc = score_heads<T>(e, st, n, nullptr)) return rc;
        lp.resize((size_t)n * kTokPerFrame);
        am.resize((size_t)n * kTokPerFrame);
        HIPCHK(e, hipMemcpyAsync(lp.data(), e->score_logp, (size_t)n * kTokPerFrame * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipMemcpyAsync(am.data(), e->score_arg, (size_t)n * kTokPerFrame * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
        stage(e->tm.oar_ms);
        copy_out(i0, n);
    }
    if (e->profiling) fold_launch_events(e);
    const hipError_t le = e->launch_status != hipSuccess ? e->launch_status : hipGetLastError();
    e->launch_status = hipSuccess;
    if (le != hipSuccess) return e->fail(UMGEN_E_HIP, "a kernel launch of this scoring pass was refused: %s", hipGetErrorString(le));
    return 0;
}

// device buffers of umgen_score_clip's shared pass, on its first call (like ensure_score_detail); no room is not an error: the call takes the per-frame path
bool ensure_score_clip(umgen_engine* e) {
    if (e->clip_state) return e->clip_state > 0;
    const size_t N = (size_t)e->cfg.max_batch * e->cfg.max_cond_frames, E = (size_t)e->E;
    void* got[9] = {};
    const size_t bytes[9] = {N * 2 * 4, N * 4, N * kTokPerFrame * 4, N * kTokPerFrame * 4, N * kNMap * E * 4, N * kSeq * E * 4, N * E * 4,
                             N * kNMap * 8 * 16, N * kTokPerFrame * 4};      // (head_nll_nsplit <= 8, records of 16 bytes)
    for (int i = 0; i < 9; ++i)
        if (hipMalloc(&got[i], bytes[i]) != hipSuccess) {
            (void)hipGetLastError();
            for (int k = 0; k < i; ++k) (void)hipFree(got[k]);
            e->clip_state = -1;
            return false;
        }
    for (void* p : got) e->allocs.push_back(p);
    e->clip_items = (int*)got[0]; e->clip_item_T = (int*)got[1]; e->clip_tokens = (int*)got[2]; e->clip_arg = (int*)got[3];
    e->clip_warped = (float*)got[4]; e->clip_cond = (float*)got[5]; e->clip_xlast = (float*)got[6]; e->clip_part = (float*)got[7]; e->clip_logp = (float*)got[8];
    e->clip_state = 1;
    return true;
}

const int kModLen[4] = {kNPose, kNMap, kNBox, kNImg}, kModOff[4] = {0, kOffMap, kOffBox, kOffImg};

// frame f of clip b as one [2199] row pose | map | bbox3d | image
void clip_frame_row(const ScoreClipIO& sc, int b, int f, int* dst) {
    const int* src[4] = {sc.pose, sc.map, sc.box, sc.img};
    for (int m = 0; m < 4; ++m) memcpy(dst + kModOff[m], src[m] + ((size_t)b * sc.L + f) * kModLen[m], (size_t)kModLen[m] * sizeof(int));
}
// blocks pose | map | bbox3d | image, each [n][S_mod], of n items -> item i to frame fr[i] of clip sc[i] in [B][L - T_in][2199]
void clip_scatter(const ScoreClipIO& sc, int n, const float* lp, const int* am, const int* item_b, const int* item_f) {
    const int F = sc.L - sc.T_in;
    for (int m = 0; m < 4; ++m)
        for (int i = 0; i < n; ++i) {
            const size_t dst = ((size_t)item_b[i] * F + (item_f[i] - sc.T_in)) * kTokPerFrame + kModOff[m], src = (size_t)n * kModOff[m] + (size_t)i * kModLen[m];
            memcpy(sc.logp + dst, lp + src, (size_t)kModLen[m] * sizeof(float));
            memcpy(sc.argmax + dst, am + src, (size_t)kModLen[m] * sizeof(int));
        }
}

// frames [f0, f1) of every clip, each against its own window: run_score on items (f, b), in chunks of at most max_batch items of one window length
template <typename T>
int score_clip_frames(umgen_engine* e, const ScoreClipIO& sc, int f0, int f1) {
    const int B = sc.B, Bm = e->cfg.max_batch;
    const int* src[4] = {sc.pose, sc.map, sc.box, sc.img};
    std::vector<int> win[4], next, am, ib, itf;
    std::vector<float> lp;
    const long N = (long)(f1 - f0) * B;
    for (long i0 = 0; i0 < N;) {
        const int Tn = std::min(f0 + (int)(i0 / B), sc.cond);
        int n = 0;
        while (n < Bm && i0 + n < N && std::min(f0 + (int)((i0 + n) / B), sc.cond) == Tn) ++n;
        ib.resize(n); itf.resize(n);
        next.resize((size_t)n * kTokPerFrame);
        for (int m = 0; m < 4; ++m) win[m].resize((size_t)n * Tn * kModLen[m]);
        for (int i = 0; i < n; ++i) {
            const int f = f0 + (int)((i0 + i) / B), b = (int)((i0 + i) % B);
            ib[i] = b; itf[i] = f;
            for (int m = 0; m < 4; ++m)
                memcpy(&win[m][(size_t)i * Tn * kModLen[m]], src[m] + ((size_t)b * sc.L + (f - Tn)) * kModLen[m], (size_t)Tn * kModLen[m] * sizeof(int));
            clip_frame_row(sc, b, f, &next[(size_t)i * kTokPerFrame]);
        }
        lp.resize((size_t)n * kTokPerFrame);
        am.resize((size_t)n * kTokPerFrame);
        const ScoreIO one{n, Tn, win[0].data(), win[1].data(), win[2].data(), win[3].data(), next.data(), lp.data(), am.data()};
        if (int rc = run_score<T>(e, one)) return rc;
        clip_scatter(sc, n, lp.data(), am.data(), ib.data(), itf.data());
        i0 += n;
    }
    return 0;
}

// The growing group of umgen_score_clip: frames f in [T_in, P], P = min(L - 1, cond), whose windows [0, f) all start at frame 0.  Slot t of a window uses tpe[t]
// whatever the window's length, the pose shift hands it the pose of frame t + 1, the spatial sub-blocks, LayerNorms and MLPs are frame-local and the temporal
// attention is causal: slot f - 1 of ONE pass over [0, P) with every block on every slot is the last slot of umgen_score's pass over [0, f).  So the four stacks
// run once, the ego decoder, the conditioning rows, the BlockOAR pass and the heads on the B * G items (b, slot), G = P - T_in + 1 -- the kernels and the row
// arithmetic of run_score, launched over other row sets.
template <typename T>
int score_clip_shared(umgen_engine* e, const ScoreClipIO& sc, int P, int G) {
    const int E = e->E, B = sc.B, L = sc.L, Bm = e->cfg.max_batch, n = B * G, pv = e->cfg.pose_vocab;
    hipStream_t const fg = e->stream;
    e->launch_status = hipSuccess;
    (void)hipGetLastError();
    struct RestoreStream { umgen_engine* e; hipStream_t s; ~RestoreStream() { e->stream = s; e->set_work(e->w_main); } } restore{e, fg};
    // the window [0, P) of every clip, [B][P][S_mod], and frame P's pose, which the shift hands to slot P - 1
    const int* src[4] = {sc.pose, sc.map, sc.box, sc.img};
    std::vector<int> win[4], pose_P((size_t)B * 3), items((size_t)n * 2), item_T(n), item_b(n), item_f(n), next((size_t)n * kTokPerFrame);
    for (int m = 0; m < 4; ++m) {
        win[m].resize((size_t)B * P * kModLen[m]);
        for (int b = 0; b < B; ++b) memcpy(&win[m][(size_t)b * P * kModLen[m]], src[m] + (size_t)b * L * kModLen[m], (size_t)P * kModLen[m] * sizeof(int));
    }
    for (int b = 0; b < B; ++b) {
        memcpy(&pose_P[(size_t)b * 3], sc.pose + ((size_t)b * L + P) * 3, 3 * sizeof(int));
        for (int g = 0; g < G; ++g) {      // item (b, g): slot t = T_in - 1 + g scores frame t + 1
            const int i = b * G + g, t = sc.T_in - 1 + g;
            items[2 * i] = b; items[2 * i + 1] = t; item_T[i] = t + 1; item_b[i] = b; item_f[i] = t + 1;
            clip_frame_row(sc, b, t + 1, &next[(size_t)i * kTokPerFrame]);
        }
    }
    static const umgen_sampling smp{UMGEN_SAMPLE_TOPK, 1, 1, 1, 1.f, 1.f, 1.f, 0, 0, 0, nullptr};      // (upload_frame_inputs reads the seeds pointer)
    const FrameIO io{B, P, win[0].data(), win[1].data(), win[2].data(), win[3].data(), nullptr, nullptr, 0, &smp, nullptr, nullptr};
    FrameCtx ctx{};
    ctx.fg = fg;
    ctx.st = fg;
    e->px.valid = false;                 // the passes below overwrite the stacks' workspaces; nothing of them is for a later rollout
    if (int rc = settle_background_pass(e, io, ctx)) return rc;
    hipStream_t const st = ctx.st;
    if (int rc = upload_frame_inputs(e, io, ctx)) return rc;
    HIPCHK(e, hipMemcpyAsync(e->clip_items, items.data(), items.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->clip_item_T, item_T.data(), item_T.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->clip_tokens, next.data(), next.size() * 4, hipMemcpyHostToDevice, st));
    // a profiled call drains the stream at every stage boundary and books host time, like run_score_candidates: ego_ms the ego stack and decoder, tar_ms the
    // three stacks and the conditioning rows, oar_ms the BlockOAR pass and the heads
    auto t_last = std::chrono::steady_clock::now();
    auto stage = [&](double& acc) {
        if (!e->profiling) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - t_last).count();
        acc += ms;
        e->tm.total_ms += ms;
        t_last = now;
    };
    double uploads_ms = 0;               // (in total_ms only)
    stage(uploads_ms);
    // the ego stack over [0, P), every block on every slot; the decoder and head_ego on the items, in chunks that fit the 3 * max_batch-row buffers
    run_stack_any(e, STACK_EGO, WindowTokens{e->d_pose, e->d_map, e->d_box, e->d_img, B, P, P, 0}, 0, TAIL_NONE);
    std::vector<long> frame_of(Bm);
    for (int i0 = 0; i0 < n; i0 += Bm) {
        const int nc = std::min(Bm, n - i0);
        for (int i = 0; i < nc; ++i) frame_of[i] = (long)items[2 * (i0 + i)] * P + items[2 * (i0 + i) + 1];
        ego_decoder_any(e, nc, frame_of.data(), 0, e->clip_item_T + i0);
        launch_logits_nll(st, e->logits, pv, pv, 3 * nc, e->clip_tokens + (long)i0 * kTokPerFrame, kNPose, kTokPerFrame, e->clip_logp + (long)i0 * 3,
                          e->clip_arg + (long)i0 * 3, nullptr, nullptr);
    }
    stage(e->tm.ego_ms);
    // one pose shift for the window: slot t carries the pose of frame t + 1, slot P - 1 that of frame P
    decode_pose_shift(win[0].data(), pose_P.data(), B, P, ctx.pshift, ctx.pdiff);
    HIPCHK(e, hipMemcpyAsync(e->d_pose_shift, ctx.pshift.data(), ctx.pshift.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->pose_diff, ctx.pdiff.data(), ctx.pdiff.size() * 4, hipMemcpyHostToDevice, st));
    const WindowTokens ws{e->d_pose_shift, e->d_map, e->d_box, e->d_img, B, P, P, 0};
    run_stack_any(e, STACK_MAP, ws, 0, TAIL_NONE, e->clip_warped);
    launch_cond_rows_slots(st, STACK_MAP, P, E, e->X, e->ln_map_tar, e->clip_warped, e->clip_items, n, e->clip_cond);
    run_stack_any(e, STACK_BOX, ws, 0, TAIL_NONE);
    launch_cond_rows_slots(st, STACK_BOX, P, E, e->X, e->ln_box_tar, nullptr, e->clip_items, n, e->clip_cond);
    run_stack_any(e, STACK_TAR, ws, 0, TAIL_NONE);
    launch_cond_rows_slots(st, STACK_TAR, P, E, e->X, e->ln_tar, nullptr, e->clip_items, n, e->clip_cond);
    stage(e->tm.tar_ms);
    // one BlockOAR pass and one head sweep for all items (n <= max_batch * max_cond_frames: the rows the stacks' workspaces hold)
    const PrefillSrc ps{e->clip_cond, e->clip_tokens, e->clip_xlast, true};
    if (int rc = run_prefix_prefill_any(e, n, kSeq, &ps)) return rc;
    const ScoreBufs sb{e->clip_tokens, e->clip_part, e->clip_logp, e->clip_arg};
    if (int rc = score_heads<T>(e, st, n, nullptr, &sb)) return rc;
    std::vector<float> lp((size_t)n * kTokPerFrame);
    std::vector<int> am((size_t)n * kTokPerFrame);
    HIPCHK(e, hipMemcpyAsync(lp.data(), e->clip_logp, lp.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(am.data(), e->clip_arg, am.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    stage(e->tm.oar_ms);
    if (e->profiling) fold_launch_events(e);
    const hipError_t le = e->launch_status != hipSuccess ? e->launch_status : hipGetLastError();
    e->launch_status = hipSuccess;
    if (le != hipSuccess) return e->fail(UMGEN_E_HIP, "a kernel launch of this scoring pass was refused: %s", hipGetErrorString(le));
    clip_scatter(sc, n, lp.data(), am.data(), item_b.data(), item_f.data());
    return 0;
}

// umgen_score_clip: every frame f in [T_in, L) of B recorded clips against the min(f, cond) frames before it (umgen_rollout's window rule, teacher-forced).
// The frames whose window still starts at frame 0 share one pass (score_clip_shared) when there are at least two of them; the frames behind them, whose
// windows slide -- every slot's tpe row changes from frame to frame -- and everything when nothing is shared (UMGEN_SCORE_CLIP_SHARE=0, no room for the clip
// buffers) are run_score itself.  Either way entry (b, f) has the bits of umgen_score on its own window.
template <typename T>
int run_score_clip(umgen_engine* e, ScoreClipIO& sc) {
    const int P = std::min(sc.L - 1, sc.cond), G = std::max(0, P - sc.T_in + 1);
    const char* she = getenv("UMGEN_SCORE_CLIP_SHARE");      // (read per call: the tests compare both forms in one process)
    const bool share = G >= 2 && !(she && she[0] == '0') && ensure_score_clip(e);
    sc.shared_frames = share ? G : 0;
    if (!share) return score_clip_frames<T>(e, sc, sc.T_in, sc.L);
    if (int rc = score_clip_shared<T>(e, sc, P, G)) return rc;
    return score_clip_frames<T>(e, sc, P + 1, sc.L);
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

}  // namespace

namespace umgen {

int run_score_any(umgen_engine* e, const ScoreIO& sc) {
    const int rc = e->cfg.precision == UMGEN_PREC_BF16 ? run_score<bf16_t>(e, sc)
                 : e->cfg.precision == UMGEN_PREC_FP16 ? run_score<f16_t>(e, sc) : run_score<float>(e, sc);
    if (rc != UMGEN_OK) drain_failed_frame(e);
    return rc;
}

int run_score_candidates_any(umgen_engine* e, ScoreCandIO& sc) {
    const int rc = e->cfg.precision == UMGEN_PREC_BF16 ? run_score_candidates<bf16_t>(e, sc)
                 : e->cfg.precision == UMGEN_PREC_FP16 ? run_score_candidates<f16_t>(e, sc) : run_score_candidates<float>(e, sc);
    if (rc != UMGEN_OK) drain_failed_frame(e);
    return rc;
}

int run_score_clip_any(umgen_engine* e, ScoreClipIO& sc) {
    const int rc = e->cfg.precision == UMGEN_PREC_BF16 ? run_score_clip<bf16_t>(e, sc)
                 : e->cfg.precision == UMGEN_PREC_FP16 ? run_score_clip<f16_t>(e, sc) : run_score_clip<float>(e, sc);
    if (rc != UMGEN_OK) drain_failed_frame(e);
    return rc;
}

int run_frame_any(umgen_engine* e, const FrameIO& io) {
    const int rc = e->cfg.precision == UMGEN_PREC_BF16 ? run_frame<bf16_t>(e, io)
                 : e->cfg.precision == UMGEN_PREC_FP16 ? run_frame<f16_t>(e, io) : run_frame<float>(e, io);
    if (rc != UMGEN_OK) drain_failed_frame(e);
    return rc;
}

int run_frame_fan_any(umgen_engine* e, const FrameIO& io, int N) {
    const int rc = e->cfg.precision == UMGEN_PREC_BF16 ? run_frame_fan<bf16_t>(e, io, N)
                 : e->cfg.precision == UMGEN_PREC_FP16 ? run_frame_fan<f16_t>(e, io, N) : run_frame_fan<float>(e, io, N);
    if (rc != UMGEN_OK) drain_failed_frame(e);
    return rc;
}

}  // namespace umgen
