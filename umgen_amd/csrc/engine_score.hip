// Scoring given frames, from run_frame's own stages (engine_frame.h): run_score<T>, the pass of umgen_score and umgen_score_detail, run_score_candidates<T>,
// which scores several next frames per scene on one pass over the history, run_score_futures<T>, which does so for futures of several frames (item tails
// behind the shared slots), run_score_clip<T>, which scores every frame of a recorded clip, the growing windows off one pass, and run_score_any /
// run_score_candidates_any / run_score_futures_any / run_score_clip_any, which pick the precision and clean up behind a failed call.  Every pass cuts
// its items' windows out of the call's TokenView with gather_windows / copy_frames and packs the scored frames with frame_rows (token_windows.h) into
// staging that lives until the chunk's synchronisation, and uploads it with upload_tokens (engine_frame.h).
#include "engine_frame.h"

// host arithmetic stays unfused in every engine file, as it was while they were one file behind the numpy-faithful helpers (engine_weights.hip)
#pragma clang fp contract(off)

namespace {

// A scoring pass samples nothing: where the ego net runs, its sampler's token is overridden by the given pose (run_ego's forced form) or not used, so any
// valid parameters do (upload_frame_inputs reads the seeds pointer)
const umgen_sampling kNoSampling{UMGEN_SAMPLE_TOPK, 1, 1, 1, 1.f, 1.f, 1.f, 0, 0, 0, nullptr};

// A profiled call (umgen_set_profiling) of the shared-history passes drains the stream at every stage boundary and books host time: ego_ms the ego net,
// tar_ms the history pass, the last-slot passes and the conditioning rows, oar_ms the BlockOAR pass and the heads; acc == nullptr: in total_ms only
struct StageClock {
    umgen_engine* e;
    hipStream_t st;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void stage(double* acc) {
        if (!e->profiling) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - last).count();
        if (acc) *acc += ms;
        e->tm.total_ms += ms;
        last = now;
    }
};

// A chunk's results -- blocks pose | map | bbox3d | image, each [n][S_mod] with `per` values per position -- to their rows of the per-modality
// destinations: item i to row row0 + i (one copy per block), or to row rows[i] when rows is given
template <typename V>
void scatter_blocks(V* const dst[4], int n, const V* blocks, long row0, const long* rows = nullptr, int per = 1) {
    for (int m = 0; m < 4; ++m) {
        if (!dst[m]) continue;
        const size_t len = (size_t)kModLen[m] * per;
        const V* src = blocks + (size_t)n * kModOff[m] * per;
        if (!rows) memcpy(dst[m] + row0 * len, src, n * len * sizeof(V));
        else for (int i = 0; i < n; ++i) memcpy(dst[m] + rows[i] * len, src + i * len, len * sizeof(V));
    }
}

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
        a.x = e->w_main.X + (long)c0[m] * E; a.ldx = E; a.rows_per_group = n[m]; a.group_stride = (long)(kSeq - 1) * E;
        a.ln_w = e->ln_oar; a.W = head[m]; a.V = V[m]; a.K = E; a.M = B * n[m];
        a.target = (sb ? sb->tokens : e->dv.d_tokens) + off[m]; a.target_group_stride = kTokPerFrame;
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

// umgen_score: log p of a GIVEN next frame for B scenes (the reference's teacher-forced loss, UMGen.py:539-582), from run_frame's own stages.  The
// window, pose shift, map warp and conditioning rows are those of a teacher-forced frame; then all 2206 decode inputs of the frame go through
// the BlockOAR layers as ONE pass (run_prefix_prefill: the stacks' arithmetic contract) and the scoring head (score.hip) reads ln_oar . head
// off the rows of X: no decode step, no sampler, no RNG, no logit buffer.  The pass works in the stacks' workspaces and the decode cache, so
// nothing an earlier rollout left in the slot caches is trusted afterwards (px.valid).
template <typename T>
int run_score(umgen_engine* e, const ScoreIO& sc) {
    if (sc.detail && sc.rows) return e->fail(UMGEN_E_INVALID, "score detail with scattered rows");      // the detail destinations take rows row0 + b only
    FrameCtx ctx = begin_call(e, kNoSampling);
    const int B = sc.B;
    const size_t rows = (size_t)B * kTokPerFrame;
    const ScoreDetailIO* dt = sc.detail;
    if (dt) { if (int rc = ensure_score_detail(e)) return rc; }
    const FrameIO io{B, sc.T, sc.win, nullptr, nullptr, 0, &kNoSampling, nullptr, nullptr};
    e->px.valid = false;                 // (before the stage below asks whether an earlier pass covers this window: the score is always a whole-window pass)
    if (int rc = settle_background_pass(e, io, ctx)) return rc;
    hipStream_t const st = ctx.st;
    const Place pl{st, &e->w_main};      // every pass of a scoring call: one stream, the main workspaces
    if (int rc = upload_frame_inputs(e, io, ctx)) return rc;
    HIPCHK(e, hipMemcpyAsync(e->d_forced, sc.next, rows * 4, hipMemcpyHostToDevice, st));
    ctx.forced = true;                   // the ego net with the next pose forced: its logits stay in e->dv.logits [3 B][pose_vocab]
    if (int rc = ego_and_pose_shift(e, io, ctx)) return rc;
    launch_logits_nll(st, e->dv.logits, e->cfg.pose_vocab, e->cfg.pose_vocab, 3 * B, e->d_forced, kNPose, kTokPerFrame, e->score_logp, e->score_arg, nullptr, nullptr);
    if (dt) HIPCHK(e, launch_logits_detail(st, e->dv.logits, e->cfg.pose_vocab, e->cfg.pose_vocab, 3 * B, e->d_forced, kNPose, kTokPerFrame, score_detail_out(e, dt, 0)));
    HIPCHK(e, hipMemcpyAsync(e->dv.d_tokens, sc.next, rows * 4, hipMemcpyHostToDevice, st));
    if (int rc = run_stacks(e, io, ctx)) return rc;
    if (int rc = run_prefix_prefill_any(e, pl, B, kSeq)) return rc;      // rows 0 .. 2205 of every scene in X; row j predicts the token at position j
    if (int rc = score_heads<T>(e, st, B, dt)) return rc;
    // the device's blocks pose | map | bbox3d | image, each [B][S_mod], and behind the synchronisation block by block to the caller's rows
    std::vector<float> lp(rows), mass(dt ? rows : 0), ent(dt ? rows : 0), tlp(dt ? rows * dt->topk : 0);
    std::vector<int> am(rows), rank(dt ? rows : 0), tok(dt ? rows * dt->topk : 0);
    HIPCHK(e, hipMemcpyAsync(lp.data(), e->score_logp, rows * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(am.data(), e->score_arg, rows * 4, hipMemcpyDeviceToHost, st));
    if (dt) {
        HIPCHK(e, hipMemcpyAsync(rank.data(), e->det_rank, rows * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipMemcpyAsync(mass.data(), e->det_mass, rows * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipMemcpyAsync(ent.data(), e->det_ent, rows * 4, hipMemcpyDeviceToHost, st));
        if (dt->topk) {
            HIPCHK(e, hipMemcpyAsync(tok.data(), e->det_tok, rows * 4 * dt->topk, hipMemcpyDeviceToHost, st));
            HIPCHK(e, hipMemcpyAsync(tlp.data(), e->det_tlp, rows * 4 * dt->topk, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(e, hipStreamSynchronize(st));
    if (int rc = finish_call(e, "scoring pass")) return rc;
    scatter_blocks(sc.out.logp, B, lp.data(), sc.row0, sc.rows);
    scatter_blocks(sc.out.argmax, B, am.data(), sc.row0, sc.rows);
    if (dt) {      // (rows row0 + b: checked at entry)
        scatter_blocks(dt->rank, B, rank.data(), sc.row0);
        scatter_blocks(dt->mass_above, B, mass.data(), sc.row0);
        scatter_blocks(dt->entropy, B, ent.data(), sc.row0);
        if (dt->topk) {
            scatter_blocks(dt->topk_tok, B, tok.data(), sc.row0, nullptr, dt->topk);
            scatter_blocks(dt->topk_logp, B, tlp.data(), sc.row0, nullptr, dt->topk);
        }
    }
    return 0;
}

// umgen_score_candidates: C given next frames per scene against one history.  Of run_score's work only the last history slot of the map / box / TAR
// stacks (the pose shift hands slot t the pose of frame t + 1, so slot T - 1 carries the candidate's pose), the conditioning rows, the BlockOAR pass and
// the heads depend on the candidate: the ego net (it reads the unshifted window) and slots [0, T - 1) of the three stacks run once per scene
// (history_slots_once: the pass launch_prefix records for the background, as stand-alone launches) and the items (b, c), in chunks of at most
// max_batch, run their last slot against the scenes' slot caches (CACHE_SHARED_ITEMS).  Every kernel's row arithmetic is that of run_score, so
// entry (b, c) has the bits of umgen_score on window b and candidate (b, c).  T == 1, slot caches that do not fit and UMGEN_SCORE_SHARE=0 take
// run_score itself on replicated windows, chunk by chunk.
template <typename T>
int run_score_candidates(umgen_engine* e, ScoreCandIO& sc) {
    const int B = sc.B, Tn = sc.T, C = sc.C, P = sc.T - 1, Bm = e->cfg.max_batch;
    const long N = (long)B * C;
    const char* she = getenv("UMGEN_SCORE_SHARE");      // (read per call: the tests compare both forms in one process)
    const bool share = Tn >= 2 && !(she && she[0] == '0') && ensure_tcache(e);
    sc.shared_slots = share ? P : 0;
    // host staging of a chunk (the asynchronous copies read it until the chunk's synchronisation)
    TokenSeqs rep;                                       // the windows of a chunk's items [i0, i0 + n): [n][T][S_mod], item i scene i / C
    std::vector<int> cand_pose, item_scene, pshift, am;
    std::vector<float> pdiff, lp;
    if (!share) {
        for (long i0 = 0; i0 < N; i0 += Bm) {
            const int n = (int)std::min<long>(Bm, N - i0);
            gather_fan_windows(sc.win, i0, n, C, 0, Tn, rep);
            const ScoreIO one{n, Tn, rep.view(), sc.next + (size_t)i0 * kTokPerFrame, sc.out, i0};
            if (int rc = run_score<T>(e, one)) return rc;
        }
        return 0;
    }
    FrameCtx ctx = begin_call(e, kNoSampling);
    const FrameIO io{B, Tn, sc.win, nullptr, nullptr, 0, &kNoSampling, nullptr, nullptr};
    e->px.valid = false;                 // the passes below overwrite the slot caches and the stacks' workspaces
    if (int rc = settle_background_pass(e, io, ctx)) return rc;
    hipStream_t const st = ctx.st;
    const Place pl{st, &e->w_main};      // every pass of a scoring call: one stream, the main workspaces
    if (int rc = upload_frame_inputs(e, io, ctx)) return rc;
    StageClock clock{e, st};
    clock.stage(nullptr);                // the uploads
    // once per scene: the ego net on the whole window (its three head_ego rows stay in e->dv.logits [3 B][pose_vocab]) ...
    run_ego_any(e, pl, WindowTokens{e->d_pose, e->d_map, e->d_box, e->d_img, B, Tn, Tn, 0}, ctx.sp, 0, false, nullptr, CACHE_NONE);
    clock.stage(&e->tm.ego_ms);
    // ... and slots [0, T - 1) of the three stacks
    if (int rc = history_slots_once(e, pl, sc.win.pose(), B, Tn, ctx.pshift, ctx.pdiff)) return rc;
    clock.stage(&e->tm.tar_ms);
    for (long i0 = 0; i0 < N; i0 += Bm) {
        const int n = (int)std::min<long>(Bm, N - i0);
        const int* next = sc.next + (size_t)i0 * kTokPerFrame;
        gather_fan_windows(sc.win, i0, n, C, 0, Tn, rep);
        cand_pose.resize((size_t)n * 3);
        item_scene.resize(n);
        for (int i = 0; i < n; ++i) {
            item_scene[i] = (int)((i0 + i) / C);
            for (int a = 0; a < 3; ++a) cand_pose[(size_t)i * 3 + a] = next[(size_t)i * kTokPerFrame + a];
        }
        if (int rc = upload_pose_shift(e, st, rep.view().pose(), cand_pose.data(), n, Tn, pshift, pdiff)) return rc;      // slot T - 1 of item (b, c): the candidate's pose
        if (int rc = upload_tokens(e, st, rep.view(), (size_t)n * Tn, false)) return rc;
        HIPCHK(e, hipMemcpyAsync(e->d_item_scene, item_scene.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(e->dv.d_tokens, next, (size_t)n * kTokPerFrame * 4, hipMemcpyHostToDevice, st));
        // a candidate's pose: a lookup in its scene's rows (the bits depend on the row and the target only)
        for (int i = 0; i < n; ++i)
            launch_logits_nll(st, e->dv.logits + (long)item_scene[i] * 3 * e->cfg.pose_vocab, e->cfg.pose_vocab, e->cfg.pose_vocab, 3, e->dv.d_tokens + (long)i * kTokPerFrame,
                              kNPose, kTokPerFrame, e->score_logp + (long)i * 3, e->score_arg + (long)i * 3, nullptr, nullptr);
        stacks_with_cond_rows(e, pl, WindowTokens{e->d_pose_shift, e->d_map, e->d_box, e->d_img, n, 1, Tn, P}, CACHE_SHARED_ITEMS, B);
        clock.stage(&e->tm.tar_ms);
        if (int rc = run_prefix_prefill_any(e, pl, n, kSeq)) return rc;
        if (int rc = score_heads<T>(e, st, n, nullptr)) return rc;
        lp.resize((size_t)n * kTokPerFrame);
        am.resize((size_t)n * kTokPerFrame);
        HIPCHK(e, hipMemcpyAsync(lp.data(), e->score_logp, (size_t)n * kTokPerFrame * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipMemcpyAsync(am.data(), e->score_arg, (size_t)n * kTokPerFrame * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
        clock.stage(&e->tm.oar_ms);
        scatter_blocks(sc.out.logp, n, lp.data(), i0);
        scatter_blocks(sc.out.argmax, n, am.data(), i0);
    }
    if (e->profiling) fold_launch_events(e);
    return finish_call(e, "scoring pass");
}

// Where future frame k of umgen_score_futures sits: its window is frames [start, start + n) of history ++ future (umgen_rollout's window rule), the first h of
// them history frames; slots [0, P) of the map / box / TAR stacks are the scene's (the shift hands slot h - 1 the pose of future frame 0)
struct FutureFrame { int start, n, h, P; };
FutureFrame future_frame(const ScoreFutIO& sc, int k) {
    const CondWindow w = cond_window(sc.T + k, sc.cond);
    const int h = std::max(0, w.n - k);
    return FutureFrame{w.start, w.n, h, h - 1};
}
// can frame k take the shared path: a shared slot, and tails the kernel holds in the three stacks (k + 1 slots behind P) and in the ego stack (k behind h)
bool future_frame_shares(const umgen_engine* e, const ScoreFutIO& sc, int k) {
    const FutureFrame w = future_frame(sc, k);
    return w.P >= 1 && attn_temporal_fan_tail_heads(e->H, w.P, k + 1) && (k == 0 || attn_temporal_fan_tail_heads(e->H, w.h, k));
}

// The windows and targets of items [i0, i0 + n) -- item i is candidate (i / C, i % C) -- at future frame k: win[m] [n][w.n][S_mod], next [n][2199], rows[i] the
// row of sc.out that takes item i's results
struct FutureChunk { TokenSeqs win; std::vector<int> next; std::vector<long> rows; };
void future_chunk(const ScoreFutIO& sc, int k, const FutureFrame& w, long i0, int n, FutureChunk& ch) {
    const int C = sc.C, k0 = w.h ? 0 : w.start - sc.T;      // k0: first future frame inside the window
    const auto scene = [i0, C](size_t i) { return (i0 + i) / C; };
    const auto item = [i0](size_t i) { return i0 + i; };
    ch.win.resize(n, w.n);
    copy_frames(sc.win, n, scene, [&w](size_t) { return w.start; }, w.h, ch.win, 0);
    copy_frames(sc.fut, n, item, [k0](size_t) { return k0; }, w.n - w.h, ch.win, w.h);
    ch.next.resize((size_t)n * kTokPerFrame);
    frame_rows(sc.fut, n, item, [k](size_t) { return k; }, ch.next.data());
    ch.rows.resize(n);
    for (int i = 0; i < n; ++i) ch.rows[i] = (i0 + i) * sc.K + k;
}

// frames [k0, k1) of every candidate, each item against its own window: run_score in chunks of at most max_batch items
template <typename T>
int score_futures_replicated(umgen_engine* e, const ScoreFutIO& sc, int k0, int k1) {
    const long N = (long)sc.B * sc.C;
    const int Bm = e->cfg.max_batch;
    FutureChunk ch;
    for (int k = k0; k < k1; ++k) {
        const FutureFrame w = future_frame(sc, k);
        for (long i0 = 0; i0 < N; i0 += Bm) {
            const int n = (int)std::min<long>(Bm, N - i0);
            future_chunk(sc, k, w, i0, n, ch);
            const ScoreIO one{n, w.n, ch.win.view(), ch.next.data(), sc.out, 0, ch.rows.data()};
            if (int rc = run_score<T>(e, one)) return rc;
        }
    }
    return 0;
}

// Frames [0, Ks) of umgen_score_futures on shared history slots.  At frame k the per-scene pass (the ego stack over the window's h history slots, unshifted, and
// history_slots_once over slots [0, P) of the other three) runs only when the window's first frame moved: while the window grows the caches already hold exactly
// those slots.  Then the items, in chunks of at most max_batch, run their tails against the scenes' caches (CACHE_SHARED_ITEMS_TAIL): k slots of the ego stack
// behind h, the decoder and head_ego on the item's last slot (k == 0: the scene's own rows, as in run_score_candidates), k + 1 slots of the other stacks behind
// P, the conditioning rows, the BlockOAR pass and the heads -- run_score's kernels and row arithmetic over other row sets.
template <typename T>
int score_futures_shared(umgen_engine* e, const ScoreFutIO& sc, int Ks) {
    const int B = sc.B, C = sc.C, Bm = e->cfg.max_batch, pv = e->cfg.pose_vocab;
    const long N = (long)B * C;
    FrameCtx ctx = begin_call(e, kNoSampling);
    const FrameIO io{B, std::min(sc.T, sc.cond), sc.win, nullptr, nullptr, 0, &kNoSampling, nullptr, nullptr};
    e->px.valid = false;                 // the passes below overwrite the slot caches and the stacks' workspaces
    if (int rc = settle_background_pass(e, io, ctx)) return rc;
    hipStream_t const st = ctx.st;
    const Place pl{st, &e->w_main};      // every pass of a scoring call: one stream, the main workspaces
    HIPCHK(e, hipMemsetAsync(e->d_counters, 0, 8 * sizeof(int), st));      // (what upload_frame_inputs clears ahead of the ego sampler)
    ctx.seeds.assign(B, 0ull);
    HIPCHK(e, hipMemcpyAsync(e->dv.d_seeds, ctx.seeds.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
    StageClock clock{e, st};
    // host staging (the asynchronous copies read it until the next synchronisation: a chunk ends with one, and nothing is rewritten before it)
    TokenSeqs hist;                      // the scenes' history frames inside the window, [B][h][S_mod]
    std::vector<int> cand_pose, item_scene, pshift, am;
    std::vector<float> pdiff, lp;
    std::vector<long> frame_of;
    FutureChunk ch;
    int prev_start = -1;
    for (int k = 0; k < Ks; ++k) {
        const FutureFrame w = future_frame(sc, k);
        const int Wt = k + 1;
        if (k == 0 || w.start != prev_start) {
            prev_start = w.start;
            ++e->fut_history_passes;
            gather_windows(sc.win, B, w.start, w.h, hist);
            if (int rc = upload_tokens(e, st, hist.view(), (size_t)B * w.h)) return rc;
            clock.stage(nullptr);            // the uploads
            const WindowTokens we{e->d_pose, e->d_map, e->d_box, e->d_img, B, w.h, w.h, 0};
            // k == 0: the whole window is history -- the ego net once per scene, its three head_ego rows in e->dv.logits [3 B][pose_vocab], and the ego stack's
            // k | v rows kept for the longer windows that follow; later: the ego stack's shared slots alone
            if (k == 0) run_ego_any(e, pl, we, ctx.sp, 0, false, nullptr, Ks > 1 ? CACHE_WINDOW_KEEP : CACHE_NONE);
            else run_stack_any(e, pl, STACK_EGO, we, CACHE_FILL_PREFIX);
            clock.stage(&e->tm.ego_ms);
            if (int rc = history_slots_once(e, pl, hist.view().pose(), B, w.h, ctx.pshift, ctx.pdiff)) return rc;
            clock.stage(&e->tm.tar_ms);
        }
        for (long i0 = 0; i0 < N; i0 += Bm) {
            const int n = (int)std::min<long>(Bm, N - i0);
            future_chunk(sc, k, w, i0, n, ch);
            cand_pose.resize((size_t)n * 3);
            item_scene.resize(n);
            for (int i = 0; i < n; ++i) {
                item_scene[i] = (int)((i0 + i) / C);
                for (int a = 0; a < 3; ++a) cand_pose[(size_t)i * 3 + a] = ch.next[(size_t)i * kTokPerFrame + a];
            }
            if (int rc = upload_tokens(e, st, ch.win.view(), (size_t)n * w.n, false)) return rc;
            HIPCHK(e, hipMemcpyAsync(e->d_item_scene, item_scene.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
            HIPCHK(e, hipMemcpyAsync(e->dv.d_tokens, ch.next.data(), (size_t)n * kTokPerFrame * 4, hipMemcpyHostToDevice, st));
            if (k == 0) {
                // the pose of future frame 0: a lookup in the scene's rows (the bits depend on the row and the target only)
                for (int i = 0; i < n; ++i)
                    launch_logits_nll(st, e->dv.logits + (long)item_scene[i] * 3 * pv, pv, pv, 3, e->dv.d_tokens + (long)i * kTokPerFrame, kNPose, kTokPerFrame,
                                      e->score_logp + (long)i * 3, e->score_arg + (long)i * 3, nullptr, nullptr);
            } else {
                // the ego net reads the unshifted window: the item's k future slots behind the scene's h, the decoder and head_ego on its last slot
                HIPCHK(e, hipMemcpyAsync(e->d_pose, ch.win.view().pose(), ch.win.mod[0].size() * 4, hipMemcpyHostToDevice, st));
                run_stack_any(e, pl, STACK_EGO, WindowTokens{e->d_pose, e->d_map, e->d_box, e->d_img, n, k, w.n, w.h}, CACHE_SHARED_ITEMS_TAIL, TAIL_AUTO, nullptr, B);
                frame_of.resize(n);
                for (int i = 0; i < n; ++i) frame_of[i] = (long)i * k + (k - 1);
                ego_decoder_any(e, pl, n, frame_of.data(), w.n, nullptr);
                launch_logits_nll(st, e->dv.logits, pv, pv, 3 * n, e->dv.d_tokens, kNPose, kTokPerFrame, e->score_logp, e->score_arg, nullptr, nullptr);
                clock.stage(&e->tm.ego_ms);
            }
            if (int rc = upload_pose_shift(e, st, ch.win.view().pose(), cand_pose.data(), n, w.n, pshift, pdiff)) return rc;      // slot n - 1: the pose of future frame k
            stacks_with_cond_rows(e, pl, WindowTokens{e->d_pose_shift, e->d_map, e->d_box, e->d_img, n, Wt, w.n, w.P}, CACHE_SHARED_ITEMS_TAIL, B);
            clock.stage(&e->tm.tar_ms);
            if (int rc = run_prefix_prefill_any(e, pl, n, kSeq)) return rc;
            if (int rc = score_heads<T>(e, st, n, nullptr)) return rc;
            lp.resize((size_t)n * kTokPerFrame);
            am.resize((size_t)n * kTokPerFrame);
            HIPCHK(e, hipMemcpyAsync(lp.data(), e->score_logp, (size_t)n * kTokPerFrame * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(e, hipMemcpyAsync(am.data(), e->score_arg, (size_t)n * kTokPerFrame * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(e, hipStreamSynchronize(st));
            clock.stage(&e->tm.oar_ms);
            scatter_blocks(sc.out.logp, n, lp.data(), 0, ch.rows.data());
            scatter_blocks(sc.out.argmax, n, am.data(), 0, ch.rows.data());
        }
    }
    if (e->profiling) fold_launch_events(e);
    return finish_call(e, "scoring pass");
}

// umgen_score_futures: C candidate futures of K frames per scene against one history, every frame under umgen_rollout's window rule.  The leading frames whose
// window still holds a shared history slot and whose tails the kernel holds take score_futures_shared; the frames behind them, and everything when the slot
// caches do not fit or UMGEN_SCORE_FUTURES_SHARE=0, are run_score itself on per-item windows.  Either way entry (b, c, k) has the bits of umgen_score on its own
// window.  (P_k never grows and the tails only do, so the frames that share are a prefix of the K.)
template <typename T>
int run_score_futures(umgen_engine* e, const ScoreFutIO& sc) {
    const char* she = getenv("UMGEN_SCORE_FUTURES_SHARE");      // (read per call: the tests compare both forms in one process)
    int Ks = 0;
    e->fut_history_passes = 0;
    if (!(she && she[0] == '0') && future_frame_shares(e, sc, 0) && ensure_tcache(e))
        while (Ks < sc.K && future_frame_shares(e, sc, Ks)) ++Ks;
    if (sc.shared_slots)
        for (int k = 0; k < sc.K; ++k) sc.shared_slots[k] = k < Ks ? future_frame(sc, k).P : 0;
    if (Ks)
        if (int rc = score_futures_shared<T>(e, sc, Ks)) return rc;
    return score_futures_replicated<T>(e, sc, Ks, sc.K);
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

// the row of sc.out [B][L - T_in][S_mod] that takes frame f of clip b
long clip_out_row(const ScoreClipIO& sc, int b, int f) { return (long)b * (sc.L - sc.T_in) + (f - sc.T_in); }

// frames [f0, f1) of every clip, each against its own window: run_score on items (f, b), in chunks of at most max_batch items of one window length
template <typename T>
int score_clip_frames(umgen_engine* e, const ScoreClipIO& sc, int f0, int f1) {
    const int B = sc.B, Bm = e->cfg.max_batch;
    TokenSeqs win;
    std::vector<int> next;
    std::vector<long> rows;
    const long N = (long)(f1 - f0) * B;
    for (long i0 = 0; i0 < N;) {      // item i0 + i: frame f0 + (i0 + i) / B of clip (i0 + i) % B
        const auto frame = [=](size_t i) { return f0 + (int)((i0 + i) / B); };
        const auto clip = [=](size_t i) { return (int)((i0 + i) % B); };
        const int Tn = cond_window(frame(0), sc.cond).n;
        int n = 0;
        while (n < Bm && i0 + n < N && cond_window(frame(n), sc.cond).n == Tn) ++n;
        rows.resize(n);
        for (int i = 0; i < n; ++i) rows[i] = clip_out_row(sc, clip(i), frame(i));
        gather_windows(sc.clip, n, clip, [&](size_t i) { return frame(i) - Tn; }, Tn, win);
        next.resize((size_t)n * kTokPerFrame);
        frame_rows(sc.clip, n, clip, frame, next.data());
        const ScoreIO one{n, Tn, win.view(), next.data(), sc.out, 0, rows.data()};
        if (int rc = run_score<T>(e, one)) return rc;
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
    const int E = e->E, B = sc.B, Bm = e->cfg.max_batch, n = B * G, pv = e->cfg.pose_vocab;
    FrameCtx ctx = begin_call(e, kNoSampling);
    // the window [0, P) of every clip, [B][P][S_mod], and frame P's pose, which the shift hands to slot P - 1
    TokenSeqs win;
    std::vector<int> pose_P((size_t)B * 3), items((size_t)n * 2), item_T(n), next((size_t)n * kTokPerFrame);
    std::vector<long> rows(n);
    gather_windows(sc.clip, B, 0, P, win);
    for (int b = 0; b < B; ++b) {
        memcpy(&pose_P[(size_t)b * 3], sc.clip.at(0, b, P), 3 * sizeof(int));
        for (int g = 0; g < G; ++g) {      // item (b, g): slot t = T_in - 1 + g scores frame t + 1
            const int i = b * G + g, t = sc.T_in - 1 + g;
            items[2 * i] = b; items[2 * i + 1] = t; item_T[i] = t + 1; rows[i] = clip_out_row(sc, b, t + 1);
        }
    }
    frame_rows(sc.clip, n, [G](size_t i) { return i / G; }, [&](size_t i) { return sc.T_in + (int)(i % G); }, next.data());
    const FrameIO io{B, P, win.view(), nullptr, nullptr, 0, &kNoSampling, nullptr, nullptr};
    e->px.valid = false;                 // the passes below overwrite the stacks' workspaces; nothing of them is for a later rollout
    if (int rc = settle_background_pass(e, io, ctx)) return rc;
    hipStream_t const st = ctx.st;
    const Place pl{st, &e->w_main};      // every pass of a scoring call: one stream, the main workspaces
    if (int rc = upload_frame_inputs(e, io, ctx)) return rc;
    HIPCHK(e, hipMemcpyAsync(e->clip_items, items.data(), items.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->clip_item_T, item_T.data(), item_T.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->clip_tokens, next.data(), next.size() * 4, hipMemcpyHostToDevice, st));
    StageClock clock{e, st};             // here ego_ms is the ego stack and decoder, tar_ms the three stacks and the conditioning rows
    clock.stage(nullptr);                // the uploads
    // the ego stack over [0, P), every block on every slot; the decoder and head_ego on the items, in chunks that fit the 3 * max_batch-row buffers
    run_stack_any(e, pl, STACK_EGO, WindowTokens{e->d_pose, e->d_map, e->d_box, e->d_img, B, P, P, 0}, CACHE_NONE, TAIL_NONE);
    std::vector<long> frame_of(Bm);
    for (int i0 = 0; i0 < n; i0 += Bm) {
        const int nc = std::min(Bm, n - i0);
        for (int i = 0; i < nc; ++i) frame_of[i] = (long)items[2 * (i0 + i)] * P + items[2 * (i0 + i) + 1];
        ego_decoder_any(e, pl, nc, frame_of.data(), 0, e->clip_item_T + i0);
        launch_logits_nll(st, e->dv.logits, pv, pv, 3 * nc, e->clip_tokens + (long)i0 * kTokPerFrame, kNPose, kTokPerFrame, e->clip_logp + (long)i0 * 3,
                          e->clip_arg + (long)i0 * 3, nullptr, nullptr);
    }
    clock.stage(&e->tm.ego_ms);
    // one pose shift for the window: slot t carries the pose of frame t + 1, slot P - 1 that of frame P
    if (int rc = upload_pose_shift(e, st, win.view().pose(), pose_P.data(), B, P, ctx.pshift, ctx.pdiff)) return rc;
    const WindowTokens ws{e->d_pose_shift, e->d_map, e->d_box, e->d_img, B, P, P, 0};
    run_stack_any(e, pl, STACK_MAP, ws, CACHE_NONE, TAIL_NONE, e->clip_warped);
    launch_cond_rows_slots(st, STACK_MAP, P, E, pl.work->X, e->ln_map_tar, e->clip_warped, e->clip_items, n, e->clip_cond);
    run_stack_any(e, pl, STACK_BOX, ws, CACHE_NONE, TAIL_NONE);
    launch_cond_rows_slots(st, STACK_BOX, P, E, pl.work->X, e->ln_box_tar, nullptr, e->clip_items, n, e->clip_cond);
    run_stack_any(e, pl, STACK_TAR, ws, CACHE_NONE, TAIL_NONE);
    launch_cond_rows_slots(st, STACK_TAR, P, E, pl.work->X, e->ln_tar, nullptr, e->clip_items, n, e->clip_cond);
    clock.stage(&e->tm.tar_ms);
    // one BlockOAR pass and one head sweep for all items (n <= max_batch * max_cond_frames: the rows the stacks' workspaces hold)
    const PrefillSrc ps{e->clip_cond, e->clip_tokens, e->clip_xlast, true};
    if (int rc = run_prefix_prefill_any(e, pl, n, kSeq, &ps)) return rc;
    const ScoreBufs sb{e->clip_tokens, e->clip_part, e->clip_logp, e->clip_arg};
    if (int rc = score_heads<T>(e, st, n, nullptr, &sb)) return rc;
    std::vector<float> lp((size_t)n * kTokPerFrame);
    std::vector<int> am((size_t)n * kTokPerFrame);
    HIPCHK(e, hipMemcpyAsync(lp.data(), e->clip_logp, lp.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(am.data(), e->clip_arg, am.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    clock.stage(&e->tm.oar_ms);
    if (e->profiling) fold_launch_events(e);
    if (int rc = finish_call(e, "scoring pass")) return rc;
    scatter_blocks(sc.out.logp, n, lp.data(), 0, rows.data());
    scatter_blocks(sc.out.argmax, n, am.data(), 0, rows.data());
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

// behind a failed pass: drain_failed_frame
template <typename Pass>
int run_pass(umgen_engine* e, Pass pass) {
    const int rc = with_precision(e, pass);
    if (rc != UMGEN_OK) drain_failed_frame(e);
    return rc;
}

}  // namespace

namespace umgen {

int run_score_any(umgen_engine* e, const ScoreIO& sc) { return run_pass(e, [&](auto t) { return run_score<decltype(t)>(e, sc); }); }
int run_score_candidates_any(umgen_engine* e, ScoreCandIO& sc) { return run_pass(e, [&](auto t) { return run_score_candidates<decltype(t)>(e, sc); }); }
int run_score_clip_any(umgen_engine* e, ScoreClipIO& sc) { return run_pass(e, [&](auto t) { return run_score_clip<decltype(t)>(e, sc); }); }
int run_score_futures_any(umgen_engine* e, const ScoreFutIO& sc) { return run_pass(e, [&](auto t) { return run_score_futures<decltype(t)>(e, sc); }); }

}  // namespace umgen
