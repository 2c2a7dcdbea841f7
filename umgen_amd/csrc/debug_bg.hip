// Test hooks on a live one-scene handle for the background pass of the decode engine's workers (bg_worker.h, bg_queue.h, engine_stacks.hip
// launch_prefix): begin a pass either as the stand-alone launches (the reference) or recorded for the workers with chunk / margin overridden, force the
// unit-time estimates, run decode launches or the drain launch, read the queue back, end the pass, move a slot cache out or in.  The pass and the
// drain launch are the product's own code (launch_prefix_any, launch_bg_drain), the decode launches umgen_dbg_oar_step's: nothing here restates them.
// tests/test_gpu_bg_pass.py holds the workers' slot caches to the stand-alone kernels' bit for bit with these, under schedules it controls through
// host-written memory alone (est[], chunk, margin_ticks).
#include "engine_state.h"

extern "C" int umgen_dbg_oar_step(umgen_engine* e, int32_t B, int32_t L, const float* x_in, float* x_out, int32_t use_engine, int32_t unmasked);

namespace {

// every hook: a finalized handle whose one scene runs on the engine with background workers
int bg_handle(umgen_engine* e) {
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_finalize_weights has not been called");
    if (!e->bg_engine || !e->d_bgq) return e->fail(UMGEN_E_UNSUPPORTED, "this engine has no background workers (one scene per call on the XCD-resident decode engine, UMGEN_BG_ENGINE)");
    if (e->cfg.max_batch != 1) return e->fail(UMGEN_E_UNSUPPORTED, "background workers serve one scene per call, not max_batch %d", e->cfg.max_batch);
    if (!ensure_tcache(e)) return e->fail(UMGEN_E_NOMEM, "no slot caches on this engine");
    return 0;
}

bool tokens_ok(const int32_t* t, size_t n, int hi) {
    for (size_t i = 0; i < n; ++i)
        if (t[i] < 0 || t[i] >= hi) return false;
    return true;
}

}  // namespace

extern "C" {

// Test hook: what launch_prefix does behind a frame whose window holds T slots (host int32 [T][S_mod]) under the window cap cond_cap -- the next window's
// known slots (T growing to T + 1 when T < cond_cap, slots 1 .. T - 1 plus the new frame when the window slides) with the next pose tokens ego3 through the
// four stacks, cache mode 1.  foreground 1: as stand-alone kernels on the engine's stream, synchronised (nothing pending afterwards).  foreground 0: recorded
// and uploaded for the workers as the product does (engine_ticks 0: the first decode launch only measures), nothing runs; chunk > 0 overrides every op's
// chunk, margin_ticks >= 0 the default margin.  n_ops / heads [max_heads][8] (BgOpHead words) report the recorded list.  A pass the recorder refuses is an error.
int umgen_dbg_bg_begin(umgen_engine* e, int32_t T, int32_t cond_cap, const int32_t* pose, const int32_t* map, const int32_t* bbox3d, const int32_t* image, const int32_t* ego3,
                       int32_t foreground, int32_t chunk, int32_t margin_ticks, int32_t* n_ops, int32_t* heads, int32_t max_heads) {
    if (!e || !pose || !map || !bbox3d || !image || !ego3) return UMGEN_E_INVALID;
    if (int rc = bg_handle(e)) return rc;
    const int Tnext = std::min(T + 1, cond_cap);
    if (T < 1 || T > e->cfg.max_cond_frames || cond_cap < 2 || Tnext - 1 < 1 || Tnext > e->cfg.max_cond_frames)
        return e->fail(UMGEN_E_INVALID, "a window of %d slots under a cap of %d: the pass covers 1 .. %d known slots of a next window of at most %d", T, cond_cap,
                       e->cfg.max_cond_frames - 1, e->cfg.max_cond_frames);
    if (!tokens_ok(pose, (size_t)T * kNPose, e->cfg.pose_vocab) || !tokens_ok(ego3, 3, e->cfg.pose_vocab) || !tokens_ok(map, (size_t)T * kNMap, e->cfg.map_vocab) ||
        !tokens_ok(bbox3d, (size_t)T * kNBox, e->cfg.bbox3d_vocab) || !tokens_ok(image, (size_t)T * kNImg, e->cfg.img_vocab))
        return e->fail(UMGEN_E_INVALID, "a token outside its vocabulary");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    (void)hipGetLastError();
    FrameIO io{};
    io.B = 1; io.T = T; io.win = TokenView{{pose, map, bbox3d, image}, T}; io.cond_cap = cond_cap; io.next_follows = true;
    const BgPassDebug dbg{foreground ? 1 : 0, chunk, margin_ticks};
    const std::vector<int> ego(ego3, ego3 + 3);
    e->bg_pending = false;
    if (int rc = launch_prefix_any(e, Place{e->stream, &e->w_main}, io, ego, &dbg)) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));      // (the uploads read the handle's staging buffers; a decode launch may take another stream)
    const int n = foreground ? 0 : (int)e->bg_rec.ops.size();
    if (n_ops) *n_ops = n;
    if (heads)
        for (int i = 0; i < std::min(n, (int)max_heads); ++i) memcpy(heads + (size_t)i * 8, &e->bg_rec.ops[i].h, sizeof(BgOpHead));
    static_assert(sizeof(BgOpHead) == 32, "BgOpHead is reported as 8 words");
    return UMGEN_OK;
}

// Test hook: every est[] entry of the queue = value; 0 puts the host's guesses of the recorded pass back.
int umgen_dbg_bg_est(umgen_engine* e, uint32_t value) {
    if (!e) return UMGEN_E_INVALID;
    if (int rc = bg_handle(e)) return rc;
    if (value) HIPCHK(e, hipMemsetD32Async((hipDeviceptr_t)&e->d_bgq->est[0], (int)value, kBgMaxOps, e->stream));
    else if (!e->bg_rec.est.empty()) HIPCHK(e, hipMemcpyAsync(&e->d_bgq->est[0], e->bg_rec.est.data(), e->bg_rec.est.size() * sizeof(unsigned), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return UMGEN_OK;
}

// Test hook: the queue behind a stream sync -- state [128][4] (op, units done | arrived << 31, batch start, -), ops_done, arrive[0 .. n_arrive).
int umgen_dbg_bg_state(umgen_engine* e, uint32_t* state, uint32_t* ops_done, uint32_t* arrive, int32_t n_arrive) {
    if (!e) return UMGEN_E_INVALID;
    if (int rc = bg_handle(e)) return rc;
    if (n_arrive < 0 || n_arrive > kBgMaxOps) return e->fail(UMGEN_E_INVALID, "n_arrive=%d", n_arrive);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (state) HIPCHK(e, hipMemcpy(state, &e->d_bgq->state[0][0], sizeof(e->d_bgq->state), hipMemcpyDeviceToHost));
    if (ops_done) HIPCHK(e, hipMemcpy(ops_done, &e->d_bgq->ops_done, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (arrive && n_arrive) HIPCHK(e, hipMemcpy(arrive, &e->d_bgq->arrive[0], (size_t)n_arrive * sizeof(unsigned), hipMemcpyDeviceToHost));
    return UMGEN_OK;
}

// Test hook: up to n decode launches back to back on the pending pass (umgen_dbg_oar_step at position 0 on the engine's own stream: the workers advance
// inside it; its x is not looked at).  est != 0: every est[] entry is set to it before every launch (far above any budget: one unit per worker per launch).
// Behind every launch the workers' states go to states [n][128][4] and ops_done to done [n] (either may be NULL); until_done: stop once ops_done equals
// the op count and every worker stands at the end of the list.  n_run: launches that ran.
int umgen_dbg_bg_steps(umgen_engine* e, int32_t n, uint32_t est, int32_t until_done, uint32_t* states, uint32_t* done, int32_t* n_run) {
    if (!e || !n_run) return UMGEN_E_INVALID;
    *n_run = 0;
    if (int rc = bg_handle(e)) return rc;
    if (!e->bg_pending) return e->fail(UMGEN_E_STATE, "no background pass is pending (umgen_dbg_bg_begin with foreground 0)");
    if (n < 0) return e->fail(UMGEN_E_INVALID, "n=%d", n);
    const unsigned n_ops = (unsigned)e->bg_rec.ops.size();
    std::vector<float> x((size_t)e->E, 0.f), y((size_t)e->E);
    std::vector<unsigned> st((size_t)kBgMaxWorkers * 4);
    for (int i = 0; i < n; ++i) {
        if (est) HIPCHK(e, hipMemsetD32Async((hipDeviceptr_t)&e->d_bgq->est[0], (int)est, kBgMaxOps, e->stream));
        if (int rc = umgen_dbg_oar_step(e, 1, 0, x.data(), y.data(), 1, 0)) return rc;      // (synchronises)
        unsigned od = 0;
        HIPCHK(e, hipMemcpy(&od, &e->d_bgq->ops_done, sizeof(unsigned), hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(st.data(), &e->d_bgq->state[0][0], sizeof(e->d_bgq->state), hipMemcpyDeviceToHost));
        if (states) memcpy(states + (size_t)i * kBgMaxWorkers * 4, st.data(), sizeof(e->d_bgq->state));
        if (done) done[i] = od;
        *n_run = i + 1;
        // the host's own criterion (check_frame_results): every worker at the end of the list.  ops_done alone moves first: a worker that arrived on the last op and
        // met its deadline before the last arrival keeps its op index until its next launch.
        bool all = od >= n_ops;
        for (int w = 0; all && w < kBgMaxWorkers; ++w) all = st[(size_t)w * 4] >= n_ops;
        if (until_done && all) break;
    }
    return UMGEN_OK;
}

// Test hook: the one launch without an engine part that drain_and_download issues behind a frame's last step, synchronised.
int umgen_dbg_bg_drain(umgen_engine* e) {
    if (!e) return UMGEN_E_INVALID;
    if (int rc = bg_handle(e)) return rc;
    if (!e->bg_pending) return e->fail(UMGEN_E_STATE, "no background pass is pending (umgen_dbg_bg_begin with foreground 0)");
    if (int rc = launch_bg_drain(e, e->stream)) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return UMGEN_OK;
}

// Test hook: ends a pass of umgen_dbg_bg_begin -- empty queue, nothing pending, no prefix to be trusted, the next pass starts from the host's unit times:
// the handle is fit for ordinary rollouts again.
int umgen_dbg_bg_end(umgen_engine* e) {
    if (!e) return UMGEN_E_INVALID;
    if (int rc = bg_handle(e)) return rc;
    HIPCHK(e, hipMemsetAsync(&e->d_bgq->n_ops, 0, 4, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->bg_pending = false;
    e->px.valid = false;
    e->bg_rec = BgRecorder{};
    return UMGEN_OK;
}

// Test hook: the whole slot cache of one (stack, block), device [max_batch][max_cond_frames][S_stack][2E] in the cache type's bits, to (upload 0) or from
// (upload 1) the host.
int umgen_dbg_tcache(umgen_engine* e, int32_t stack, int32_t block, void* host, int32_t upload) {
    if (!e || !host) return UMGEN_E_INVALID;
    if (int rc = bg_handle(e)) return rc;
    if (stack < 0 || stack > 3 || block < 0 || block >= (int)e->tcache[stack].size()) return e->fail(UMGEN_E_INVALID, "stack=%d block=%d", stack, block);
    const size_t bytes = (size_t)e->cfg.max_batch * e->cfg.max_cond_frames * (size_t)stack_len(stack) * 2 * e->E * e->tsz;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (upload) HIPCHK(e, hipMemcpy(e->tcache[stack][block], host, bytes, hipMemcpyHostToDevice));
    else HIPCHK(e, hipMemcpy(host, e->tcache[stack][block], bytes, hipMemcpyDeviceToHost));
    return UMGEN_OK;
}

// Test hook: how many per-scene history passes the engine's last umgen_score_futures call launched (0: every frame took the replicated path)
int umgen_dbg_score_futures_passes(umgen_engine* e) { return e ? e->fut_history_passes : UMGEN_E_INVALID; }

}  // extern "C"
