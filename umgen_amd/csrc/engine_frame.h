// What generation (engine_frame.hip, which defines everything here) and scoring (engine_score.hip) share of a call: its scope, the locals of
// its stages, and the stages a scoring pass takes from a frame.  Nothing else belongs here: engine state is engine_state.h's.
#pragma once

#include "engine_state.h"

namespace umgen {

// The locals of run_frame that more than one stage uses, or that the frame's asynchronous copies read until the stream is drained (so they
// live as long as the frame does).  Filled stage by stage, in run_frame's order; begin_call zero-initialises it.
struct FrameCtx {
    hipStream_t fg, st, pre, dec;       // the engine's foreground stream; the stream in use (the only record of it: every stage passes it on as an
                                        // argument, the stack passes inside a Place); the streams of the ego / TAR phase and of the decode loop
    SamplerParams sp;
    bool forced;                        // teacher-forced trace frame
    bool use_px, ov_active, fg_write;   // last slot only against the slot caches; a background pass may follow; this frame's passes fill the caches
    int t0, Tc;                         // first slot and slot count of this frame's passes through the stacks
    CacheMode cmode;                    // ... and what they do with the slot caches
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

// A call's scope.  begin_call forgets the last call's refused launch and a stale HIP error another user of this thread left behind (torch, RCCL),
// and returns the call's locals with the engine's stream (the decode stream of overlapped rollouts: 6 of the 8 XCDs when the overlap exists) and
// the sampler's parameters filled in; a call changes nothing about the engine's stream or workspaces, so nothing is handed back when it ends;
// finish_call, behind the call's last synchronisation, fails it when one of its launches was refused (`what`: "frame" | "scoring pass").
FrameCtx begin_call(umgen_engine* e, const umgen_sampling& smp);
int finish_call(umgen_engine* e, const char* what);
void drain_failed_frame(umgen_engine* e);      // behind a failed call

// run_frame's first stages, in its order, as run_score takes them
int settle_background_pass(umgen_engine* e, const FrameIO& io, FrameCtx& ctx);
int upload_frame_inputs(umgen_engine* e, const FrameIO& io, FrameCtx& ctx);
int ego_and_pose_shift(umgen_engine* e, const FrameIO& io, FrameCtx& ctx);
int run_stacks(umgen_engine* e, const FrameIO& io, FrameCtx& ctx);

// `rows` frames of v -- rows * S_mod tokens from the start of every modality -- into d_pose (with_pose; callers whose pose goes through the shift
// leave it out), d_map, d_box and d_img.  The copies are asynchronous: what v points at outlives the call's next synchronisation of st
int upload_tokens(umgen_engine* e, hipStream_t st, const TokenView& v, size_t rows, bool with_pose = true);
// decode_pose_shift of B windows [B][Tn][3] and the new frames' poses ego [B][3] into d_pose_shift and pose_diff; the copies are asynchronous, so
// pshift and pdiff outlive the call's next synchronisation of st
int upload_pose_shift(umgen_engine* e, hipStream_t st, const int* pose, const int* ego, int B, int Tn, std::vector<int>& pshift, std::vector<float>& pdiff);
// the map, box and TAR stacks one behind the other at pl, each followed by its conditioning rows; fan_scenes: run_stack's
void stacks_with_cond_rows(umgen_engine* e, const Place& pl, const WindowTokens& w, CacheMode mode, int fan_scenes = 0);
// Slots [0, Tn - 1) of the map / box / TAR stacks once per scene for callers whose items share them (CACHE_SHARED_ITEMS): the shift of the B windows
// pose [B][Tn][3] without a new pose (slot Tn - 1 is not read), then the three stacks, their temporal k | v rows into the scenes' blocks of the slot caches
int history_slots_once(umgen_engine* e, const Place& pl, const int* pose, int B, int Tn, std::vector<int>& pshift, std::vector<float>& pdiff);
// a profiled call's per-launch events (gemm_timed, tar_sub, the decode loops) into the timings
void fold_launch_events(umgen_engine* e);

}  // namespace umgen
