#!/usr/bin/env python
"""Timing of umgen_score (one forward pass over a given frame) against the only earlier route to the same numbers, a teacher-forced
umgen_frame (2206 decode steps): UMGen_Large, synthetic weights, bf16, one engine of 8 scenes, a window of T history frames.
After one warm-up call each: the median of 5 host-clock calls of Engine.score at B = 1 and B = 8 and of Engine.frame(forced=..., trace=False).
    python tools/score_bench.py [out.json] [--T=20] [--detail]  ->  one JSON line (also written to out.json, default profiles/score_bench.json)
--detail adds the cost of asking for the score diagnostics (umgen_score_detail at topk 16, one more sweep of the heads): after one warm-up call each, 5
alternating pairs of Engine.score and Engine.score(detail=True, topk=16) at B = 1 and B = 8, the median of each side.
--candidates C (or --candidates=C) measures only umgen_score_candidates: one scene, C candidate next frames, Engine.score_candidates against
Engine.score with the window replicated C times (the same numbers, bit for bit), 5 alternating pairs behind one warm-up call each; the result
is stored under "candidates" in out.json, whose other entries are kept.
--clip measures only umgen_score_clip: one scene, a clip of L = 21 frames, input_frames 1, cond_frames 20, an engine of one scene; Engine.score_clip
against the loop of 20 Engine.score calls on the growing windows (the same numbers, bit for bit) and against itself with UMGEN_SCORE_CLIP_SHARE=0, 5
alternating rounds behind one warm-up call of each kind, and one profiled call's stage split; stored under "clip" in out.json.
--futures C K measures only umgen_score_futures: one scene, 20 history frames, cond_frames 20, C candidate futures of K frames, an engine of 8 scenes;
Engine.score_futures against the loop of C * K Engine.score calls on the same engine (the same numbers, bit for bit) and against itself with
UMGEN_SCORE_FUTURES_SHARE=0, 5 alternating rounds behind one warm-up call of each kind, the bytes compared, the shared_slots and one profiled call's
ego / stacks / BlockOAR+heads split; stored under "futures" in out.json."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from umgen_amd.config import MOD_ORDER, large_config  # noqa: E402
from umgen_amd.engine import Engine  # noqa: E402
from umgen_amd.synth import synthetic_scene  # noqa: E402
from umgen_amd.weights import synthetic_items  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
T = next((int(a[4:]) for a in sys.argv[1:] if a.startswith("--T=")), 20)
DETAIL = "--detail" in sys.argv[1:]
CAND = next((int(a[13:]) for a in sys.argv[1:] if a.startswith("--candidates=")), 0)
if "--candidates" in sys.argv[1:]:
    k = sys.argv.index("--candidates")
    CAND = int(sys.argv[k + 1])
    args.remove(sys.argv[k + 1])
CLIP = "--clip" in sys.argv[1:]
FUT = None
if "--futures" in sys.argv[1:]:
    k = sys.argv.index("--futures")
    FUT = (int(sys.argv[k + 1]), int(sys.argv[k + 2]))
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and i not in (k + 1, k + 2)]
REPS = 5


def median_ms(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def alternating_ms(fa, fb):
    """medians of REPS calls of each, taken in turns behind one warm-up call each"""
    fa()
    fb()
    ta, tb = [], []
    for _ in range(REPS):
        for fn, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ta), statistics.median(tb)


def candidates_bench(e, sc, out):
    """one scene's window against CAND candidates (the frames behind the other synthetic scenes' windows)"""
    w = {m: sc[0][m][0, :T] for m in MOD_ORDER}
    cand = {m: np.stack([sc[i % 8][m][0, T] for i in range(CAND)]) for m in MOD_ORDER}
    rep_w = {m: np.repeat(w[m][None], CAND, axis=0) for m in MOD_ORDER}
    got = {}
    fa = lambda: got.__setitem__("c", e.score_candidates(w, cand))  # noqa: E731
    fb = lambda: got.__setitem__("r", e.score(rep_w, cand))  # noqa: E731
    fa()
    fb()
    ta, tb = [], []
    for _ in range(REPS):
        for fn, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    same = all(got["c"]["logp"][m].tobytes() == got["r"]["logp"][m].tobytes() for m in MOD_ORDER)
    r = {"candidates": CAND, "history_frames": T, "score_candidates_ms": statistics.median(ta), "score_candidates_all_ms": ta,
         "replicated_score_ms": statistics.median(tb), "replicated_score_all_ms": tb, "replicated_spread_ms": max(tb) - min(tb),
         "ratio": statistics.median(tb) / statistics.median(ta), "shared_slots": got["c"]["shared_slots"], "same_bytes": same,
         "best": int(np.argmax(got["c"]["total"]))}
    if "--profile" in sys.argv[1:]:      # one profiled call: where the time of a candidates call goes (per-launch events serialise the stacks)
        e.set_profiling(True)
        t0 = time.perf_counter()
        e.score_candidates(w, cand)
        r["profiled_call_ms"] = (time.perf_counter() - t0) * 1e3
        r["profiled_timings"] = {k: v for k, v in e.timings().items() if k in ("total_ms", "ego_ms", "tar_ms", "oar_ms", "gemm_ms", "gemm_launches", "attn_ms", "attn_launches")}
        e.set_profiling(False)
    res = {}
    if os.path.exists(out):
        with open(out) as f:
            res = json.loads(f.read())
    res["candidates"] = r
    line = json.dumps(res)
    print(json.dumps(r))
    with open(out, "w") as f:
        f.write(line + "\n")


def clip_bench(out, L=21, cond=20):
    """one recorded clip of L frames: the clip call, the loop of Engine.score calls a user writes without it, and the clip call with nothing shared"""
    cfg = large_config()
    e = Engine(cfg, precision="bf16", max_batch=1, max_cond_frames=cond)
    e.load_state_dict(synthetic_items(cfg, seed=0))
    e.finalize()
    clip = {m: v[0] for m, v in synthetic_scene(0, n_frames=L).items()}
    windows = Engine.clip_windows(L, 1, cond)
    got = {}

    def loop():
        got["l"] = [e.score({m: clip[m][s:s + n] for m in MOD_ORDER}, {m: clip[m][f] for m in MOD_ORDER}) for f, s, n in windows]

    def unshared():
        os.environ["UMGEN_SCORE_CLIP_SHARE"] = "0"
        try:
            got["u"] = e.score_clip(clip, 1, cond)
        finally:
            del os.environ["UMGEN_SCORE_CLIP_SHARE"]
    kinds = ((lambda: got.__setitem__("c", e.score_clip(clip, 1, cond)), []), (loop, []), (unshared, []))
    for fn, _ in kinds:
        fn()
    for _ in range(REPS):
        for fn, ts in kinds:
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    tc, tl, tu = (ts for _, ts in kinds)
    same = all(got["c"][k][m][i].tobytes() == got["l"][i][k][m].tobytes() == got["u"][k][m][i].tobytes()
               for k in ("logp", "argmax") for m in MOD_ORDER for i in range(len(windows)))
    med = statistics.median
    r = {"frames": L, "input_frames": 1, "cond_frames": cond, "reps": REPS, "score_clip_ms": med(tc), "score_clip_all_ms": tc, "score_clip_spread_ms": max(tc) - min(tc),
         "score_loop_ms": med(tl), "score_loop_all_ms": tl, "score_loop_spread_ms": max(tl) - min(tl), "loop_over_clip": med(tl) / med(tc),
         "unshared_clip_ms": med(tu), "unshared_clip_all_ms": tu, "unshared_clip_spread_ms": max(tu) - min(tu), "unshared_over_clip": med(tu) / med(tc),
         "shared_frames": got["c"]["shared_frames"], "unshared_shared_frames": got["u"]["shared_frames"], "same_bytes": same,
         "nll_per_frame": {m: (-got["c"]["logp"][m].astype(np.float64).mean(-1)).tolist() for m in MOD_ORDER}}
    e.set_profiling(True)      # one profiled call: the stage split (the stream is drained at every stage boundary, per-launch events serialise the stacks)
    t0 = time.perf_counter()
    e.score_clip(clip, 1, cond)
    r["profiled_call_ms"] = (time.perf_counter() - t0) * 1e3
    r["profiled_timings"] = {k: v for k, v in e.timings().items() if k in ("total_ms", "ego_ms", "tar_ms", "oar_ms", "gemm_ms", "gemm_launches", "attn_ms", "attn_launches")}
    e.set_profiling(False)
    e.close()
    res = {}
    if os.path.exists(out):
        with open(out) as f:
            res = json.loads(f.read())
    res["clip"] = r
    print(json.dumps(r))
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


def futures_bench(out, Cn, K, T=20, cond=20):
    """one scene's history against Cn futures of K frames (the frames behind the other synthetic scenes' histories): the futures call, the loop of
    Engine.score calls a user writes without it, and the futures call with nothing shared"""
    cfg = large_config()
    e = Engine(cfg, precision="bf16", max_batch=8, max_cond_frames=cond)
    e.load_state_dict(synthetic_items(cfg, seed=0))
    e.finalize()
    sc = [synthetic_scene(i, n_frames=T + K) for i in range(8)]
    w = {m: sc[0][m][0, :T] for m in MOD_ORDER}
    fut = {m: np.stack([sc[i % 8][m][0, T:] for i in range(Cn)]) for m in MOD_ORDER}
    windows = Engine.future_windows(T, K, cond)
    got = {}

    def loop():
        res = []
        for c in range(Cn):
            seq = {m: np.concatenate([w[m], fut[m][c]]) for m in MOD_ORDER}
            res.append([e.score({m: seq[m][s:s + n] for m in MOD_ORDER}, {m: seq[m][T + k] for m in MOD_ORDER}) for k, s, n, _ in windows])
        got["l"] = res

    def unshared():
        os.environ["UMGEN_SCORE_FUTURES_SHARE"] = "0"
        try:
            got["u"] = e.score_futures(w, fut, cond)
        finally:
            del os.environ["UMGEN_SCORE_FUTURES_SHARE"]
    kinds = ((lambda: got.__setitem__("f", e.score_futures(w, fut, cond)), []), (loop, []), (unshared, []))
    for fn, _ in kinds:
        fn()
    for _ in range(REPS):
        for fn, ts in kinds:
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    tf, tl, tu = (ts for _, ts in kinds)
    same = all(got["f"][kind][m][c, k].tobytes() == got["l"][c][k][kind][m].tobytes() == got["u"][kind][m][c, k].tobytes()
               for kind in ("logp", "argmax") for m in MOD_ORDER for c in range(Cn) for k in range(K))
    med = statistics.median
    r = {"candidates": Cn, "future_frames": K, "history_frames": T, "cond_frames": cond, "reps": REPS,
         "score_futures_ms": med(tf), "score_futures_all_ms": tf, "score_futures_spread_ms": max(tf) - min(tf),
         "score_loop_ms": med(tl), "score_loop_all_ms": tl, "score_loop_spread_ms": max(tl) - min(tl), "loop_over_futures": med(tl) / med(tf),
         "unshared_futures_ms": med(tu), "unshared_futures_all_ms": tu, "unshared_futures_spread_ms": max(tu) - min(tu), "unshared_over_futures": med(tu) / med(tf),
         "shared_slots": got["f"]["shared_slots"].tolist(), "unshared_shared_slots": got["u"]["shared_slots"].tolist(),
         "bytes_compared": int(sum(got["f"][kind][m].nbytes for kind in ("logp", "argmax") for m in MOD_ORDER)), "same_bytes": same,
         "best": int(np.argmax(got["f"]["cum_total"])), "cum_total": got["f"]["cum_total"].tolist()}
    e.set_profiling(True)      # one profiled call: the stage split (the stream is drained at every stage boundary, per-launch events serialise the stacks)
    t0 = time.perf_counter()
    e.score_futures(w, fut, cond)
    r["profiled_call_ms"] = (time.perf_counter() - t0) * 1e3
    r["profiled_timings"] = {k: v for k, v in e.timings().items() if k in ("total_ms", "ego_ms", "tar_ms", "oar_ms", "gemm_ms", "gemm_launches", "attn_ms", "attn_launches")}
    e.set_profiling(False)
    e.close()
    res = {}
    if os.path.exists(out):
        with open(out) as f:
            res = json.loads(f.read())
    res["futures"] = r
    print(json.dumps(r))
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


if FUT:
    futures_bench(args[0] if args else os.path.join(ROOT, "profiles", "score_bench.json"), *FUT)
    sys.exit(0)

if CLIP:
    clip_bench(args[0] if args else os.path.join(ROOT, "profiles", "score_bench.json"))
    sys.exit(0)

cfg = large_config()
e = Engine(cfg, precision="bf16", max_batch=8, max_cond_frames=T)
e.load_state_dict(synthetic_items(cfg, seed=0))
e.finalize()
sc = [synthetic_scene(i, n_frames=T + 1) for i in range(8)]
window = {m: np.concatenate([s[m][:, :T] for s in sc]) for m in MOD_ORDER}
frame = {m: np.concatenate([s[m][:, T] for s in sc]) for m in MOD_ORDER}
one_w, one_f = {m: window[m][0] for m in MOD_ORDER}, {m: frame[m][0] for m in MOD_ORDER}
if CAND:
    candidates_bench(e, sc, args[0] if args else os.path.join(ROOT, "profiles", "score_bench.json"))
    e.close()
    sys.exit(0)

res = {"config": "UMGen_Large synthetic", "precision": "bf16", "history_frames": T, "reps": REPS}
res["score_b1_ms"], res["score_b1_all_ms"] = median_ms(lambda: e.score(one_w, one_f))
res["score_b8_ms"], res["score_b8_all_ms"] = median_ms(lambda: e.score(window, frame))
res["forced_frame_b1_ms"], res["forced_frame_b1_all_ms"] = median_ms(lambda: e.frame(one_w, forced=one_f, trace=False))
res["score_b8_ms_per_scene"] = res["score_b8_ms"] / 8
res["forced_frame_over_score_b1"] = res["forced_frame_b1_ms"] / res["score_b1_ms"]
if DETAIL:
    for tag, w, f in (("b1", one_w, one_f), ("b8", window, frame)):
        plain, det = alternating_ms(lambda: e.score(w, f), lambda: e.score(w, f, detail=True, topk=16, temperature=0.7))
        res[f"detail_{tag}"] = {"score_ms": plain, "score_detail_topk16_ms": det, "extra_ms": det - plain, "ratio": det / plain}
r = e.score(one_w, one_f)
res["nll_b1"] = {m: float(-r["logp"][m].astype(np.float64).mean()) for m in MOD_ORDER}
e.close()
line = json.dumps(res)
print(line)
out = args[0] if args else os.path.join(ROOT, "profiles", "score_bench.json")
with open(out, "w") as f:
    f.write(line + "\n")
