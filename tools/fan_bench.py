#!/usr/bin/env python
"""Timing of umgen_rollout_fan (Engine.rollout(samples=N): N sampled futures of one scene, the history once per scene) against the only earlier route
to the same tokens, Engine.rollout on the history replicated N times: UMGen_Large, synthetic weights, bf16, one scene, an engine of 8 scenes, N = 8,
in two settings --
    full:    20 history frames, cond_frames 20, 1 new frame (the window is full: only the first frame's history is shared);
    growing: 13 history frames, cond_frames 20, 3 new frames (the window grows: the fan frame must also leave the slot caches ready for frames 2, 3).
Protocol: host clock, one warm-up call of each kind, then 5 alternating calls of the fan call and the replicated call on the same engine; medians,
ranges (max - min), shared_slots, overlapped_frames of either call, byte equality of tokens and log-likelihoods, the ego / stacks / decode split of
the last timed call of each kind (the engine's own events, summed over the call's frames), and in the one-frame setting one profiled call of each
kind (per-launch events, no step graphs: its decode time is not comparable with the unprofiled one).
"keep_default": the fan call's median lies below the replicated call's by more than the larger of the two ranges, in both settings.
    python tools/fan_bench.py [out.json]  ->  one JSON line (also written to out.json, default profiles/fan_bench.json)"""
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

REPS, N = 5, 8
SETTINGS = {"full": dict(history=20, cond_frames=20, new_frames=1), "growing": dict(history=13, cond_frames=20, new_frames=3)}
SPLIT = ("total_ms", "ego_ms", "tar_ms", "oar_ms", "frames", "overlapped_frames")


def setting(e, history, cond_frames, new_frames):
    sc = synthetic_scene(0, n_frames=history)
    rep = {m: np.repeat(sc[m], N, axis=0) for m in MOD_ORDER}
    seeds = np.arange(100, 100 + N)
    kw = dict(cond_frames=cond_frames, input_cond_frames=history, return_logp=True)
    got, tm = {}, {}

    def fan():
        got["f"] = e.rollout(sc, new_frames, seeds=seeds, samples=N, **kw)
        tm["f"] = {k: v for k, v in e.timings().items() if k in SPLIT}

    def replicated():
        got["r"] = e.rollout(rep, new_frames, seeds=seeds, **kw)
        tm["r"] = {k: v for k, v in e.timings().items() if k in SPLIT}
    fan()
    replicated()
    tf, tr = [], []
    for _ in range(REPS):
        for fn, ts in ((fan, tf), (replicated, tr)):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    same = all(got["f"][k][m].tobytes() == got["r"][k][m].tobytes() for k in (0, 1) for m in MOD_ORDER)
    med = statistics.median
    r = {"history_frames": history, "cond_frames": cond_frames, "new_frames": new_frames, "samples": N, "reps": REPS,
         "fan_ms": med(tf), "fan_all_ms": tf, "fan_range_ms": max(tf) - min(tf),
         "replicated_ms": med(tr), "replicated_all_ms": tr, "replicated_range_ms": max(tr) - min(tr),
         "saved_ms": med(tr) - med(tf), "ratio": med(tr) / med(tf), "shared_slots": e.last_shared_slots,
         "overlapped_frames_fan": tm["f"]["overlapped_frames"], "overlapped_frames_replicated": tm["r"]["overlapped_frames"], "same_bytes": same,
         "fan_timings": tm["f"], "replicated_timings": tm["r"]}
    r["fan_wins"] = r["saved_ms"] > max(r["fan_range_ms"], r["replicated_range_ms"])
    if new_frames == 1:
        e.set_profiling(True)
        for tag, key, fn in (("fan", "f", fan), ("replicated", "r", replicated)):
            t0 = time.perf_counter()
            fn()
            r[f"profiled_{tag}_call_ms"] = (time.perf_counter() - t0) * 1e3
            r[f"profiled_{tag}_timings"] = tm[key]
        e.set_profiling(False)
    return r


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "profiles", "fan_bench.json"))
    cfg = large_config()
    e = Engine(cfg, precision="bf16", max_batch=8, max_cond_frames=20)
    e.load_state_dict(synthetic_items(cfg, seed=0))
    e.finalize()
    res = {"config": "UMGen_Large synthetic", "precision": "bf16", "scenes": 1, "max_batch": 8}
    for name, kw in SETTINGS.items():
        res[name] = setting(e, **kw)
        print(name, json.dumps(res[name]), flush=True)
    e.close()
    res["keep_default"] = all(res[name]["fan_wins"] for name in SETTINGS)
    line = json.dumps(res)
    print(line)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
