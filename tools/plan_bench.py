#!/usr/bin/env python
"""What a sampling plan (Engine.rollout(sampling=[...], logit_bias=constraints.schedule(...)), umgen_rollout_planned) costs, and what it buys: UMGen_Large,
synthetic weights, bf16, 20 history frames, one engine (max_batch 8), host clock, ms per call; one warm-up call of each kind, then REPS alternating calls.
    settings: an unplanned 8-scene call | the same call with 8 distinct temperatures (one per scene);
    schedule: a one-scene call of 3 frames under one set of ban tables | the same call under a per-frame schedule of three sets, each a copy of those tables
              (the same sampling work: what differs is the pool upload and the per-scene lookup);
    sweep:    8 one-scene calls, one temperature each | the ONE planned 8-scene call that replaces them (the same 8 temperatures, the same scene 8 times).
Every comparison is against the unplanned call of the same shape on the same build.  Run it plainly, not under a tracer.
    python tools/plan_bench.py [out.json]  ->  one JSON line (also written to out.json, default profiles/plan_bench.json)"""
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tools.bias_bench import ban_tables  # noqa: E402
from umgen_amd import constraints  # noqa: E402
from umgen_amd.config import MOD_ORDER, large_config  # noqa: E402
from umgen_amd.engine import Engine  # noqa: E402
from umgen_amd.synth import synthetic_scene  # noqa: E402
from umgen_amd.weights import synthetic_items  # noqa: E402

REPS, NEW, HISTORY, SCENES = 3, 2, 20, 8


def timed(kinds):
    """kinds: name -> callable; one warm-up each, then REPS alternating rounds -> name -> {ms_per_call (median), all, range}"""
    times = {k: [] for k in kinds}
    for fn in kinds.values():
        fn()
    for _ in range(REPS):
        for k, fn in kinds.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"ms_per_call": statistics.median(ts), "all": ts, "range": max(ts) - min(ts)} for k, ts in times.items()}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "plan_bench.json")
    cfg = large_config()
    e = Engine(cfg, precision="bf16", max_batch=SCENES, max_cond_frames=HISTORY)
    e.load_state_dict(synthetic_items(cfg, seed=0))
    e.finalize()
    one = synthetic_scene(0, n_frames=HISTORY)
    eight = {m: np.concatenate([one[m]] * SCENES) for m in MOD_ORDER}
    temps = [0.6 + 0.1 * i for i in range(SCENES)]
    per_scene = [dataclasses.replace(cfg, sfmx_temp=t) for t in temps]
    kw = dict(cond_frames=HISTORY, input_cond_frames=HISTORY)
    seeds8 = list(range(SCENES))
    res = {"config": "UMGen_Large synthetic", "precision": "bf16", "new_frames": NEW, "reps": REPS, "history_frames": HISTORY, "scenes": SCENES}

    res["settings"] = timed({"unplanned_8_scenes": lambda: e.rollout(eight, NEW, seeds=seeds8, **kw),
                             "planned_8_temperatures": lambda: e.rollout(eight, NEW, seeds=seeds8, sampling=per_scene, **kw)})
    tabs = ban_tables(cfg)
    three = constraints.per_frame([{m: t.copy() for m, t in tabs.items()} for _ in range(3)])      # the SAME tables as three sets of the pool, one per frame
    res["schedule"] = timed({"one_set": lambda: e.rollout(one, 3, seeds=[0], logit_bias=tabs, **kw),
                             "three_sets_per_frame": lambda: e.rollout(one, 3, seeds=[0], logit_bias=three, **kw)})
    res["schedule"]["new_frames"] = 3

    def eight_calls():
        for i in range(SCENES):
            e.rollout(one, NEW, seeds=[i], sampling=per_scene[i], **kw)
    res["sweep"] = timed({"eight_one_scene_calls": eight_calls,
                          "one_planned_8_scene_call": lambda: e.rollout(eight, NEW, seeds=seeds8, sampling=per_scene, **kw)})
    e.close()
    res["settings_extra_ms_per_call"] = res["settings"]["planned_8_temperatures"]["ms_per_call"] - res["settings"]["unplanned_8_scenes"]["ms_per_call"]
    res["schedule_extra_ms_per_call"] = res["schedule"]["three_sets_per_frame"]["ms_per_call"] - res["schedule"]["one_set"]["ms_per_call"]
    res["sweep_speedup"] = res["sweep"]["eight_one_scene_calls"]["ms_per_call"] / res["sweep"]["one_planned_8_scene_call"]["ms_per_call"]
    line = json.dumps(res)
    print(line)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
