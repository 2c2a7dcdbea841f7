#!/usr/bin/env python
"""What constrained sampling (Engine.rollout(logit_bias=..., return_logz=True), umgen_rollout_biased) costs: UMGen_Large, synthetic weights, bf16, one
scene, 20 history frames, the flagship rollout of bench.py.
    off: the cost the default path pays for the feature existing.  `bench.py --gpus 1 --steps 30 --warmup 1` of the parent commit and of this tree, three
         runs each, alternating, in one session: pass the six JSON result lines with --off parent.jsonl branch.jsonl (one line per run).  "off_ok": the
         branch's median ms_per_step exceeds the parent's by no more than the spread (max - min) of the parent's own three runs.
    on:  measured here, on one engine: NEW new frames per call, one warm-up call of each kind, then REPS alternating calls of
         plain (no tables) | bans (ban tables on all four classes) | bans + logz (the same with return_logz), host clock, ms per frame; medians and ranges.
    python tools/bias_bench.py [out.json] [--off parent.jsonl branch.jsonl]  ->  one JSON line (also written to out.json, default profiles/bias_bench.json)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from umgen_amd import constraints  # noqa: E402
from umgen_amd.config import large_config  # noqa: E402
from umgen_amd.engine import Engine  # noqa: E402
from umgen_amd.synth import synthetic_scene  # noqa: E402
from umgen_amd.weights import synthetic_items  # noqa: E402

REPS, NEW, HISTORY = 3, 3, 20


def ban_tables(cfg):
    """bans on all four classes: no pedestrians, a pose envelope, and every fourth map / image code"""
    val = constraints.scene_io.decode_ego_numpy(np.repeat(np.arange(cfg.pose_vocab_size)[:, None], 3, axis=1)).reshape(-1, 3)
    lim = [tuple(sorted((float(val[256, c]), float(val[768, c])))) for c in range(3)]
    return constraints.merge(constraints.ban_categories(["pedestrian"], vocab=cfg.bbox3d_vocab_size),
                             constraints.pose_limits(dx=lim[0], dy=lim[1], dheading=lim[2], vocab=cfg.pose_vocab_size),
                             constraints.ban("map", range(0, cfg.map_vocab_size, 4), vocab=cfg.map_vocab_size),
                             constraints.ban("image", range(0, cfg.img_vocab_size, 4), vocab=cfg.img_vocab_size))


def cost_when_on():
    cfg = large_config()
    e = Engine(cfg, precision="bf16", max_batch=1, max_cond_frames=HISTORY)
    e.load_state_dict(synthetic_items(cfg, seed=0))
    e.finalize()
    sc = synthetic_scene(0, n_frames=HISTORY)
    tabs = ban_tables(cfg)
    kw = dict(cond_frames=HISTORY, input_cond_frames=HISTORY, seeds=[0])
    kinds = {"plain": {}, "bans": dict(logit_bias=tabs), "bans_logz": dict(logit_bias=tabs, return_logz=True)}
    times = {k: [] for k in kinds}
    for extra in kinds.values():
        e.rollout(sc, NEW, **kw, **extra)
    for _ in range(REPS):
        for k, extra in kinds.items():
            t0 = time.perf_counter()
            e.rollout(sc, NEW, **kw, **extra)
            times[k].append((time.perf_counter() - t0) * 1e3 / NEW)
    e.close()
    res = {"new_frames": NEW, "reps": REPS, "history_frames": HISTORY}
    for k, ts in times.items():
        res[k] = {"ms_per_frame": statistics.median(ts), "all": ts, "range": max(ts) - min(ts)}
    res["bans_extra_ms_per_frame"] = res["bans"]["ms_per_frame"] - res["plain"]["ms_per_frame"]
    res["logz_extra_ms_per_frame"] = res["bans_logz"]["ms_per_frame"] - res["bans"]["ms_per_frame"]
    return res


def cost_when_off(parent_path, branch_path):
    def runs(path):
        return [json.loads(ln)["ms_per_step"] for ln in open(path) if ln.strip().startswith("{")]
    p, b = runs(parent_path), runs(branch_path)
    res = {"parent_ms_per_step": p, "branch_ms_per_step": b, "parent_median": statistics.median(p), "branch_median": statistics.median(b),
           "parent_spread": max(p) - min(p)}
    res["off_ok"] = res["branch_median"] - res["parent_median"] <= res["parent_spread"]
    return res


def main():
    args = sys.argv[1:]
    off = None
    if "--off" in args:
        i = args.index("--off")
        off = cost_when_off(args[i + 1], args[i + 2])
        del args[i:i + 3]
    out = args[0] if args else os.path.join(ROOT, "profiles", "bias_bench.json")
    res = {"config": "UMGen_Large synthetic", "precision": "bf16", "scenes": 1, "on": cost_when_on()}
    if off is not None:
        res["off"] = off
    line = json.dumps(res)
    print(line)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
