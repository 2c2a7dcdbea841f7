#!/usr/bin/env python
"""What asking for the diagnostics of a rollout costs: the bench shape (UMGen_Large, synthetic weights, bf16, one scene, a window of T = 20 history
frames, top-k 5 / 5 / 16 sampling) rolled out for --frames new frames with return_logp, and with return_logp + return_detail, topk=16.  After one
warm-up call of each kind: the median of 5 host-clock calls, alternating the two kinds of call; tokens and logp of both must have the same bits.
    python tools/detail_bench.py [out.json] [--frames=5] [--T=20]  ->  one JSON line (also written to out.json, default profiles/rollout_detail_bench.json)"""
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
FRAMES = next((int(a[9:]) for a in sys.argv[1:] if a.startswith("--frames=")), 5)
REPS = 5
TOPK = 16

cfg = large_config()
e = Engine(cfg, precision="bf16", max_batch=1, max_cond_frames=T)
e.load_state_dict(synthetic_items(cfg, seed=0))
e.finalize()
scene = synthetic_scene(0, n_frames=T)
kw = dict(cond_frames=T, input_cond_frames=T, seeds=[1000], return_logp=True)


def timed(detail):
    t0 = time.perf_counter()
    out = e.rollout(scene, FRAMES, return_detail=detail, topk=TOPK if detail else 0, **kw)
    return (time.perf_counter() - t0) * 1e3, out


_, (plain, plain_lp) = timed(False)      # warm-up of both kinds (the step graphs are captured once and serve both)
_, (toks, logp, det) = timed(True)
assert all(np.array_equal(plain[m], toks[m]) for m in MOD_ORDER), "return_detail changed the tokens"
assert all(plain_lp[m].tobytes() == logp[m].tobytes() for m in MOD_ORDER), "return_detail changed logp"
ts = {False: [], True: []}
for _ in range(REPS):
    for kind in (False, True):
        ts[kind].append(timed(kind)[0])
tm = e.timings()
res = {"config": "UMGen_Large synthetic", "precision": "bf16", "history_frames": T, "new_frames": FRAMES, "reps": REPS, "topk": TOPK,
       "rollout_logp_ms": statistics.median(ts[False]), "rollout_logp_all_ms": ts[False],
       "rollout_detail_ms": statistics.median(ts[True]), "rollout_detail_all_ms": ts[True],
       "decode_engine": int(tm["decode_engine"]), "overlapped_frames": int(tm["overlapped_frames"])}
res["extra_ms_per_frame"] = (res["rollout_detail_ms"] - res["rollout_logp_ms"]) / FRAMES
res["extra_us_per_decode_step"] = res["extra_ms_per_frame"] * 1e3 / 2206
res["extra_fraction"] = res["rollout_detail_ms"] / res["rollout_logp_ms"] - 1.0
res["mean_entropy"] = {m: float(np.nanmean(det["entropy"][m].astype(np.float64))) for m in MOD_ORDER}
res["mean_rank"] = {m: float(det["rank"][m].mean()) for m in MOD_ORDER}
e.close()
line = json.dumps(res)
print(line)
out = args[0] if args else os.path.join(ROOT, "profiles", "rollout_detail_bench.json")
with open(out, "w") as f:
    f.write(line + "\n")
