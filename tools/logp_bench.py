#!/usr/bin/env python
"""What asking for the log-likelihoods of a rollout costs: the bench shape (UMGen_Large, synthetic weights, bf16, one scene, a window of T = 20
history frames, top-k 5 / 5 / 16 sampling) rolled out for --frames new frames with and without return_logp.  After one warm-up call each: the median
of 5 host-clock calls, alternating the two kinds of call; the tokens of both must be equal.
    python tools/logp_bench.py [out.json] [--frames=5] [--T=20]  ->  one JSON line (also written to out.json, default profiles/rollout_logp_bench.json)"""
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

cfg = large_config()
e = Engine(cfg, precision="bf16", max_batch=1, max_cond_frames=T)
e.load_state_dict(synthetic_items(cfg, seed=0))
e.finalize()
scene = synthetic_scene(0, n_frames=T)
kw = dict(cond_frames=T, input_cond_frames=T, seeds=[1000])


def timed(return_logp):
    t0 = time.perf_counter()
    out = e.rollout(scene, FRAMES, return_logp=return_logp, **kw)
    return (time.perf_counter() - t0) * 1e3, out


_, plain = timed(False)      # warm-up of both kinds (the step graphs are captured once and serve both)
_, (toks, logp) = timed(True)
assert all(np.array_equal(plain[m], toks[m]) for m in MOD_ORDER), "return_logp changed the tokens"
ts = {False: [], True: []}
for _ in range(REPS):
    for kind in (False, True):
        ts[kind].append(timed(kind)[0])
tm = e.timings()
res = {"config": "UMGen_Large synthetic", "precision": "bf16", "history_frames": T, "new_frames": FRAMES, "reps": REPS,
       "rollout_ms": statistics.median(ts[False]), "rollout_all_ms": ts[False],
       "rollout_logp_ms": statistics.median(ts[True]), "rollout_logp_all_ms": ts[True],
       "decode_engine": int(tm["decode_engine"]), "overlapped_frames": int(tm["overlapped_frames"])}
res["extra_ms_per_frame"] = (res["rollout_logp_ms"] - res["rollout_ms"]) / FRAMES
res["extra_us_per_decode_step"] = res["extra_ms_per_frame"] * 1e3 / 2206
res["extra_fraction"] = res["rollout_logp_ms"] / res["rollout_ms"] - 1.0
res["mean_logp"] = {m: float(np.nanmean(logp[m].astype(np.float64))) for m in MOD_ORDER}
e.close()
line = json.dumps(res)
print(line)
out = args[0] if args else os.path.join(ROOT, "profiles", "rollout_logp_bench.json")
with open(out, "w") as f:
    f.write(line + "\n")
