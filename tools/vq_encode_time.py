#!/usr/bin/env python
"""Timing line of the VQ encoders, the counterpart of tools/vq_time.py: umgen_vqenc_encode of the two
production configurations (image: 3 x 256 x 512 -> 16 x 32 tokens, map: 5 x 256 x 256 -> 32 x 32 tokens), 20 frames per call after
one warm-up call, fp32 on the matrix cores (v_mfma_f32_32x32x2_f32; UMGEN_FP32_MFMA=0: the VALU FMA-chain kernel).  The host clock
spans the whole call (it ends in the last frame's stream synchronise) and so includes the uploads and the host-side finite check.
    python tools/vq_encode_time.py [out.json]  ->  one JSON line (also written to out.json, default profiles/vq_encode_time.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.golden.make_vq_golden import FULL, SEED  # noqa: E402
from umgen_amd.vq import VQEncoder, encoder_keys, synth_vq_raster, synth_vq_tensor  # noqa: E402

res = {"mode": "valu" if os.environ.get("UMGEN_FP32_MFMA") == "0" else "mfma_f32_32x32x2"}
for name, cfg in FULL.items():
    e = VQEncoder(cfg)
    e.load_state_dict({k: synth_vq_tensor(k, s, SEED) for k, s in encoder_keys(cfg).items()})
    x = synth_vq_raster(cfg, 20, 1)
    e.encode(x[:1])
    t0 = time.perf_counter()
    codes = e.encode(x)
    dt = time.perf_counter() - t0
    e.close()
    res[name] = {"frames": 20, "seconds": dt, "ms_per_frame": dt * 1e3 / 20, "codes_shape": list(codes.shape)}
line = json.dumps(res)
print(line)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vq_encode_time.json")
with open(out, "w") as f:
    f.write(line + "\n")
