"""tests/golden/detail_tiny.npz: the frame tests/test_gpu_rollout_detail.py forces when it holds the decode steps' rank to the one-pass rank of
Engine.score(detail=True).  The two differ in summation order (bar 2e-3 on a log-probability, tests/test_gpu_score.py), so the ranks can only be
compared where no other logit lies within 2e-3 of the scored token's.

The frame scored in tests/golden/score_tiny.npz is a recorded one: its tokens sit at random ranks of 8192-wide rows whose logits have a standard
deviation of 0.58, and the CPU oracle's rows put another logit within 2e-3 of the token's at 2001 of its 2199 positions -- nothing would be left to
compare.  This frame is chosen on the CPU instead, by the oracle alone: the same weights and window, and at every decode step, among the step's
top-k logits (the reference's 5 / 5 / 16), the token whose logit is farthest from its nearest neighbour; no resampling through head_tar_bbox3d and no
rule constraint, so every token is chosen on the AR row it is later ranked on.  Stored: the tokens, and `near`, the count of positions where the
oracle's own rows still have another logit within 2e-3 of the token's (the test excludes positions by the traced rows of its own call and holds
their count to 1 % of 2199).

    python tests/golden/make_detail_golden.py"""
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.umgen_oracle import OracleUMGen  # noqa: E402
from tests.golden.make_score_golden import case  # noqa: E402
from umgen_amd.config import MOD_ORDER  # noqa: E402

NEAR = 2e-3


class IsolatedChoice(OracleUMGen):
    def sample(self, logits, k, p, u):
        v = logits.double().numpy()
        top = np.argsort(-v, kind="stable")[:max(1, int(k))]
        srt = np.sort(v)
        at = np.searchsorted(srt, v[top])
        lo = np.where(at > 0, v[top] - srt[np.maximum(at - 1, 0)], np.inf)
        hi = np.where(at + 1 < len(srt), srt[np.minimum(at + 1, len(srt) - 1)] - v[top], np.inf)
        return int(top[np.argmax(np.minimum(lo, hi))])


def compute():
    cfg, sd, scene, T, _ = case("tiny")
    cfg = dataclasses.replace(cfg, sample_method="topk", top_k=5, top_k_map=5, topk_image=16, rule_constrain=False, merage_ar_tar=False)
    o = IsolatedChoice(cfg, sd, weight_dtype="fp32")
    out = o.inference(1, T, scene, input_cond_frames=T, trace=True, seed=0)
    frame = {m: np.asarray(out[m])[0, T] for m in MOD_ORDER}
    rows = dict(o.trace["logits"][0], pose=o.trace["ego_logits"][0])
    near = 0
    for m in MOD_ORDER:
        lg = rows[m].astype(np.float64)
        t = lg[np.arange(lg.shape[0]), frame[m]][:, None]
        near += int((((np.abs(lg - t) <= NEAR).sum(1) - 1) > 0).sum())
    res = {f"tok_{m}": frame[m].astype(np.int16) for m in MOD_ORDER}
    res["near"] = np.int64(near)
    return res


if __name__ == "__main__":
    res = compute()
    path = os.path.join(ROOT, "tests", "golden", "detail_tiny.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "positions with another logit within", NEAR, "of the token's:", int(res["near"]), "of 2199")
