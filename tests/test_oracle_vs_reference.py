"""The oracle against the reference on inputs that none of the other fixtures cover: the reference's outputs are recorded in
tests/golden/reference_checks.npz by tests/golden/make_reference_checks.py, which also regenerates the seeded inputs used here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_reference_checks as rc  # noqa: E402

from oracle.umgen_oracle import OracleUMGen, check_collision, decode_pose_values  # noqa: E402
from umgen_amd.config import MOD_ORDER  # noqa: E402
from umgen_amd.synth import synthetic_scene  # noqa: E402
from umgen_amd.weights import synthetic_state_dict  # noqa: E402


@pytest.fixture(scope="module")
def ref():
    return np.load(rc.OUT)


def test_live_greedy_frame_matches_reference(ref):
    cfg = rc.greedy_config()
    sd = synthetic_state_dict(cfg, seed=rc.GREEDY_WEIGHT_SEED)
    scene = synthetic_scene(rc.GREEDY_SCENE, n_frames=2)
    out = OracleUMGen(cfg, sd).inference(1, 2, scene, input_cond_frames=2)
    for m in MOD_ORDER:
        np.testing.assert_array_equal(out[m], ref[f"greedy_{m}"], err_msg=m)


def test_pose_decode_and_collision_helpers_match_reference_functions(ref):
    np.testing.assert_array_equal(decode_pose_values(rc.pose_tokens()), ref["pose_values"])
    cases = rc.collision_cases()
    assert len(cases) == len(ref["collision"]) == 200
    for i, boxes in enumerate(cases):
        assert check_collision(boxes) == bool(ref["collision"][i]), i


def test_top_p_sampler_matches_reference_nucleus(ref):
    """sample_top_p (UMGen.py:915-965) with torch.multinomial replaced by the build's inverse-CDF draw must pick the
    same token as OracleUMGen.sample on the same uniform."""
    cfg = rc.topp_config()
    o = OracleUMGen(cfg, synthetic_state_dict(cfg, seed=rc.TOPP_WEIGHT_SEED))
    cases = rc.top_p_cases()
    assert len(cases) == len(ref["topp_tokens"]) == 40
    for trial, (logits, p, u) in enumerate(cases):
        assert o.sample(logits, 5, p, u) == int(ref["topp_tokens"][trial]), (trial, logits.shape[0], p)
