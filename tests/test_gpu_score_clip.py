"""-m gpu: umgen_score_clip on the engine -- every frame of a recorded clip against the frames before it, bit for bit what umgen_score returns for
that frame on its own window (Engine.clip_windows): the growing windows off one pass, the sliding ones in chunks, the per-frame path
(UMGEN_SCORE_CLIP_SHARE=0), two values of max_batch; against the oracle's anchor; around rollouts; refused calls.

The fp32 bar is tests/test_gpu_score.py's: max |logp - anchor| <= 2e-3 per modality."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.golden.make_full_width_golden import SCENE_ID, WEIGHT_SEED, config as width_config
from tests.golden.make_score_golden import TINY_HISTORY, TINY_SCENE, TINY_WEIGHT_SEED
from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.synth import synthetic_scene
from umgen_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
_engines = {}
_refs = {}


def engine(width, precision, max_batch=2):
    key = (width, precision, max_batch)
    if key not in _engines:
        cfg = tiny_config() if width == "tiny" else width_config(width)
        e = Engine(cfg, precision=precision, max_batch=max_batch, max_cond_frames=4)
        e.load_state_dict(synthetic_state_dict(cfg, seed=TINY_WEIGHT_SEED if width == "tiny" else WEIGHT_SEED))
        e.finalize()
        _engines[key] = e
    return _engines[key]


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()
    _refs.clear()


def clips(B, L, scene0=SCENE_ID + 1):
    """B recorded clips [B, L, S]"""
    sc = [synthetic_scene(scene0 + i, n_frames=L) for i in range(B)]
    return {m: np.concatenate([s[m][:, :L] for s in sc]) for m in MOD_ORDER}


def singles(e, clip, input_frames, cond_frames):
    """Engine.score per (b, f) on the frame's own window, stacked to [B, F, S]"""
    B, L = clip["pose"].shape[:2]
    res = [[e.score({m: clip[m][b, s:s + n] for m in MOD_ORDER}, {m: clip[m][b, f] for m in MOD_ORDER})
            for f, s, n in Engine.clip_windows(L, input_frames, cond_frames)] for b in range(B)]
    return {kind: {m: np.stack([np.stack([r[kind][m] for r in row]) for row in res]) for m in MOD_ORDER} for kind in ("logp", "argmax")}


def growing_ref(width, precision):
    """the per-frame reference of the growing-only case, computed once per engine kind"""
    key = (width, precision)
    if key not in _refs:
        _refs[key] = singles(engine(width, precision), clips(2, 5), 1, 4)
    return _refs[key]


def same_bytes(a, b, what):
    for kind in ("logp", "argmax"):
        for m in MOD_ORDER:
            assert a[kind][m].shape == b[kind][m].shape and a[kind][m].dtype == b[kind][m].dtype, (what, kind, m)
            assert a[kind][m].tobytes() == b[kind][m].tobytes(), (what, kind, m, np.argwhere(a[kind][m] != b[kind][m])[:4].tolist())


class share_off:
    def __enter__(self):
        self.old = os.environ.get("UMGEN_SCORE_CLIP_SHARE")
        os.environ["UMGEN_SCORE_CLIP_SHARE"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["UMGEN_SCORE_CLIP_SHARE"]
        else:
            os.environ["UMGEN_SCORE_CLIP_SHARE"] = self.old


@pytest.mark.parametrize("width,precision", [("tiny", "fp32"), ("full_width", "bf16"), ("full_width", "fp16")])
def test_growing_windows_share_one_pass_with_the_bits_of_their_own_score_calls(width, precision):
    e = engine(width, precision)
    clip = clips(2, 5)
    got = e.score_clip(clip, 1, 4)
    assert got["shared_frames"] == 4 and got["frames"].tolist() == [1, 2, 3, 4]
    same_bytes(got, growing_ref(width, precision), "growing windows")
    for m in MOD_ORDER:
        assert got["logp"][m].shape == (2, 4, CONTENT_LEN[m]) and np.isfinite(got["logp"][m]).all() and (got["logp"][m] <= 0).all()
    total = sum(got["logp"][m].astype(np.float64).sum(-1) for m in MOD_ORDER)
    assert got["total"].dtype == np.float64 and got["total"].shape == (2, 4) and np.array_equal(got["total"], total)
    # frame 3's pose tokens alone: the pose shift hands them to slot 2, which only frame 3's (and later frames') windows read as their
    # last slot -- frame 3's map scores move (the warp by the ego motion), frames 1 and 2 keep their bytes (causality)
    other = dict(clip, pose=clip["pose"].copy())
    other["pose"][:, 3] = synthetic_scene(SCENE_ID + 7, n_frames=5)["pose"][0, 3]
    assert not np.array_equal(other["pose"][:, 3], clip["pose"][:, 3])
    moved = e.score_clip(other, 1, 4)
    assert not np.array_equal(moved["logp"]["map"][:, 2], got["logp"]["map"][:, 2])
    for kind in ("logp", "argmax"):
        for m in MOD_ORDER:
            assert moved[kind][m][:, :2].tobytes() == got[kind][m][:, :2].tobytes(), (kind, m)


@pytest.mark.parametrize("width,precision", [("tiny", "fp32"), ("full_width", "bf16")])
def test_growing_then_sliding_windows(width, precision):
    e = engine(width, precision)      # max_batch 2: frames 2 and 3 shared, frames 4, 5, 6 sliding -- 6 items in 3 chunks
    clip = clips(2, 7)
    got = e.score_clip(clip, 2, 3)
    assert got["shared_frames"] == 2 and got["frames"].tolist() == [2, 3, 4, 5, 6]
    same_bytes(got, singles(e, clip, 2, 3), "growing + sliding")


def test_edge_plans():
    e = engine("tiny", "fp32")
    clip = clips(2, 6)
    got = e.score_clip(clip, 4, 2)      # input_frames > cond_frames: every window slides
    assert got["shared_frames"] == 0 and got["frames"].tolist() == [4, 5]
    same_bytes(got, singles(e, clip, 4, 2), "sliding only")
    two = {m: clip[m][:, :3] for m in MOD_ORDER}
    got = e.score_clip(two, 2)          # L = input_frames + 1: one frame, Engine.score itself
    assert got["shared_frames"] == 0 and got["logp"]["map"].shape == (2, 1, 1024)
    one = e.score({m: two[m][:, :2] for m in MOD_ORDER}, {m: two[m][:, 2] for m in MOD_ORDER})
    for kind in ("logp", "argmax"):
        for m in MOD_ORDER:
            assert got[kind][m][:, 0].tobytes() == one[kind][m].tobytes(), (kind, m)
    # un-batched inputs: [L, S]
    five = clips(2, 5)
    flat = e.score_clip({m: five[m][1] for m in MOD_ORDER}, 1, 4)
    ref = growing_ref("tiny", "fp32")
    assert flat["shared_frames"] == 4 and flat["total"].shape == (4,)
    for kind in ("logp", "argmax"):
        for m in MOD_ORDER:
            assert flat[kind][m].tobytes() == ref[kind][m][1].tobytes(), (kind, m)


@pytest.mark.parametrize("width,precision", [("tiny", "fp32"), ("full_width", "bf16")])
def test_same_bytes_on_the_per_frame_path_and_with_another_max_batch(width, precision):
    clip = clips(2, 7)
    e = engine(width, precision)
    got = e.score_clip(clip, 2, 3)
    with share_off():
        rep = e.score_clip(clip, 2, 3)
    assert got["shared_frames"] == 2 and rep["shared_frames"] == 0
    same_bytes(rep, got, "per-frame path against the shared path")
    wide = engine(width, precision, max_batch=8).score_clip(clip, 2, 3)
    assert wide["shared_frames"] == 2
    same_bytes(wide, got, "max_batch 8 against max_batch 2")


def test_fp32_tiny_last_frame_lies_within_the_bar_of_the_oracle_anchor():
    g = np.load(os.path.join(GOLD, "score_tiny.npz"))
    full = synthetic_scene(TINY_SCENE, n_frames=TINY_HISTORY + 1)
    res = engine("tiny", "fp32").score_clip({m: full[m][0] for m in MOD_ORDER}, 1)
    assert res["shared_frames"] == TINY_HISTORY == 3 and res["frames"].tolist() == [1, 2, 3]
    for m in MOD_ORDER:
        d = float(np.abs(res["logp"][m][-1] - g[f"logp_{m}"]).max())
        print(f"tiny fp32 {m}: max |logp - anchor| {d:.3g}")
        assert d <= 2e-3, (m, d)


def test_clip_scoring_leaves_a_rollout_unchanged_and_repeats_itself():
    e = engine("full_width", "bf16", max_batch=1)      # one scene per call: the background workers of the decode engine are on
    scene = synthetic_scene(SCENE_ID, n_frames=2)
    clip = {m: v[0] for m, v in clips(1, 5).items()}
    before = e.rollout(scene, 2, cond_frames=3, input_cond_frames=2, seeds=[5])
    a = e.score_clip(clip, 1, 3)
    after = e.rollout(scene, 2, cond_frames=3, input_cond_frames=2, seeds=[5])
    b = e.score_clip(clip, 1, 3)
    assert a["shared_frames"] == b["shared_frames"] == 3
    for m in MOD_ORDER:
        np.testing.assert_array_equal(before[m], after[m], err_msg=m)
    same_bytes(a, b, "the call repeated")


def raw_call(e, clip, B, L, T_in, cond, out="make", shared=None):
    """umgen_score_clip itself, past the Python checks"""
    c = [np.ascontiguousarray(clip[m], dtype=np.int64) for m in MOD_ORDER]
    keep = [np.zeros(max(B * (L - T_in), 1) * CONTENT_LEN[m], np.float32) for m in MOD_ORDER]
    if out == "make":
        out = C.byref(_lib.ScoreOut(**{f"logp_{m}": k.ctypes.data_as(C.POINTER(C.c_float)) for m, k in zip(MOD_ORDER, keep)}))      # arg-max pointers NULL
    rc = e.lib.umgen_score_clip(e._h, B, L, T_in, cond, *[a.ctypes.data_as(C.POINTER(C.c_int64)) for a in c], out, shared)
    return rc, e.lib.umgen_last_error(e._h).decode(), keep


def test_refused_calls_leave_the_engine_usable():
    e = engine("tiny", "fp32")
    clip = clips(2, 5)
    ref = growing_ref("tiny", "fp32")
    c3 = clips(3, 5)
    bad = dict(clip, image=clip["image"].copy())
    bad["image"][1, 2, 9] = 8192
    for what, args, needle in (("T_in = 0", (clip, 2, 5, 0, 4), "T_in=0"), ("T_in = L", (clip, 2, 5, 5, 4), "T_in=5"),
                               ("cond_frames > max_cond_frames", (clip, 2, 5, 1, 5), "cond_frames=5"), ("B > max_batch", (c3, 3, 5, 1, 4), "B=3"),
                               ("NULL out", (clip, 2, 5, 1, 4, None), "null output"), ("token >= vocab", (bad, 2, 5, 1, 4), "8192")):
        rc, msg, _ = raw_call(e, *args)
        assert rc == -1 and needle in msg, (what, rc, msg)
    with pytest.raises(UMGenError):
        e.score_clip(c3, 1, 4)
    rc, _, keep = raw_call(e, clip, 2, 5, 1, 4)      # NULL arg-max pointers and a NULL shared_frames are fine
    assert rc == 0
    again = e.score_clip(clip, 1, 4)
    for m, k in zip(MOD_ORDER, keep):
        assert k.tobytes() == ref["logp"][m].tobytes() == again["logp"][m].tobytes(), m
