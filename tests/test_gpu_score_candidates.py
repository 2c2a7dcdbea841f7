"""-m gpu: umgen_score_candidates on the engine -- C candidate next frames per scene against one history, bit for bit what umgen_score
returns per (scene, candidate), on the shared path (history slots once per scene, the candidates' last slots through attn_temporal_fan_kernel),
on the replicated path (UMGEN_SCORE_SHARE=0, T = 1), in one chunk and in two; against the oracle's anchor; around rollouts; refused calls.

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


def engine(width, precision, max_batch=1):
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


def case(B, T, scene0=SCENE_ID + 1):
    """B windows [B, T, S] and 3 candidates per scene [B, 3, S]: the scene's own next frame, that frame with another scene's pose tokens, and the
    next frame of another scene"""
    sc = [synthetic_scene(scene0 + i, n_frames=T + 1) for i in range(B + 1)]
    window = {m: np.concatenate([s[m][:, :T] for s in sc[:B]]) for m in MOD_ORDER}
    cand = {}
    for m in MOD_ORDER:
        rows = []
        for b in range(B):
            own, other = sc[b][m][0, T], sc[b + 1][m][0, T]
            rows.append(np.stack([own, other if m == "pose" else own, other]))
        cand[m] = np.stack(rows)
    assert all(not np.array_equal(cand["pose"][b, 0], cand["pose"][b, 1]) for b in range(B))
    return window, cand


def singles(e, window, cand):
    """Engine.score per (b, c), stacked to [B, C, S]"""
    B, Cn = cand["pose"].shape[:2]
    res = [[e.score({m: window[m][b] for m in MOD_ORDER}, {m: cand[m][b, c] for m in MOD_ORDER}) for c in range(Cn)] for b in range(B)]
    return {kind: {m: np.stack([np.stack([res[b][c][kind][m] for c in range(Cn)]) for b in range(B)]) for m in MOD_ORDER} for kind in ("logp", "argmax")}


def same_bytes(a, b, what):
    for kind in ("logp", "argmax"):
        for m in MOD_ORDER:
            assert a[kind][m].shape == b[kind][m].shape and a[kind][m].dtype == b[kind][m].dtype, (what, kind, m)
            assert a[kind][m].tobytes() == b[kind][m].tobytes(), (what, kind, m, np.argwhere(a[kind][m] != b[kind][m])[:4].tolist())


class share_off:
    def __enter__(self):
        self.old = os.environ.get("UMGEN_SCORE_SHARE")
        os.environ["UMGEN_SCORE_SHARE"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["UMGEN_SCORE_SHARE"]
        else:
            os.environ["UMGEN_SCORE_SHARE"] = self.old


@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("width,precision", [("tiny", "fp32"), ("full_width", "bf16"), ("full_width", "fp16")])
def test_every_candidate_has_the_bits_of_its_own_score_call(width, precision, T):
    window, cand = case(2, T)
    chunked, whole = engine(width, precision, max_batch=3), engine(width, precision, max_batch=8)      # 6 items: two chunks | one
    ref = singles(chunked, window, cand)
    got = chunked.score_candidates(window, cand)
    assert got["shared_slots"] == T - 1
    same_bytes(got, ref, "two chunks")
    one = whole.score_candidates(window, cand)
    assert one["shared_slots"] == T - 1
    same_bytes(one, got, "one chunk against two")
    for m in MOD_ORDER:
        assert got["logp"][m].shape == (2, 3, CONTENT_LEN[m]) and np.isfinite(got["logp"][m]).all() and (got["logp"][m] <= 0).all()
    # the pose tokens alone change what the map stack sees in its last slot (the warp by the ego motion)
    assert not np.array_equal(got["logp"]["map"][:, 0], got["logp"]["map"][:, 1])
    total = sum(got["logp"][m].astype(np.float64).sum(-1) for m in MOD_ORDER)
    assert got["total"].dtype == np.float64 and np.array_equal(got["total"], total)
    with share_off():
        rep = chunked.score_candidates(window, cand)
    assert rep["shared_slots"] == 0
    same_bytes(rep, got, "replicated path against the shared path")
    # un-batched inputs: [T, S] with [C, S]
    flat = chunked.score_candidates({m: window[m][1] for m in MOD_ORDER}, {m: cand[m][1] for m in MOD_ORDER})
    for m in MOD_ORDER:
        assert flat["logp"][m].tobytes() == got["logp"][m][1].tobytes() and flat["total"].shape == (3,)


def test_one_history_frame_takes_the_replicated_path():
    e = engine("tiny", "fp32", max_batch=3)
    window, cand = case(2, 1)
    got = e.score_candidates(window, cand)
    assert got["shared_slots"] == 0
    same_bytes(got, singles(e, window, cand), "T = 1")


def test_fp32_tiny_candidate_lies_within_the_bar_of_the_oracle_anchor():
    g = np.load(os.path.join(GOLD, "score_tiny.npz"))
    full = synthetic_scene(TINY_SCENE, n_frames=TINY_HISTORY + 1)
    other = synthetic_scene(TINY_SCENE + 1, n_frames=TINY_HISTORY + 1)
    window = {m: full[m][0, :TINY_HISTORY] for m in MOD_ORDER}
    cand = {m: np.stack([full[m][0, TINY_HISTORY], other[m][0, TINY_HISTORY]]) for m in MOD_ORDER}
    res = engine("tiny", "fp32", max_batch=3).score_candidates(window, cand)
    assert res["shared_slots"] == TINY_HISTORY - 1 == 2
    for m in MOD_ORDER:
        d = float(np.abs(res["logp"][m][0] - g[f"logp_{m}"]).max())
        print(f"tiny fp32 {m}: max |logp - anchor| {d:.3g}")
        assert d <= 2e-3, (m, d)


def test_candidates_leave_a_rollout_unchanged_and_repeat_themselves():
    e = engine("full_width", "bf16")      # one scene per call: the background workers of the decode engine are on
    scene = synthetic_scene(SCENE_ID, n_frames=2)
    window, cand = case(1, 2)
    before = e.rollout(scene, 2, cond_frames=3, input_cond_frames=2, seeds=[5])
    a = e.score_candidates(window, cand)
    after = e.rollout(scene, 2, cond_frames=3, input_cond_frames=2, seeds=[5])
    b = e.score_candidates(window, cand)
    assert a["shared_slots"] == b["shared_slots"] == 1
    for m in MOD_ORDER:
        np.testing.assert_array_equal(before[m], after[m], err_msg=m)
    same_bytes(a, b, "the call repeated")


def raw_call(e, window, cand, B, T, Cn, out="make"):
    """umgen_score_candidates itself, past the Python checks"""
    p = lambda a: np.ascontiguousarray(a, dtype=np.int64)  # noqa: E731
    w, f = [p(window[m]) for m in MOD_ORDER], [p(cand[m]) for m in MOD_ORDER]
    keep = [np.zeros(max(B * Cn, 1) * CONTENT_LEN[m], np.float32) for m in MOD_ORDER]
    if out == "make":
        out = C.byref(_lib.ScoreOut(**{f"logp_{m}": k.ctypes.data_as(C.POINTER(C.c_float)) for m, k in zip(MOD_ORDER, keep)}))      # arg-max pointers NULL
    i64p = C.POINTER(C.c_int64)
    rc = e.lib.umgen_score_candidates(e._h, B, T, Cn, *[a.ctypes.data_as(i64p) for a in w], *[a.ctypes.data_as(i64p) for a in f], out, None)
    return rc, e.lib.umgen_last_error(e._h).decode(), keep


def test_refused_calls_leave_the_engine_usable():
    e = engine("tiny", "fp32", max_batch=3)
    window, cand = case(2, 2)
    ref = e.score_candidates(window, cand)
    w4, c4 = case(4, 2)
    w5, c5 = case(1, 5)
    bad = dict(cand, image=cand["image"].copy())
    bad["image"][1, 2, 9] = 8192
    for what, args, needle in (("C = 0", (window, cand, 2, 2, 0), "C=0"), ("NULL out", (window, cand, 2, 2, 3, None), "null output"),
                               ("token >= vocab", (window, bad, 2, 2, 3), "8192"), ("B > max_batch", (w4, c4, 4, 2, 3), "B=4"),
                               ("T > max_cond_frames", (w5, c5, 1, 5, 3), "T=5")):
        rc, msg, _ = raw_call(e, *args)
        assert rc == -1 and needle in msg, (what, rc, msg)
    with pytest.raises(UMGenError):
        e.score_candidates(w4, c4)
    rc, _, keep = raw_call(e, window, cand, 2, 2, 3)      # NULL arg-max pointers and a NULL shared_slots are fine
    assert rc == 0
    again = e.score_candidates(window, cand)
    for m, k in zip(MOD_ORDER, keep):
        assert k.tobytes() == ref["logp"][m].tobytes() == again["logp"][m].tobytes(), m
