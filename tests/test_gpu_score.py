"""umgen_score on the engine: per-token log-likelihoods of a given next frame as ONE forward pass, against the CPU oracle's fixtures
(tests/golden/make_score_golden.py), against the same engine's teacher-forced trace, across batch sizes and around rollouts.

Bars.  fp32: max |logp - anchor| <= 2e-3 per modality -- twice the 1e-3 the project holds fp32 logits to
(test_fp32_teacher_forced_logits_vs_oracle_golden), a log-probability being a target logit minus a log-sum-exp of logits.  16-bit modes:
<= 2 x dist_{bf16,fp16} of the fixture, the CPU restatement's own distance to the fp32 anchor (never measured on the engine), the
project's "inside 2 x the spread" margin."""
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


def golden_case(width):
    """(fixture, window mod -> [T, S], scored frame mod -> [S], arg-max / gap source)"""
    g = np.load(os.path.join(GOLD, f"score_{width}.npz"))
    if width == "tiny":
        full = synthetic_scene(TINY_SCENE, n_frames=TINY_HISTORY + 1)
        return g, {m: full[m][0, :TINY_HISTORY] for m in MOD_ORDER}, {m: full[m][0, TINY_HISTORY] for m in MOD_ORDER}, g
    f32 = np.load(os.path.join(GOLD, f"{width}_fp32.npz"))
    assert [int(x) for x in f32["meta"]] == [WEIGHT_SEED, SCENE_ID]
    scene = synthetic_scene(SCENE_ID, n_frames=2)
    return g, {m: scene[m][0] for m in MOD_ORDER}, {m: f32[f"tok_{m}"].astype(np.int64) for m in MOD_ORDER}, f32


def scenes(n, T=2):
    """n distinct scenes: windows [n, T, S] and the frame behind each [n, S]"""
    sc = [synthetic_scene(SCENE_ID + 1 + i, n_frames=T + 1) for i in range(n)]
    return ({m: np.concatenate([s[m][:, :T] for s in sc]) for m in MOD_ORDER}, {m: np.concatenate([s[m][:, T] for s in sc]) for m in MOD_ORDER})


def log_softmax_at(logits, tokens):
    lg = logits.astype(np.float64)
    mx = lg.max(-1, keepdims=True)
    return lg[np.arange(lg.shape[0]), tokens] - (mx[:, 0] + np.log(np.exp(lg - mx).sum(-1)))


@pytest.mark.parametrize("width", ["tiny", "full_width"])
def test_fp32_scores_match_the_oracle_anchor_and_the_engines_own_trace(width):
    g, window, frame, gaps = golden_case(width)
    e = engine(width, "fp32")
    res = e.score(window, frame)
    _, tr = e.frame(window, frame_idx=0, trace=True, forced=frame)
    traced = dict(pose=tr["ego_logits"], map=tr["logits_map"], bbox3d=tr["logits_bbox3d"], image=tr["logits_image"])
    flips = 0
    for m in MOD_ORDER:
        assert res["logp"][m].shape == (CONTENT_LEN[m],) and res["logp"][m].dtype == np.float32 and res["argmax"][m].dtype == np.int64
        d_anchor = np.abs(res["logp"][m] - g[f"logp_{m}"]).max()
        d_trace = np.abs(res["logp"][m] - log_softmax_at(traced[m], frame[m])).max()
        print(f"{width} fp32 {m}: max |logp - anchor| {d_anchor:.3g}, max |logp - own trace| {d_trace:.3g}")
        assert d_anchor <= 2e-3, (m, d_anchor)
        assert d_trace <= 2e-3, (m, d_trace)
        if f"argmax_{m}" in gaps.files:
            f = np.nonzero(res["argmax"][m] != gaps[f"argmax_{m}"].astype(np.int64))[0]
            assert (gaps[f"gap_{m}"][f] < 2e-3).all(), (m, f, gaps[f"gap_{m}"][f])      # flips at oracle near-ties only
            flips += len(f)
    assert flips <= 3, flips


@pytest.mark.parametrize("width", ["full_width", "deep"])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_16bit_scores_lie_within_twice_the_cpu_restatements_distance(width, precision):
    g, window, frame, _ = golden_case(width)
    res = engine(width, precision).score(window, frame)
    bar = 2.0 * float(g[f"dist_{precision}"])
    worst = 0.0
    for m in MOD_ORDER:
        d = float(np.abs(res["logp"][m] - g[f"logp_{m}"]).max())
        print(f"{width} {precision} {m}: max |logp - anchor| {d:.3g} (bar {bar:.3g})")
        worst = max(worst, d)
    assert worst <= bar, (worst, bar)


@pytest.mark.parametrize("width,precision", [("full_width", "bf16"), ("tiny", "fp32")])
def test_a_batch_equals_its_one_scene_calls_bit_for_bit(width, precision):
    e = engine(width, precision, max_batch=3)
    window, frame = scenes(3)
    both = e.score(window, frame)
    for i in range(3):
        one = e.score({m: window[m][i] for m in MOD_ORDER}, {m: frame[m][i] for m in MOD_ORDER})
        for kind in ("logp", "argmax"):
            for m in MOD_ORDER:
                assert both[kind][m].shape == (3, CONTENT_LEN[m])
                assert both[kind][m][i].tobytes() == one[kind][m].tobytes(), (kind, m, i)
    assert not np.array_equal(both["logp"]["map"][0], both["logp"]["map"][1])


def test_score_leaves_a_rollout_unchanged_and_repeats_itself():
    e = engine("full_width", "bf16")      # one scene per call: the background workers of the decode engine are on
    scene = synthetic_scene(SCENE_ID, n_frames=2)
    window, frame = scenes(1)
    before = e.rollout(scene, 2, cond_frames=3, input_cond_frames=2, seeds=[5])
    a = e.score(window, frame)
    after = e.rollout(scene, 2, cond_frames=3, input_cond_frames=2, seeds=[5])
    b = e.score(window, frame)
    for m in MOD_ORDER:
        np.testing.assert_array_equal(before[m], after[m], err_msg=m)
        assert a["logp"][m].tobytes() == b["logp"][m].tobytes() and np.array_equal(a["argmax"][m], b["argmax"][m]), m
        assert np.isfinite(a["logp"][m]).all() and (a["logp"][m] <= 0).all()


def raw_score(e, window, frame, B, T, out="make"):
    """umgen_score itself, past the Python checks"""
    p = lambda a: np.ascontiguousarray(a, dtype=np.int64)  # noqa: E731
    w, f = [p(window[m]) for m in MOD_ORDER], [p(frame[m]) for m in MOD_ORDER]
    keep = [np.zeros(B * CONTENT_LEN[m], np.float32) for m in MOD_ORDER]
    if out == "make":
        out = C.byref(_lib.ScoreOut(**{f"logp_{m}": k.ctypes.data_as(C.POINTER(C.c_float)) for m, k in zip(MOD_ORDER, keep)}))      # arg-max pointers NULL
    i64p = C.POINTER(C.c_int64)
    rc = e.lib.umgen_score(e._h, B, T, *[a.ctypes.data_as(i64p) for a in w], *[a.ctypes.data_as(i64p) for a in f], out)
    return rc, e.lib.umgen_last_error(e._h).decode(), keep


def test_edges_one_history_frame_and_refused_calls_leave_the_engine_usable():
    e = engine("tiny", "fp32", max_batch=3)
    window, frame = scenes(1, T=1)
    ref = e.score(window, frame)
    assert all(np.isfinite(ref["logp"][m]).all() for m in MOD_ORDER)
    w5, f5 = scenes(1, T=5)
    w4, f4 = scenes(4, T=1)
    bad = dict(frame, image=frame["image"].copy())
    bad["image"][0, 9] = 8192
    for what, args, needle in (("B > max_batch", (w4, f4, 4, 1), "B=4"), ("T > max_cond_frames", (w5, f5, 1, 5), "T=5"),
                               ("token >= vocab", (window, bad, 1, 1), "8192"), ("NULL out", (window, frame, 1, 1, None), "null output")):
        rc, msg, _ = raw_score(e, *args)
        assert rc == -1 and needle in msg, (what, rc, msg)
    with pytest.raises(UMGenError):
        e.score(w4, f4)
    rc, _, keep = raw_score(e, window, frame, 1, 1)      # NULL arg-max pointers are fine, and the engine still answers the same
    assert rc == 0
    again = e.score(window, frame)
    for m, k in zip(MOD_ORDER, keep):
        assert k.tobytes() == ref["logp"][m].tobytes() == again["logp"][m].tobytes(), m
