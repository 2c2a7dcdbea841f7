"""-m gpu: umgen_score_futures on the engine -- C candidate futures of K frames per scene against one history, every entry (b, c, k) bit for bit
what umgen_score returns on the window Engine.future_windows names, on the shared path (history slots once per scene, the candidates' tails through
attn_temporal_fan_tail_kernel), on the replicated path (UMGEN_SCORE_FUTURES_SHARE=0, frames without a shared slot), in one chunk and in two; a full
window that slides and one that grows; against the oracle's anchor; around rollouts; refused calls.

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
    _refs.clear()


def case(B, T, K, scene0=SCENE_ID + 1):
    """B histories [B, T, S] and 3 futures per scene [B, 3, K, S]: the scene's own continuation, that continuation with another scene's pose tokens,
    and the frames of another scene"""
    sc = [synthetic_scene(scene0 + i, n_frames=T + K) for i in range(B + 1)]
    window = {m: np.concatenate([s[m][:, :T] for s in sc[:B]]) for m in MOD_ORDER}
    fut = {}
    for m in MOD_ORDER:
        rows = []
        for b in range(B):
            own, other = sc[b][m][0, T:], sc[b + 1][m][0, T:]
            rows.append(np.stack([own, other if m == "pose" else own, other]))
        fut[m] = np.stack(rows)
    assert all(not np.array_equal(fut["pose"][b, 0, k], fut["pose"][b, 1, k]) for b in range(B) for k in range(K))
    return window, fut


def singles(e, window, fut, cond):
    """Engine.score per (b, c, k) on the window future_windows names inside window[b] ++ fut[b, c], stacked to [B, C, K, S]"""
    B, Cn, K = fut["pose"].shape[:3]
    T = window["pose"].shape[1]
    res = {}
    for b in range(B):
        for c in range(Cn):
            seq = {m: np.concatenate([window[m][b], fut[m][b, c]]) for m in MOD_ORDER}
            for k, start, n, _ in Engine.future_windows(T, K, cond):
                res[b, c, k] = e.score({m: seq[m][start:start + n] for m in MOD_ORDER}, {m: seq[m][T + k] for m in MOD_ORDER})
    return {kind: {m: np.stack([np.stack([np.stack([res[b, c, k][kind][m] for k in range(K)]) for c in range(Cn)]) for b in range(B)]) for m in MOD_ORDER}
            for kind in ("logp", "argmax")}


def reference(width, precision, T, K, cond):
    """The per-item scores of case(2, T, K), computed once per engine and shape"""
    key = (width, precision, T, K, cond)
    if key not in _refs:
        _refs[key] = singles(engine(width, precision, max_batch=3), *case(2, T, K), cond)
    return _refs[key]


def same_bytes(a, b, what):
    for kind in ("logp", "argmax"):
        for m in MOD_ORDER:
            assert a[kind][m].shape == b[kind][m].shape and a[kind][m].dtype == b[kind][m].dtype, (what, kind, m)
            assert a[kind][m].tobytes() == b[kind][m].tobytes(), (what, kind, m, np.argwhere(a[kind][m] != b[kind][m])[:4].tolist())


def history_passes(e):
    return e.lib.umgen_dbg_score_futures_passes(e._h)


class share_off:
    def __enter__(self):
        self.old = os.environ.get("UMGEN_SCORE_FUTURES_SHARE")
        os.environ["UMGEN_SCORE_FUTURES_SHARE"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["UMGEN_SCORE_FUTURES_SHARE"]
        else:
            os.environ["UMGEN_SCORE_FUTURES_SHARE"] = self.old


# a full window that slides: tails of 1, 2, 3 behind 3, 2, 1 shared slots, then a frame without a shared slot; a window that grows to the cap: one
# shared slot and ONE history pass for the frames 0 .. 2
@pytest.mark.parametrize("T,shared,passes", [(4, [3, 2, 1, 0], 3), (2, [1, 1, 1, 0], 1)])
@pytest.mark.parametrize("width,precision", [("tiny", "fp32"), ("full_width", "bf16"), ("full_width", "fp16")])
def test_every_future_frame_has_the_bits_of_its_own_score_call(width, precision, T, shared, passes):
    K, cond = 4, 4
    window, fut = case(2, T, K)
    assert [s for *_, s in Engine.future_windows(T, K, cond)] == shared
    chunked, whole = engine(width, precision, max_batch=3), engine(width, precision, max_batch=8)      # 6 items: two chunks | one
    ref = reference(width, precision, T, K, cond)
    got = chunked.score_futures(window, fut, cond)
    assert got["shared_slots"].tolist() == shared and history_passes(chunked) == passes
    same_bytes(got, ref, "two chunks")
    one = whole.score_futures(window, fut)      # cond_frames defaults to max_cond_frames = 4
    assert one["shared_slots"].tolist() == shared and history_passes(whole) == passes
    same_bytes(one, got, "one chunk against two")
    for m in MOD_ORDER:
        assert got["logp"][m].shape == (2, 3, K, CONTENT_LEN[m]) and np.isfinite(got["logp"][m]).all() and (got["logp"][m] <= 0).all()
    total = sum(got["logp"][m].astype(np.float64).sum(-1) for m in MOD_ORDER)
    assert got["total"].dtype == np.float64 and np.array_equal(got["total"], total) and np.array_equal(got["cum_total"], total.sum(-1))
    with share_off():
        rep = chunked.score_futures(window, fut, cond)
    assert rep["shared_slots"].tolist() == [0] * K and history_passes(chunked) == 0
    same_bytes(rep, got, "replicated path against the shared path")
    # un-batched inputs: [T, S] with [C, K, S]
    flat = chunked.score_futures({m: window[m][1] for m in MOD_ORDER}, {m: fut[m][1] for m in MOD_ORDER}, cond)
    for m in MOD_ORDER:
        assert flat["logp"][m].tobytes() == got["logp"][m][1].tobytes() and flat["total"].shape == (3, K) and flat["cum_total"].shape == (3,)


def test_a_later_frames_pose_moves_only_that_candidate_from_that_frame_on():
    e = engine("tiny", "fp32", max_batch=3)
    window, fut = case(2, 4, 4)
    base = e.score_futures(window, fut)
    moved = {m: fut[m].copy() for m in MOD_ORDER}
    moved["pose"][0, 1, 1] = fut["pose"][1, 2, 1]       # only the pose tokens of future frame 1 of candidate (0, 1)
    assert not np.array_equal(moved["pose"][0, 1, 1], fut["pose"][0, 1, 1])
    got = e.score_futures(window, moved)
    assert got["shared_slots"].tolist() == [3, 2, 1, 0]
    keep = np.ones((2, 3, 4), bool)
    keep[0, 1, 1:] = False
    for m in MOD_ORDER:
        assert got["logp"][m][keep].tobytes() == base["logp"][m][keep].tobytes(), m      # its frame 0 and every other candidate: the same bytes
    assert not np.array_equal(got["logp"]["pose"][0, 1, 1], base["logp"]["pose"][0, 1, 1])      # frame 1: another target
    for k in (1, 2, 3):      # frame 1's map sees the pose through the warp of its last slot; frames 2 and 3 see it one and two slots back, and in the ego window
        assert not np.array_equal(got["logp"]["map"][0, 1, k], base["logp"]["map"][0, 1, k]), k
    ref = singles(e, {m: window[m][:1] for m in MOD_ORDER}, {m: moved[m][:1, 1:2] for m in MOD_ORDER}, 4)
    for m in MOD_ORDER:
        assert got["logp"][m][0, 1].tobytes() == ref["logp"][m][0, 0].tobytes(), m


def test_one_future_frame_has_the_bytes_of_score_candidates():
    e = engine("tiny", "fp32", max_batch=3)
    for T, shared in ((1, 0), (3, 2)):
        window, fut = case(2, T, 1)
        got = e.score_futures(window, fut)
        cand = e.score_candidates(window, {m: fut[m][:, :, 0] for m in MOD_ORDER})
        assert got["shared_slots"].tolist() == [shared] and cand["shared_slots"] == shared
        for m in MOD_ORDER:
            assert got["logp"][m][:, :, 0].tobytes() == cand["logp"][m].tobytes() and got["argmax"][m][:, :, 0].tobytes() == cand["argmax"][m].tobytes(), (T, m)
    # one history frame and two future frames: nothing is ever shared
    window, fut = case(2, 1, 2)
    got = e.score_futures(window, fut, 1)
    assert got["shared_slots"].tolist() == [0, 0] and history_passes(e) == 0
    same_bytes(got, singles(e, window, fut, 1), "T = 1, cond_frames = 1")


def test_fp32_tiny_future_frame_lies_within_the_bar_of_the_oracle_anchor():
    g = np.load(os.path.join(GOLD, "score_tiny.npz"))
    full = synthetic_scene(TINY_SCENE, n_frames=TINY_HISTORY + 1)
    other = synthetic_scene(TINY_SCENE + 1, n_frames=TINY_HISTORY + 1)
    T = TINY_HISTORY - 1      # the anchor's frame as future frame 1: its window [0, TINY_HISTORY) is T history frames and future frame 0
    window = {m: full[m][0, :T] for m in MOD_ORDER}
    fut = {m: np.stack([full[m][0, T:], other[m][0, T:]]) for m in MOD_ORDER}
    res = engine("tiny", "fp32", max_batch=3).score_futures(window, fut)
    assert res["shared_slots"].tolist() == [T - 1, T - 1] == [1, 1]      # frame 1: a tail of two slots behind one shared slot
    for m in MOD_ORDER:
        d = float(np.abs(res["logp"][m][0, 1] - g[f"logp_{m}"]).max())
        print(f"tiny fp32 {m}: max |logp - anchor| {d:.3g}")
        assert d <= 2e-3, (m, d)


def test_futures_leave_a_rollout_unchanged_and_repeat_themselves():
    e = engine("full_width", "bf16")      # one scene per call: the background workers of the decode engine are on
    scene = synthetic_scene(SCENE_ID, n_frames=2)
    window, fut = case(1, 2, 2)
    before = e.rollout(scene, 2, cond_frames=3, input_cond_frames=2, seeds=[5])
    a = e.score_futures(window, fut, 3)
    after = e.rollout(scene, 2, cond_frames=3, input_cond_frames=2, seeds=[5])
    b = e.score_futures(window, fut, 3)
    assert a["shared_slots"].tolist() == b["shared_slots"].tolist() == [1, 1]
    for m in MOD_ORDER:
        np.testing.assert_array_equal(before[m], after[m], err_msg=m)
    same_bytes(a, b, "the call repeated")


def raw_call(e, window, fut, B, T, Cn, K, cond, out="make"):
    """umgen_score_futures itself, past the Python checks"""
    p = lambda a: np.ascontiguousarray(a, dtype=np.int64)  # noqa: E731
    w, f = [p(window[m]) for m in MOD_ORDER], [p(fut[m]) for m in MOD_ORDER]
    keep = [np.zeros(max(B * Cn * K, 1) * CONTENT_LEN[m], np.float32) for m in MOD_ORDER]
    if out == "make":
        out = C.byref(_lib.ScoreOut(**{f"logp_{m}": k.ctypes.data_as(C.POINTER(C.c_float)) for m, k in zip(MOD_ORDER, keep)}))      # arg-max pointers NULL
    i64p = C.POINTER(C.c_int64)
    rc = e.lib.umgen_score_futures(e._h, B, T, Cn, K, cond, *[a.ctypes.data_as(i64p) for a in w], *[a.ctypes.data_as(i64p) for a in f], out, None)
    return rc, e.lib.umgen_last_error(e._h).decode(), keep


def test_refused_calls_leave_the_engine_usable():
    e = engine("tiny", "fp32", max_batch=3)
    window, fut = case(2, 2, 2)
    ref = e.score_futures(window, fut)
    w4, f4 = case(4, 2, 2)
    bad = dict(fut, image=fut["image"].copy())
    bad["image"][1, 2, 1, 9] = 8192
    flat = ((1 * 3 + 2) * 2 + 1) * 512 + 9
    for what, args, needle in (("C = 0", (window, fut, 2, 2, 0, 2, 4), "C=0"), ("K = 0", (window, fut, 2, 2, 3, 0, 4), "K=0"),
                               ("T = 0", (window, fut, 2, 0, 3, 2, 4), "T=0"), ("NULL out", (window, fut, 2, 2, 3, 2, 4, None), "null output"),
                               ("token >= vocab", (window, bad, 2, 2, 3, 2, 4), "8192"), ("its flat index", (window, bad, 2, 2, 3, 2, 4), str(flat)),
                               ("B > max_batch", (w4, f4, 4, 2, 3, 2, 4), "B=4"), ("cond_frames > max_cond_frames", (window, fut, 2, 2, 3, 2, 5), "cond_frames=5"),
                               ("cond_frames = 0", (window, fut, 2, 2, 3, 2, 0), "cond_frames=0")):
        rc, msg, _ = raw_call(e, *args)
        assert rc == -1 and needle in msg, (what, rc, msg)
    with pytest.raises(UMGenError):
        e.score_futures(w4, f4)
    rc, _, keep = raw_call(e, window, fut, 2, 2, 3, 2, 4)      # NULL arg-max pointers and a NULL shared_slots are fine
    assert rc == 0
    again = e.score_futures(window, fut)
    for m, k in zip(MOD_ORDER, keep):
        assert k.tobytes() == ref["logp"][m].tobytes() == again["logp"][m].tobytes(), m
