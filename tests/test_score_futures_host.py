"""umgen_score_futures without a GPU: the ABI surface, the window rule and the Python argument handling."""
import ctypes
import os

import numpy as np
import pytest

from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.model import UMGen

HI = {"pose": 1024, "map": 8192, "bbox3d": 1028, "image": 8192}


def test_library_exports_the_futures_entry_points_with_their_argtypes():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    for name in ("umgen_score_futures", "umgen_dbg_attn_temporal_fan_tail", "umgen_dbg_score_futures_passes"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    i32, i64p = ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)
    assert lib.umgen_score_futures.argtypes == [ctypes.c_void_p, i32, i32, i32, i32, i32] + [i64p] * 8 + [ctypes.POINTER(_lib.ScoreOut), ctypes.POINTER(i32)]
    assert lib.umgen_score_futures.restype is ctypes.c_int
    # prec, qkv, N, Wt, scene_of_item, B, S, H, P, q0, Tcap, cache, y
    assert len(lib.umgen_dbg_attn_temporal_fan_tail.argtypes) == 13 and lib.umgen_dbg_attn_temporal_fan_tail.restype is ctypes.c_int
    assert len(lib.umgen_dbg_attn_temporal_fan_tail.argtypes) == len(lib.umgen_dbg_attn_temporal_fan.argtypes) + 2
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "umgen.h")).read()
    assert "int umgen_score_futures(" in header and "#define UMGEN_ABI_VERSION 4" in header      # no struct changed: the version stays


@pytest.mark.parametrize("T,cond,K", [(2, 4, 4), (4, 4, 5), (1, 1, 2), (6, 4, 3), (3, 20, 1)])
def test_future_windows_is_the_clip_rule_on_the_concatenated_sequence(T, cond, K):
    fw = Engine.future_windows(T, K, cond)
    cw = Engine.clip_windows(T + K, T, cond)
    assert len(fw) == len(cw) == K
    for (k, start, n, shared), (f, cstart, cn) in zip(fw, cw):
        assert f == T + k and (start, n) == (cstart, cn)
        assert n == min(T + k, cond) and start == T + k - n


def test_shared_follows_the_history_slot_formula():
    def formula(T, cond, K):      # P_k = h_k - 1 with h_k = max(0, n_k - k) history frames inside the window; never negative
        return [max(0, max(0, min(T + k, cond) - k) - 1) for k in range(K)]
    # a growing window: the two history frames stay inside until the cap pushes frame 0 out
    assert [s for *_, s in Engine.future_windows(2, 4, 4)] == [1, 1, 1, 0] == formula(2, 4, 4)
    # a full window: one history frame leaves per future frame
    assert [s for *_, s in Engine.future_windows(4, 5, 4)] == [3, 2, 1, 0, 0] == formula(4, 4, 5)
    # a window of one: nothing to share
    assert [s for *_, s in Engine.future_windows(1, 2, 1)] == [0, 0] == formula(1, 1, 2)
    assert [(k, st, n) for k, st, n, _ in Engine.future_windows(2, 4, 4)] == [(0, 0, 2), (1, 0, 3), (2, 0, 4), (3, 1, 4)]
    assert [(k, st, n) for k, st, n, _ in Engine.future_windows(4, 5, 4)] == [(0, 0, 4), (1, 1, 4), (2, 2, 4), (3, 3, 4), (4, 4, 4)]


# ---- Python argument handling: everything below raises before a device call (no engine exists on this machine) -------------------

def _engine_without_device(result=None, max_batch=2, max_cond_frames=4):
    e = Engine.__new__(Engine)
    e.cfg = tiny_config()
    e._h = None
    e.max_batch, e.max_cond_frames = max_batch, max_cond_frames

    class NoDevice:
        def __getattr__(self, name):
            if result is not None and name == "umgen_score_futures":
                return result
            raise AssertionError(f"device call {name} reached")
    e.lib = NoDevice()
    return e


def _tokens(B=None, T=2, Cn=3, Kn=2, rng=None):
    rng = rng or np.random.default_rng(0)
    lead = () if B is None else (B,)
    w = {m: rng.integers(0, HI[m], lead + (T, CONTENT_LEN[m])) for m in MOD_ORDER}
    fu = {m: rng.integers(0, HI[m], lead + (Cn, Kn, CONTENT_LEN[m])) for m in MOD_ORDER}
    return w, fu


def test_score_futures_accepts_batched_and_unbatched_inputs_and_refuses_bad_ones():
    e = _engine_without_device()
    w, fu = _tokens()
    w3, f4, cond, batched = e._future_args(w, fu, None)
    assert not batched and cond == 4 and w3["map"].shape == (1, 2, 1024) and f4["image"].shape == (1, 3, 2, 512) and f4["map"].dtype == np.int64
    w, fu = _tokens(B=2, Cn=5, Kn=3)
    w3, f4, cond, batched = e._future_args(w, fu, 2)
    assert batched and cond == 2 and w3["bbox3d"].shape == (2, 2, 660) and f4["pose"].shape == (2, 5, 3, 3)
    with pytest.raises(UMGenError, match="shape"):      # wrong S
        e.score_futures(w, dict(fu, map=fu["map"][..., :1000]))
    with pytest.raises(UMGenError, match="shape"):      # 3-D window with un-batched futures
        e.score_futures(w, {m: fu[m][0] for m in MOD_ORDER})
    with pytest.raises(UMGenError, match="shape"):      # B differs
        e.score_futures(w, {m: fu[m][:1] for m in MOD_ORDER})
    with pytest.raises(UMGenError, match="shape"):      # C differs between the modalities
        e.score_futures(w, dict(fu, image=fu["image"][:, :4]))
    with pytest.raises(UMGenError, match="shape"):      # K differs between the modalities
        e.score_futures(w, dict(fu, bbox3d=fu["bbox3d"][:, :, :2]))
    with pytest.raises(UMGenError, match="no candidate"):
        e.score_futures(w, {m: fu[m][:, :0] for m in MOD_ORDER})
    with pytest.raises(UMGenError, match="no future frame"):
        e.score_futures(w, {m: fu[m][:, :, :0] for m in MOD_ORDER})
    with pytest.raises(UMGenError, match="no history frame"):
        e.score_futures({m: w[m][:, :0] for m in MOD_ORDER}, fu)
    with pytest.raises(UMGenError, match=r"futures\[map\] has dtype float32"):
        e.score_futures(w, dict(fu, map=fu["map"].astype(np.float32)))
    with pytest.raises(UMGenError, match=r"window\[image\] has dtype float64"):
        e.score_futures(dict(w, image=w["image"].astype(np.float64)), fu)
    bad = dict(fu, bbox3d=fu["bbox3d"].copy())
    bad["bbox3d"][1, 2, 1, 7] = 1028
    with pytest.raises(UMGenError, match=rf"futures\[bbox3d\] token 1028 at flat index {((1 * 5 + 2) * 3 + 1) * 660 + 7}"):
        e.score_futures(w, bad)
    badw = dict(w, pose=w["pose"].copy())
    badw["pose"][0, 1, 2] = -1
    with pytest.raises(UMGenError, match=r"window\[pose\] token -1 at flat index 5"):
        e.score_futures(badw, fu)
    for cond in (0, 5, 2.0, True):                      # 1 <= cond_frames <= max_cond_frames, an integer
        with pytest.raises(UMGenError, match="cond_frames"):
            e.score_futures(w, fu, cond)
    w3, fu3 = _tokens(B=3)
    with pytest.raises(UMGenError, match="max_batch=2"):
        e.score_futures(w3, fu3)


@pytest.mark.parametrize("batched", [True, False])
def test_total_and_cum_total_are_float64_sums(batched):
    rng = np.random.default_rng(2)
    B, Cn, Kn, T = (2 if batched else 1), 3, 4, 2
    stub = {m: -rng.random((B, Cn, Kn, CONTENT_LEN[m])).astype(np.float32) * 9 for m in MOD_ORDER}
    seen = {}

    def fake(h, b, t, c, k, cond, *rest):      # the C entry point: fills the caller's buffers, reports the shared slots per frame
        out, shared = rest[8]._obj, rest[9]
        seen["args"] = (b, t, c, k, cond)
        for m in MOD_ORDER:
            ctypes.memmove(getattr(out, f"logp_{m}"), stub[m].ctypes.data, stub[m].nbytes)
        for i, (*_, s) in enumerate(Engine.future_windows(t, k, cond)):
            shared[i] = s
        return 0
    e = _engine_without_device(result=fake)
    w, fu = _tokens(B=B if batched else None, T=T, Cn=Cn, Kn=Kn)
    res = e.score_futures(w, fu)
    assert seen["args"] == (B, T, Cn, Kn, 4)            # cond_frames defaults to max_cond_frames
    pick = (lambda a: a) if batched else (lambda a: a[0])
    want = pick(sum(stub[m].astype(np.float64).sum(-1) for m in MOD_ORDER))
    lead = (B, Cn, Kn) if batched else (Cn, Kn)
    assert res["total"].dtype == np.float64 and res["total"].shape == lead and np.array_equal(res["total"], want)
    assert res["cum_total"].dtype == np.float64 and res["cum_total"].shape == lead[:-1] and np.array_equal(res["cum_total"], want.sum(-1))
    assert res["shared_slots"].dtype == np.int64 and res["shared_slots"].tolist() == [1, 1, 1, 0]
    assert all(res["logp"][m].tobytes() == stub[m].tobytes() and res["logp"][m].shape == lead + (CONTENT_LEN[m],) for m in MOD_ORDER)
    assert all(res["argmax"][m].dtype == np.int64 and res["argmax"][m].shape == lead + (CONTENT_LEN[m],) for m in MOD_ORDER)


def test_model_score_futures_splits_a_num_samples_output_and_refuses_bad_calls():
    rng = np.random.default_rng(1)
    B, T, N, K = 2, 3, 4, 2
    clip, new = _tokens(B=B, T=T, Cn=N, Kn=K, rng=rng)
    # what inference(num_samples=N) returns: [B, N, T + K, S], every branch's first T frames the conditioning clip
    sampled = {m: np.concatenate([np.broadcast_to(clip[m][:, None], (B, N, T, CONTENT_LEN[m])), new[m]], axis=2) for m in MOD_ORDER}
    for flag in (None, True):
        fut = UMGen._future_split(clip, sampled, flag)
        assert all(fut[m].shape == (B, N, K, CONTENT_LEN[m]) and np.array_equal(fut[m], new[m]) and fut[m].flags.c_contiguous for m in MOD_ORDER)
    fut = UMGen._future_split(clip, sampled, False)     # every frame a future frame
    assert all(fut[m].shape == (B, N, T + K, CONTENT_LEN[m]) for m in MOD_ORDER)
    fut = UMGen._future_split(clip, new, None)          # plain futures pass through
    assert all(fut[m] is new[m] for m in MOD_ORDER)
    other = {m: sampled[m].copy() for m in MOD_ORDER}
    other["image"][1, 2, 0, 5] ^= 1                     # one branch's history differs in one token: not a rollout of this clip
    assert all(np.array_equal(UMGen._future_split(clip, other, None)[m], other[m]) for m in MOD_ORDER)
    with pytest.raises(UMGenError, match="includes_history"):
        UMGen._future_split(clip, other, True)
    with pytest.raises(UMGenError, match="includes_history"):
        UMGen._future_split(clip, new, True)            # K <= T frames: there is no room for the history
    for args in (({m: clip[m][0] for m in MOD_ORDER}, new),                          # 2-D conditioning tokens
                 (clip, {m: new[m][:, 0] for m in MOD_ORDER}),                       # 3-D futures
                 (clip, {m: new[m][:1] for m in MOD_ORDER}),                         # B differs
                 (clip, dict(new, map=new["map"][:, :, :1]))):                       # K differs between the modalities
        with pytest.raises(UMGenError, match="score_futures"):
            UMGen._future_split(*args, None)
    m = UMGen(tiny_config())
    with pytest.raises(UMGenError, match="load_state_dict"):      # no weights: refused before an engine is created
        m.score_futures(clip, sampled)
    assert m._engine is None
