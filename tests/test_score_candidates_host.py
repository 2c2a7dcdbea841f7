"""umgen_score_candidates without a GPU: the ABI surface and the Python argument handling."""
import ctypes
import os

import numpy as np
import pytest

from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.model import UMGen


def test_library_exports_the_candidate_entry_points_with_their_argtypes():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    for name in ("umgen_score_candidates", "umgen_dbg_attn_temporal_fan"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    i32, i64p = ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)
    assert lib.umgen_score_candidates.argtypes == [ctypes.c_void_p, i32, i32, i32] + [i64p] * 8 + [ctypes.POINTER(_lib.ScoreOut), ctypes.POINTER(i32)]
    assert lib.umgen_score_candidates.restype is ctypes.c_int
    assert len(lib.umgen_dbg_attn_temporal_fan.argtypes) == 11 and lib.umgen_dbg_attn_temporal_fan.restype is ctypes.c_int
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "umgen.h")).read()
    assert "int umgen_score_candidates(" in header and "#define UMGEN_ABI_VERSION 4" in header      # no struct changed: the version stays


# ---- Python argument handling: everything below raises before a device call (no engine exists on this machine) -------------------

def _engine_without_device(result=None):
    e = Engine.__new__(Engine)
    e.cfg = tiny_config()
    e._h = None

    class NoDevice:
        def __getattr__(self, name):
            if result is not None and name == "umgen_score_candidates":
                return result
            raise AssertionError(f"device call {name} reached")
    e.lib = NoDevice()
    return e


def _tokens(B=None, T=2, Cn=3, rng=None):
    rng = rng or np.random.default_rng(0)
    lead = () if B is None else (B,)
    hi = {"pose": 1024, "map": 8192, "bbox3d": 1028, "image": 8192}
    w = {m: rng.integers(0, hi[m], lead + (T, CONTENT_LEN[m])) for m in MOD_ORDER}
    cd = {m: rng.integers(0, hi[m], lead + (Cn, CONTENT_LEN[m])) for m in MOD_ORDER}
    return w, cd


def test_score_candidates_accepts_batched_and_unbatched_inputs_and_refuses_bad_ones():
    e = _engine_without_device()
    w, cd = _tokens()
    w3, c3, batched = e._candidate_args(w, cd)
    assert not batched and w3["map"].shape == (1, 2, 1024) and c3["image"].shape == (1, 3, 512) and c3["map"].dtype == np.int64
    w, cd = _tokens(B=2, Cn=5)
    w3, c3, batched = e._candidate_args(w, cd)
    assert batched and w3["bbox3d"].shape == (2, 2, 660) and c3["pose"].shape == (2, 5, 3)
    with pytest.raises(UMGenError, match="shape"):      # wrong S
        e.score_candidates(w, dict(cd, map=cd["map"][:, :, :1000]))
    with pytest.raises(UMGenError, match="shape"):      # 3-D window with 2-D candidates
        e.score_candidates(w, {m: cd[m][0] for m in MOD_ORDER})
    with pytest.raises(UMGenError, match="shape"):      # B differs
        e.score_candidates(w, {m: cd[m][:1] for m in MOD_ORDER})
    with pytest.raises(UMGenError, match="shape"):      # C differs between the modalities
        e.score_candidates(w, dict(cd, image=cd["image"][:, :4]))
    with pytest.raises(UMGenError, match="no candidate"):
        e.score_candidates(w, {m: cd[m][:, :0] for m in MOD_ORDER})
    with pytest.raises(UMGenError, match=r"candidates\[map\] has dtype float32"):
        e.score_candidates(w, dict(cd, map=cd["map"].astype(np.float32)))
    with pytest.raises(UMGenError, match=r"window\[image\] has dtype float64"):
        e.score_candidates(dict(w, image=w["image"].astype(np.float64)), cd)
    bad = dict(cd, bbox3d=cd["bbox3d"].copy())
    bad["bbox3d"][1, 2, 7] = 1028
    with pytest.raises(UMGenError, match=rf"candidates\[bbox3d\] token 1028 at flat index {(1 * 5 + 2) * 660 + 7}"):
        e.score_candidates(w, bad)
    badw = dict(w, pose=w["pose"].copy())
    badw["pose"][0, 1, 2] = -1
    with pytest.raises(UMGenError, match=r"window\[pose\] token -1 at flat index 5"):
        e.score_candidates(badw, cd)


def test_total_is_the_float64_sum_over_all_content_positions():
    rng = np.random.default_rng(2)
    B, Cn = 2, 3
    stub = {m: -rng.random((B, Cn, CONTENT_LEN[m])).astype(np.float32) * 9 for m in MOD_ORDER}

    def fake(h, b, t, c, *rest):      # the C entry point: fills the caller's buffers, reports the shared path
        out, shared = rest[8]._obj, rest[9]._obj
        assert (b, t, c) == (B, 2, Cn)
        for m in MOD_ORDER:
            ctypes.memmove(getattr(out, f"logp_{m}"), stub[m].ctypes.data, stub[m].nbytes)
        shared.value = t - 1
        return 0
    e = _engine_without_device(result=fake)
    w, cd = _tokens(B=B, Cn=Cn)
    res = e.score_candidates(w, cd)
    want = sum(stub[m].astype(np.float64).sum(-1) for m in MOD_ORDER)
    assert res["total"].dtype == np.float64 and res["total"].shape == (B, Cn) and np.array_equal(res["total"], want)
    assert sum(CONTENT_LEN[m] for m in MOD_ORDER) == 2199
    assert res["shared_slots"] == 1 and all(res["logp"][m].tobytes() == stub[m].tobytes() for m in MOD_ORDER)
    assert all(res["argmax"][m].dtype == np.int64 and res["argmax"][m].shape == (B, Cn, CONTENT_LEN[m]) for m in MOD_ORDER)


def test_model_score_candidates_selects_the_window_and_refuses_bad_calls():
    rng = np.random.default_rng(1)
    clip, cd = _tokens(B=2, T=6, rng=rng)
    w = UMGen._candidate_window(clip, cd, -1, 4)
    assert all(np.array_equal(w[m], clip[m][:, 2:6]) for m in MOD_ORDER)
    w = UMGen._candidate_window(clip, cd, 2, 4)
    assert all(np.array_equal(w[m], clip[m][:, 4:6]) for m in MOD_ORDER)
    for args in ((clip, cd, 5, 4),                                                  # more frames than the engine's window
                 (clip, cd, 0, 4),
                 ({m: clip[m][0] for m in MOD_ORDER}, cd, -1, 4),                   # 2-D conditioning tokens
                 (clip, {m: cd[m][:1] for m in MOD_ORDER}, -1, 4)):                 # B differs
        with pytest.raises(UMGenError):
            UMGen._candidate_window(*args)
    m = UMGen(tiny_config())
    with pytest.raises(UMGenError, match="load_state_dict"):      # no weights: refused before an engine is created
        m.score_candidates(clip, cd)
    assert m._engine is None
