"""umgen_score_clip without a GPU: the ABI surface, the window rule and the Python argument handling."""
import ctypes
import os

import numpy as np
import pytest

from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.model import UMGen

HOOKS = ("umgen_dbg_cond_rows_slots", "umgen_dbg_ego_queries_slots", "umgen_dbg_embed_warp_slots")


def test_library_exports_the_clip_entry_points_with_their_argtypes():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    for name in ("umgen_score_clip",) + HOOKS:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).restype is ctypes.c_int
    i32, i64p, i32p, fp = ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    assert lib.umgen_score_clip.argtypes == [ctypes.c_void_p, i32, i32, i32, i32] + [i64p] * 4 + [ctypes.POINTER(_lib.ScoreOut), i32p]
    assert lib.umgen_dbg_cond_rows_slots.argtypes == [i32, i32, i32, i32, fp, fp, fp, i32p, i32, fp]
    assert lib.umgen_dbg_ego_queries_slots.argtypes == [ctypes.POINTER(_lib.DbgTables), i32, i32p, fp]
    assert lib.umgen_dbg_embed_warp_slots.argtypes == lib.umgen_dbg_embed_warp.argtypes + [fp]
    # the hooks they extend keep their signatures
    assert lib.umgen_dbg_cond_rows.argtypes == [i32, i32, i32, i32, fp, fp, fp, fp] and len(lib.umgen_dbg_embed_warp.argtypes) == 15
    assert lib.umgen_dbg_ego_queries.argtypes == [ctypes.POINTER(_lib.DbgTables), i32, i32, fp]


def test_header_carries_the_prototype_and_the_abi_version_stays():
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "umgen.h")).read()
    assert "int umgen_score_clip(umgen_engine *e, int32_t B, int32_t L, int32_t T_in, int32_t cond_frames," in header
    assert "int32_t *shared_frames);" in header
    assert "#define UMGEN_ABI_VERSION 4" in header      # no struct changed: the version stays


@pytest.mark.parametrize("args,want", [
    ((5, 1, 4), [(1, 0, 1), (2, 0, 2), (3, 0, 3), (4, 0, 4)]),                       # growing only
    ((7, 2, 3), [(2, 0, 2), (3, 0, 3), (4, 1, 3), (5, 2, 3), (6, 3, 3)]),            # growing, then sliding
    ((6, 4, 2), [(4, 2, 2), (5, 3, 2)]),                                             # input_frames > cond_frames: sliding only
    ((2, 1, 4), [(1, 0, 1)]),                                                        # one frame
])
def test_clip_windows_states_the_window_rule(args, want):
    assert Engine.clip_windows(*args) == want


# ---- Python argument handling: everything below raises before a device call (no engine exists on this machine) -------------------

def _engine_without_device(result=None, max_batch=2, max_cond_frames=4):
    e = Engine.__new__(Engine)
    e.cfg = tiny_config()
    e._h = None
    e.max_batch, e.max_cond_frames = max_batch, max_cond_frames

    class NoDevice:
        def __getattr__(self, name):
            if result is not None and name == "umgen_score_clip":
                return result
            raise AssertionError(f"device call {name} reached")
    e.lib = NoDevice()
    return e


def _clip(B=None, L=5, rng=None):
    rng = rng or np.random.default_rng(0)
    lead = () if B is None else (B,)
    hi = {"pose": 1024, "map": 8192, "bbox3d": 1028, "image": 8192}
    return {m: rng.integers(0, hi[m], lead + (L, CONTENT_LEN[m])) for m in MOD_ORDER}


def test_score_clip_accepts_batched_and_unbatched_inputs_and_refuses_bad_ones():
    e = _engine_without_device()
    c, cond, batched = e._clip_args(_clip(), 1, None)
    assert not batched and cond == 4 and c["map"].shape == (1, 5, 1024) and c["image"].dtype == np.int64
    c, cond, batched = e._clip_args(_clip(B=2, L=3), 2, None)
    assert batched and cond == 2 and c["bbox3d"].shape == (2, 3, 660)      # the default: min(max_cond_frames, L - 1)
    assert e._clip_args(_clip(B=2, L=9), 1, 3)[1] == 3
    clip = _clip(B=2)
    with pytest.raises(UMGenError, match="shape"):      # wrong S
        e.score_clip(dict(clip, map=clip["map"][:, :, :1000]), 1)
    with pytest.raises(UMGenError, match="shape"):      # L differs between the modalities
        e.score_clip(dict(clip, image=clip["image"][:, :4]), 1)
    with pytest.raises(UMGenError, match="shape"):      # 3-D pose with 2-D map
        e.score_clip(dict(clip, map=clip["map"][0]), 1)
    with pytest.raises(UMGenError, match=r"clip\[map\] has dtype float32"):
        e.score_clip(dict(clip, map=clip["map"].astype(np.float32)), 1)
    bad = dict(clip, bbox3d=clip["bbox3d"].copy())
    bad["bbox3d"][1, 2, 7] = 1028
    with pytest.raises(UMGenError, match=rf"clip\[bbox3d\] token 1028 at flat index {(1 * 5 + 2) * 660 + 7}"):
        e.score_clip(bad, 1)
    badp = dict(clip, pose=clip["pose"].copy())
    badp["pose"][0, 1, 2] = -1
    with pytest.raises(UMGenError, match=r"clip\[pose\] token -1 at flat index 5"):
        e.score_clip(badp, 1)
    for frames in (0, 5, 6, 1.0, True):                 # 1 <= input_frames < L, an integer
        with pytest.raises(UMGenError, match="input_frames"):
            e.score_clip(clip, frames)
    for cond in (0, 5, 2.0):                            # 1 <= cond_frames <= max_cond_frames
        with pytest.raises(UMGenError, match="cond_frames"):
            e.score_clip(clip, 1, cond)
    with pytest.raises(UMGenError, match="max_batch=2"):
        e.score_clip(_clip(B=3), 1)


def test_total_frames_and_the_scatter_order():
    rng = np.random.default_rng(2)
    B, L, T_in = 2, 6, 2
    F = L - T_in
    stub = {m: -rng.random((B, F, CONTENT_LEN[m])).astype(np.float32) * 9 for m in MOD_ORDER}
    stub_arg = {m: rng.integers(0, 1000, (B, F, CONTENT_LEN[m])).astype(np.int32) for m in MOD_ORDER}
    seen = {}

    def fake(h, b, l, t_in, cond, *rest):      # the C entry point: fills the caller's buffers [B][L - T_in][S_mod], reports the shared frames
        out, shared = rest[4]._obj, rest[5]._obj
        seen["args"] = (b, l, t_in, cond)
        for m in MOD_ORDER:
            ctypes.memmove(getattr(out, f"logp_{m}"), stub[m].ctypes.data, stub[m][:b].nbytes)
            ctypes.memmove(getattr(out, f"argmax_{m}"), stub_arg[m].ctypes.data, stub_arg[m][:b].nbytes)
        shared.value = 2
        return 0
    e = _engine_without_device(result=fake)
    res = e.score_clip(_clip(B=B, L=L), T_in, 3)
    assert seen["args"] == (B, L, T_in, 3)
    want = sum(stub[m].astype(np.float64).sum(-1) for m in MOD_ORDER)
    assert res["total"].dtype == np.float64 and res["total"].shape == (B, F) and np.array_equal(res["total"], want)
    assert res["frames"].dtype == np.int64 and res["frames"].tolist() == [2, 3, 4, 5] == [f for f, _, _ in Engine.clip_windows(L, T_in, 3)]
    assert res["shared_frames"] == 2
    for m in MOD_ORDER:
        assert res["logp"][m].dtype == np.float32 and res["logp"][m].tobytes() == stub[m].tobytes()
        assert res["argmax"][m].dtype == np.int64 and np.array_equal(res["argmax"][m], stub_arg[m])
    flat = e.score_clip(_clip(L=L), T_in, 3)      # [L, S]: the same call with B = 1, the B axis dropped again
    assert seen["args"] == (1, L, T_in, 3) and flat["total"].shape == (F,) and flat["logp"]["map"].shape == (F, 1024)
    assert flat["logp"]["pose"].tobytes() == stub["pose"][0].tobytes() and np.array_equal(flat["total"], want[0])


def test_model_score_clip_refuses_without_weights():
    m = UMGen(tiny_config())
    with pytest.raises(UMGenError, match="load_state_dict"):      # no weights: refused before an engine is created
        m.score_clip(_clip(B=2), input_cond_frames=1, cond_frames=4)
    assert m._engine is None
