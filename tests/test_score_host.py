"""umgen_score without a GPU: the ABI surface, the recorded fixtures and the Python argument handling."""
import ctypes
import os

import numpy as np
import pytest

from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.model import UMGen

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def tiny():
    return np.load(os.path.join(GOLD, "score_tiny.npz"))


def test_library_exports_the_score_entry_points_and_the_struct_layout():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    for name in ("umgen_score", "umgen_dbg_head_nll"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.ScoreOut) == 64
    assert [n for n, _ in _lib.ScoreOut._fields_] == [f"{k}_{m}" for k in ("logp", "argmax") for m in MOD_ORDER]


def test_recorded_tiny_fixture_is_what_the_generator_produces(tiny):
    from tests.golden.make_score_golden import compute
    live = compute("tiny")
    assert set(live) == set(tiny.files)
    # the oracle computes in fp32 on however many threads the machine has: its logits repeat to 1e-5 (tests/test_oracle.py), an arg-max
    # only where the top-2 gap is above that
    for k in tiny.files:
        if k.startswith("tok_"):
            assert np.array_equal(live[k], tiny[k]), k
        elif k.startswith("argmax_"):
            sure = tiny["gap_" + k[7:]] > 1e-5
            assert np.array_equal(live[k][sure], tiny[k][sure]), k
        elif k.startswith("dist_"):
            np.testing.assert_allclose(live[k], tiny[k], rtol=5e-3, err_msg=k)
        else:
            np.testing.assert_allclose(live[k], tiny[k], atol=1e-5, rtol=0, err_msg=k)


@pytest.mark.parametrize("name", ["tiny", "full_width", "deep"])
def test_one_pass_restatement_equals_the_decode_oracle_in_fp32(name):
    g = np.load(os.path.join(GOLD, f"score_{name}.npz"))
    for m in MOD_ORDER:
        assert g[f"logp_{m}"].shape == (CONTENT_LEN[m],) and g[f"logp_{m}"].dtype == np.float64
        assert np.isfinite(g[f"logp_{m}"]).all() and (g[f"logp_{m}"] <= 0).all()
        assert np.abs(g[f"logp_onepass_fp32_{m}"] - g[f"logp_{m}"]).max() <= 1e-5, m
    assert 0 < g["dist_fp16"] < g["dist_bf16"] < 0.05


def test_tiny_argmax_margins_are_wide_enough_for_the_flip_checks(tiny):
    gaps = np.concatenate([tiny[f"gap_{m}"] for m in ("map", "bbox3d", "image")])
    assert gaps.size == 2196
    assert (gaps < 1e-3).sum() <= 0.01 * gaps.size, int((gaps < 1e-3).sum())


# ---- Python argument handling: everything below raises before a device call (no engine exists on this machine) -------------------

def _engine_without_device():
    e = Engine.__new__(Engine)
    e.cfg = tiny_config()
    e._h = None

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"device call {name} reached")
    e.lib = NoDevice()
    return e


def _tokens(B=None, T=2, rng=None):
    rng = rng or np.random.default_rng(0)
    lead = () if B is None else (B,)
    hi = {"pose": 1024, "map": 8192, "bbox3d": 1028, "image": 8192}
    w = {m: rng.integers(0, hi[m], lead + (T, CONTENT_LEN[m])) for m in MOD_ORDER}
    nx = {m: rng.integers(0, hi[m], lead + (CONTENT_LEN[m],)) for m in MOD_ORDER}
    return w, nx


def test_engine_score_accepts_batched_and_unbatched_inputs_and_refuses_bad_ones():
    e = _engine_without_device()
    w, nx = _tokens()
    w3, nx3, batched = e._score_args(w, nx)
    assert not batched and w3["map"].shape == (1, 2, 1024) and nx3["image"].shape == (1, 512) and w3["map"].dtype == np.int64
    w, nx = _tokens(B=3)
    w3, nx3, batched = e._score_args(w, nx)
    assert batched and w3["bbox3d"].shape == (3, 2, 660) and nx3["pose"].shape == (3, 3)
    with pytest.raises(UMGenError, match="shape"):      # wrong S
        e.score(w, dict(nx, map=nx["map"][:, :1000]))
    with pytest.raises(UMGenError, match="shape"):      # 3-D window with a 1-D frame
        e.score(w, {m: nx[m][0] for m in MOD_ORDER})
    with pytest.raises(UMGenError, match="shape"):      # B differs
        e.score(w, {m: nx[m][:2] for m in MOD_ORDER})
    bad = dict(nx, bbox3d=nx["bbox3d"].copy())
    bad["bbox3d"][1, 7] = 1028
    with pytest.raises(UMGenError, match=r"next_frame\[bbox3d\] token 1028 at flat index 667"):
        e.score(w, bad)
    badw = dict(w, pose=w["pose"].copy())
    badw["pose"][0, 1, 2] = -1
    with pytest.raises(UMGenError, match=r"window\[pose\] token -1 at flat index 5"):
        e.score(badw, nx)


def test_model_score_selects_the_window_and_the_scored_frame():
    rng = np.random.default_rng(1)
    clip, _ = _tokens(B=2, T=6, rng=rng)
    cap = 4
    # a clip and t: frame t against the frames before it
    w, f = UMGen._score_window(clip, clip, -1, 5, cap)
    assert all(np.array_equal(w[m], clip[m][:, 1:5]) and np.array_equal(f[m], clip[m][:, 5]) for m in MOD_ORDER)
    w, f = UMGen._score_window(clip, clip, 2, 3, cap)
    assert all(np.array_equal(w[m], clip[m][:, 1:3]) and np.array_equal(f[m], clip[m][:, 3]) for m in MOD_ORDER)
    # default t: the frame behind the conditioning clip
    w, f = UMGen._score_window({m: clip[m][:, :3] for m in MOD_ORDER}, clip, -1, None, cap)
    assert all(np.array_equal(w[m], clip[m][:, :3]) and np.array_equal(f[m], clip[m][:, 3]) for m in MOD_ORDER)
    # one frame [B, S]: against the last frames of the conditioning clip
    w, f = UMGen._score_window(clip, {m: clip[m][:, 0] for m in MOD_ORDER}, 3, None, cap)
    assert all(np.array_equal(w[m], clip[m][:, 3:6]) and np.array_equal(f[m], clip[m][:, 0]) for m in MOD_ORDER)
    for args in ((clip, clip, 5, 5, cap),               # more frames than the engine's window
                 (clip, clip, -1, 0, cap),              # nothing before frame 0
                 (clip, clip, -1, 6, cap),              # t past the clip
                 (clip, clip, 4, 3, cap),               # more frames than lie before t
                 ({m: clip[m][0] for m in MOD_ORDER}, clip, -1, None, cap),                     # 2-D conditioning tokens
                 (clip, {m: clip[m][:1] for m in MOD_ORDER}, -1, None, cap)):                   # B differs
        with pytest.raises(UMGenError):
            UMGen._score_window(*args)
    m = UMGen(tiny_config())
    with pytest.raises(UMGenError, match="load_state_dict"):      # no weights: refused before an engine is created
        m.score(clip, clip)
    assert m._engine is None
