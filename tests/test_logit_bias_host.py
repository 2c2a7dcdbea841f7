"""Constrained generation without a GPU: the table builders of umgen_amd/constraints.py, the ABI surface (exports, struct layouts, the header's
declarations) and the Python argument handling of Engine.rollout(logit_bias=..., return_logz=...), Engine.frame(...) and UMGen.inference(...) on an
engine without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_rollout_logp_host import _engine_without_device, _scene
from umgen_amd import _lib, constraints, scene_io
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import UMGenError
from umgen_amd.model import UMGen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("umgen_rollout_biased", "umgen_frame_biased", "umgen_dbg_token_steps_biased", "umgen_dbg_token_steps_biased_detail", "umgen_dbg_sample_ego_biased",
       "umgen_dbg_sample_biased")


# ---- the builders ------------------------------------------------------------------------------------------------------------------------
def test_builders_give_the_table_shapes_of_the_c_call():
    assert constraints.ban("map", [3, 4])["map"].shape == (8192,)
    assert constraints.ban("image", [0], vocab=56)["image"].shape == (56,)
    assert constraints.ban("bbox3d", [1027])["bbox3d"].shape == (11, 1028)
    assert constraints.ban("pose", [0, 1023], attr=1)["pose"].shape == (3, 1024)
    t = constraints.ban("bbox3d", [7, 9], attr=3)["bbox3d"]
    assert t.dtype == np.float32 and np.isneginf(t[3, [7, 9]]).all() and np.isneginf(t).sum() == 2 and not t[np.isfinite(t)].any()
    t = constraints.allow_only("pose", range(500, 520), attr=(0, 2))["pose"]
    assert np.isneginf(t[0]).sum() == 1004 and not t[1].any() and (t[2] == t[0]).all() and not t[0, 500:520].any()
    v = np.linspace(-1, 1, 1028).astype(np.float32)
    t = constraints.bias("bbox3d", v)["bbox3d"]
    assert (t == v[None]).all()


def test_merge_adds_and_minus_inf_wins():
    a = constraints.bias("map", np.full(8192, 0.5, np.float32))
    b = constraints.ban("map", [10])
    c = constraints.bias("map", np.full(8192, 0.25, np.float32))
    m = constraints.merge(a, b, c, None, constraints.ban("pose", [1], attr=0))
    assert set(m) == {"map", "pose"} and np.isneginf(m["map"][10]) and (np.delete(m["map"], 10) == 0.75).all()
    assert np.isneginf(constraints.merge(b, b)["map"][10]) and constraints.merge(b, b)["map"].dtype == np.float32
    # a [vocab] table of a many-row class is every row's
    m = constraints.merge({"bbox3d": np.full(1028, 1.0, np.float32)}, constraints.ban("bbox3d", [5], attr=10))
    assert m["bbox3d"].shape == (11, 1028) and np.isneginf(m["bbox3d"][10, 5]) and m["bbox3d"][0, 5] == 1.0


def test_ban_categories_bans_the_category_tokens_at_attribute_10():
    t = constraints.ban_categories(["pedestrian"])["bbox3d"]
    assert scene_io.CATEGORIES.index("pedestrian") == 2
    assert np.isneginf(t[10, 1026]) and np.isneginf(t).sum() == 1
    t = constraints.ban_categories(["vehicle", "bicycle"])["bbox3d"]
    assert np.isneginf(t[10, [1024, 1025]]).all() and np.isneginf(t).sum() == 2
    with pytest.raises(ValueError):
        constraints.ban_categories(["tram"])


def test_pose_limits_against_the_decoder_on_all_bins():
    val = scene_io.decode_ego_numpy(np.repeat(np.arange(1024)[:, None], 3, axis=1)).reshape(1024, 3)
    lim = {"dx": (float(val[300, 0]), float(val[800, 0])), "dheading": (float(np.sort(val[:, 2])[100]), float(np.sort(val[:, 2])[110]))}
    t = constraints.pose_limits(**lim)["pose"]
    assert t.shape == (3, 1024) and not t[1].any()
    for c, name in ((0, "dx"), (2, "dheading")):
        inside = (val[:, c] >= lim[name][0]) & (val[:, c] <= lim[name][1])
        assert (np.isneginf(t[c]) == ~inside).all() and not t[c][inside].any() and inside.any()
    assert int((~np.isneginf(t[2])).sum()) == 11


def test_an_empty_allowed_set_raises():
    with pytest.raises(ValueError):
        constraints.allow_only("map", [])
    with pytest.raises(ValueError):
        constraints.ban("image", range(56), vocab=56)
    with pytest.raises(ValueError):
        constraints.merge(constraints.allow_only("map", [1]), constraints.allow_only("map", [2]))
    with pytest.raises(ValueError):
        constraints.pose_limits(dx=(1e6, 2e6))
    with pytest.raises(ValueError):
        constraints.bias("map", np.full(8192, np.nan, np.float32))
    with pytest.raises(ValueError):
        constraints.ban("lidar", [0])


# ---- the ABI surface ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_biased_entry_points_and_the_struct_layouts():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LogitBias) == 32 and ctypes.sizeof(_lib.LogzOut) == 32
    assert lib.umgen_rollout_biased.argtypes[:-2] == lib.umgen_rollout_detail.argtypes
    assert lib.umgen_frame_biased.argtypes[:-2] == lib.umgen_frame_detail.argtypes
    for f in (lib.umgen_rollout_biased, lib.umgen_frame_biased):
        assert f.argtypes[-2] is ctypes.POINTER(_lib.LogitBias) and f.argtypes[-1] is ctypes.POINTER(_lib.LogzOut)


def test_header_declares_the_entry_points_and_the_structs_in_the_bindings_field_order():
    header = open(os.path.join(ROOT, "include", "umgen.h")).read()
    declared = set(re.findall(r"\b(umgen_[a-z_0-9]+)\s*\(", header))
    assert {"umgen_rollout_biased", "umgen_frame_biased", "umgen_rollout_detail", "umgen_frame_detail"} <= declared
    assert re.search(r"#define UMGEN_ABI_VERSION 4\b", header)
    bias = re.search(r"typedef struct umgen_logit_bias \{(.*?)\} umgen_logit_bias;", header, re.S).group(1)
    assert re.findall(r"\*([a-z0-9]+)", bias) == [n for n, _ in _lib.LogitBias._fields_] == list(MOD_ORDER)
    logz = re.search(r"typedef struct umgen_logz_out\s*\{(.*?)\} umgen_logz_out;", header, re.S).group(1)
    assert re.findall(r"\*(logz_[a-z0-9]+)", logz) == [n for n, _ in _lib.LogzOut._fields_] == [f"logz_{m}" for m in MOD_ORDER]
    # the consequences are part of the contract: documented where the functions are declared
    for words in ("last ALLOWED entry", "rank < top_k", "lp + r[tok] - logz", "UMGEN_E_INVALID"):
        assert words in header, words


# ---- Python argument handling: no engine exists on this machine ------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith(("umgen_rollout", "umgen_frame")):
            raise AssertionError(f"device call {name} reached")

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _tables():
    return {"pose": np.zeros((3, 1024), np.float32), "map": np.zeros(8192, np.float32), "bbox3d": np.zeros((11, 1028), np.float32),
            "image": np.zeros(8192, np.float32)}


def test_rollout_takes_the_biased_entry_point_only_when_asked():
    rec = Recorder()
    e = _engine_without_device(rec)
    sc = _scene(B=2)
    kw = dict(cond_frames=3, input_cond_frames=2, seeds=[1, 2])
    e.rollout(sc, 3, **kw)
    assert rec.calls[-1][0] == "umgen_rollout"
    e.rollout(sc, 3, return_logp=True, **kw)
    assert rec.calls[-1][0] == "umgen_rollout_logp"
    out = e.rollout(sc, 3, logit_bias={"bbox3d": np.zeros(1028)}, **kw)          # a [vocab] array is every row's; float64 is converted
    name, args = rec.calls[-1]
    assert name == "umgen_rollout_biased" and len(args) == 27 and isinstance(out, dict)
    out, logp, logz, det = e.rollout(sc, 3, logit_bias=_tables(), return_logz=True, return_logp=True, return_detail=True, topk=2, **kw)
    for m in MOD_ORDER:
        assert logz[m].shape == logp[m].shape == (2, 3, CONTENT_LEN[m]) and logz[m].dtype == np.float32 and np.isnan(logz[m]).all()
    assert det["topk_tokens"]["map"].shape == (2, 3, 1024, 2)
    out, logz = e.rollout(sc, 3, return_logz=True, **kw)                            # logz without a bias is allowed
    assert rec.calls[-1][0] == "umgen_rollout_biased" and logz["pose"].shape == (2, 3, 3)
    out, logz = e.rollout(sc, 1, return_logz=True, samples=2, cond_frames=3, input_cond_frames=2)
    assert logz["image"].shape == (2, 2, 1, 512) and out["image"].shape == (2, 2, 3, 512)
    e.rollout(sc, 3, logit_bias={"map": None}, **kw)                                # no table at all: the plain call
    assert rec.calls[-1][0] == "umgen_rollout"


def test_rollout_and_frame_refuse_bad_tables_before_any_device_call():
    e = _engine_without_device()
    sc = _scene()
    bad = [{"lidar": np.zeros(4, np.float32)}, {"map": np.zeros(8191, np.float32)}, {"bbox3d": np.zeros((10, 1028), np.float32)},
           {"pose": np.zeros((3, 1024), np.int64)}, {"map": np.full(8192, np.nan, np.float32)}, {"image": np.full(8192, np.inf, np.float32)},
           {"pose": np.full((3, 1024), -np.inf, np.float32)}, [np.zeros(8192, np.float32)]]
    w = {m: a[0] for m, a in sc.items()}
    for tabs in bad:
        with pytest.raises(UMGenError):
            e.rollout(sc, 1, cond_frames=3, input_cond_frames=2, logit_bias=tabs)
        with pytest.raises(UMGenError):
            e.frame(w, logit_bias=tabs)
    one_inf = _tables()
    one_inf["bbox3d"][4, 7] = np.inf
    with pytest.raises(UMGenError, match=r"bbox3d.*row 4 index 7"):
        e.rollout(sc, 1, cond_frames=3, input_cond_frames=2, logit_bias=one_inf)


def test_frame_adds_logz_to_the_trace_dict():
    rec = Recorder()
    e = _engine_without_device(rec)
    w = {m: a[0] for m, a in _scene().items()}
    toks, tr = e.frame(w, seed=3)
    assert tr is None and rec.calls[-1][0] == "umgen_frame"
    toks, tr = e.frame(w, seed=3, logz=True)
    assert rec.calls[-1][0] == "umgen_frame_biased" and len(rec.calls[-1][1]) == 21 and set(tr) == {"logz"}
    assert [tr["logz"][m].shape for m in MOD_ORDER] == [(CONTENT_LEN[m],) for m in MOD_ORDER]
    toks, tr = e.frame(w, seed=3, logit_bias=_tables(), logp=True, detail=True, topk=3)
    assert rec.calls[-1][0] == "umgen_frame_biased" and set(tr) == {"logp", "detail"}


def test_model_inference_passes_the_tables_through():
    m = UMGen(tiny_config())
    sc = {k: torch.from_numpy(v) for k, v in _scene().items()}
    rec = Recorder()
    m._engine, m._loaded = _engine_without_device(rec), True
    kw = dict(cond_frames=2, pred_task="pose_map_bbox3d_image", input_cond_tokens=sc)
    out = m.inference(2, **kw)
    assert rec.calls[-1][0] == "umgen_rollout"
    tabs = {"bbox3d": torch.from_numpy(constraints.ban_categories(["pedestrian"])["bbox3d"])}
    out = m.inference(2, logit_bias=tabs, **kw)
    assert rec.calls[-1][0] == "umgen_rollout_biased" and isinstance(out, dict)
    out, logp, logz = m.inference(2, logit_bias=tabs, return_logz=True, return_logp=True, **kw)
    for k in MOD_ORDER:
        assert isinstance(logz[k], torch.Tensor) and logz[k].dtype == torch.float32 and tuple(logz[k].shape) == tuple(logp[k].shape) == (1, 2, CONTENT_LEN[k])
    out, logz, det = m.inference(2, return_logz=True, return_detail=True, num_samples=1, **kw)
    assert tuple(logz["map"].shape) == (1, 1, 2, 1024) and isinstance(det["rank"]["map"], torch.Tensor)
    with pytest.raises(UMGenError):
        m.inference(2, logit_bias=[1, 2], **kw)
    m._engine = None
