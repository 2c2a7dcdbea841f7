"""Log-likelihoods of generated frames without a GPU: the ABI surface (exports, umgen_logp_out's layout, the header's declarations) and the Python
argument handling of Engine.rollout(return_logp=...), Engine.frame(logp=...) and UMGen.inference(return_logp=...) on an engine without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.model import UMGen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("umgen_rollout_logp", "umgen_frame_logp", "umgen_dbg_token_steps_logp", "umgen_dbg_sample_ego_logp")


def test_library_exports_the_logp_entry_points_and_the_struct_layout():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LogpOut) == 32
    assert [n for n, _ in _lib.LogpOut._fields_] == [f"logp_{m}" for m in MOD_ORDER]
    # the old entry points' arguments, then the struct
    assert lib.umgen_rollout_logp.argtypes[:-1] == lib.umgen_rollout.argtypes and lib.umgen_frame_logp.argtypes[:-1] == lib.umgen_frame.argtypes
    assert lib.umgen_rollout_logp.argtypes[-1] is lib.umgen_frame_logp.argtypes[-1] is ctypes.POINTER(_lib.LogpOut)


def test_header_declares_both_functions_and_keeps_the_abi_version():
    header = open(os.path.join(ROOT, "include", "umgen.h")).read()
    declared = set(re.findall(r"\b(umgen_[a-z_0-9]+)\s*\(", header))
    assert {"umgen_rollout_logp", "umgen_frame_logp", "umgen_rollout", "umgen_frame"} <= declared
    assert re.search(r"#define UMGEN_ABI_VERSION 4\b", header)
    struct = re.search(r"typedef struct umgen_logp_out \{(.*?)\} umgen_logp_out;", header, re.S).group(1)
    assert re.findall(r"\*(logp_[a-z0-9]+)", struct) == [f"logp_{m}" for m in MOD_ORDER]
    # the rule-constraint semantics are part of the contract: documented where the functions are declared
    assert "DRAWN" in header and "blank" in header


# ---- Python argument handling: no engine exists on this machine; a device call is an assertion failure --------------------------------

class Recorder:
    """stands where the C library stands: records the calls the wrapper makes and fills nothing"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in ("umgen_rollout", "umgen_rollout_logp", "umgen_frame", "umgen_frame_logp"):
            raise AssertionError(f"device call {name} reached")

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _engine_without_device(lib=None):
    e = Engine.__new__(Engine)
    e.cfg = tiny_config()
    e._h = None

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"device call {name} reached")
    e.lib = lib or NoDevice()
    return e


def _scene(B=1, T=2, seed=0):
    rng = np.random.default_rng(seed)
    hi = {"pose": 1024, "map": 8192, "bbox3d": 1028, "image": 8192}
    return {m: rng.integers(0, hi[m], (B, T, CONTENT_LEN[m])) for m in MOD_ORDER}


def test_logp_buffers_start_as_nan_with_the_documented_shapes():
    logp, lp = Engine._logp_out((3, 2))
    for m in MOD_ORDER:
        assert logp[m].shape == (3, 2, CONTENT_LEN[m]) and logp[m].dtype == np.float32 and np.isnan(logp[m]).all()
        assert ctypes.addressof(getattr(lp, f"logp_{m}").contents) == logp[m].ctypes.data
    one, _ = Engine._logp_out(())
    assert [one[m].shape for m in MOD_ORDER] == [(CONTENT_LEN[m],) for m in MOD_ORDER]


def test_rollout_picks_the_entry_point_and_returns_tokens_or_a_pair():
    rec = Recorder()
    e = _engine_without_device(rec)
    sc = _scene(B=2)
    out = e.rollout(sc, 3, cond_frames=3, input_cond_frames=2, seeds=[1, 2])
    assert isinstance(out, dict) and rec.calls[-1][0] == "umgen_rollout" and len(rec.calls[-1][1]) == 20
    out, logp = e.rollout(sc, 3, cond_frames=3, input_cond_frames=2, seeds=[1, 2], return_logp=True)
    name, args = rec.calls[-1]
    assert name == "umgen_rollout_logp" and len(args) == 21
    for m in MOD_ORDER:
        assert out[m].shape == (2, 5, CONTENT_LEN[m]) and out[m].dtype == np.int64
        assert logp[m].shape == (2, 3, CONTENT_LEN[m]) and logp[m].dtype == np.float32 and np.isnan(logp[m]).all()      # nothing wrote them here
    out, logp = e.rollout(sc, 0, cond_frames=3, input_cond_frames=2, seeds=[1, 2], return_logp=True)
    assert logp["map"].shape == (2, 0, 1024)


def test_rollout_refuses_bad_arguments_before_any_device_call():
    e = _engine_without_device()
    sc = _scene()
    for kw in (dict(tokens=dict(sc, map=sc["map"][:, :, :1000]), new_frames=1),                                  # wrong S
               dict(tokens=sc, new_frames=-1),
               dict(tokens=sc, new_frames=1, init_tokens={"image": sc["image"]}),                             # not a supported given modality
               dict(tokens=sc, new_frames=1, init_tokens={"pose": sc["pose"][:, :, :2]})):                    # wrong control shape
        with pytest.raises(UMGenError):
            e.rollout(cond_frames=3, input_cond_frames=2, return_logp=True, **kw)


def test_frame_adds_logp_to_the_trace_dict_with_and_without_a_trace():
    rec = Recorder()
    e = _engine_without_device(rec)
    w = {m: a[0] for m, a in _scene().items()}
    toks, tr = e.frame(w, seed=3)
    assert tr is None and rec.calls[-1][0] == "umgen_frame" and len(rec.calls[-1][1]) == 16
    toks, tr = e.frame(w, seed=3, logp=True)
    assert rec.calls[-1][0] == "umgen_frame_logp" and len(rec.calls[-1][1]) == 17 and set(tr) == {"logp"}
    assert [tr["logp"][m].shape for m in MOD_ORDER] == [(CONTENT_LEN[m],) for m in MOD_ORDER] and tr["logp"]["image"].dtype == np.float32
    forced = {m: a[0, 0] for m, a in _scene(seed=1).items()}
    toks, tr = e.frame(w, forced=forced, trace=True, logp=True, given={"map": forced["map"]})
    assert {"logp", "counters", "logits_map", "ego_logits", "cond"} <= set(tr)
    toks, tr = e.frame(w, forced=forced, logp=False)
    assert set(tr) == {"counters"} and rec.calls[-1][0] == "umgen_frame"


def test_model_inference_passes_return_logp_through_as_torch_tensors():
    m = UMGen(tiny_config())
    sc = {k: torch.from_numpy(v) for k, v in _scene().items()}
    with pytest.raises(UMGenError, match="load_state_dict"):      # no weights: refused before an engine is created
        m.inference(1, cond_frames=2, pred_task="pose_map_bbox3d_image", input_cond_tokens=sc, return_logp=True)
    with pytest.raises(UMGenError, match="pred_task"):
        m.inference(1, cond_frames=2, input_cond_tokens=sc, return_logp=True)
    assert m._engine is None
    rec = Recorder()
    m._engine, m._loaded = _engine_without_device(rec), True
    out = m.inference(2, cond_frames=2, pred_task="pose_map_bbox3d_image", input_cond_tokens=sc)
    assert isinstance(out, dict) and isinstance(out["map"], np.ndarray) and rec.calls[-1][0] == "umgen_rollout"
    out, logp = m.inference(2, cond_frames=2, pred_task="pose_map_bbox3d_image", input_cond_tokens=sc, return_logp=True)
    assert rec.calls[-1][0] == "umgen_rollout_logp"
    for k in MOD_ORDER:
        assert isinstance(out[k], np.ndarray) and out[k].shape == (1, 4, CONTENT_LEN[k])
        assert isinstance(logp[k], torch.Tensor) and logp[k].dtype == torch.float32 and tuple(logp[k].shape) == (1, 2, CONTENT_LEN[k])
    m._engine = None
