"""Rollout diagnostics without a GPU: the ABI surface (exports, umgen_gen_detail_out's layout, the header's declarations) and the Python argument
handling of Engine.rollout(return_detail=..., topk=...), Engine.frame(detail=...) and UMGen.inference(return_detail=...) on an engine without a
device (the style of tests/test_rollout_logp_host.py), and score_stats.in_sampler_support on a rollout's detail dict."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_rollout_logp_host import _engine_without_device, _scene
from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.model import UMGen
from umgen_amd.score_stats import in_sampler_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("umgen_rollout_detail", "umgen_frame_detail", "umgen_dbg_token_steps_detail", "umgen_dbg_sample_ego_detail")
KEYS = ("rank", "mass_above", "entropy", "topk_tokens", "topk_logp")
FIELDS = ("rank", "mass_above", "entropy", "topk_tok", "topk_logp")


def test_library_exports_the_detail_entry_points_and_the_struct_layout():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.GenDetailOut) == 20 * 8
    assert [n for n, _ in _lib.GenDetailOut._fields_] == [f"{f}_{m}" for f in FIELDS for m in MOD_ORDER]
    assert [n for n, _ in _lib.GenDetailOut._fields_] == [n for n, _ in _lib.ScoreDetailOut._fields_]
    # the existing entry points' arguments, then topk and the struct
    assert lib.umgen_rollout_detail.argtypes[:-2] == lib.umgen_rollout_fan.argtypes
    assert lib.umgen_frame_detail.argtypes[:-2] == lib.umgen_frame_logp.argtypes
    for f in (lib.umgen_rollout_detail, lib.umgen_frame_detail):
        assert f.argtypes[-2] is ctypes.c_int32 and f.argtypes[-1] is ctypes.POINTER(_lib.GenDetailOut)
    assert lib.umgen_dbg_token_steps_detail.argtypes[:3] == lib.umgen_dbg_token_steps_logp.argtypes
    assert lib.umgen_dbg_sample_ego_detail.argtypes[:9] == lib.umgen_dbg_sample_ego_logp.argtypes
    assert len(lib.umgen_dbg_token_steps_detail.argtypes) == 3 + 6 and len(lib.umgen_dbg_sample_ego_detail.argtypes) == 9 + 6


def test_header_declares_both_functions_and_keeps_the_abi_version():
    header = open(os.path.join(ROOT, "include", "umgen.h")).read()
    declared = set(re.findall(r"\b(umgen_[a-z_0-9]+)\s*\(", header))
    assert {"umgen_rollout_detail", "umgen_frame_detail", "umgen_rollout_fan", "umgen_frame_logp"} <= declared
    assert re.search(r"#define UMGEN_ABI_VERSION 4\b", header)
    struct = re.search(r"typedef struct umgen_gen_detail_out \{(.*?)\} umgen_gen_detail_out;", header, re.S).group(1)
    assert re.findall(r"\*((?:rank|mass_above|entropy|topk_tok|topk_logp)_[a-z0-9]+)", struct) == [f"{f}_{m}" for f in FIELDS for m in MOD_ORDER]
    doc = header[header.index("rollout diagnostics"):header.index("typedef struct umgen_gen_detail_out")]
    for word in ("DRAWN", "blanked", "head_tar_bbox3d", "UMGEN_SCORE_TOPK_MAX", "sampling->temperature", "NaN"):
        assert word in doc, word


class Recorder:
    """stands where the C library stands: records the calls the wrapper makes and fills nothing"""
    ALLOWED = ("umgen_rollout", "umgen_rollout_logp", "umgen_rollout_fan", "umgen_rollout_detail", "umgen_frame", "umgen_frame_logp", "umgen_frame_detail")

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in self.ALLOWED:
            raise AssertionError(f"device call {name} reached")

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_detail_buffers_start_as_no_head_ran_with_the_documented_shapes():
    bufs, out = Engine._gen_detail_out((3, 2), 5)
    assert tuple(bufs) == KEYS
    for k, f in zip(KEYS, FIELDS):
        for m in MOD_ORDER:
            a = bufs[k][m]
            assert a.shape == (3, 2, CONTENT_LEN[m]) + ((5,) if k.startswith("topk_") else ())
            if k in ("rank", "topk_tokens"):
                assert a.dtype == np.int32 and (a == -1).all()
            else:
                assert a.dtype == np.float32 and np.isnan(a).all()
            assert ctypes.addressof(getattr(out, f"{f}_{m}").contents) == a.ctypes.data
    bufs, out = Engine._gen_detail_out((), 0)
    assert tuple(bufs) == KEYS[:3] and bufs["rank"]["bbox3d"].shape == (660,)
    assert not out.topk_tok_map and not out.topk_logp_image      # NULL: lists are not asked for


def test_rollout_picks_the_entry_point_and_returns_the_detail_dict_last():
    rec = Recorder()
    e = _engine_without_device(rec)
    sc = _scene(B=2)
    out = e.rollout(sc, 3, cond_frames=3, input_cond_frames=2, seeds=[1, 2])
    assert isinstance(out, dict) and rec.calls[-1][0] == "umgen_rollout"
    out, det = e.rollout(sc, 3, cond_frames=3, input_cond_frames=2, seeds=[1, 2], return_detail=True, topk=4)
    name, args = rec.calls[-1]
    assert name == "umgen_rollout_detail" and len(args) == 25 and args[1:3] == (2, 1) and args[-2] == 4 and args[-4] is None
    assert tuple(det) == KEYS
    for m in MOD_ORDER:
        assert out[m].shape == (2, 5, CONTENT_LEN[m])
        assert det["rank"][m].shape == (2, 3, CONTENT_LEN[m]) and det["rank"][m].dtype == np.int64 and (det["rank"][m] == -1).all()
        assert det["topk_tokens"][m].shape == (2, 3, CONTENT_LEN[m], 4) and det["topk_tokens"][m].dtype == np.int64
        assert det["topk_logp"][m].shape == (2, 3, CONTENT_LEN[m], 4) and det["entropy"][m].dtype == np.float32
    out, logp, det = e.rollout(sc, 3, cond_frames=3, input_cond_frames=2, seeds=[1, 2], return_logp=True, return_detail=True)
    assert rec.calls[-1][0] == "umgen_rollout_detail" and rec.calls[-1][1][-4] is not None and tuple(det) == KEYS[:3]
    assert logp["map"].shape == (2, 3, 1024)
    # with samples=N: [B, N, ...]
    out, logp, det = e.rollout(sc, 2, cond_frames=3, input_cond_frames=2, seeds=np.arange(6), return_logp=True, samples=3, topk=16)
    name, args = rec.calls[-1]
    assert name == "umgen_rollout_detail" and args[1:3] == (2, 3) and args[-2] == 16
    assert out["pose"].shape == (2, 3, 4, 3) and logp["pose"].shape == (2, 3, 2, 3) and det["topk_logp"]["image"].shape == (2, 3, 2, 512, 16)
    # the calls without detail are the ones they were
    e.rollout(sc, 2, cond_frames=3, input_cond_frames=2, seeds=np.arange(6), samples=3)
    assert rec.calls[-1][0] == "umgen_rollout_fan"
    e.rollout(sc, 2, cond_frames=3, input_cond_frames=2, seeds=[0, 1], return_logp=True)
    assert rec.calls[-1][0] == "umgen_rollout_logp"


def test_bad_detail_arguments_are_refused_before_any_device_call():
    e = _engine_without_device()
    sc = _scene()
    w = {m: a[0] for m, a in sc.items()}
    for topk in (17, -1, 2.0, True):
        with pytest.raises(UMGenError, match="topk"):
            e.rollout(sc, 1, cond_frames=3, input_cond_frames=2, return_detail=True, topk=topk)
        with pytest.raises(UMGenError, match="topk"):
            e.frame(w, detail=True, topk=topk)
    hot = tiny_config()
    hot.sfmx_temp = float("inf")
    with pytest.raises(UMGenError, match="temperature"):
        e.rollout(sc, 1, cond_frames=3, input_cond_frames=2, return_detail=True, sampling=hot)
    with pytest.raises(UMGenError):
        e.rollout(dict(sc, map=sc["map"][:, :, :1000]), 1, cond_frames=3, input_cond_frames=2, return_detail=True)


def test_frame_adds_detail_to_the_trace_dict():
    rec = Recorder()
    e = _engine_without_device(rec)
    w = {m: a[0] for m, a in _scene().items()}
    toks, tr = e.frame(w, seed=3, detail=True, topk=2)
    name, args = rec.calls[-1]
    assert name == "umgen_frame_detail" and len(args) == 19 and args[-3] is None and args[-2] == 2 and set(tr) == {"detail"}
    assert tr["detail"]["topk_tokens"]["bbox3d"].shape == (660, 2) and tr["detail"]["mass_above"]["pose"].shape == (3,)
    toks, tr = e.frame(w, seed=3, detail=True, logp=True, trace=True)
    assert rec.calls[-1][0] == "umgen_frame_detail" and rec.calls[-1][1][-3] is not None
    assert {"detail", "logp", "counters", "logits_map"} <= set(tr) and tuple(tr["detail"]) == KEYS[:3]
    toks, tr = e.frame(w, seed=3, logp=True)
    assert rec.calls[-1][0] == "umgen_frame_logp"


def test_model_inference_passes_return_detail_through_as_torch_tensors():
    m = UMGen(tiny_config())
    sc = {k: torch.from_numpy(v) for k, v in _scene().items()}
    rec = Recorder()
    m._engine, m._loaded = _engine_without_device(rec), True
    m._engine_args = dict(getattr(m, "_engine_args", {}) or {}, max_batch=8)
    out, det = m.inference(2, cond_frames=2, pred_task="pose_map_bbox3d_image", input_cond_tokens=sc, return_detail=True, topk=3)
    assert rec.calls[-1][0] == "umgen_rollout_detail"
    assert isinstance(out["map"], np.ndarray) and isinstance(det["rank"]["map"], torch.Tensor) and det["rank"]["map"].dtype == torch.int64
    assert tuple(det["topk_logp"]["image"].shape) == (1, 2, 512, 3)
    out, logp, det = m.inference(1, cond_frames=2, pred_task="pose_map_bbox3d_image", input_cond_tokens=sc, return_logp=True, return_detail=True,
                                 num_samples=2)
    assert rec.calls[-1][0] == "umgen_rollout_detail" and rec.calls[-1][1][1:3] == (1, 2)
    assert tuple(out["pose"].shape) == (1, 2, 3, 3) and tuple(logp["total"].shape) == (1, 2, 1) and tuple(det["entropy"]["bbox3d"].shape) == (1, 2, 1, 660)
    m._engine = None


def test_in_sampler_support_reads_a_rollout_detail_dict():
    """a hand-made detail dict in Engine.rollout's layout [B, new_frames, S_mod]: the helper takes its arrays unchanged"""
    rank = np.array([[[0, 4, 5, 16, -1]]])
    mass = np.array([[[0.0, 0.39, 0.41, 0.95, np.nan]]], np.float32)
    det = {"rank": {"map": rank}, "mass_above": {"map": mass}}
    assert in_sampler_support(det["rank"]["map"], det["mass_above"]["map"], "topk", top_k=5).tolist() == [[[True, True, False, False, True]]]
    assert in_sampler_support(det["rank"]["map"], det["mass_above"]["map"], "topk", top_k=16).tolist() == [[[True, True, True, False, True]]]
    assert in_sampler_support(det["rank"]["map"], det["mass_above"]["map"], "topp", p=0.4).tolist() == [[[True, True, False, False, False]]]
    with pytest.raises(ValueError):
        in_sampler_support(rank, mass, "greedy")
