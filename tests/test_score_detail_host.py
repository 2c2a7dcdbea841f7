"""umgen_score_detail without a GPU: the ABI surface, the Python argument handling and the host helpers that read its outputs."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.test_score_host import _engine_without_device, _tokens
from umgen_amd import _lib
from umgen_amd.config import MOD_ORDER
from umgen_amd.engine import UMGenError
from umgen_amd.model import UMGen
from umgen_amd.score_stats import in_sampler_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_detail_entry_points_and_the_struct_layout():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    for name in ("umgen_score_detail", "umgen_dbg_head_detail", "umgen_dbg_logits_detail"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.ScoreDetailOut) == 160
    assert [n for n, _ in _lib.ScoreDetailOut._fields_] == [f"{k}_{m}" for k in ("rank", "mass_above", "entropy", "topk_tok", "topk_logp")
                                                            for m in MOD_ORDER]
    assert ctypes.sizeof(_lib.ScoreOut) == 64      # umgen_score's struct is untouched


def test_header_declares_the_call_at_abi_4():
    h = open(os.path.join(ROOT, "include", "umgen.h")).read()
    assert re.search(r"#define\s+UMGEN_ABI_VERSION\s+4\b", h)
    assert re.search(r"#define\s+UMGEN_SCORE_TOPK_MAX\s+16\b", h) and _lib.SCORE_TOPK_MAX == 16
    assert re.search(r"int\s+umgen_score_detail\s*\(", h)
    body = re.search(r"typedef struct umgen_score_detail_out \{(.*?)\} umgen_score_detail_out;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*\s*(\w+)", body)
    assert names == [n for n, _ in _lib.ScoreDetailOut._fields_]
    call = re.search(r"int\s+umgen_score_detail\s*\((.*?)\);", h, re.S).group(1)
    assert re.search(r"int32_t\s+topk,\s*float\s+temperature,\s*umgen_score_out\s*\*out,\s*umgen_score_detail_out\s*\*detail\s*$", call)


@pytest.mark.parametrize("kwargs,needle", [
    (dict(topk=17), "topk"), (dict(topk=-1), "topk"), (dict(detail=True, topk=17), "topk"),
    (dict(detail=True, temperature=0.0), "temperature"), (dict(detail=True, temperature=float("nan")), "temperature"),
    (dict(topk=4, temperature=float("inf")), "temperature"), (dict(detail=True, temperature=-0.5), "temperature"),
    (dict(detail=("topk_tokens",), topk=0), "topk=0"), (dict(detail=("rank", "topk_logp")), "topk=0"),
    (dict(detail=("ranks",)), "unknown"),
])
def test_engine_score_refuses_bad_detail_arguments_before_a_device_call(kwargs, needle):
    e = _engine_without_device()      # any device call raises AssertionError
    w, nx = _tokens()
    with pytest.raises(UMGenError, match=needle):
        e.score(w, nx, **kwargs)


def test_detail_arguments_select_the_outputs():
    e = _engine_without_device()
    assert e._detail_args(False, 0, 1.0) == (None, 0, 1.0)      # the default call stays umgen_score
    assert e._detail_args(True, 0, 0.7) == (("rank", "mass_above", "entropy"), 0, 0.7)
    assert e._detail_args(False, 5, 1)[0] == e.DETAIL_KEYS
    assert e._detail_args(("entropy",), 0, 1.0)[0] == ("entropy",)
    m = UMGen(e.cfg)
    w, nx = _tokens(B=1)
    with pytest.raises(UMGenError, match="topk"):      # UMGen.score checks them before asking for weights or an engine
        m.score(w, nx, topk=17)
    with pytest.raises(UMGenError, match="temperature"):
        m.score(w, nx, detail=True, temperature=0.0)
    assert m._engine is None


def _reference_masks(lg, top_k, p, temp):
    """the reference sampler's keep masks per token, restated in float64 numpy: UMGen.topk removes `logits < k-th value`; its nucleus step
    sorts softmax(logits / temp) in descending order and removes where (cumsum - sorted) > p"""
    kth = np.sort(lg, axis=-1)[..., -min(top_k, lg.shape[-1])]
    keep_k = ~(lg < kth[..., None])
    z = lg / temp
    pr = np.exp(z - z.max(-1, keepdims=True))
    pr /= pr.sum(-1, keepdims=True)
    idx = np.argsort(-pr, axis=-1, kind="stable")
    srt = np.take_along_axis(pr, idx, -1)
    removed_sorted = (np.cumsum(srt, -1) - srt) > p
    keep_p = np.empty_like(removed_sorted)
    np.put_along_axis(keep_p, idx, ~removed_sorted, -1)
    return keep_k, keep_p


@pytest.mark.parametrize("V", [56, 1028])
def test_in_sampler_support_equals_the_reference_masks_at_every_token(V):
    rng = np.random.default_rng(V)
    lg = (2.5 * rng.standard_normal((6, V))).astype(np.float32).astype(np.float64)
    temp = 0.7
    z = lg / temp
    pr = np.exp(z - z.max(-1, keepdims=True))
    pr /= pr.sum(-1, keepdims=True)
    above = lg[:, None, :] > lg[:, :, None]                       # [row, token, other]: other's logit strictly above token's
    rank = above.sum(-1)
    mass_above = (above * pr[:, None, :]).sum(-1)
    for top_k, p in ((5, 0.9), (16, 0.5), (1, 0.05)):
        keep_k, keep_p = _reference_masks(lg, top_k, p, temp)
        assert np.array_equal(in_sampler_support(rank, mass_above, "topk", top_k=top_k), keep_k), (V, top_k)
        assert np.array_equal(in_sampler_support(rank, mass_above, "topp", p=p), keep_p), (V, p)
        assert keep_k.sum() == 6 * min(top_k, V) and 0 < keep_p.sum() < keep_p.size
    with pytest.raises(ValueError):
        in_sampler_support(rank, mass_above, "greedy")


def test_topk_acc_arithmetic():
    rank = {m: np.array([[0, 0, 1, 4, 5, 15, 16, 100]]) for m in MOD_ORDER}
    rank["pose"] = np.array([[0, 3, 20]])
    acc = UMGen._topk_acc(rank)
    assert acc["map"] == {1: 2 / 8, 5: 4 / 8, 16: 6 / 8}
    assert acc["pose"] == {1: 1 / 3, 5: 2 / 3, 16: 2 / 3}
    assert set(acc) == set(MOD_ORDER)
