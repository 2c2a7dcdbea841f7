"""-m gpu: attn_temporal_fan_kernel through umgen_dbg_attn_temporal_fan -- the last slot of N items over their scenes' cached slots [0, P),
the launch umgen_score_candidates' last-slot pass makes for every temporal sub-block.

Four scenes with 3, 0, 1 and 37 items: a scene without items, and more items than one LDS group holds (8 at four heads per workgroup, 16
otherwise), so the workgroup's further rounds over the same cached rows run.  (H, P) reach every kernel variant: four heads per workgroup
(P + 1 <= 32, H % 4 == 0), two (H = 2; H = 4 would take it from P + 1 = 33 on, H = 2 at P = 63 is that kernel at its largest LDS request) and
one (H = 1).  Cache slots >= P and all of y start as NaN words.

Checks: (1) float64 on the operands as handed over, the project's bars for this arithmetic (test_gpu_stack_forms.py: 1.6e-2 in bf16, an
eighth of it in fp16, 2e-5 in fp32); (2) byte equality with launch_attn_temporal (t0 = P, write = 0) on the same items with the cache
replicated per item; (3) the cache's bytes unchanged; (4) every y row finite: no slot >= P was read; (5) the 37-item scene alone gives the
bytes it gave among the 41 items.
"""
import ctypes as C

import numpy as np
import pytest

from tests.gpu_util import NAN16, NAN32, SCALE_QK, bits16, check, from_bits16, lib, vp

EPS16 = {1: 1.0, 2: 0.125}     # as in test_gpu_kernels.py: 16-bit tolerances are quoted for bf16
COUNTS = [3, 0, 1, 37]

pytestmark = pytest.mark.gpu


def nan_buf(shape, prec):
    return np.full(shape, NAN16[prec], dtype=np.uint16) if prec else np.full(shape, NAN32, dtype=np.uint32)


def values(words, prec):
    return from_bits16(np.ascontiguousarray(words), prec).astype(np.float64) if prec else np.ascontiguousarray(words).view(np.float32).astype(np.float64)


def ref_last_slot(hist_kv, own, H):
    """float64 softmax of every item's query over its P cached keys and its own: hist_kv [N][P][S][2E], own [N][S][3E] -> [N][S][E]"""
    N, P, S, E2 = hist_kv.shape
    E = E2 // 2
    q = own[..., :E].reshape(N, S, H, 48)
    k = np.concatenate([hist_kv[..., :E], own[:, None, :, E:2 * E]], axis=1).reshape(N, P + 1, S, H, 48)
    v = np.concatenate([hist_kv[..., E:], own[:, None, :, 2 * E:]], axis=1).reshape(N, P + 1, S, H, 48)
    att = np.einsum("nshd,nkshd->nshk", q, k) * SCALE_QK
    att = np.exp(att - att.max(-1, keepdims=True))
    att /= att.sum(-1, keepdims=True)
    return np.einsum("nshk,nkshd->nshd", att, v).reshape(N, S, E)


def fan(prec, qkv, scene_of_item, H, P, cache, y):
    N, S, _ = qkv.shape
    sc = np.ascontiguousarray(scene_of_item, dtype=np.int32)
    check(lib().umgen_dbg_attn_temporal_fan(prec, vp(qkv), N, sc.ctypes.data_as(C.POINTER(C.c_int32)), cache.shape[0], S, H, P, cache.shape[1], vp(cache), vp(y)))


@pytest.mark.parametrize("H,P", [(4, 1), (4, 19), (4, 31), (2, 4), (1, 5), (2, 63)])
@pytest.mark.parametrize("S", [7, 33])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_fan_launch_equals_the_last_slot_launch_on_replicated_caches(prec, S, H, P):
    B, E, Tcap = len(COUNTS), H * 48, P + 3
    scene_of_item = np.repeat(np.arange(B), COUNTS).astype(np.int32)
    N = scene_of_item.size
    rng = np.random.default_rng(1000 * prec + 10 * S + 7 * H + P)
    to_words = (lambda a: bits16(a, prec)) if prec else (lambda a: a.view(np.uint32).copy())
    qkv = to_words(rng.standard_normal((N, S, 3 * E)).astype(np.float32))
    cache = nan_buf((B, Tcap, S, 2 * E), prec)
    cache[:, :P] = to_words(rng.standard_normal((B, P, S, 2 * E)).astype(np.float32))
    c0 = cache.copy()
    y = nan_buf((N, S, E), prec)
    fan(prec, qkv, scene_of_item, H, P, cache, y)
    # (3) (4)
    assert np.array_equal(cache, c0), "the launch changed the cache"
    got = values(y, prec)
    assert np.isfinite(got).all(), "a y row is not finite: a row was left out, or a slot >= P was read"
    # (1)
    ref = ref_last_slot(values(c0[scene_of_item, :P], prec), values(qkv, prec), H)
    d = float(np.abs(got - ref).max())
    bar = 1.6e-2 * EPS16[prec] if prec else 2e-5
    print(f"DIST fan[{prec}] S {S} H {H} P {P}: {d:.3e} bar {bar:.3e}")
    assert d <= bar, f"{d:.3e} from float64 (bar {bar:.3e})"
    # (2) the stand-alone last-slot launch: every item a "scene" with its own copy of the cache
    rep = np.ascontiguousarray(c0[scene_of_item])
    r0 = rep.copy()
    y_ref = nan_buf((N, 1, S, E), prec)
    check(lib().umgen_dbg_attn_temporal_range(prec, vp(qkv), N, 1, S, H, P, 0, 0, Tcap, vp(rep), vp(y_ref)))
    assert np.array_equal(rep, r0)
    assert y.tobytes() == y_ref.tobytes(), "the bytes differ from launch_attn_temporal's on per-item copies of the cache"
    # (5) the 37-item scene alone (its cache block at the same scene index; the other scenes have no items)
    big = scene_of_item == 3
    y_big = nan_buf((int(big.sum()), S, E), prec)
    fan(prec, np.ascontiguousarray(qkv[big]), scene_of_item[big], H, P, cache, y_big)
    assert y_big.tobytes() == y[big].tobytes(), "the 37-item scene alone differs from the launch of 41"
    assert np.array_equal(cache, c0)
