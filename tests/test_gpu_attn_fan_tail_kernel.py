"""-m gpu: attn_temporal_fan_tail_kernel through umgen_dbg_attn_temporal_fan_tail -- the tails of Wt slots of N items over their scenes' cached
slots [0, P), the launch umgen_score_futures' tail passes make for every temporal sub-block.

Four scenes with 3, 0, 1 and 11 items: a scene without items, and more items than one round of the workgroup holds (kFanItems / Wt whole items:
8 rows at four heads per workgroup, 16 otherwise).  (H, P, Wt) reach every form: a tail of one (the fan kernel's case), tails that do not divide a
round (4,17,3: two items and two idle rows; 2,4,5: three items and one idle row), tails that fill it (4,12,8; 2,9,16; 1,5,16: one item per round,
eleven rounds), four / two / one head per workgroup, and P = 40, past the four-head form's LDS.  Cache slots >= P and all of y start as NaN words.

Checks: (1) float64 on the operands as handed over, with the bars test_gpu_attn_fan_kernel.py uses for this arithmetic (2e-5 in fp32, 1.6e-2 in
bf16, an eighth of it in fp16); (2) byte equality with launch_attn_temporal (t0 = P, Tn = Wt, write = 0) on per-item copies of the cache; (3) for
Wt == 1 byte equality with umgen_dbg_attn_temporal_fan; (4) the cache's bytes unchanged and every y row finite; (5) with q0 = P + Wt - 1 and NaN q
rows below it only the last tail slot's y is written, with the bytes it had with q0 = P; (6) the 11-item scene alone gives the bytes it gave in
the full launch; (7) a tail no form of the kernel holds is refused with an error code and nothing is launched.
"""
import ctypes as C

import numpy as np
import pytest

from tests.gpu_util import NAN16, NAN32, SCALE_QK, bits16, check, from_bits16, lib, vp

EPS16 = {1: 1.0, 2: 0.125}     # as in test_gpu_kernels.py: 16-bit tolerances are quoted for bf16
COUNTS = [3, 0, 1, 11]
UNSUPPORTED = -5               # UMGEN_E_UNSUPPORTED (include/umgen.h)

pytestmark = pytest.mark.gpu


def nan_buf(shape, prec):
    return np.full(shape, NAN16[prec], dtype=np.uint16) if prec else np.full(shape, NAN32, dtype=np.uint32)


def values(words, prec):
    return from_bits16(np.ascontiguousarray(words), prec).astype(np.float64) if prec else np.ascontiguousarray(words).view(np.float32).astype(np.float64)


def ref_tails(hist_kv, own, H):
    """float64 softmax of query (i, j) over item i's P cached keys and its own tail rows 0 .. j: hist_kv [N][P][S][2E], own [N][Wt][S][3E] -> [N][Wt][S][E]"""
    N, P, S, E2 = hist_kv.shape
    E, Wt = E2 // 2, own.shape[1]
    q = own[..., :E].reshape(N, Wt, S, H, 48)
    k = np.concatenate([hist_kv[..., :E], own[..., E:2 * E]], axis=1).reshape(N, P + Wt, S, H, 48)
    v = np.concatenate([hist_kv[..., E:], own[..., 2 * E:]], axis=1).reshape(N, P + Wt, S, H, 48)
    att = np.einsum("njshd,nkshd->njshk", q, k) * SCALE_QK
    causal = np.arange(P + Wt)[None, :] <= (P + np.arange(Wt))[:, None]          # [Wt][P + Wt]
    att = np.where(causal[None, :, None, None, :], att, -np.inf)
    att = np.exp(att - att.max(-1, keepdims=True))
    att /= att.sum(-1, keepdims=True)
    return np.einsum("njshk,nkshd->njshd", att, v).reshape(N, Wt, S, E)


def fan_tail(prec, qkv, scene_of_item, H, P, q0, cache, y):
    N, Wt, S, _ = qkv.shape
    sc = np.ascontiguousarray(scene_of_item, dtype=np.int32)
    return lib().umgen_dbg_attn_temporal_fan_tail(prec, vp(qkv), N, Wt, sc.ctypes.data_as(C.POINTER(C.c_int32)), cache.shape[0], S, H, P, q0, cache.shape[1],
                                                  vp(cache), vp(y))


@pytest.mark.parametrize("H,P,Wt", [(4, 1, 1), (4, 3, 2), (4, 12, 8), (4, 17, 3), (2, 4, 5), (2, 9, 16), (1, 5, 16), (2, 40, 3)])
@pytest.mark.parametrize("S", [7, 33])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_tail_launch_equals_the_range_launch_on_replicated_caches(prec, S, H, P, Wt):
    B, E, Tcap = len(COUNTS), H * 48, P + Wt + 1
    scene_of_item = np.repeat(np.arange(B), COUNTS).astype(np.int32)
    N = scene_of_item.size
    rng = np.random.default_rng(100000 * prec + 1000 * S + 100 * H + 10 * P + Wt)
    to_words = (lambda a: bits16(a, prec)) if prec else (lambda a: a.view(np.uint32).copy())
    qkv = to_words(rng.standard_normal((N, Wt, S, 3 * E)).astype(np.float32))
    cache = nan_buf((B, Tcap, S, 2 * E), prec)
    cache[:, :P] = to_words(rng.standard_normal((B, P, S, 2 * E)).astype(np.float32))
    c0 = cache.copy()
    y = nan_buf((N, Wt, S, E), prec)
    check(fan_tail(prec, qkv, scene_of_item, H, P, P, cache, y))
    # (4)
    assert np.array_equal(cache, c0), "the launch changed the cache"
    got = values(y, prec)
    assert np.isfinite(got).all(), "a y row is not finite: a row was left out, or a slot >= P of the cache was read"
    # (1)
    ref = ref_tails(values(c0[scene_of_item, :P], prec), values(qkv, prec), H)
    d = float(np.abs(got - ref).max())
    bar = 1.6e-2 * EPS16[prec] if prec else 2e-5
    print(f"DIST fan_tail[{prec}] S {S} H {H} P {P} Wt {Wt}: {d:.3e} bar {bar:.3e}")
    assert d <= bar, f"{d:.3e} from float64 (bar {bar:.3e})"
    # (2) the stand-alone range launch: every item a "scene" with its own copy of the cache
    rep = np.ascontiguousarray(c0[scene_of_item])
    r0 = rep.copy()
    y_ref = nan_buf((N, Wt, S, E), prec)
    check(lib().umgen_dbg_attn_temporal_range(prec, vp(qkv), N, Wt, S, H, P, 0, 0, Tcap, vp(rep), vp(y_ref)))
    assert np.array_equal(rep, r0)
    assert y.tobytes() == y_ref.tobytes(), "the bytes differ from launch_attn_temporal's on per-item copies of the cache"
    # (3) a tail of one is the fan kernel's launch
    if Wt == 1:
        y_fan = nan_buf((N, S, E), prec)
        sc = np.ascontiguousarray(scene_of_item, dtype=np.int32)
        check(lib().umgen_dbg_attn_temporal_fan(prec, vp(np.ascontiguousarray(qkv[:, 0])), N, sc.ctypes.data_as(C.POINTER(C.c_int32)), B, S, H, P, Tcap,
                                                vp(cache), vp(y_fan)))
        assert y_fan.tobytes() == y.tobytes(), "Wt == 1 differs from attn_temporal_fan_kernel"
    # (5) only the last tail slot has a query: the q rows below it are NaN and never read, their y rows never written
    q_nan = qkv.copy()
    q_nan[:, :Wt - 1, :, :E] = NAN16[prec] if prec else NAN32
    y_last = nan_buf((N, Wt, S, E), prec)
    check(fan_tail(prec, q_nan, scene_of_item, H, P, P + Wt - 1, cache, y_last))
    assert y_last[:, Wt - 1].tobytes() == y[:, Wt - 1].tobytes(), "the last tail slot with q0 = P + Wt - 1 differs from its bytes with q0 = P"
    assert np.array_equal(y_last[:, :Wt - 1], nan_buf((N, Wt - 1, S, E), prec)), "a y row below q0 was written"
    # (6) the 11-item scene alone (its cache block at the same scene index; the other scenes have no items)
    big = scene_of_item == 3
    y_big = nan_buf((int(big.sum()), Wt, S, E), prec)
    check(fan_tail(prec, np.ascontiguousarray(qkv[big]), scene_of_item[big], H, P, P, cache, y_big))
    assert y_big.tobytes() == y[big].tobytes(), "the 11-item scene alone differs from the launch of 15"
    assert np.array_equal(cache, c0)


@pytest.mark.parametrize("H,P,Wt", [(4, 3, 17), (1, 3, 17), (2, 2, 40), (1, 200, 2)])      # tails past 16 rows; cached rows past the LDS request
@pytest.mark.parametrize("prec", [0, 1])
def test_a_tail_the_kernel_does_not_hold_is_refused_without_a_launch(prec, H, P, Wt):
    B, S, E, Tcap = 2, 3, H * 48, P + 1
    scene_of_item = np.array([0, 0, 1], np.int32)
    rng = np.random.default_rng(5)
    to_words = (lambda a: bits16(a, prec)) if prec else (lambda a: a.view(np.uint32).copy())
    qkv = to_words(rng.standard_normal((3, Wt, S, 3 * E)).astype(np.float32))
    cache = to_words(rng.standard_normal((B, Tcap, S, 2 * E)).astype(np.float32))
    c0 = cache.copy()
    y = nan_buf((3, Wt, S, E), prec)
    assert fan_tail(prec, qkv, scene_of_item, H, P, P, cache, y) == UNSUPPORTED
    assert np.array_equal(y, nan_buf(y.shape, prec)) and np.array_equal(cache, c0)
