"""-m gpu: the two kernels behind a fan frame whose window grows next (umgen_rollout_fan), through their hooks.

attn_temporal_fan_write_kernel (umgen_dbg_attn_temporal_fan_write): the fan launch that also leaves item i's k | v rows of slot P in block i of the
cache.  Four scenes with 3, 0, 1 and 9 items (9 > 8, the items one LDS group holds at four heads per workgroup: a second round), P = 1 and 3 under
Tcap = 4, the three precisions, and H = 4 / 2 / 1 for the three heads-per-workgroup variants the launcher selects.  The cache has 13 blocks (one per
item), NaN words everywhere but the scenes' slots < P.  Checks, all on bytes: y equals the read-only hook's on the same inputs; block i, slot P holds
item i's k | v rows; every other byte of the cache is what went in.

tcache_spread_kernel (umgen_dbg_tcache_spread): B = 2, N = 3 (scene 1's source block is scene 0's destination: the descending order matters) and
B = 1, N = 6, P = 1 and 3: every destination's slots < P equal the ORIGINAL source, slots >= P and the blocks behind B * N are untouched; N = 1
changes nothing; one case with more 16-byte vectors than the grid has threads (the grid-stride loop)."""
import ctypes as C

import numpy as np
import pytest

from tests.gpu_util import NAN16, NAN32, bits16, check, lib, vp

COUNTS = [3, 0, 1, 9]

pytestmark = pytest.mark.gpu


def nan_buf(shape, prec):
    return np.full(shape, NAN16[prec], dtype=np.uint16) if prec else np.full(shape, NAN32, dtype=np.uint32)


@pytest.mark.parametrize("H", [4, 2, 1])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_writing_fan_launch_appends_every_items_rows_and_keeps_y(prec, P, H):
    B, E, Tcap, S = len(COUNTS), H * 48, 4, 7
    scene_of_item = np.repeat(np.arange(B), COUNTS).astype(np.int32)
    N = scene_of_item.size
    rng = np.random.default_rng(100 * prec + 10 * P + H)
    to_words = (lambda a: bits16(a, prec)) if prec else (lambda a: a.view(np.uint32).copy())
    qkv = to_words(rng.standard_normal((N, S, 3 * E)).astype(np.float32))
    cache = nan_buf((N, Tcap, S, 2 * E), prec)                # 13 blocks: the scenes' are blocks 0 .. 3
    cache[:B, :P] = to_words(rng.standard_normal((B, P, S, 2 * E)).astype(np.float32))
    c0 = cache.copy()
    sc = scene_of_item.ctypes.data_as(C.POINTER(C.c_int32))
    y_ref = nan_buf((N, S, E), prec)
    ro = np.ascontiguousarray(c0[:B])
    check(lib().umgen_dbg_attn_temporal_fan(prec, vp(qkv), N, sc, B, S, H, P, Tcap, vp(ro), vp(y_ref)))
    assert np.array_equal(ro, c0[:B])
    y = nan_buf((N, S, E), prec)
    check(lib().umgen_dbg_attn_temporal_fan_write(prec, vp(qkv), N, sc, B, S, H, P, Tcap, N, vp(cache), vp(y)))
    assert y.tobytes() == y_ref.tobytes(), "y differs from the read-only launch's"
    want = c0.copy()
    want[:, P] = qkv[:, :, E:]
    assert np.array_equal(cache[:, P], want[:, P]), "block i, slot P does not hold item i's k | v rows"
    assert cache.tobytes() == want.tobytes(), "a byte outside the items' slot P changed"


def test_writing_fan_hook_refuses_a_cache_without_room():
    prec, H, S, P = 1, 4, 7, 3
    qkv = np.zeros((2, S, 3 * 48 * H), np.uint16)
    sc = np.zeros(2, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    y = np.zeros((2, S, 48 * H), np.uint16)
    for Tcap, blocks in ((3, 2), (4, 1)):                    # no slot P in a block | fewer blocks than items
        cache = np.zeros((2, 4, S, 2 * 48 * H), np.uint16)
        assert lib().umgen_dbg_attn_temporal_fan_write(prec, vp(qkv), 2, sc, 1, S, H, P, Tcap, blocks, vp(cache), vp(y)) == -1


def spread(cache, B, N, P):
    blocks, Tcap, words = cache.shape
    check(lib().umgen_dbg_tcache_spread(vp(cache), blocks, B, N, P, Tcap, words * cache.itemsize))


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("B,N", [(2, 3), (1, 6), (3, 1)])
def test_spread_hands_every_item_its_scenes_slots(B, N, P):
    rng = np.random.default_rng(7 * B + N + P)
    c0 = rng.integers(0, 1 << 16, (B * N + 1, 4, 7 * 2 * 48), dtype=np.uint16)      # one block behind the items': nobody's
    cache = c0.copy()
    spread(cache, B, N, P)
    want = c0.copy()
    for b in range(B):
        want[b * N:(b + 1) * N, :P] = c0[b, :P]
    assert np.array_equal(cache[:, :P], want[:, :P]), "a destination's slots < P are not the original source's"
    assert cache.tobytes() == want.tobytes(), "slots >= P or a block behind the items' changed"
    if N == 1:
        assert cache.tobytes() == c0.tobytes()


def test_spread_of_more_vectors_than_threads():
    B, N, P, Tcap = 2, 2, 3, 3
    words = (3 << 20) // 4 + 4                               # 3 slots of 3 MiB + 16 B: 589827 vectors against 2048 * 256 threads
    rng = np.random.default_rng(5)
    c0 = rng.integers(0, 1 << 32, (B * N, Tcap, words), dtype=np.uint32)
    cache = c0.copy()
    spread(cache, B, N, P)
    want = np.repeat(c0[:B], N, axis=0)
    assert cache.tobytes() == want.tobytes()
