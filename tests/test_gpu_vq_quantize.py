"""-m gpu: vq_quantize_kernel alone (csrc/vq_common.h), one launch at a time on crafted rows, through umgen_dbg_vq_quantize: the code-norm
kernel, then the quantiser launched by the one launcher (tile and LDS formula included) that umgen_vqenc_encode uses.

embed_dim D in {4, 16, 32, 64} gives codebook tiles t of 512, 512, 256 and 128 rows (asked from the library, umgen_dbg_vq_quant_tile).
Codebook sizes sit on the seams: 1, 63, 65, t, t + 1, 2 t + 44 rows (no full lane stride, a partial last tile, one row in the last tile).

Random rows are compared with the float64 arg-min wherever the float64 margin exceeds (8 D + 24) 2^-24: each of |z|^2, |e|^2 and z.e is
a D-term fma chain on unit vectors (error at most D 2^-24 each, z.e counted twice in the distance), combining three terms of magnitude at
most 4 adds three roundings, and two distances are compared.  The rows the kernel returns are its own normalisation, within 1e-6 of float64.
"""
import ctypes as C

import numpy as np
import pytest

from tests import vq_ref
from tests.gpu_util import NAN32, check, fp, lib

pytestmark = pytest.mark.gpu
DIMS = (4, 16, 32, 64)
TILES = {4: 512, 16: 512, 32: 256, 64: 128}
CODE_SENTINEL = -0x0123456789ABCDEF


def tile(D):
    t = lib().umgen_dbg_vq_quant_tile(D)
    assert t == TILES[D]
    return t


def bound(D):
    return (8 * D + 24) * 2.0 ** -24


def codebook(rng, N, D):
    """unit rows, like NormEMAVectorQuantizer's"""
    w = rng.standard_normal((N, D))
    return (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(np.float32)


def quantize(h, emb, n_pos=None):
    """h [P, ldh] float32 (ldh >= D: the columns behind D are the row stride's gap), emb [N, D] -> (codes [n_pos], zn [n_pos, D]).  The 4
    entries behind n_pos of either output, where the dead waves of the last workgroup would write, are preset and must come back untouched."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    N, D = emb.shape
    n_pos = h.shape[0] if n_pos is None else n_pos
    codes = np.full(n_pos + 4, CODE_SENTINEL, np.int64)
    zn = np.full((n_pos + 4, D), NAN32, np.uint32).view(np.float32)
    check(lib().umgen_dbg_vq_quantize(fp(h), h.shape[1], fp(emb), N, D, n_pos, codes.ctypes.data_as(C.POINTER(C.c_int64)), fp(zn)))
    assert (codes[n_pos:] == CODE_SENTINEL).all(), "a dead wave wrote a code"
    assert (zn[n_pos:].view(np.uint32) == NAN32).all(), "a dead wave wrote a row"
    assert (codes[:n_pos] >= 0).all() and (codes[:n_pos] < N).all() and np.isfinite(zn[:n_pos]).all()
    return codes[:n_pos].copy(), zn[:n_pos].copy()


def unit64(h):
    h = np.asarray(h, dtype=np.float64)
    return h / np.maximum(np.linalg.norm(h, axis=-1, keepdims=True), 1e-12)


def sizes(D):
    t = tile(D)
    return (1, 63, 65, t, t + 1, 2 * t + 44)


@pytest.mark.parametrize("D", DIMS)
def test_hits(D):
    """A positive multiple of codebook row k must come back as code k with zn = row k, for k at every seam of the lane stride and the tile."""
    t = tile(D)
    rng = np.random.default_rng(100 + D)
    for N in sizes(D):
        emb = codebook(rng, N, D)
        ks = sorted({k for k in (0, 63, 64, t - 1, t, N - 1) if 0 <= k < N})
        h = np.stack([np.float32(0.25 + 3.0 * i) * emb[k] for i, k in enumerate(ks)])
        _, _, margin = vq_ref.argmin_codes(unit64(h), emb)
        assert N == 1 or (margin > bound(D)).all()                     # (a condition on the random codebook: no second row that close)
        codes, zn = quantize(h, emb)
        np.testing.assert_array_equal(codes, ks, err_msg=f"D {D}, N {N}")
        np.testing.assert_allclose(zn, emb[ks], atol=1e-6, rtol=0)


def tie_codebooks(rng, N, D, t):
    """codebooks in which row a is copied bit for bit to row b: same lane (b = a + 64), neighbours, adjacent tiles (b = a + t), and the last
    row of the partial tile"""
    for pairs in ([(0, 64), (5, 69), (63, 127), (t - 60, t + 4)],              # same lane; the last one across the tile seam as well
                  [(10, 11), (63, 64), (t - 1, t), (N - 2, N - 1)],            # neighbours: across the lane stride and across the tile seam
                  [(0, t), (70, 70 + t), (t - 1, 2 * t - 1), (43, 2 * t + 43)],  # adjacent tiles, and first tile against the partial one
                  [(3, N - 1)], [(t + 1, N - 1)], [(2 * t, N - 1)]):           # against the last row of the partial tile
        emb = codebook(rng, N, D)
        for a, b in pairs:
            emb[b] = emb[a]
        yield pairs, emb


@pytest.mark.parametrize("D", DIMS)
def test_exact_ties_go_to_the_lower_index(D):
    """Rows that are multiples of a duplicated codebook row see two bit-equal smallest distances: the lower index must win, like
    torch.argmin's first minimum, whichever lanes and tiles hold the two rows, also with the codebook stored in reverse order."""
    t = tile(D)
    N = 2 * t + 44
    rng = np.random.default_rng(200 + D)
    for pairs, emb in tie_codebooks(rng, N, D, t):
        for cb in (emb, np.ascontiguousarray(emb[::-1])):
            rows = [a for a, _ in pairs] if cb is emb else [N - 1 - b for _, b in pairs]
            h = np.stack([np.float32(1.5 + i) * cb[r] for i, r in enumerate(rows)])
            first = [int(np.flatnonzero((cb == cb[r]).all(1))[0]) for r in rows]
            twins = [int(np.flatnonzero((cb == cb[r]).all(1))[-1]) for r in rows]
            assert first == rows and all(tw > r for tw, r in zip(twins, rows))       # each row has its copy at a higher index
            best, _, _ = vq_ref.argmin_codes(unit64(h), cb)
            assert (cb[best] == cb[rows]).all()             # float64 agrees that the pair is the nearest one (its two distances need not be bit-equal there)
            codes, _ = quantize(h, cb)
            np.testing.assert_array_equal(codes, rows, err_msg=f"D {D}, pairs {pairs}, reversed {cb is not emb}")


def random_case(D, n_pos, seed):
    t = tile(D)
    rng = np.random.default_rng(seed)
    emb = codebook(rng, 2 * t + 44, D)
    h = (rng.standard_normal((n_pos, D)) * rng.uniform(0.1, 10.0, (n_pos, 1))).astype(np.float32)
    best, _, margin = vq_ref.argmin_codes(unit64(h), emb)
    return emb, h, best, margin > bound(D)


@pytest.mark.parametrize("D", DIMS)
def test_random_rows_against_float64(D):
    emb, h, best, clear = random_case(D, 403, 300 + D)             # 101 workgroups, the last one with a single live wave
    print(f"D {D}: {int((~clear).sum())} of {clear.size} positions under the margin bound {bound(D):.2e}")
    assert (~clear).mean() < 0.005
    codes, zn = quantize(h, emb)
    np.testing.assert_array_equal(codes[clear], best[clear])
    np.testing.assert_allclose(zn, unit64(h), atol=1e-6, rtol=0)
    np.testing.assert_allclose(np.linalg.norm(zn.astype(np.float64), axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("n_pos", (1, 2, 3, 5))
@pytest.mark.parametrize("D", DIMS)
def test_dead_waves(D, n_pos):
    """A workgroup holds 4 positions: with n_pos in {1, 2, 3, 5} the last one has 3, 2, 1 and 3 waves without a position, which stay for the
    barriers and must write nothing (quantize() checks the entries behind n_pos); every live position must be right."""
    emb, h, best, clear = random_case(D, 8, 400 + D)
    assert clear.all()
    codes, zn = quantize(h[:n_pos], emb)
    np.testing.assert_array_equal(codes, best[:n_pos])
    np.testing.assert_allclose(zn, unit64(h[:n_pos]), atol=1e-6, rtol=0)


@pytest.mark.parametrize("D", DIMS)
def test_row_stride_gap_is_never_read(D):
    """Rows ldh > D floats apart, as behind a quant_conv whose padded width exceeds embed_dim: NaN bits in the gap change nothing, bit for bit."""
    emb, h, _, _ = random_case(D, 37, 500 + D)
    wide = np.full((37, D + 4), NAN32, np.uint32).view(np.float32)
    wide[:, :D] = h
    c0, z0 = quantize(h, emb)
    c1, z1 = quantize(wide, emb)
    np.testing.assert_array_equal(c1, c0)
    assert z1.tobytes() == z0.tobytes()


@pytest.mark.parametrize("D", DIMS)
def test_zero_row(D):
    """|row| = 0 takes the max(|row|, 1e-12) branch: zn is all zeros, every distance is |e_n|^2, and the code is its first minimum.  The
    codebook's norms differ by 1e-3 and more (squares by 2e-3, far above the bound); the smallest norm appears twice, bit for bit."""
    t = tile(D)
    N = 2 * t + 44
    rng = np.random.default_rng(600 + D)
    scale = (1.0 + 1e-3 * (1 + rng.permutation(N))).astype(np.float32)
    lo, hi = t + 7, 2 * t + 40                                       # the smallest norm: a row of the second tile and its negative in the partial one
    scale[lo] = scale[hi] = np.float32(1.0)
    emb = codebook(rng, N, D) * scale[:, None]
    emb[hi] = -emb[lo]
    e2 = (emb.astype(np.float64) ** 2).sum(1)
    assert int(np.argmin(e2)) == lo and e2[hi] == e2[lo] and np.sort(e2)[2] - e2[lo] > 1e-3
    h = np.zeros((3, D), np.float32)
    h[1] = rng.standard_normal(D)                                    # a live neighbour in the same workgroup
    h[2, 0] = -0.0
    best, _, margin = vq_ref.argmin_codes(unit64(h[1]), emb)
    assert margin > 1e-3
    codes, zn = quantize(h, emb)
    assert codes[0] == lo and codes[2] == lo and codes[1] == best
    assert not zn[0].any() and not zn[2].any()


@pytest.mark.parametrize("D", DIMS)
def test_scales(D):
    """Unit rows scaled by 1e15 and by 1e-10 give the code and the normalised row of the unscaled row wherever the float64 margin is clear.
    A row scaled by 1e-15 has |row| under the 1e-12 floor of z = row / max(|row|, 1e-12), so by that definition its z is 1e-3 x the unit row
    (1e-6 x the distances' spread): its code is still the unscaled row's wherever the float64 margin of THAT z is clear, and zn is that z."""
    emb, h, best, clear = random_case(D, 64, 700 + D)
    h = unit64(h).astype(np.float32)
    assert clear.mean() > 0.9
    c0, z0 = quantize(h, emb)
    np.testing.assert_array_equal(c0[clear], best[clear])
    for s, floor in ((1e15, 1.0), (1e-10, 1.0), (1e-15, 1e-3)):
        hs = h * np.float32(s)
        z64 = hs.astype(np.float64) / np.maximum(np.linalg.norm(hs.astype(np.float64), axis=1, keepdims=True), 1e-12)
        np.testing.assert_allclose(np.linalg.norm(z64, axis=1), floor, rtol=1e-6)
        b, _, margin = vq_ref.argmin_codes(z64, emb)
        ok = clear & (margin > bound(D))
        assert ok.mean() > 0.5
        np.testing.assert_array_equal(b[ok], best[ok])
        c, z = quantize(hs, emb)
        np.testing.assert_array_equal(c[ok], c0[ok], err_msg=f"scale {s}")
        np.testing.assert_allclose(z, z64, atol=1e-6 * floor, rtol=0)
        np.testing.assert_allclose(z, z0 * np.float32(floor), atol=1e-6 * floor, rtol=0)
