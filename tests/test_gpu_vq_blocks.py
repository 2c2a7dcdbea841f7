"""-m gpu: the small kernels of the VQ decoder / encoder (csrc/vq_common.h), one launch each through the launcher the handles use
(umgen_dbg_vq_* in csrc/debug_vq.hip).

The movers (im2col, the stride-2 im2col of Downsample, nearest 2x upsampling, the NCHW ingest and output) must equal numpy bit for bit on
distinct integers, with pad taps and pad lanes exactly 0; every output starts as NaN bits, must come back fully written, and the elements
behind its end (and the guard band behind those, checked by the hook) must be untouched.  GroupNorm is held to float64 at 10 x the
float32 restatement's own distance on the same input; the row softmax to (4 + n) 2^-24 of the row maximum (one expf and one division per
element, n roundings of the row sum), on scores for which scaling and subtracting the maximum are exact.  The exact-fp32 GEMM is run in the
form the attention block launches it for its scores when the number of positions is no multiple of 4.

Measured on an MI355X, max |gpu - float64| over the shapes (range of the bars beside it):
  GroupNorm, centred values            1.8e-7 .. 1.1e-6   (bars 1.7e-6 .. 9.1e-6; at most 0.17 of the bar)
  GroupNorm, values 1e3 + 1e-2 N(0,1)  2.9e-3 .. 1.5e-2   (bars 9.5e-2 .. 4.1e-1; the fp32 mean that the apply kernel subtracts, 3e-5 on values 1e-2 wide)
  softmax, n = 1 .. 257                0 .. 1.7e-7 of the row maximum, row sums within 1.8e-7 of 1   (bars 3.0e-7 .. 1.6e-5)
  score GEMM, n = 1 .. 99              at most 3.6e-7 (bar 2e-5, the project's fp32 bar)
"""
import numpy as np
import pytest
import torch

from tests.gpu_util import NAN32, check, fp, lib
from tests.test_gpu_stack_forms import RESID, STORE, check_window, gemm, window

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 2), (3, 5), (9, 11)]
TAIL = 64             # NaN elements behind the end of every output that must come back untouched


def nan_out(n):
    return np.full(n + TAIL, NAN32, np.uint32).view(np.float32)


def written(out, n):
    """the first n elements, after checking that all of them were written and none behind them was"""
    bits = out.view(np.uint32)
    assert (bits[n:] == NAN32).all(), "an element past the end of the output was written"
    assert not np.isnan(out[:n]).any(), "an output element was left unwritten"
    return out[:n]


def integers(*shape):
    """distinct positive integers (exact in float32)"""
    return (1.0 + np.arange(int(np.prod(shape)))).astype(np.float32).reshape(shape)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("H,W", SHAPES)
def test_im2col(H, W):
    for C in (4, 8, 96):
        for KS, pad in ((1, 0), (3, 1)):
            x = integers(H, W, C)
            n = H * W * KS * KS * C
            col = nan_out(n)
            check(lib().umgen_dbg_vq_im2col(fp(x), H, W, C, KS, pad, fp(col), col.size))
            xp = np.zeros((H + 2 * pad, W + 2 * pad, C), np.float32)
            xp[pad:pad + H, pad:pad + W] = x
            ref = np.stack([xp[ky:ky + H, kx:kx + W] for ky in range(KS) for kx in range(KS)], axis=2)       # [H][W][tap][C]
            assert same_bits(written(col, n).reshape(H, W, KS * KS, C), ref), (C, KS)
            if KS == 3:
                assert (ref == 0).sum() == (9 * H * W - (3 * H - 2) * (3 * W - 2)) * C        # the pad taps, exactly 0


@pytest.mark.parametrize("H,W", SHAPES)
def test_im2col_stride2(H, W):
    """Downsample on a 2H x 2W grid: pad 1 on the right and bottom, 3 x 3 taps at stride 2 -> H x W positions"""
    for C in (4, 8, 96):
        x = integers(2 * H, 2 * W, C)
        n = H * W * 9 * C
        col = nan_out(n)
        check(lib().umgen_dbg_vq_im2col_s2(fp(x), 2 * H, 2 * W, C, fp(col), col.size))
        xp = np.zeros((2 * H + 1, 2 * W + 1, C), np.float32)
        xp[:2 * H, :2 * W] = x
        ref = np.stack([xp[ky:ky + 2 * H:2, kx:kx + 2 * W:2] for ky in range(3) for kx in range(3)], axis=2)
        assert same_bits(written(col, n).reshape(H, W, 9, C), ref), C
        assert (ref[H - 1, :, 6:] == 0).all() and (ref[:, W - 1, 2::3] == 0).all()             # the pad row and the pad column


@pytest.mark.parametrize("H,W", SHAPES)
def test_upsample(H, W):
    for C in (4, 8, 96):
        x = integers(H, W, C)
        n = 4 * H * W * C
        y = nan_out(n)
        check(lib().umgen_dbg_vq_upsample(fp(x), H, W, C, fp(y), y.size))
        assert same_bits(written(y, n).reshape(2 * H, 2 * W, C), np.ascontiguousarray(x.repeat(2, axis=0).repeat(2, axis=1))), C


@pytest.mark.parametrize("H,W", SHAPES)
def test_nchw_in_and_out(H, W):
    n_px = H * W
    for c_in in (1, 2, 3, 5, 7):
        C = (c_in + 3) & ~3
        x = integers(c_in, n_px)
        y = nan_out(n_px * C)
        check(lib().umgen_dbg_vq_from_nchw(fp(x), n_px, c_in, C, fp(y), y.size))
        ref = np.zeros((n_px, C), np.float32)
        ref[:, :c_in] = x.T
        got = written(y, n_px * C).reshape(n_px, C)
        assert same_bits(got, ref), c_in                                                      # (the pad lanes: +0.0 bits)
        # and back: rows C floats apart, of which the first c_in are channels; NaN in the gap must not be read
        rows = got.copy()
        rows[:, c_in:] = np.float32(np.nan)
        out = nan_out(n_px * c_in)
        check(lib().umgen_dbg_vq_to_nchw(fp(rows), n_px, c_in, C, fp(out), out.size))
        assert same_bits(written(out, n_px * c_in).reshape(c_in, n_px), x), c_in


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------------
def gn_ref(x, gamma, beta, swish, dtype):
    xt = torch.from_numpy(x).to(dtype).T[None]                                                 # [1][C][n_px]
    y = torch.nn.functional.group_norm(xt, 32, torch.from_numpy(gamma).to(dtype), torch.from_numpy(beta).to(dtype), eps=1e-6)
    if swish:
        y = y * torch.sigmoid(y)
    return y[0].T.numpy().astype(np.float64)


def gn_gpu(x, gamma, beta, swish):
    n_px, C = x.shape
    y = nan_out(n_px * C)
    check(lib().umgen_dbg_vq_group_norm(fp(x), n_px, C, fp(gamma), fp(beta), int(swish), fp(y), y.size))
    return written(y, n_px * C).reshape(n_px, C)


# (C = 32 at n_px = 1 is one value per group: held to the exact answer below, not to a bar)
GN_CASES = [(C, n) for n in (1, 15, 99) for C in (32, 96, 192) if (C, n) != (32, 1)] + [(96, 4096)]


@pytest.mark.parametrize("offset", (False, True), ids=("centred", "offset1e3"))
@pytest.mark.parametrize("swish", (False, True), ids=("plain", "swish"))
@pytest.mark.parametrize("C,n_px", GN_CASES)
def test_group_norm(C, n_px, swish, offset):
    """against float64 at 10 x the float32 restatement's own distance.  `offset`: values 1e3 + 1e-2 N(0, 1), where statistics accumulated in fp32
    lose the variance."""
    rng = np.random.default_rng(C + n_px)
    x = ((1e3 + 1e-2 * rng.standard_normal((n_px, C))) if offset else rng.standard_normal((n_px, C)) * rng.uniform(0.2, 3.0, (1, C))).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.uniform(-1, 1, C)).astype(np.float32)
    beta = (0.1 * rng.uniform(-1, 1, C)).astype(np.float32)
    ref = gn_ref(x, gamma, beta, swish, torch.float64)
    err32 = float(np.abs(gn_ref(x, gamma, beta, swish, torch.float32) - ref).max())
    err = float(np.abs(gn_gpu(x, gamma, beta, swish).astype(np.float64) - ref).max())
    print(f"GN C {C} n_px {n_px} swish {swish} offset {offset}: max |gpu - float64| = {err:.3e}, bar = {10 * err32:.3e} (float32 restatement {err32:.3e})")
    assert err32 > 0.0
    assert err <= 10.0 * err32


@pytest.mark.parametrize("swish", (False, True), ids=("plain", "swish"))
def test_group_norm_of_one_value_per_group(swish):
    """n_px = 1, C = 32: the variance is exactly 0, rstd = 1e3, x - mean = 0: the output is exactly beta; with swish beta * sigmoid(beta) within the 4
    roundings of expf, the addition and the division"""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((1, 32)) * 100.0).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.uniform(-1, 1, 32)).astype(np.float32)
    beta = (0.1 * rng.uniform(-1, 1, 32)).astype(np.float32)
    y = gn_gpu(x, gamma, beta, swish)
    if not swish:
        assert same_bits(y, beta[None].copy())
    else:
        b = beta.astype(np.float64)
        ref = b / (1.0 + np.exp(-b))
        assert (np.abs(y[0] - ref) <= 4 * 2.0 ** -24 * np.abs(ref)).all()


# ---- softmax ------------------------------------------------------------------------------------------------------------------------------
SM_C = 64            # scale 64^-0.5 = 1 / 8, exact: with scores on the 1 / 8 grid the scaling and the subtraction of the maximum are exact too


def softmax_rows(n):
    """n rows of n scores on the 1 / 8 grid: all-equal rows, one dominant entry at column 0 / 63 / 64 / n - 1, +-300, random"""
    rng = np.random.default_rng(n)
    s = np.round(rng.uniform(-8, 8, (n, n)) * 8) / 8
    for i in range(n):
        k = i % 8
        if k == 0:
            s[i] = 1.25
        elif k in (1, 2, 3, 4):
            col = (0, 63, 64, n - 1)[k - 1]
            if col < n:
                s[i, col] = 40.0
        elif k == 5:
            s[i] = np.where(rng.random(n) < 0.5, 300.0, -300.0)
            s[i, i] = 300.0
        elif k == 6:
            s[i] = -300.0
    return s.astype(np.float32)


@pytest.mark.parametrize("n", (1, 3, 15, 63, 64, 65, 99, 257))
def test_softmax(n):
    ld = (n + 3) & ~3                                              # rows as attn_block lays them out; the gap keeps its NaN bits
    s = softmax_rows(n)
    buf = nan_out(n * ld)
    buf[:n * ld].reshape(n, ld)[:, :n] = s
    check(lib().umgen_dbg_vq_softmax(fp(buf), n, ld, SM_C, buf.size))
    bits = buf.view(np.uint32)
    assert (bits[n * ld:] == NAN32).all() and (bits[:n * ld].reshape(n, ld)[:, n:] == NAN32).all()
    got = buf[:n * ld].reshape(n, ld)[:, :n].astype(np.float64)
    assert np.isfinite(got).all()
    a = s.astype(np.float64) / 8.0
    e = np.exp(a - a.max(1, keepdims=True))
    ref = e / e.sum(1, keepdims=True)
    bar = (4 + n) * 2.0 ** -24
    rel = float((np.abs(got - ref) / ref.max(1, keepdims=True)).max())
    dsum = float(np.abs(got.sum(1) - 1.0).max())
    print(f"SM n {n}: max |gpu - float64| / row max = {rel:.3e}, max |row sum - 1| = {dsum:.3e}, bar = {bar:.3e}")
    assert rel <= bar
    assert dsum <= bar


# ---- the exact-fp32 GEMM as the attention block launches it for its scores ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", (STORE, RESID), ids=("store", "resid"))
@pytest.mark.parametrize("n", (1, 2, 3, 15, 35, 99))
def test_score_gemm_with_a_row_count_that_is_no_multiple_of_4(n, mode):
    """scores[j][i] = q_j . k_i: Mi = Nj = n, rows ld = n rounded up to 4 floats apart.  The last 1 - 3 scores of a row must not run into the next
    row or past the last one: the gap columns and everything behind the window keep their bits (NaN for the store, the residual's values for the
    residual form, which also takes a bias), and the window is the fp32 chain's distance from float64."""
    K = 32
    ld = (n + 3) & ~3
    rng = np.random.default_rng(n)
    k = rng.standard_normal((n, K)).astype(np.float32)
    q = rng.standard_normal((n, K)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32) if mode == RESID else None
    before = (rng.standard_normal(n * ld + TAIL).astype(np.float32).view(np.uint32) if mode == RESID else np.full(n * ld + TAIL, NAN32, np.uint32))
    out = before.copy()
    gemm(0, 0, 0, k, q, bias, n, n, K, out, mode=mode, ldo=ld)
    idx = window(0, 1, 0, n, ld, n)
    ref = q.astype(np.float64) @ k.astype(np.float64).T
    if mode == RESID:
        ref = ref + bias.astype(np.float64)[None] + before.view(np.float32)[idx[0]].astype(np.float64)
    check_window(f"scores n {n} mode {mode}", out, before, idx, ref[None], 0, 2e-5)
