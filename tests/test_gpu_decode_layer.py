"""The five-launch decode layer of umgen_amd/csrc/gemv.hip -- gemv_ln_kernel, attn_partial_kernel, gemv_resid_kernel -- one launch form at
a time, through the hooks umgen_dbg_gemv_modes / _gemv_resid / _attn_partial / _decode_layer.  The hooks launch what the product launches:
launch_decode_layer (oar_layers), launch_ego_self_attn and launch_ego_cross_attn (run_ego).  Every test needs a GPU except the check of the
fp64 restatement against the oracle's BlockOAR.

References are fp64 restatements on the kernel's own operands: weights as stored (16-bit in bf16 / fp16), K/V history as stored, the new
K/V row as the kernel stored it (checked to be within 1 ulp of its fp64 value), fp32 queries and activations, LayerNorm with weight only and
eps 1e-5, exact erf GELU, float32(1 / sqrt(48)) as the score scale.  Values must satisfy |got - ref| <= bar * max(1, |ref|).  The three
rows-per-workgroup forms (0: row loop, 1, 2) sum every row in the same order, so they must agree bit for bit.

Buffers the kernels must not write come back whole: output columns past N, cache rows other than pos (history bits, NaN), guard bands
behind every output (the hooks return an error when a band changed).  Rows past the key count are finite garbage the attention loads (its
loads are clamped to kAttnSplit * kAttnChunk rows) but must mask; unused split slots of the partials hold stale finite values that the merge
must weigh 0.

Largest relative errors measured on an MI355X over all cases (fp32 | bf16 | fp16), and the bars:
  gemv_ln, F32 / GELU / QKV modes       3.7e-5 | 3.3e-5 | 3.1e-5    GEMV_BAR  1e-4  (LayerNorm of rows with |mean| / sd = 80: fp32 mean)
  gemv_resid, plain form (K = 4E)       6.4e-7 | 5.7e-7 | 5.9e-7    RESID_BAR 2e-6
  attention + merge + c_proj: decode    8.4e-7 | 7.1e-7 | 7.3e-7    ATTN_BAR  2.5e-6
                              ego self  4.7e-7 | 4.6e-7 | 4.7e-7
                              ego cross 7.4e-7 | 5.3e-7 | 5.7e-7
  whole BlockOAR layer                  6.9e-7 | 7.9e-7 | 8.5e-7    LAYER_BAR 2.5e-6
"""
import functools
import types

import numpy as np
import pytest
import torch

from tests.gpu_util import NAN16, NAN32, SCALE_QK, bits16, check, fp, from_bits16, gelu64, lib, ln_input, ref_ln, round16, ulp16, vp

GEMV_F32, GEMV_GELU, GEMV_QKV = 0, 1, 2
GEO_DECODE, GEO_EGO_SELF, GEO_EGO_CROSS = 0, 1, 2
PRECS = [0, 1, 2]
WIDTHS = [96, 768, 1536]
M_SET = [1, 2, 3, 5, 7, 8, 9, 17, 23]               # every rows-per-workgroup form, the odd tail of the two-row form, chunks of 8
POS_SET = [0, 1, 126, 127, 128, 129, 1000, 2206, 2303]   # split boundaries, the last position of a frame, the last cache row
EGO_B = [1, 2, 3, 6]                                  # ego queries M = 3B: 3, 6, 9 (8 + 1), 18 (8 + 8 + 2)
LMAX = 2304                                           # kAttnSplit * kAttnChunk: cache rows per (scene, K / V, head)
KSEQ = 2207
CHUNK = 128
GEMV_BAR = 1e-4
RESID_BAR = 2e-6
ATTN_BAR = 2.5e-6
LAYER_BAR = 2.5e-6
CACHE_BYTES = 200 << 20                               # largest decode cache a case builds


# ---------------------------------------------------------------------------------------------------------------------------
# operands and fp64 restatements
# ---------------------------------------------------------------------------------------------------------------------------
def store(a, prec):
    """(what the hook receives, the values as stored in fp64): fp32 as it is, else the 16-bit bits"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if prec == 0:
        return a, a.astype(np.float64)
    return bits16(a, prec), round16(a, prec).astype(np.float64)


def stored(b, prec):
    return b.astype(np.float64) if prec == 0 else from_bits16(np.ascontiguousarray(b), prec).astype(np.float64)


def nan_array(shape, prec):
    return np.full(shape, NAN32, np.uint32).view(np.float32) if prec == 0 else np.full(shape, NAN16[prec], np.uint16)


def raw(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def rel_err(got, ref):
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def check_kv_row(got, ref, prec, bar):
    """the stored K/V row: the fp32 result rounded to the cache type, so within 1 ulp (+ the fp32 error the bar allows) of fp64"""
    v = stored(got, prec)
    assert np.all(np.isfinite(v)), "non-finite K/V row"
    slack = ulp16(ref, prec) if prec else 0.0
    excess = np.abs(v - ref) - slack - bar * np.maximum(1.0, np.abs(ref))
    assert excess.max() <= 0, f"K/V row: {excess.max():.3e} beyond 1 ulp + bar of the fp64 value"


@functools.lru_cache(maxsize=None)
def weights(prec, N, K, seed):
    rng = np.random.default_rng(seed)
    return store((rng.standard_normal((N, K), dtype=np.float32) / np.sqrt(K)).astype(np.float32), prec)


def attn64(q, K, V):
    """q [S][nq][H][48], K, V [S][H][n][48] (fp64) -> softmax(q K^T * scale) V as rows [S * nq][H * 48], and the scores [S][nq][H][n]"""
    s = np.einsum("bqhd,bhnd->bqhn", q, K) * SCALE_QK
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = np.einsum("bqhn,bhnd->bqhd", p, V)
    return o.reshape(q.shape[0] * q.shape[1], -1), s


def boundary_key(L, b):
    """a key on a split boundary below L: 128 s - 1 or 128 s (alternating by scene) of the last boundary, key 0 below one split"""
    if L <= CHUNK:
        return 0
    return CHUNK * ((L - 1) // CHUNK) - (b % 2)


def shape_scores(q, K, L, seed):
    """In place on q [S][nq][H][48] and K [S][H][>= L][48] (fp32, before rounding).  Head h of scene b gets pattern (h + b) % 4:
    0 the newest key L - 1 dominates the softmax, 1 a key on a split boundary dominates, 2 every score equal, 3 random."""
    rng = np.random.default_rng(seed)
    S, _, H = q.shape[:3]
    for b in range(S):
        for h in range(H):
            pat = (h + b) % 4
            if pat == 2:
                K[b, h, :L] = K[b, h, :1]
            elif pat < 2:
                u = rng.standard_normal(48)
                u /= np.linalg.norm(u)
                q[b, :, h] = 4.0 * u + 0.3 * q[b, :, h]
                K[b, h, L - 1 if pat == 0 else boundary_key(L, b)] += 20.0 * u


def check_patterns(s, L):
    """the scores [S][nq][H][n] show the intended patterns"""
    S, _, H = s.shape[:3]
    for b in range(S):
        for h in range(H):
            pat = (h + b) % 4
            if pat == 2:
                assert np.ptp(s[b, :, h], axis=-1).max() == 0, "the all-equal head has unequal scores"
            elif pat < 2 and L > 1:
                key = L - 1 if pat == 0 else boundary_key(L, b)
                assert np.all(s[b, :, h].argmax(-1) == key), f"scene {b} head {h}: key {key} does not dominate"


def rpb_forms(call):
    """call(rpb) for rows_per_block 0, 1, 2 -> the first result; the three must agree bit for bit (same summation order per row)"""
    res = [call(rpb) for rpb in (0, 1, 2)]
    for rpb, r in zip((1, 2), res[1:]):
        for a, b in zip(res[0], r):
            if a is not None:
                np.testing.assert_array_equal(raw(b), raw(a), err_msg=f"rows_per_block {rpb} differs from the row loop")
    return res[0]


# ---------------------------------------------------------------------------------------------------------------------------
# gemv_ln_kernel: LayerNorm + W x + bias in the F32, GELU and QKV output modes, with and without the device-side row offset
# ---------------------------------------------------------------------------------------------------------------------------
def gemv_call(prec, mode, rpb, x, xoff, lw, Wb, bias, N, E, ldo, cache, Lmax, pos):
    K = x.shape[1]
    M = x.shape[0] - max(xoff, 0)
    out = np.zeros((M, ldo), np.float32)
    c = None if cache is None else cache.copy()
    check(lib().umgen_dbg_gemv_modes(prec, mode, rpb, fp(x), xoff, fp(lw), vp(Wb), fp(bias), M, N, K, E, fp(out), ldo,
                                     None if c is None else vp(c), Lmax, pos))
    return out, c


def gemv_case(prec, mode, E, M, pos=None, Lmax=None):
    """Runs one gemv_ln case in the three row forms and checks everything but the value bar; returns the max relative error."""
    N = {GEMV_F32: 1028 if E > 96 else 100, GEMV_GELU: 4 * E, GEMV_QKV: 3 * E}[mode]
    ncol = E if mode == GEMV_QKV else N
    ldo = ncol + 12
    seed = 1000 * E + N + 7 * prec
    rng = np.random.default_rng(31 * seed + M)
    Wb, W = weights(prec, N, E, seed)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    lw = (1 + 0.2 * rng.standard_normal(E)).astype(np.float32)
    xr = ln_input(rng, M, E)
    xoff = [-1, 0, 3][M % 3]                       # -1: no device offset; rows in front of the offset are NaN
    x = np.concatenate([np.full((max(xoff, 0), E), np.nan, np.float32), xr])
    ref = ref_ln(xr, lw) @ W.T + bias
    if mode == GEMV_GELU:
        ref = gelu64(ref)
    cache = None
    H = E // 48
    if mode == GEMV_QKV:
        pos = [0, 1, 129][M % 3] if pos is None else pos
        Lmax = pos + 1 + M % 2 if Lmax is None else Lmax
        cache = nan_array((M, 2, H, Lmax, 48), prec)
        cache[:, :, :, :pos] = store(rng.standard_normal((M, 2, H, pos, 48)).astype(np.float32), prec)[0]
    out, c = rpb_forms(lambda rpb: gemv_call(prec, mode, rpb, x, xoff, lw, Wb, bias, N, E, ldo, cache, Lmax or 0, pos or 0))
    assert np.all(out[:, ncol:].view(np.uint32) == NAN32), "columns past the output were written"
    got = out[:, :ncol]
    assert np.all(np.isfinite(got)), "non-finite output"
    err = rel_err(got, ref[:, :ncol])
    if mode == GEMV_QKV:
        kv_ref = ref[:, E:].reshape(M, 2, H, 48)
        check_kv_row(c[:, :, :, pos], kv_ref, prec, GEMV_BAR)
        if prec == 0:                              # fp32 cache: the K/V rows are values like the q rows
            err = max(err, rel_err(c[:, :, :, pos], kv_ref))
        np.testing.assert_array_equal(raw(np.delete(c, pos, axis=3)), raw(np.delete(cache, pos, axis=3)),
                                      err_msg="a cache row other than pos changed")
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("M", M_SET)
@pytest.mark.parametrize("mode", [GEMV_F32, GEMV_GELU, GEMV_QKV])
@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("prec", PRECS)
def test_gemv_modes(prec, E, mode, M):
    err = gemv_case(prec, mode, E, M)
    assert err <= GEMV_BAR, f"max error {err:.3e} > bar {GEMV_BAR}"


@pytest.mark.gpu
@pytest.mark.parametrize("pos", POS_SET)
@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("prec", PRECS)
def test_gemv_qkv_positions(prec, E, pos):
    """the q|k|v launch of the decode step at every position class, in the product's cache of LMAX rows"""
    err = gemv_case(prec, GEMV_QKV, E, 2, pos=pos, Lmax=LMAX)
    assert err <= GEMV_BAR, f"max error {err:.3e} > bar {GEMV_BAR}"


# ---------------------------------------------------------------------------------------------------------------------------
# gemv_resid_kernel, plain form: x += a W^T (+ bias), K = 4E (NCH 1 | 6 | 12 at E = 96 | 768 | 1536)
# ---------------------------------------------------------------------------------------------------------------------------
def resid_case(prec, E, M):
    K, N = 4 * E, E
    lda = K + 8                                   # columns K .. lda - 1 are NaN: the kernel must not read them
    seed = 77 * E + 3 * prec
    rng = np.random.default_rng(seed + M)
    Wb, W = weights(prec, N, K, seed)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32) if M % 2 == 0 else None
    a = np.full((M, lda), np.nan, np.float32)
    a[:, :K] = gelu64(rng.standard_normal((M, K))).astype(np.float32)
    x0 = (0.5 * rng.standard_normal((M, N))).astype(np.float32)

    def call(rpb):
        x = x0.copy()
        check(lib().umgen_dbg_gemv_resid(prec, rpb, fp(a), lda, vp(Wb), fp(bias), M, N, K, fp(x)))
        return (x,)
    x, = rpb_forms(call)
    ref = x0.astype(np.float64) + a[:, :K].astype(np.float64) @ W.T + (0.0 if bias is None else bias.astype(np.float64))
    assert np.all(np.isfinite(x)), "non-finite output"
    return rel_err(x, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("M", M_SET)
@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("prec", PRECS)
def test_gemv_resid_plain(prec, E, M):
    err = resid_case(prec, E, M)
    assert err <= RESID_BAR, f"max error {err:.3e} > bar {RESID_BAR}"


# ---------------------------------------------------------------------------------------------------------------------------
# attn_partial_kernel at its three call sites, merged and projected by gemv_resid_kernel (COMBINE) with a real Wo, bias and residual
# ---------------------------------------------------------------------------------------------------------------------------
def attn_call(prec, geom, q, kv, B, H, pos, Wb, bo, x0):
    ns = (pos + CHUNK) // CHUNK

    def call(rpb):
        x = x0.copy()
        check(lib().umgen_dbg_attn_partial(prec, geom, rpb, fp(q), None if kv is None else vp(kv), B, H, LMAX, pos, ns, vp(Wb), fp(bo), fp(x)))
        return (x,)
    x, = rpb_forms(call)
    assert np.all(np.isfinite(x)), "non-finite output (a masked key or an unused split slot leaked in?)"
    return x


def proj_operands(prec, E, M, seed):
    rng = np.random.default_rng(seed)
    Wb, W = weights(prec, E, E, 5 * E + prec)
    bo = (0.1 * rng.standard_normal(E)).astype(np.float32)
    x0 = (0.5 * rng.standard_normal((M, E))).astype(np.float32)
    return Wb, W, bo, x0


def decode_attn_case(prec, E, B, pos):
    """the decode step's geometry: one query per scene over keys 0 .. pos of the scene's head-major cache (*d_len = pos, len_add 1)"""
    H, L = E // 48, pos + 1
    rng = np.random.default_rng(13 * pos + B + 1000 * prec)
    q = rng.standard_normal((B, 1, H, 48)).astype(np.float32)
    K = rng.standard_normal((B, H, L, 48)).astype(np.float32)
    V = rng.standard_normal((B, H, L, 48)).astype(np.float32)
    shape_scores(q, K, L, seed=L + B)
    Kb, Kv = store(K, prec)
    Vb, Vv = store(V, prec)
    cache = np.empty((B, 2, H, LMAX, 48), Kb.dtype)
    cache[:, 0, :, :L], cache[:, 1, :, :L] = Kb, Vb
    # rows past the length: keys along the query (they would dominate), values of 1000
    cache[:, 0, :, L:] = store(4.0 * np.sign(q[:, 0])[:, :, None], prec)[0]
    cache[:, 1, :, L:] = store(np.full((1, 1, 1, 48), 1000.0), prec)[0]
    Wb, W, bo, x0 = proj_operands(prec, E, B, pos + B)
    x = attn_call(prec, GEO_DECODE, q.reshape(B, E), cache, B, H, pos, Wb, bo, x0)
    o, s = attn64(q.astype(np.float64), Kv, Vv)
    check_patterns(s, L)
    return rel_err(x, x0 + o @ W.T + bo)


def ego_self_case(prec, E, B):
    """run_ego's self-attention: the 3 queries of a scene over its own 3 packed q|k|v rows (fp32 in every mode), one split"""
    H, M = E // 48, 3 * B
    rng = np.random.default_rng(E + B)
    q = rng.standard_normal((B, 3, H, 48)).astype(np.float32)
    K = rng.standard_normal((B, H, 3, 48)).astype(np.float32)
    V = rng.standard_normal((B, H, 3, 48)).astype(np.float32)
    shape_scores(q, K, 3, seed=B)
    qkv3 = np.concatenate([q.reshape(M, E), K.transpose(0, 2, 1, 3).reshape(M, E), V.transpose(0, 2, 1, 3).reshape(M, E)], axis=1)
    Wb, W, bo, x0 = proj_operands(prec, E, M, B)
    x = attn_call(prec, GEO_EGO_SELF, np.ascontiguousarray(qkv3), None, B, H, 0, Wb, bo, x0)
    o, s = attn64(q.astype(np.float64), K.astype(np.float64), V.astype(np.float64))
    check_patterns(s, 3)
    return rel_err(x, x0 + o @ W.T + bo)


def ego_cross_case(prec, E, B):
    """run_ego's cross-attention: the 3 queries of a scene over the scene's kSeq k|v rows [kSeq][2E], 18 splits"""
    H, M = E // 48, 3 * B
    rng = np.random.default_rng(3 * E + B + prec)
    q = rng.standard_normal((B, 3, H, 48)).astype(np.float32)
    K = rng.standard_normal((B, H, KSEQ, 48)).astype(np.float32)
    V = rng.standard_normal((B, H, KSEQ, 48)).astype(np.float32)
    shape_scores(q, K, KSEQ, seed=B + 1)
    Kb, Kv = store(K, prec)
    Vb, Vv = store(V, prec)
    kv = np.concatenate([Kb.transpose(0, 2, 1, 3).reshape(B * KSEQ, E), Vb.transpose(0, 2, 1, 3).reshape(B * KSEQ, E)], axis=1)
    Wb, W, bo, x0 = proj_operands(prec, E, M, B + 7)
    x = attn_call(prec, GEO_EGO_CROSS, q.reshape(M, E), np.ascontiguousarray(kv), B, H, 0, Wb, bo, x0)
    o, s = attn64(q.astype(np.float64), Kv, Vv)
    check_patterns(s, KSEQ)
    return rel_err(x, x0 + o @ W.T + bo)


def cache_fits(prec, E, B):
    return B * 2 * (E // 48) * LMAX * 48 * (4 if prec == 0 else 2) <= CACHE_BYTES


# (scenes, position): every scene count with one position class each, and every position at two scenes
STEP_CASES = sorted(set(zip(M_SET, POS_SET)) | {(2, p) for p in POS_SET})


@pytest.mark.gpu
@pytest.mark.parametrize("B,pos", STEP_CASES)
@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("prec", PRECS)
def test_attn_decode_step(prec, E, B, pos):
    if not cache_fits(prec, E, B):
        B = 2 if B > 2 else B                       # the widest caches: the same position at two scenes
    err = decode_attn_case(prec, E, B, pos)
    assert err <= ATTN_BAR, f"max error {err:.3e} > bar {ATTN_BAR}"


@pytest.mark.gpu
@pytest.mark.parametrize("B", EGO_B)
@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("prec", PRECS)
def test_attn_ego_self(prec, E, B):
    err = ego_self_case(prec, E, B)
    assert err <= ATTN_BAR, f"max error {err:.3e} > bar {ATTN_BAR}"


@pytest.mark.gpu
@pytest.mark.parametrize("B", EGO_B)
@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("prec", PRECS)
def test_attn_ego_cross(prec, E, B):
    err = ego_cross_case(prec, E, B)
    assert err <= ATTN_BAR, f"max error {err:.3e} > bar {ATTN_BAR}"


# ---------------------------------------------------------------------------------------------------------------------------
# one whole BlockOAR layer through launch_decode_layer
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_params(prec, E, seed):
    """(hook operands, fp64 values as stored) of one BlockOAR layer"""
    rng = np.random.default_rng(seed)
    op, val = {}, {}
    for name, (n, k) in (("Wqkv", (3 * E, E)), ("Wo", (E, E)), ("Wfc", (4 * E, E)), ("Wproj", (E, 4 * E))):
        op[name], val[name] = weights(prec, n, k, seed + n + 7 * k)
    for name, n, s in (("bqkv", 3 * E, 0.1), ("bo", E, 0.1)):
        op[name] = (s * rng.standard_normal(n)).astype(np.float32)
        val[name] = op[name].astype(np.float64)
    for name in ("ln_a", "ln_b"):
        op[name] = (1 + 0.2 * rng.standard_normal(E)).astype(np.float32)
        val[name] = op[name].astype(np.float64)
    return op, val


def layer_ref(x, P, Khist, Vhist, knew, vnew):
    """fp64 BlockOAR.forward_func (module.py:402-416) at one position: x [B][E]; P the layer's values as stored; Khist, Vhist
    [B][H][pos][48] and the new row knew, vnew [B][H][48] as stored.  -> (x out, q rows, the new K/V rows [B][2][H][48] before rounding)"""
    B, E = x.shape
    H = E // 48
    qkv = ref_ln(x, P["ln_a"]) @ P["Wqkv"].T + P["bqkv"]
    q = qkv[:, :E]
    K = np.concatenate([Khist, knew[:, :, None]], axis=2)
    V = np.concatenate([Vhist, vnew[:, :, None]], axis=2)
    o, _ = attn64(q.reshape(B, 1, H, 48), K, V)
    x1 = x.astype(np.float64) + o @ P["Wo"].T + P["bo"]
    h = gelu64(ref_ln(x1, P["ln_b"]) @ P["Wfc"].T)
    return x1 + h @ P["Wproj"].T, q, qkv[:, E:].reshape(B, 2, H, 48)


def layer_case(prec, E, B, pos):
    H = E // 48
    op, P = layer_params(prec, E, 9 * E + prec)
    rng = np.random.default_rng(pos + 100 * B)
    x0 = (rng.uniform(0.5, 2.0, (B, 1)) * rng.standard_normal((B, E)) + rng.uniform(-1, 1, (B, 1))).astype(np.float32)
    hist = rng.standard_normal((B, 2, H, pos, 48)).astype(np.float32)
    cache0 = np.empty((B, 2, H, LMAX, 48), np.float32 if prec == 0 else np.uint16)
    cache0[:, :, :, :pos] = store(hist, prec)[0]
    cache0[:, :, :, pos] = nan_array((B, 2, H, 48), prec)            # written by the q|k|v launch before the attention reads it
    cache0[:, :, :, pos + 1:] = store(np.full((1, 2, 1, 1, 48), 7.0), prec)[0]   # finite rows the attention loads and masks
    ns = (pos + CHUNK) // CHUNK

    def call(rpb):
        x, q, c = x0.copy(), np.zeros((B, E), np.float32), cache0.copy()
        check(lib().umgen_dbg_decode_layer(prec, rpb, B, E, pos, ns, fp(op["ln_a"]), vp(op["Wqkv"]), fp(op["bqkv"]), vp(op["Wo"]), fp(op["bo"]),
                                           fp(op["ln_b"]), vp(op["Wfc"]), vp(op["Wproj"]), fp(x), fp(q), vp(c)))
        return x, q, c
    x, q, c = rpb_forms(call)
    np.testing.assert_array_equal(raw(np.delete(c, pos, axis=3)), raw(np.delete(cache0, pos, axis=3)), err_msg="a cache row other than pos changed")
    new = stored(c[:, :, :, pos], prec)
    Hv = stored(cache0[:, :, :, :pos], prec)
    ref_x, ref_q, ref_kv = layer_ref(x0, P, Hv[:, 0], Hv[:, 1], new[:, 0], new[:, 1])
    check_kv_row(c[:, :, :, pos], ref_kv, prec, LAYER_BAR)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(q)), "non-finite output"
    return max(rel_err(x, ref_x), rel_err(q, ref_q))


LAYER_CASES = sorted(set(zip(M_SET, POS_SET)) | {(1, 2303), (3, 0)})


@pytest.mark.gpu
@pytest.mark.parametrize("B,pos", LAYER_CASES)
@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("prec", PRECS)
def test_decode_layer(prec, E, B, pos):
    if not cache_fits(prec, E, B):
        B = 2
    err = layer_case(prec, E, B, pos)
    assert err <= LAYER_BAR, f"max error {err:.3e} > bar {LAYER_BAR}"


def test_layer_restatement_matches_oracle():
    """CPU: the fp64 restatement above is the oracle's BlockOAR (OracleUMGen._block_oar, bf16_engine: bf16 weights, K/V rows rounded to
    bf16) up to the oracle's fp32 arithmetic -- the referee's referee is pinned to the oracle.  Measured 3.2e-7."""
    from oracle.umgen_oracle import OracleUMGen
    prec, E, B, pos = 1, 96, 3, 130
    H = E // 48
    op, P = layer_params(prec, E, 4242)
    key = "transformer.OAR.0"
    sd = {f"{key}.ln_1.weight": P["ln_a"], f"{key}.ln_2.weight": P["ln_b"],
          f"{key}.temporal_attn.c_attn.weight": P["Wqkv"], f"{key}.temporal_attn.c_attn.bias": P["bqkv"],
          f"{key}.temporal_attn.c_proj.weight": P["Wo"], f"{key}.temporal_attn.c_proj.bias": P["bo"],
          f"{key}.mlp.c_fc.weight": P["Wfc"], f"{key}.mlp.c_proj.weight": P["Wproj"]}
    oracle = OracleUMGen(types.SimpleNamespace(n_embd=E, n_head=H), {k: v.astype(np.float32) for k, v in sd.items()}, weight_dtype="bf16_engine")
    rng = np.random.default_rng(5)
    x0 = (rng.uniform(0.5, 2.0, (B, 1)) * rng.standard_normal((B, E))).astype(np.float32)
    hist = round16(rng.standard_normal((B, 2, H, pos, 48)).astype(np.float32), prec)
    kt = torch.from_numpy(np.ascontiguousarray(hist[:, 0].transpose(0, 2, 1, 3).reshape(B, pos, E)))
    vt = torch.from_numpy(np.ascontiguousarray(hist[:, 1].transpose(0, 2, 1, 3).reshape(B, pos, E)))
    with torch.no_grad():
        xo, (k, v) = oracle._block_oar(torch.from_numpy(x0)[:, None], key, (kt, vt))
    knew = k[:, -1].numpy().reshape(B, H, 48).astype(np.float64)
    vnew = v[:, -1].numpy().reshape(B, H, 48).astype(np.float64)
    ref_x, _, ref_kv = layer_ref(x0, P, hist[:, 0].astype(np.float64), hist[:, 1].astype(np.float64), knew, vnew)
    assert np.all(np.abs(np.stack([knew, vnew], 1) - ref_kv) <= ulp16(ref_kv, prec) + 1e-5 * np.maximum(1.0, np.abs(ref_kv)))
    err = rel_err(xo[:, 0].numpy(), ref_x)
    assert err <= 1e-6, f"restatement vs oracle: {err:.3e}"
