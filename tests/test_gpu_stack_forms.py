"""-m gpu: the GEMM and temporal-attention LAUNCH FORMS of the prefill stacks that umgen_dbg_linear / umgen_dbg_attn_temporal cannot express,
through umgen_dbg_gemm (the whole GemmArgs geometry) and umgen_dbg_attn_temporal_range (one launch on any TemporalRange).

GEMM: the tail form of tar_sub (k | v rows of every frame into [R][3E] at column E, then q rows of the last frame), begin_decode's batched
logits_tar, build_tables' GMLP pair, fp32 GEMM_VT (batched, and the VQ attention block's), the VQ convolutions' Mi = 4.  Every case checks
(a) the written window against float64 on the rounded operands, (b) that every element outside the window kept its bits (NaN fill, or what
an earlier call wrote), (c) where stated, bit equality with another call.  Widths are small (E' = 256): the forms, not the sizes, are new.
Which kernel a case reaches follows from launch_gemm_mfma / launch_gemm_valu's dispatch (gemm.hip) at the shape and tile256 flag given.

Temporal attention: every kernel variant (heads per workgroup x query slots) on one pass, split passes at P = 1, T // 2, T - 1, the growing
window (cache_mode 4) and the tail form (q0 = T - 1, the q rows of the other slots NaN) -- y bit-equal to the one pass, the slot cache
holding exactly the k | v bits of the written slots and its fill everywhere else.

Bars are those of test_gpu_kernels.py (test_linear, test_gemv, test_attn_temporal).  Largest distance / bar observed on an MI355X
(each as a fraction of max(1, |ref|max) for the GEMMs):
    tail k|v and q, 16-bit stores   bf16 3.3e-3 (bar 1.2e-2), fp16 4.5e-4 (bar 1.5e-3)
    tail k|v and q, fp32            5.9e-7 (bar 2e-5)
    logits_tar                      1.3e-6 (bar 2e-5)
    GMLP                            1.2e-6 (bar 2e-5)
    fp32 GEMM_VT                    4.3e-7 (bar 2e-5)
    VQ convolution                  8.5e-7 (bar 2e-5)
    temporal, one pass (absolute)   fp32 7.7e-7 (bar 2e-5), bf16 7.8e-3 (bar 1.6e-2), fp16 9.8e-4 (bar 2e-3)
Every bit comparison held exactly.
"""
import numpy as np
import pytest

from tests.gpu_util import NAN16, NAN32, SCALE_QK, bits16, check, fp, from_bits16, gelu64, lib, round16, vp

EPS16 = {1: 1.0, 2: 0.125}     # as in test_gpu_kernels.py: 16-bit tolerances are quoted for bf16
BAR32 = 2e-5                   # fp32 chains, 16-bit weights x fp32 activations, 16-bit operands with fp32 / residual output
STORE, RESID, STORE_F32, VT = 0, 1, 2, 3
E1 = 256                       # E': the small stand-in for n_embd
KV_OFF = E1                    # column of the k | v segment inside a [R][3E'] row
N_BOX = 660                    # kNBox (csrc/frame.h)

pytestmark = pytest.mark.gpu


def bar_store(prec):
    return 1.2e-2 * EPS16[prec] if prec else BAR32


def operand(rng, shape, prec, scale=1.0):
    """random values of precision code prec: (what the hook takes: fp32 values or 16-bit patterns, the same values as float64)"""
    a = (rng.standard_normal(shape) * scale).astype(np.float32)
    if prec:
        return bits16(a, prec), round16(a, prec).astype(np.float64)
    return a, a.astype(np.float64)


def nan_buf(n, prec):
    """n output elements holding the quiet-NaN pattern of precision code prec, as unsigned words"""
    return np.full(n, NAN16[prec], dtype=np.uint16) if prec else np.full(n, NAN32, dtype=np.uint32)


def values(words, prec):
    return from_bits16(np.ascontiguousarray(words), prec).astype(np.float64) if prec else np.ascontiguousarray(words).view(np.float32).astype(np.float64)


def window(off, batch, stride_o, Nj, ldo, Mi):
    """flat element indices [batch][Nj][Mi] of a GEMM_STORE / RESID / STORE_F32 output"""
    z, j, i = np.arange(batch)[:, None, None], np.arange(Nj)[None, :, None], np.arange(Mi)[None, None, :]
    return off + z * stride_o + j * ldo + i


def gemm(pP, pQ, mfma, P, Q, bias, Mi, Nj, K, out, *, mode=STORE, ldo, off=0, gelu=0, tile256=0, batch=1, sP=0, sQ=0, sO=0, H=0, ldp=None, ldq=None):
    check(lib().umgen_dbg_gemm(pP, pQ, mfma, vp(P), P.size, vp(Q), Q.size, fp(bias), Mi, Nj, K, ldp or K, ldq or K, sP, sQ, batch, mode, gelu,
                               ldo, sO, H, tile256, vp(out), off, out.size))


def check_window(name, out, before, idx, ref, prec_o, bar):
    """(a) out[idx] within bar * max(1, |ref|max) of ref; (b) every other element of out still holds the bits of `before`"""
    got = values(out[idx], prec_o)
    d = float(np.abs(got - ref).max()) if np.isfinite(got).all() else float("inf")
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"DIST {name} {d / scale:.3e} bar {bar:.3e}")
    assert d <= bar * scale, f"{name}: {d:.3e} from float64 (bar {bar * scale:.3e})"
    outside = np.ones(out.size, dtype=bool)
    outside[idx.ravel()] = False
    assert np.array_equal(out[outside], before[outside]), f"{name}: an element outside the written window changed"


# ---- the tail form of tar_sub: k | v rows of every frame, then q rows of the last frame, in [R][3E'] rows ------------------------------
# (prec, tile256, K, R) -> the kernel launch_gemm_mfma / launch_gemm_valu picks
TAIL_CASES = [pytest.param(p, t, K, R, id=f"{n}-{'fp32 bf16 fp16'.split()[p]}") for p, t, K, R, n in
              [(p, 1, 128, 300, "gemm16_256") for p in (1, 2)] +          # forced 256-tile kernel (Mi % 256 == 0, K % 128 == 0)
              [(p, -1, 128, 300, "glds") for p in (1, 2)] +               # K % 64 == 0, 4 x 3 tiles
              [(p, 0, 96, 300, "mfma128") for p in (1, 2)] +              # K % 64 != 0: gemm_bf16_mfma_kernel
              [(p, 0, 64, 32641, "persistent") for p in (1, 2)] +         # 4 x 256 = 1024 tiles, K % 128 != 0 keeps the 256-tile kernel out
              [(0, 0, 130, 300, "f32_mfma"), (0, -1, 130, 300, "f32_valu")]]


@pytest.mark.parametrize("prec,tile256,K,R", TAIL_CASES)
def test_tail_kv_then_q(prec, tile256, K, R):
    """GEMM_STORE with Mi = 2E', ldo = 3E', out = QKV + E' (+ bias): the q columns keep their NaN bits, the k | v window is within the bar
    and bit-equal to the dense (ldo = Mi) launch of the same kernel choice.  Then (R = 300) Mi = E' q rows of the last 131 rows -- and of
    the first 131 -- into the same buffer: the k | v columns and the other rows' q columns keep their bits."""
    rng = np.random.default_rng(1000 * prec + K + R)
    mfma = 1 if prec else 0
    W, Wv = operand(rng, (3 * E1, K), prec, 1.0 / np.sqrt(K))
    A, Av = operand(rng, (R, K), prec)
    bias = (rng.standard_normal(3 * E1) * 0.1).astype(np.float32)
    ref = Av @ Wv.T + bias                                               # [R][3E']: q | k | v
    bar = bar_store(prec)
    buf = nan_buf(R * 3 * E1, prec)
    before = buf.copy()
    gemm(prec, prec, mfma, W[E1:], A, bias[E1:], 2 * E1, R, K, buf, ldo=3 * E1, off=KV_OFF, tile256=tile256)
    idx = window(KV_OFF, 1, 0, R, 3 * E1, 2 * E1)
    check_window("tail_kv", buf, before, idx, ref[None, :, E1:], prec, bar)
    dense = nan_buf(R * 2 * E1, prec)
    gemm(prec, prec, mfma, W[E1:], A, bias[E1:], 2 * E1, R, K, dense, ldo=2 * E1, tile256=tile256)
    assert np.array_equal(buf[idx].ravel(), dense), "the strided k | v store differs from the dense one in more than its address"
    if R > 1000:
        return
    for row0 in (R - 131, 0):
        before = buf.copy()
        gemm(prec, prec, mfma, W[:E1], A[row0:row0 + 131], bias[:E1], E1, 131, K, buf, ldo=3 * E1, off=row0 * 3 * E1, tile256=tile256)
        check_window("tail_q", buf, before, window(row0 * 3 * E1, 1, 0, 131, 3 * E1, E1), ref[None, row0:row0 + 131, :E1], prec, bar)


# ---- begin_decode's logits_tar: batched GEMM_STORE_F32, one weight matrix, fp32 activation rows with a gap between the scenes ------------
@pytest.mark.parametrize("K", [96, 768])
@pytest.mark.parametrize("Nj", [N_BOX, 5])
@pytest.mark.parametrize("precP", [1, 2, 0])
def test_logits_tar_form(precP, Nj, K):
    """launch_gemm_valu<T, float>: batch 3, strideP = 0, strideQ and strideO larger than a scene's rows (the rows between are NaN inputs that
    must not be read, NaN outputs that must not be written), Mi = 1028 (no multiple of a tile)."""
    rng = np.random.default_rng(precP + Nj + K)
    Mi, batch, gapq, gapo = 1028, 3, 3, 2
    W, Wv = operand(rng, (Mi, K), precP, 1.0 / np.sqrt(K))
    Q = np.full((batch, Nj + gapq, K), np.nan, dtype=np.float32)
    Q[:, :Nj] = rng.standard_normal((batch, Nj, K)).astype(np.float32)
    bias = (rng.standard_normal(Mi) * 0.1).astype(np.float32) if Nj == 5 else None       # (the engine's launch has none)
    ref = Q[:, :Nj].astype(np.float64) @ Wv.T + (bias if bias is not None else 0.0)
    sO = (Nj + gapo) * Mi
    out = nan_buf(batch * sO, 0)
    before = out.copy()
    gemm(precP, 0, 0, W, Q, bias, Mi, Nj, K, out, mode=STORE_F32, ldo=Mi, batch=batch, sP=0, sQ=(Nj + gapq) * K, sO=sO)
    check_window("logits_tar", out, before, window(0, batch, sO, Nj, Mi, Mi), ref, 0, BAR32)
    if precP == 0:       # fp32 weights: that was the matrix-core kernel; the VALU kernel is the same FMA chain
        valu = before.copy()
        gemm(0, 0, 0, W, Q, bias, Mi, Nj, K, valu, mode=STORE_F32, ldo=Mi, batch=batch, sP=0, sQ=(Nj + gapq) * K, sO=sO, tile256=-1)
        assert np.array_equal(valu, out)


# ---- build_tables' GMLP(codebook): c_fc + GELU at K = n_map_embd / n_img_embd, then c_proj at K = 4E' -----------------------------------
@pytest.mark.parametrize("Mi,K,gelu", [(4 * E1, 16, 1), (4 * E1, 8, 1), (E1, 4 * E1, 0)])
@pytest.mark.parametrize("precP", [1, 2])
def test_gmlp_form(precP, Mi, K, gelu):
    """launch_gemm_valu<T, float> in GEMM_STORE: 16-bit weights, fp32 activations, fp32 output (the type of Q), Nj = 1029 rows"""
    rng = np.random.default_rng(precP + Mi + K)
    Nj = 1029
    W, Wv = operand(rng, (Mi, K), precP, 1.0 / np.sqrt(K))
    Q, Qv = operand(rng, (Nj, K), 0)
    ref = Qv @ Wv.T
    if gelu:
        ref = gelu64(ref)
    out = nan_buf(Nj * Mi + 64, 0)
    before = out.copy()
    gemm(precP, 0, 0, W, Q, None, Mi, Nj, K, out, ldo=Mi, gelu=gelu)
    check_window("gmlp", out, before, window(0, 1, 0, Nj, Mi, Mi), ref[None], 0, BAR32)


# ---- fp32 GEMM_VT: the spatial attention's V^T of fp32 mode (batched over frames) and of the VQ attention block ---------------------------
def vt_window(batch, rows, ldo, Mi):
    z, r, i = np.arange(batch)[:, None, None], np.arange(rows)[None, :, None], np.arange(Mi)[None, None, :]
    return (z * rows + r) * ldo + i


@pytest.mark.parametrize("batch,S,ldo", [(3, 131, 192), (3, 132, 192), (1, 128, 128)])
def test_fp32_gemm_vt(batch, S, ldo):
    """out[z][feature][token] with ldo = pad64(S) (the VQ block: batch 1, ldo = S = 128), Nj = 96 features = 2 heads.  The launcher's choice
    (tile256 0: gemm_f32_mfma_kernel<GEMM_VT> when S % 4 == 0, the VALU kernel at S = 131) and the VALU kernel (tile256 -1) agree bit for
    bit; the pad columns keep their fill."""
    rng = np.random.default_rng(batch + S)
    Nj = K = 96
    P, Pv = operand(rng, (batch, S, K), 0)
    W, Wv = operand(rng, (Nj, K), 0, 1.0 / np.sqrt(K))
    bias = (rng.standard_normal(Nj) * 0.1).astype(np.float32)
    ref = (Pv @ Wv.T + bias).transpose(0, 2, 1)                            # [batch][Nj][S]
    idx = vt_window(batch, Nj, ldo, S)
    outs = []
    for tile256 in (0, -1):
        out = nan_buf(batch * Nj * ldo, 0)
        before = out.copy()
        gemm(0, 0, 0, P, W, bias, S, Nj, K, out, mode=VT, ldo=ldo, batch=batch, sP=S * K, sQ=0, H=2, tile256=tile256)
        check_window(f"gemm_vt_f32[{tile256}]", out, before, idx, ref, 0, BAR32)
        outs.append(out)
    assert np.array_equal(outs[0], outs[1]), "the launcher's kernel and the VALU kernel differ"


# ---- the VQ convolutions: cout_pad = 4 output features ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [STORE, RESID])
def test_vq_conv_form(mode):
    rng = np.random.default_rng(mode)
    Mi, Nj, K = 4, 1000, 288
    W, Wv = operand(rng, (Mi, K), 0, 1.0 / np.sqrt(K))
    A, Av = operand(rng, (Nj, K), 0)
    bias = (rng.standard_normal(Mi) * 0.1).astype(np.float32)
    ref = Av @ Wv.T + bias
    out = nan_buf(Nj * Mi + 64, 0)
    if mode == RESID:
        x0 = rng.standard_normal((Nj, Mi)).astype(np.float32)
        out[:Nj * Mi] = x0.view(np.uint32).ravel()
        ref = ref + x0
    before = out.copy()
    outs = []
    for tile256 in (0, -1):                                               # matrix cores, VALU: the same FMA chain
        o = out.copy()
        gemm(0, 0, 0, W, A, bias, Mi, Nj, K, o, mode=mode, ldo=Mi, tile256=tile256)
        check_window(f"vq_conv[{tile256}]", o, before, window(0, 1, 0, Nj, Mi, Mi), ref[None], 0, BAR32)
        outs.append(o)
    assert np.array_equal(outs[0], outs[1])


# ---- temporal attention on every slot range ------------------------------------------------------------------------------------------------
def ref_temporal(qkv, H):
    """float64 causal softmax over the slots per (scene, position, head): qkv [B][T][S][3E] -> [B][T][S][E]"""
    B, T, S, E3 = qkv.shape
    E = E3 // 3
    x = qkv.astype(np.float64).reshape(B, T, S, 3, H, 48)
    q, k, v = x[:, :, :, 0], x[:, :, :, 1], x[:, :, :, 2]                   # [B][T][S][H][48]
    att = np.einsum("bqshd,bkshd->bshqk", q, k) * SCALE_QK
    tq, tk = np.arange(T), np.arange(T)
    att = np.where(tk[None, :] > tq[:, None], -np.inf, att)
    att = np.exp(att - att.max(-1, keepdims=True))
    att /= att.sum(-1, keepdims=True)
    return np.einsum("bshqk,bkshd->bqshd", att, v).reshape(B, T, S, E)


def attn_range(prec, qkv, H, t0, q0, write, cache, y):
    B, Tn, S, _ = qkv.shape
    qkv = np.ascontiguousarray(qkv)
    check(lib().umgen_dbg_attn_temporal_range(prec, vp(qkv), B, Tn, S, H, t0, q0, write, cache.shape[1], vp(cache), vp(y)))


# (H, T) -> attn_temporal_kernel<T, heads per workgroup, query slots>
@pytest.mark.parametrize("H,T", [(4, 20), (4, 21), (4, 32), (2, 5), (1, 6), (1, 33), (2, 64), (4, 40)],
                         ids=["4x20", "4x32-T21", "4x32-T32", "2x32", "1x32", "1x64", "2x64-T64", "2x64-H4"])
@pytest.mark.parametrize("S", [7, 33])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_temporal_ranges(prec, S, H, T):
    B, E, Tcap = 2, H * 48, T + 3
    rng = np.random.default_rng(100 * prec + S + 7 * H + T)
    a = rng.standard_normal((B, T, S, 3 * E)).astype(np.float32)
    qkv = bits16(a, prec) if prec else a.view(np.uint32).copy()              # the words the kernel reads
    kv = qkv[..., E:]

    def fresh(Tn):
        return nan_buf(B * Tcap * S * 2 * E, prec).reshape(B, Tcap, S, 2 * E), nan_buf(B * Tn * S * E, prec).reshape(B, Tn, S, E)

    def cache_holds(cache, n, what):
        assert np.array_equal(cache[:, :n], kv[:, :n]), f"{what}: cache slots [0, {n}) are not the k | v bits"
        assert np.all(cache[:, n:] == cache.dtype.type(NAN16[prec] if prec else NAN32)), f"{what}: a cache slot >= {n} lost its fill"

    # one pass: against float64, and the bit reference of every other form
    cache, one = fresh(T)
    c0 = cache.copy()
    attn_range(prec, qkv, H, 0, 0, 0, cache, one)
    assert np.array_equal(cache, c0), "one pass, write = 0: the cache changed"
    got, ref = values(one, prec), ref_temporal(values(qkv, prec), H)
    d = float(np.abs(got - ref).max()) if np.isfinite(got).all() else float("inf")
    bar = 1.6e-2 * EPS16[prec] if prec else 2e-5
    print(f"DIST temporal[{prec}] {d:.3e} bar {bar:.3e}")
    assert d <= bar, f"one pass: {d:.3e} from float64 (bar {bar:.3e})"

    def prefix(P):
        cache, y = fresh(P)
        attn_range(prec, qkv[:, :P], H, 0, 0, 1, cache, y)
        assert np.array_equal(y, one[:, :P]), f"prefix pass of {P} slots differs from the one pass"
        cache_holds(cache, P, f"prefix pass of {P} slots")
        return cache

    # splits: slots [0, P) with write = 1, then [P, T) against the cache
    for P in sorted({1, T // 2, T - 1}):
        cache = prefix(P)
        c0, (_, y) = cache.copy(), fresh(T - P)
        attn_range(prec, qkv[:, P:], H, P, 0, 0, cache, y)
        assert np.array_equal(y, one[:, P:]), f"split at {P}: the second pass differs from the one pass"
        assert np.array_equal(cache, c0), f"split at {P}: the write = 0 pass changed the cache"

    # growing window (cache_mode 4): a one-slot pass that appends its own k | v rows, then one more slot against them
    for P in sorted({1, T // 2, T - 2}):
        cache = prefix(P)
        _, y = fresh(1)
        attn_range(prec, qkv[:, P:P + 1], H, P, 0, 1, cache, y)
        assert np.array_equal(y, one[:, P:P + 1]), f"growing window: slot {P} differs from the one pass"
        cache_holds(cache, P + 1, f"growing window, slot {P}")
        c0, (_, y) = cache.copy(), fresh(1)
        attn_range(prec, qkv[:, P + 1:P + 2], H, P + 1, 0, 0, cache, y)
        assert np.array_equal(y, one[:, P + 1:P + 2]), f"growing window: slot {P + 1} differs from the one pass"
        assert np.array_equal(cache, c0), f"growing window: the write = 0 pass of slot {P + 1} changed the cache"

    # tail (q0 = T - 1): the q rows of the slots nobody consumes do not exist
    tail = qkv.copy()
    tail[:, :T - 1, :, :E] = NAN16[prec] if prec else NAN32
    for write in (0, 1):
        cache, y = fresh(T)
        attn_range(prec, tail, H, 0, T - 1, write, cache, y)
        assert np.array_equal(y[:, T - 1], one[:, T - 1]) and np.isfinite(values(y[:, T - 1], prec)).all(), f"tail (write {write}): slot {T - 1} differs from the one pass"
        assert np.all(y[:, :T - 1] == y.dtype.type(NAN16[prec] if prec else NAN32)), f"tail (write {write}): a row of an unconsumed slot was written"
        cache_holds(cache, T if write else 0, f"tail (write {write})")
