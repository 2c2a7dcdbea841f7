"""-m gpu: the kernels of the batched decode layer (umgen_amd/csrc/decode_batched.hip) and the sampler paths of the decode step
(umgen_amd/csrc/frame.hip) one kernel at a time, through the hooks umgen_dbg_rows / _attn_decode_batched / _sample / _collision.

References are fp64 restatements on the kernel's own operands: weights, K and V rounded to the 16-bit type, activations exact fp32;
LayerNorm with weight only and eps 1e-5, exact erf GELU, float32(1 / sqrt(48)) as the score scale.  The batched GEMM's activations
enter the matrix cores as hi + lo 16-bit pairs, so its error is ~2^-17 (bf16) / 2^-22 (fp16) of the activations plus fp32
accumulation; every case also shows that a hi-only product (the activations rounded to 16 bit) would miss its bar by more than 4x.
The samplers and the collision test must give the oracle's / the reference's answer exactly.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import NAN16, NAN32, SCALE_QK, bits16, check, fp, gelu64, lib, ln_input, ref_ln, round16, ulp16, vp

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_reference_checks as rc  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_GELU, ROWS_QKV, ROWS_RESID = 0, 1, 2, 3
# relative to max(1, max |ref|), bf16 | fp16: at most 3x the largest error measured over all cases on an MI355X (8.6e-6 | 8.4e-6, both from
# fp32 accumulation and the LayerNorm, not from the hi + lo split); a hi-only product misses by more than 40x | 7.8x the bar
ROWS_BAR = {1: 2.5e-5, 2: 2e-5}
ATTN_BAR = 2e-5                        # absolute (V ~ N(0, 1)), as tests/test_gpu_kernels.py::test_attn_decode; measured 9.7e-6 | 1.1e-5
M_SET = [1, 15, 16, 17, 31, 32, 33, 48, 49, 64]      # 1 .. 4 column blocks of 16 scenes, full and ragged
ROWS_LMAX = 160


def test_guard_bands_and_fragment_pads_detect_a_write():
    """What every "was not written" assertion below rests on (csrc/debug_util.h): the hooks' guard bands notice one changed byte at either
    end of a band, and the fragment-major download one written word in a scene column >= M or a pad column >= C.  The hook launches no
    kernel and returns the number of the first step that gave another answer than expected."""
    assert lib().umgen_dbg_guard_selftest() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# rows_mfma_kernel (with rows_to_frag_kernel in front)
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(prec, N, K, seed):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((N, K), dtype=np.float32) / np.sqrt(K)).astype(np.float32)
    return bits16(W, prec), round16(W, prec).astype(np.float64)


def rows_call(prec, mode, x, lw, Wb, bias, N, K, E, ldo, x0=None, Lmax=ROWS_LMAX, pos=0):
    """one umgen_dbg_rows launch; returns (out [M][ldo] or None, out_rows [M][N] or None, cache [M][2][H][Lmax][48] bits or None)"""
    M = x.shape[0]
    out = None
    if mode != ROWS_GELU:
        out = np.zeros((M, ldo), np.float32)
        if mode == ROWS_RESID:
            out[:, :N] = x0
    out_rows = np.zeros((M, N), np.float32) if mode in (ROWS_GELU, ROWS_RESID) else None
    cache = np.zeros((M, 2, E // 48, Lmax, 48), np.uint16) if mode == ROWS_QKV else None
    check(lib().umgen_dbg_rows(prec, mode, fp(np.ascontiguousarray(x)), fp(lw), vp(Wb), fp(bias), M, N, K, E, fp(out), ldo, fp(out_rows),
                               vp(cache) if cache is not None else None, Lmax if cache is not None else 0, pos))
    return out, out_rows, cache


ROWS_CASES = [  # (name, mode, N: "3E" | "4E" | "E" | absolute, K as a multiple of E, ldo - N)
    ("qkv", ROWS_QKV, "3E", 1, 0),
    ("gelu", ROWS_GELU, "4E", 1, 0),
    ("resid", ROWS_RESID, "E", 1, 0),
    ("resid_k4e", ROWS_RESID, "E", 4, 0),
    ("head1024", ROWS_F32, 1024, 1, 24),
    ("head1028", ROWS_F32, 1028, 1, 36),
    ("head8192", ROWS_F32, 8192, 1, 8),
]


def rows_case(prec, case, E, M):
    """Runs one rows_mfma case and checks everything but the bar; returns (max error, bar, max hi-only miss)."""
    _, mode, nspec, kmul, pad = next(c for c in ROWS_CASES if c[0] == case)
    N = {"3E": 3 * E, "4E": 4 * E, "E": E}.get(nspec, nspec)
    K = kmul * E
    ldo = E if mode == ROWS_QKV else N + pad
    seed = 1000 * E + 10 * K + N
    rng = np.random.default_rng(seed + M)
    Wb, W = weights(prec, N, K, seed)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    lw = (1 + 0.2 * rng.standard_normal(K)).astype(np.float32)
    x0 = None
    if mode == ROWS_RESID:
        x = (rng.uniform(0.5, 2.0, (M, 1)) * rng.standard_normal((M, K))).astype(np.float32)
        x0 = (0.5 * rng.standard_normal((M, N))).astype(np.float32)
        act = x.astype(np.float64)
    else:
        x = ln_input(rng, M, K)
        act = ref_ln(x, lw)
    act_hi = round16(act.astype(np.float32), prec).astype(np.float64)
    pos = [0, 47, ROWS_LMAX - 1][M % 3]
    out, out_rows, cache = rows_call(prec, mode, x, lw, Wb, bias, N, K, E, ldo, x0=x0, pos=pos)

    def full(a):
        v = a @ W.T + bias.astype(np.float64)
        if mode == ROWS_GELU:
            v = gelu64(v)
        if mode == ROWS_RESID:
            v = v + x0.astype(np.float64)
        return v
    ref, ref_hi = full(act), full(act_hi)
    if mode == ROWS_QKV:
        got, ref, ref_hi = out[:, :E], ref[:, :E], ref_hi[:, :E]
        H = E // 48
        # the K / V rows: the fp32 result rounded to 16 bit, so within 1 ulp of the fp64 reference -- plus the fp32 error the bar allows,
        # which only matters for values near zero, where the 16-bit spacing is finer than the fp32 accumulation error
        kv_ref = full(act)[:, E:].reshape(M, 2, H, 48)
        kv_got = from16(cache[:, :, :, pos, :], prec).astype(np.float64)
        assert np.all(np.isfinite(kv_got)), "non-finite K/V row"
        kv_bar = ROWS_BAR[prec] * max(1.0, float(np.abs(kv_ref).max()))
        excess = np.abs(kv_got - kv_ref) - ulp16(kv_ref, prec) - kv_bar
        assert excess.max() <= 0, f"K/V rows at pos {pos}: {excess.max():.3e} beyond 1 ulp + {kv_bar:.1e} of the fp64 reference"
        others = np.delete(cache, pos, axis=3)
        assert np.all(others == NAN16[prec]), "a cache row other than pos was written"
    elif mode == ROWS_GELU:
        got = out_rows
    else:
        got = out[:, :N]
        if mode == ROWS_RESID:
            np.testing.assert_array_equal(out_rows.view(np.uint32), got.view(np.uint32), err_msg="fragment-major copy != out")
    if out is not None:
        assert np.all(out[:, (E if mode == ROWS_QKV else N):].view(np.uint32) == NAN32), "columns past the output were written"
    assert np.all(np.isfinite(got)), "non-finite output of a scene m < M (NaN fragment columns m >= M leaked in?)"
    bar = ROWS_BAR[prec] * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    miss_hi = float(np.abs(got - ref_hi).max())
    # the one-scene launches of a few rows: bit-identical to their rows of the M-scene launch
    for m in sorted({0, M // 2, M - 1}):
        o1, r1, c1 = rows_call(prec, mode, x[m:m + 1], lw, Wb, bias, N, K, E, ldo, x0=None if x0 is None else x0[m:m + 1], pos=pos)
        if out is not None:
            np.testing.assert_array_equal(o1[0].view(np.uint32), out[m].view(np.uint32), err_msg=f"scene {m}: out differs from one-scene launch")
        if out_rows is not None:
            np.testing.assert_array_equal(r1[0].view(np.uint32), out_rows[m].view(np.uint32), err_msg=f"scene {m}: fragment output differs")
        if cache is not None:
            np.testing.assert_array_equal(c1[0], cache[m], err_msg=f"scene {m}: K/V rows differ from one-scene launch")
    return err, bar, miss_hi


def from16(b, prec):
    return b.view(np.float16).astype(np.float32) if prec == 2 else (b.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("M", M_SET)
@pytest.mark.parametrize("case", [c[0] for c in ROWS_CASES])
@pytest.mark.parametrize("E", [768, 96])
@pytest.mark.parametrize("prec", [1, 2])
def test_rows_mfma(prec, E, case, M):
    err, bar, miss_hi = rows_case(prec, case, E, M)
    assert err <= bar, f"max error {err:.3e} > bar {bar:.3e}"
    assert miss_hi > 4 * bar, f"the hi-only reference misses by only {miss_hi:.3e} (4 x bar {4 * bar:.3e}): the bar could not see a lost lo term"


# ---------------------------------------------------------------------------------------------------------------------------
# attn_decode_batched_kernel
# ---------------------------------------------------------------------------------------------------------------------------
def attn_inputs(prec, M, H, L, seed):
    """q [M][H*48] fp32 and K, V [M][H][L + 1][48] rounded to 16 bit; heads 0 .. 3 of every scene are adversarial: scores spanning
    about +-60, the largest score on the last key (rising maximum), the largest on the first key, all scores equal."""
    rng = np.random.default_rng(seed)
    n = L + 1
    q = rng.standard_normal((M, H, 48)).astype(np.float32)
    K = rng.standard_normal((M, H, n, 48)).astype(np.float32)
    V = rng.standard_normal((M, H, n, 48)).astype(np.float32)
    t = np.linspace(-1.0, 1.0, n) if n > 1 else np.ones(1)
    for b in range(M):
        u = rng.standard_normal(48)
        u /= np.linalg.norm(u)
        q[b, 1] = 4.0 * u
        K[b, 1] = 0.2 * K[b, 1] + (6.0 * t)[:, None] * u         # scores rise with the key index
        K[b, 1, -1] += 3.0 * u
        q[b, 2] = -4.0 * u
        K[b, 2] = 0.2 * K[b, 2] + (6.0 * t)[:, None] * u
        K[b, 2, 0] -= 3.0 * u                                      # the largest score on the first key
        K[b, 3] = K[b, 3, :1]                                      # every key equal: equal scores
    K, V = round16(K, prec), round16(V, prec)
    for b in range(M):                                             # head 0: scores span about +-60
        s = np.abs(K[b, 0].astype(np.float64) @ q[b, 0].astype(np.float64)).max() * SCALE_QK
        q[b, 0] *= np.float32(60.0 / max(s, 1e-3))
    return q.reshape(M, H * 48), K, V


def attn_ref(q, K, V):
    M, H = K.shape[:2]
    s = np.einsum("bhd,bhnd->bhn", q.reshape(M, H, 48).astype(np.float64), K.astype(np.float64)) * SCALE_QK
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhn,bhnd->bhd", p, V.astype(np.float64)).reshape(M, H * 48), s


ATTN_CASES = [(3, 2304, L) for L in (0, 1, 15, 16, 63, 64, 65, 255, 256, 257, 1000, 2303)] + \
             [(M, 320, L) for M in (17, 64) for L in (0, 1, 15, 16, 63, 64, 65, 255, 256, 257, 319)]


def attn_case(prec, M, Lmax, L):
    H = 16
    q, K, V = attn_inputs(prec, M, H, L, seed=7 * L + M)
    cache = np.full((M, 2, H, Lmax, 48), NAN16[prec], np.uint16)    # rows past len stay NaN
    cache[:, 0, :, :L + 1] = bits16(K, prec)
    cache[:, 1, :, :L + 1] = bits16(V, prec)
    y = np.zeros((M, H * 48), np.float32)
    check(lib().umgen_dbg_attn_decode_batched(prec, fp(q), vp(cache), M, H, Lmax, L, fp(y)))
    ref, s = attn_ref(q, K, V)
    assert np.all(np.isfinite(y)), "non-finite attention output (a NaN row past len was read?)"
    if L >= 8:
        assert np.ptp(s[:, 0], axis=-1).min() > 60, "head 0 does not span the intended score range"
        assert np.all(s[:, 1].argmax(-1) == L) and np.all(s[:, 2].argmax(-1) == 0)
    assert np.all(np.ptp(s[:, 3], axis=-1) == 0)
    return float(np.abs(y - ref).max())


@pytest.mark.parametrize("M,Lmax,L", ATTN_CASES)
@pytest.mark.parametrize("prec", [1, 2])
def test_attn_decode_batched(prec, M, Lmax, L):
    err = attn_case(prec, M, Lmax, L)
    assert err <= ATTN_BAR, f"max error {err:.3e} > {ATTN_BAR}"


# ---------------------------------------------------------------------------------------------------------------------------
# block_sample (top-k and top-p, masked index, temperature) and check_collision_dev
# ---------------------------------------------------------------------------------------------------------------------------
I32P = C.POINTER(C.c_int32)


def dev_sample(method, L, k, p, temp, mask_idx, u):
    L = np.ascontiguousarray(L, dtype=np.float32)
    u = np.ascontiguousarray(u, dtype=np.float32)
    tok = np.full(L.shape[0], -7, np.int32)
    check(lib().umgen_dbg_sample(method, fp(L), L.shape[0], L.shape[1], k, C.c_float(p), C.c_float(temp), mask_idx, fp(u), tok.ctypes.data_as(I32P)))
    return tok


@pytest.fixture(scope="module")
def ref_checks():
    return np.load(rc.OUT)


@pytest.fixture(scope="module")
def oracle():
    from oracle.umgen_oracle import OracleUMGen
    from umgen_amd.weights import synthetic_state_dict
    cfg = rc.topp_config()
    return OracleUMGen(cfg, synthetic_state_dict(cfg, seed=rc.TOPP_WEIGHT_SEED))


def test_topp_matches_reference_answers(ref_checks):
    """the reference's own sample_top_p answers (tests/golden/reference_checks.npz, 40 cases) from block_sample_topp"""
    want = ref_checks["topp_tokens"]
    for i, (logits, p, u) in enumerate(rc.top_p_cases()):
        got = dev_sample(1, logits.numpy()[None], 5, p, 1.0, -1, np.array([u]))
        assert int(got[0]) == int(want[i]), (i, logits.shape[0], p, int(got[0]), int(want[i]))


def sampler_rows(V, seed):
    """logit rows where samplers go wrong: random at several scales, ties straddling the nucleus boundary and the k-th value, an
    all-equal row, one dominant logit, logits spanning +-100 (exp underflows), heavy quantisation"""
    rng = np.random.default_rng(seed)
    rows = [rng.standard_normal(V) * s for s in (0.5, 2.0, 4.0)]
    for m in (3, 10, 40):                  # m equal top logits at scattered indices: the cumulative mass crosses p inside the tie run
        r = rng.standard_normal(V)
        r[rng.choice(V, m, replace=False)] = 5.0
        rows.append(r)
    r = rng.standard_normal(V)
    r[rng.choice(V, 6, replace=False)] = 4.0
    r[rng.choice(V, 6, replace=False)] = 3.5
    rows.append(r)
    rows.append(np.full(V, 1.5))
    r = rng.standard_normal(V)
    r[rng.integers(V)] = 30.0
    rows.append(r)
    rows.append(rng.uniform(-100, 100, V))
    rows.append(np.round(rng.standard_normal(V) * 4) / 4)
    return np.array(rows, dtype=np.float32)


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("temp", [0.7, 1.0, 1.3])
@pytest.mark.parametrize("V", [1000, 1024, 1028, 8192])
def test_sampler_matches_oracle(oracle, V, temp, mask):
    """block_sample through both methods (top-p: p from a hair to the image head's 16, UMGen.py:1133; top-k: k 1 / 5 / 16) with a
    temperature and the control resample's masked index (vocab - 1, made the row maximum): the oracle's token exactly"""
    base = sampler_rows(V, seed=V + int(temp * 10) + 7 * mask)
    us = np.array([0.0, 0.5, 1.0 - 2.0 ** -24, 0.8317], np.float32)
    L = np.repeat(base, len(us), axis=0)
    u = np.tile(us, base.shape[0])
    mask_idx = V - 1 if mask else -1
    if mask:
        L[:, V - 1] = L.max(axis=1) + 5.0
    masked = L.copy()
    if mask:
        masked[:, V - 1] = -np.inf             # what the oracle receives (umgen_oracle.py _sample_bbox)
    oracle.cfg.sfmx_temp = temp
    for method, params in ((1, [1e-6, 0.1, 0.4, 0.9, 16.0]), (0, [1, 5, 16])):
        oracle.cfg.sample_method = "topp" if method else "topk"
        for prm in params:
            k, p = (5, prm) if method else (prm, 0.9)
            got = dev_sample(method, L, k, p, temp, mask_idx, u)
            for r in range(L.shape[0]):
                want = oracle.sample(torch.from_numpy(masked[r]), k, p, np.float32(u[r]))
                assert int(got[r]) == want, (method, prm, r, float(u[r]), int(got[r]), want)
            if mask:
                assert np.all(got != V - 1)


def dev_collision(sets):
    max_n = max(len(s) for s in sets)
    boxes = np.zeros((len(sets), max_n, 10), np.float64)
    counts = np.array([len(s) for s in sets], np.int32)
    for i, s in enumerate(sets):
        boxes[i, :len(s)] = np.array(s, np.float64)
    out = np.full(len(sets), -1, np.int32)
    check(lib().umgen_dbg_collision(boxes.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(I32P), len(sets), max_n,
                                    out.ctypes.data_as(I32P)))
    return out


def test_collision_matches_reference_answers(ref_checks):
    cases = rc.collision_cases()
    got = dev_collision(cases)
    np.testing.assert_array_equal(got.astype(bool), ref_checks["collision"])


def collision_sets(seed, n_sets=400):
    """seeded sets of 1 .. 40 boxes at densities from sparse to crowded, some with boxes at x >= 63 (filtered out), the query box (the
    last survivor of the filter) sometimes followed by filtered boxes"""
    rng = np.random.default_rng(seed)
    sets = []
    for i in range(n_sets):
        n = 1 if i % 10 == 0 else int(rng.integers(2, 41))
        span = rng.choice([8.0, 25.0, 60.0])
        s = []
        for _ in range(n):
            x = rng.uniform(-span, span)
            if rng.random() < 0.06:
                x = rng.choice([63.0, rng.uniform(63.0, 70.0)])
            s.append(np.concatenate([[x, rng.uniform(-span, span), 0.0], rng.uniform(0.1, 8, 2), [1.5], rng.uniform(-3.14, 3.14, 1), [0, 0, 0]]))
        sets.append(s)
    return sets


def test_collision_matches_oracle():
    from oracle.umgen_oracle import check_collision
    sets = collision_sets(5)
    got = dev_collision(sets)
    want = np.array([check_collision(s) for s in sets])
    assert 40 < want.sum() < len(sets) - 40, "the seeded sets should collide sometimes, not always"
    np.testing.assert_array_equal(got.astype(bool), want)
