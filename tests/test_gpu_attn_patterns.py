"""The S x S attention kernels of the prefill side -- attn_spatial_mfma_kernel<QT, bf16_t | f16_t> (umgen_amd/csrc/attn_body.h), its CAUSAL
instantiation (the OAR prefix pass), attn_spatial_f32_mfma_kernel with and without the causal mask and, as a cross-check, the fp32 VALU kernel
(attn.hip) -- against fp64 attention on inputs whose right answer is exact or nearly so, through umgen_dbg_attn_spatial.  Every test needs a GPU
except the ones at the end of the file.

Reference: head_ref, fp64 softmax attention per (frame, head) on the values the kernel is handed (the operands after rounding to the operand
type; SCALE_QK is the fp32 1/sqrt(48)).  Every (frame, head) pair of a case carries one pattern, (f + h) % 5:
  0 uniform     q = 0: every score is exactly 0 and every p exactly 1; v[j][d] = -1 if (j >> (d % 6)) & 1 else +1, so every partial sum is an
                integer of magnitude <= 32 and the output of query i is exactly (sum over its visible keys) / (their count).  Bar: 1 ulp of the
                16-bit output type (4 ulp of fp32), and exactly 0 where the sum is 0.  A dropped or double-counted key moves the mean of every
                column that is not constant over the visible keys by at least 1 / 33 relative, or away from 0.
  1 permutation k rows are random sign vectors, q[i] = 24 k[pi(i)], pi(i) = (37 i + 11) % S (41 when 37 divides S), causal pi(i) = i (the key
                on the mask's edge); asserted from the fp64 scores: pi(i) leads every other visible key of query i by >= 30 nats.  v random.
                Bar: y[i] == v[pi(i)] within 1 ulp of the output type: every key's V column in every tile position is held to its identity.
  2 late max    scores rise by 3 nats per 64-key tile (k[j][0] = j // 64, k[j][1] = (j % 64) / 64, both exact in bf16) plus noise of 0.3 nats:
                the running maximum moves in every tile, so every tile rescales O.  The next head that draws the pattern gets the mirror image:
                the maximum is in tile 0, alpha == 1 from then on and the kernel's skip path runs.  Both asserted from the fp64 scores.
  3 one lane    falling scores as in the mirror image (noise below half a key's step, so the scores are strictly monotone), but exactly one query
                out of each group of 16 consecutive ones has the ramp's sign turned: its maximum is the last key it sees, in the last tile it
                sees.  The __all(alpha == 1.0f) shortcut must not skip that lane's rescale.  Asserted from the fp64 scores.
  4 random      test_attn_spatial's distribution (q, k x 1.5).
Bar of patterns 2 .. 4 (tests/gpu_util.py attn_bound), componentwise, with A = sum p |v| / sum p from the reference:
  u (A + |ref|) + 2e-5 max(1, A), u = 2^-8 | 2^-11 | 0 -- rounding p to the operand type while l sums the unrounded p, the output rounding, the
  project's fp32 bar -- and S 2^-25 max|v| in fp16 (a p below the subnormal range is lost).

Shapes: (F, H) = (3, 4) -- 12 pairs, the 8-pair XCD grouping's last group half empty -- at S = 1, 2, 17 (fewer queries than a wave's 32), 63, 64, 65
(the 64-key tile edge; 32-key edges in fp32), 128, 129 (the 128-query workgroup edge), 321 (five tiles + 1 key, the prefetch two tiles ahead, three
causal workgroups with different ntile), 449 (S % 64 = 1, four workgroups); (F, H) = (1, 2), patterns 0 and 1, at production length: S = 2207, and
1692 causal (a given map + boxes).  Every case runs with hook flag 128 (V^T pad columns hold 7.0, not 0: the kernels load them with the ragged
last tile and must give them the weight 0); one case per kernel form runs again without it and must be bit-equal.  The hook fills the output with
NaN first: no NaN may come back.

The CPU tests at the end show, on the cases' own inputs, that deliberately wrong fp64 references are outside the tests' own bars in every
affected row: key S-1 dropped / counted twice (pattern 0), the causal mask admitting key i+1 (pattern 0) or hiding key i (patterns 0 and 1), the V
rows of keys k0 + 4 and k0 + 20 of every tile swapped (pattern 1).

Smallest asserted permutation margin (nats; the inputs' own, the same in every precision: sign vectors and 24 are exact):
  S            1     2     17    63    64    65    128   129   321   449   2207 | 1692
  non-causal   -     159.3 103.9 90.1  69.3  90.1  69.3  69.3  76.2  62.4  55.4
  causal       -     131.6 97.0  83.1  69.3  90.1  76.2  83.1  62.4  69.3  55.4
  (S = 1: one key, nothing to lead.  The bar is 30; 24 x SCALE_QK x 2 = 6.9 nats per sign in which the nearest other key differs less.)

Measured on an MI355X, largest |got - ref| / bound over all cases per kernel form and pattern 2 | 3 | 4, and the number of elements of
patterns 0 | 1 that were not the correctly rounded value (all of them within the 1 ulp bar):
  form               pattern 2 (its mirror image) | 3 | 4        pattern 0 | 1: not correctly rounded
  bf16               0.494 (0.473) | 0.559 | 0.662             0 of 224880 | 0 of 224880
  fp16               0.478 (0.547) | 0.504 | 0.561             0 of 224880 | 0 of 224880
  bf16 causal        0.691 (0.642) | 0.641 | 0.672             0 of 200160 | 0 of 200160
  fp16 causal        0.559 (0.622) | 0.578 | 0.722             0 of 200160 | 0 of 200160
  fp32 MFMA          0.217 (0.037) | 0.124 | 0.079             17656 of 224880 | 0 of 224880
  fp32 MFMA causal   0.192 (0.024) | 0.083 | 0.065             18688 of 200160 | 0 of 200160
  fp32 VALU          0.217 (0.052) | 0.124 | 0.104             17656 of 224880 | 0 of 224880
The 16-bit kernels return the correctly rounded value in every element of patterns 0 and 1 (nothing is off by an ulp); the fp32 kernels are off
by at most 4 fp32 ulp in 8 % of pattern 0 (o x (1 / l): two roundings where the reference divides once) and exact in pattern 1.  An fp32 CPU
restatement of the 16-bit body's arithmetic (64-key tiles, fp32 online softmax, p rounded to the operand type, l summed unrounded) gives the same
bf16 ratios to three digits.  The componentwise bar inside test_attn_spatial / test_attn_causal (tests/test_gpu_kernels.py, Gaussian rows up to
2207 keys x 16 heads): at most 0.80.
Memory-safe mutants of attn_spatial_mfma_body, built outside the tree and run once through this file: the key-tail mask at >= S - 1 (key S - 1
dropped) or > S (the clamped duplicate counted), the causal mask at >= (key i hidden) or > i + 1 (key i + 1 admitted), two P registers swapped
ahead of the P.V product (keys k0 + 4 g and k0 + 16 + 4 g), __any for __all in the rescale shortcut -- every one fails this file in every 16-bit
form it can change (dropped key: every S but 64 and 128, where no tail is masked; duplicate: the same S, non-causal only, the causal mask
hides key S anyway; causal masks: every S above 1; the swap: every S; the shortcut: from S = 65, causal from 128), and in none of the fp32
forms, which do not run that body.
"""
import functools
import types

import numpy as np
import pytest

from tests.gpu_util import SCALE_QK, attn_bound, bits16, check, from_bits16, lib, round16, ulp16, vp

D = 48
SMALL_S = [1, 2, 17, 63, 64, 65, 128, 129, 321, 449]
SMALL_FH = (3, 4)
PROD_FH = (1, 2)
PROD_S = {0: 2207, 64: 1692}
GUARD = 128                                            # hook flag: 7.0 in the pad columns of V^T
# kernel form -> (precision code, hook flags)
FORMS = {"bf16": (1, 0), "fp16": (2, 0), "bf16_causal": (1, 64), "fp16_causal": (2, 64), "fp32_mfma": (0, 0), "fp32_mfma_causal": (0, 64),
         "fp32_valu": (0, 32)}
PERM_GAIN = 24.0
PERM_MARGIN = 30.0                                     # nats
RAMP = float(np.float32(3.0 / SCALE_QK))               # q's ramp component: 3 nats per unit of k's


def perm(S, causal):
    i = np.arange(S)
    return i if causal else ((37 if S % 37 else 41) * i + 11) % S


def one_lane(S):
    """pattern 3: the one query out of each 16 consecutive ones whose maximum is late"""
    i = np.arange(S)
    return i % 16 == ((i // 16) * 5 + 3) % 16


def visible(S, causal):
    i = np.arange(S)
    return (i[None, :] <= i[:, None]) if causal else np.ones((S, S), bool)


def head_ref(q, k, v, vis, mult=None):
    """fp64 attention of one head: query i over the keys vis[i], key j counted mult[j] times -> (y, A = sum p |v| / sum p, masked scores)"""
    sc = (q.astype(np.float64) @ k.astype(np.float64).T) * SCALE_QK
    sc = np.where(vis, sc, -np.inf)
    with np.errstate(invalid="ignore"):                # (a wrong reference may leave a query without keys: NaN)
        p = np.exp(sc - sc.max(1, keepdims=True))
        if mult is not None:
            p = p * mult
        l = p.sum(1, keepdims=True)
        v64 = v.astype(np.float64)
        return p @ v64 / l, p @ np.abs(v64) / l, sc


def head_inputs(S, causal, f, h, pat, mirror):
    rng = np.random.default_rng([S, int(causal), f, h])
    j = np.arange(S)
    q = np.zeros((S, D), np.float32)
    k = rng.standard_normal((S, D), dtype=np.float32)
    v = rng.standard_normal((S, D), dtype=np.float32)
    if pat == 0:
        v = np.where((j[:, None] >> (np.arange(D)[None, :] % 6)) & 1, -1.0, 1.0).astype(np.float32)
    elif pat == 1:
        k = np.where(rng.integers(0, 2, (S, D)) == 1, 1.0, -1.0).astype(np.float32)
        q = (PERM_GAIN * k[perm(S, causal)]).astype(np.float32)
    elif pat in (2, 3):
        amp = 0.55 if pat == 2 else 0.03               # noise: 0.144 sqrt(46) 0.55^2 = 0.3 nats | at most 0.144 x 46 x 0.03^2 = 0.006 nats
        q = rng.standard_normal((S, D), dtype=np.float32) * amp if pat == 2 else rng.uniform(-amp, amp, (S, D)).astype(np.float32)
        k = rng.standard_normal((S, D), dtype=np.float32) * amp if pat == 2 else rng.uniform(-amp, amp, (S, D)).astype(np.float32)
        k[:, 0], k[:, 1] = j // 64, (j % 64) / 64.0
        sign = np.where(one_lane(S), 1.0, -1.0) if pat == 3 else (-1.0 if mirror else 1.0)
        q[:, 0] = q[:, 1] = RAMP * sign
    else:
        q = rng.standard_normal((S, D), dtype=np.float32) * 1.5
        k = k * 1.5
    return q, k, v


def tile_maxima(sc):
    S = sc.shape[0]
    nt = (S + 63) // 64
    pad = np.full((S, nt * 64), -np.inf)
    pad[:, :S] = sc
    return pad.reshape(S, nt, 64).max(2)


def check_premises(sc, S, causal, pat, mirror):
    """what the patterns claim about their inputs, from the fp64 scores; returns the permutation margin"""
    nvis = np.arange(S) + 1 if causal else np.full(S, S)
    arg = sc.argmax(1)
    last_tile = 64 * ((nvis - 1) // 64)
    if pat == 1:
        pi = perm(S, causal)
        own = sc[np.arange(S), pi]
        rest = sc.copy()
        rest[np.arange(S), pi] = -np.inf
        margin = float((own - rest.max(1)).min())      # (+inf where pi(i) is the only visible key)
        assert margin >= PERM_MARGIN, f"pattern 1: key pi(i) leads by {margin:.1f} nats only"
        return margin
    if pat == 2 and not mirror:
        tm = tile_maxima(sc)
        run = np.maximum.accumulate(tm, axis=1)
        rises = (tm[:, 1:] > run[:, :-1]).sum(1)
        ntile = (nvis + 63) // 64
        # every tile moves the maximum (a ragged last tile of a few keys may not reach above the noise of the full tile before it)
        assert np.all(rises >= ntile - 2) and np.all(rises[nvis % 64 == 0] == ntile[nvis % 64 == 0] - 1)
        assert np.all(arg >= nvis - 64)
    if pat == 2 and mirror:
        assert np.all(arg < 64)
    if pat == 3:
        sel = one_lane(S)
        assert np.all(arg[sel] == nvis[sel] - 1) and np.all(arg[sel] >= last_tile[sel]) and np.all(arg[~sel] == 0)
    return None


@functools.lru_cache(maxsize=32)
def case(prec, causal, S, F, H):
    """inputs (rounded to the operand type), fp64 reference, A and the pattern of every (frame, head); premises asserted"""
    E = H * D
    q, k, v = (np.zeros((F, S, E), np.float32) for _ in range(3))
    ref, A = np.zeros((F, S, E)), np.zeros((F, S, E))
    pats, margin, seen2 = {}, np.inf, 0
    vis = visible(S, causal)
    for f in range(F):
        for h in range(H):
            pat = (f + h) % 5
            mirror = pat == 2 and seen2 % 2 == 1
            seen2 += pat == 2
            sl = slice(h * D, (h + 1) * D)
            qh, kh, vh = head_inputs(S, causal, f, h, pat, mirror)
            if prec:
                qh, kh, vh = round16(qh, prec), round16(kh, prec), round16(vh, prec)
            q[f, :, sl], k[f, :, sl], v[f, :, sl] = qh, kh, vh
            ref[f, :, sl], A[f, :, sl], sc = head_ref(qh, kh, vh, vis)
            m = check_premises(sc, S, causal, pat, mirror)
            margin = min(margin, m) if m is not None else margin
            pats[(f, h)] = (pat, mirror)
    for a in (q, k, v, ref, A):
        a.setflags(write=False)
    return types.SimpleNamespace(prec=prec, causal=causal, S=S, F=F, H=H, q=q, k=k, v=v, ref=ref, A=A, pats=pats, margin=margin)


def out_ulp(x, prec, n32):
    """1 ulp of the 16-bit output type at |x|, n32 ulp of fp32"""
    return ulp16(x, prec) if prec else n32 * np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def tolerance(c, f, h):
    """(target, componentwise tolerance) of head (f, h): what got must satisfy as |got - target| <= tolerance"""
    pat, _ = c.pats[(f, h)]
    sl = slice(h * D, (h + 1) * D)
    ref = c.ref[f, :, sl]
    if pat == 0:
        return ref, np.where(ref == 0.0, 0.0, out_ulp(ref, c.prec, 4))
    if pat == 1:
        tgt = c.v[f, perm(c.S, c.causal), sl].astype(np.float64)
        return tgt, out_ulp(tgt, c.prec, 1)
    return ref, attn_bound(ref, c.A[f, :, sl], c.prec, c.S, np.abs(c.v[f, :, sl]).max())


def run_kernel(c, flags):
    qk, v = np.ascontiguousarray(np.concatenate([c.q, c.k], axis=-1)), c.v.copy()          # (the case's arrays are read-only)
    y = np.zeros((c.F, c.S, c.H * D), dtype=np.uint16 if c.prec else np.float32)
    check(lib().umgen_dbg_attn_spatial(c.prec | flags, vp(bits16(qk, c.prec) if c.prec else qk), vp(bits16(v, c.prec) if c.prec else v),
                                       c.F, c.S, c.H, vp(y)))
    return y


def verify(form, c, y):
    got = (from_bits16(y, c.prec) if c.prec else y).astype(np.float64)
    assert not np.isnan(got).any(), "a NaN came back: an output row was not written, or a masked key was not given the weight 0"
    fails = []
    for (f, h), (pat, mirror) in c.pats.items():
        sl = slice(h * D, (h + 1) * D)
        tgt, tol = tolerance(c, f, h)
        err = np.abs(got[f, :, sl] - tgt)
        if pat < 2:
            exact = round16(tgt.astype(np.float32), c.prec) if c.prec else tgt.astype(np.float32)
            fig = f"not_correctly_rounded {int((got[f, :, sl] != exact).sum())} of {err.size}"
        else:
            fig = f"ratio {float((err / tol).max()):.3f}"
        print(f"ATTN_PATTERNS form {form} S {c.S} f {f} h {h} pattern {pat}{'m' if mirror else ''} {fig}")
        bad = err > tol
        if bad.any():
            i, d = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(tol, 1e-300), 0)), err.shape)
            fails.append(f"(f {f}, h {h}) pattern {pat}{'m' if mirror else ''}: {int(bad.sum())} elements in {int(bad.any(1).sum())} rows, worst at "
                         f"query {i} dim {d}: got {got[f, i, h * D + d]!r} target {tgt[i, d]!r} tolerance {tol[i, d]:.3e}")
    assert not fails, f"{form} S = {c.S}:\n" + "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SMALL_S)
@pytest.mark.parametrize("form", list(FORMS))
def test_patterns(form, S):
    prec, flags = FORMS[form]
    c = case(prec, bool(flags & 64), S, *SMALL_FH)
    verify(form, c, run_kernel(c, flags | GUARD))


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_patterns_at_production_length(form):
    """patterns 0 and 1 on 2207 keys (1692 causal): 35 (27) tiles, 18 (14) workgroups per pair"""
    prec, flags = FORMS[form]
    c = case(prec, bool(flags & 64), PROD_S[flags & 64], *PROD_FH)
    assert {p for p, _ in c.pats.values()} == {0, 1}
    verify(form, c, run_kernel(c, flags | GUARD))


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_guard_columns_do_not_change_a_bit(form):
    """S = 321: 63 pad columns behind the one key of the last tile; 7.0 in them against the product's zeros"""
    prec, flags = FORMS[form]
    c = case(prec, bool(flags & 64), 321, *SMALL_FH)
    np.testing.assert_array_equal(run_kernel(c, flags | GUARD), run_kernel(c, flags))


# ---------------------------------------------------------------------------------------------------------------------------
# no GPU below: the cases' premises, and deliberately wrong references against the tests' own tolerances
# ---------------------------------------------------------------------------------------------------------------------------
ALL_CASES = [(causal, S, *SMALL_FH) for causal in (False, True) for S in SMALL_S] + [(False, PROD_S[0], *PROD_FH), (True, PROD_S[64], *PROD_FH)]


@pytest.mark.parametrize("causal,S,F,H", ALL_CASES)
def test_case_premises_hold_on_the_reference(causal, S, F, H):
    """case() asserts them while it builds; the permutation margin is a property of the inputs alone"""
    margins = {prec: case(prec, causal, S, F, H).margin for prec in (0, 1, 2)}
    print(f"ATTN_PATTERNS margin S {S} causal {int(causal)} {margins[1]:.1f}")
    assert margins[0] == margins[1] == margins[2] >= PERM_MARGIN


def caught_rows(c, pat, wrong):
    """per head of pattern `pat`: (rows in which the wrong reference is outside the test's tolerance of the right one, elements likewise)"""
    out = []
    for (f, h), (p, _) in c.pats.items():
        if p != pat:
            continue
        sl = slice(h * D, (h + 1) * D)
        tgt, tol = tolerance(c, f, h)
        y = wrong(c.q[f, :, sl], c.k[f, :, sl], c.v[f, :, sl])
        bad = ~(np.abs(y - tgt) <= tol)                # (NaN, a query left without keys, counts as caught)
        out.append((bad.any(1), bad))
    assert out
    return out


WRONG_S = [(2, *SMALL_FH), (65, *SMALL_FH), (449, *SMALL_FH)]


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("twice", [False, True])
@pytest.mark.parametrize("causal,S,F,H", [(False, *s) for s in WRONG_S] + [(True, *s) for s in WRONG_S] + [(False, 2207, *PROD_FH), (True, 1692, *PROD_FH)])
def test_pattern_0_catches_key_S_minus_1_dropped_or_counted_twice(prec, twice, causal, S, F, H):
    c = case(prec, causal, S, F, H)
    mult = np.ones(S)
    mult[S - 1] = 2.0 if twice else 0.0
    for rows, elems in caught_rows(c, 0, lambda q, k, v: head_ref(q, k, v, visible(S, causal), mult)[0]):
        affected = np.arange(S) == S - 1 if causal else np.ones(S, bool)
        assert rows[affected].all(), f"{int((~rows[affected]).sum())} affected rows inside the tolerance"
        assert not rows[~affected].any()
        if S >= 64:                                    # no column is constant over the visible keys: every element of an affected row moves
            assert elems[affected].all()


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("S,F,H", WRONG_S + [(1692, *PROD_FH)])
def test_pattern_0_catches_a_causal_mask_that_admits_key_i_plus_1(prec, S, F, H):
    c = case(prec, True, S, F, H)
    i = np.arange(S)
    for rows, _ in caught_rows(c, 0, lambda q, k, v: head_ref(q, k, v, i[None, :] <= i[:, None] + 1)[0]):
        assert rows[:-1].all() and not rows[-1]        # (the last query has no key i + 1)


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("pat", [0, 1])
@pytest.mark.parametrize("S,F,H", WRONG_S + [(1692, *PROD_FH)])
def test_patterns_0_and_1_catch_a_causal_mask_that_hides_key_i(prec, pat, S, F, H):
    c = case(prec, True, S, F, H)
    i = np.arange(S)
    for rows, _ in caught_rows(c, pat, lambda q, k, v: head_ref(q, k, v, i[None, :] < i[:, None])[0]):
        assert rows.all()                              # (query 0 is left without a key)


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("causal,S,F,H", [(False, 65, *SMALL_FH), (True, 65, *SMALL_FH), (False, 449, *SMALL_FH), (True, 449, *SMALL_FH),
                                           (False, 2207, *PROD_FH), (True, 1692, *PROD_FH)])
def test_pattern_1_catches_two_v_rows_swapped_inside_a_tile(prec, causal, S, F, H):
    """keys k0 + 4 and k0 + 20 are the k-slots (hh 0, g 1, r 0) and its + 16 partner of the P.V product's key map k0 + 32 hh + 4 g + r"""
    c = case(prec, causal, S, F, H)
    a = np.arange(4, S - 16, 64)
    swap = np.arange(S)
    swap[a], swap[a + 16] = a + 16, a
    affected = np.isin(perm(S, causal), np.concatenate([a, a + 16]))
    assert affected.sum() == 2 * len(a) > 0
    for rows, _ in caught_rows(c, 1, lambda q, k, v: head_ref(q, k, v[swap], visible(S, causal))[0]):
        assert rows[affected].all() and not rows[~affected].any()
