"""The score-detail sweep (csrc/score.hip head_detail_kernel / logits_detail_kernel) through its hooks umgen_dbg_head_detail and
umgen_dbg_logits_detail: rank, mass above, entropy and the 16 most likely tokens per row, against float64.

Inputs are those of tests/test_gpu_score_kernel.py (its weights, rows and planted rows; weights rounded to the operand type before either side
sees them) plus three ladder rows: a spike feature whose weight column holds 16 planted values (30 - i) / sqrt(K), zeros elsewhere, placed
(a) scrambled inside one 16-column tile, (b) one per vocabulary split, cycling, one of them on V - 1 in the partly filled last tile, (c) on the four
columns one lane owns in each of the tiles t, t + 4, t + 8, t + 12 that one wave sweeps.

Targets are chosen here on the CPU: row i takes the token nearest a wanted float64 rank (cycling through WANTED) whose float64 logit has no other
logit within 4 delta_row, delta_row = 1e-4 max(1, max |logit| of the row) being that file's logit bar.  So a logit error of delta on both sides
cannot move a logit across the target's.

Bars (derived, not measured):
  rank        exact.
  mass_above  inside [L e^(-2 delta / tau) - 1e-6, U e^(+2 delta / tau) + 1e-6], L / U the float64 masses above t + 2 delta / t - 2 delta (equal by the
              choice of targets): what a logit error of delta does to a probability ratio.
  entropy     |H - H64| <= 2 delta (1 + H64) + c: a logit error of delta moves lse by at most delta and E_p(max - v) <= H by at most 2 delta H; c is
              the fp32 summation term, 4 x the distance of a float32 numpy restatement of the centred sum to float64 on the same logits, computed per
              case below.  Over the 12 cases with the seeds used here c lies between 1.7e-06 and 3.4e-06.
  top-K       tokens distinct; |lg64[tok[i]] - sorted64[i]| <= 2 delta at every position; topk_logp within 2e-4 max(1, max |logit|) of float64's
              log-probability of the returned token; the lists equal float64's exactly on >= 98 % of the random rows of a case.
The row seed of a case is chosen on the CPU (SEEDS) so that float64 alone leaves at most 2 % of the random rows with two of its 17 best logits closer
than 1e-5 max(1, max |logit|): the hi + lo 16-bit activation pairs carry 16 mantissa bits, a product is off by 2^-17 relative, the sum of K such errors of
random sign by about 2^-17 sigma_logit ~ 4e-6, and the fp32 accumulation by less."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.gpu_util import bits16, check, fp, lib, ln_input, ref_ln, round16, vp
from tests.test_gpu_score_kernel import BAR, M_FULL, ROW_ALONE, ROW_EQUAL, ROW_FIRST, ROW_LAST, ROW_SCALE80, ROW_SPLIT, SHAPES, weights

pytestmark = pytest.mark.gpu

ROW_LADDER_A, ROW_LADDER_B, ROW_LADDER_C = 6, 7, 8
PLANTED = [ROW_EQUAL, ROW_SCALE80, ROW_FIRST, ROW_LAST, ROW_SPLIT, ROW_LADDER_A, ROW_LADDER_B, ROW_LADDER_C]
LADDER_POS = 7                      # the ladder rows' target: planted position 7
TAUS = (0.7, 1.0)
FRAGILE = 1e-5
i32p = C.POINTER(C.c_int32)
# row seeds chosen on the CPU (see the docstring): (prec, K, V) -> seed
SEEDS = {(0, 96, 1028): 2, (0, 768, 8192): 1, (0, 768, 1028): 1, (0, 1536, 8192): 1, (1, 96, 1028): 2, (1, 768, 8192): 1, (1, 768, 1028): 2,
         (1, 1536, 8192): 1, (2, 96, 1028): 3, (2, 768, 8192): 4, (2, 768, 1028): 5, (2, 1536, 8192): 1}


def wanted_ranks(V):
    return [0, 1, 4, 5, 15, 16, 100, V // 2, V - 1]


def ladder_columns(V, split):
    ns = (V + split - 1) // split
    a = [32 + (5 * i + 3) % 16 for i in range(16)]                                       # one tile, scrambled
    b = [(i % ns) * split + 7 + 3 * (i // ns) for i in range(16)]                        # one per split, cycling
    b[ns - 1] = V - 1                                                                    # the last split's first: the last column
    t = split // 16                                                                       # the second split's first tile; t + 12 lies inside it (>= 13 tiles)
    c = [16 * (t + 4 * (i % 4)) + 4 * 2 + (i // 4) for i in range(16)]                   # lane (col, kg = 2): its 4 columns of 4 tiles, interleaved
    for cols in (a, b, c):
        assert len(set(cols)) == 16 and min(cols) > 0 and max(cols) < V, cols
    return a, b, c


@functools.lru_cache(maxsize=None)
def detail_weights(K, V):
    W, dims, split = weights(K, V)
    W = W.copy()
    ldims = (5, 9, K // 3)
    assert not set(ldims) & set(dims)
    cols = ladder_columns(V, split)
    for d, cc in zip(ldims, cols):
        W[:, d] = 0.0
        W[cc, d] = (30.0 - np.arange(16)) / np.sqrt(K)
    return W, dims, ldims, cols, split


def pick_target(lg_row, wanted, delta):
    """the token nearest float64 rank `wanted` with no other logit within 4 delta"""
    order = np.argsort(-lg_row, kind="stable")
    s = lg_row[order]
    gap_up = np.concatenate([[np.inf], s[:-1] - s[1:]])
    gap_dn = np.concatenate([s[:-1] - s[1:], [np.inf]])
    ok = np.flatnonzero((gap_up > 4 * delta) & (gap_dn > 4 * delta))
    if ok.size == 0:
        return -1
    return int(order[ok[np.abs(ok - wanted).argmin()]])


def build(prec, K, V, seed):
    W, dims, ldims, cols, split = detail_weights(K, V)
    Wr = W if prec == 0 else round16(W, prec)
    Wb = np.ascontiguousarray(Wr) if prec == 0 else bits16(W, prec)
    rng = np.random.default_rng(seed)
    x = ln_input(rng, M_FULL, K)
    others = np.delete(np.arange(K), dims[3])
    x[:, dims[3]] = x[:, others].astype(np.float64).mean(1)      # the scale-80 column stays out of every other row
    x[ROW_EQUAL] = 1.5
    for row, d in ((ROW_FIRST, dims[0]), (ROW_LAST, dims[1]), (ROW_SPLIT, dims[2]), (ROW_SCALE80, dims[3]), (ROW_LADDER_A, ldims[0]),
                   (ROW_LADDER_B, ldims[1]), (ROW_LADDER_C, ldims[2])):
        x[row] = (0.1 * rng.standard_normal(K)).astype(np.float32)
        x[row, d] = 1000.0
        if d != dims[3]:
            x[row, dims[3]] = x[row, others].astype(np.float64).mean()
    ln_w = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    lg = ref_ln(x, ln_w) @ Wr.astype(np.float64).T
    maxabs = np.abs(lg).max(1)
    delta = BAR * np.maximum(1.0, maxabs)
    target = np.zeros(M_FULL, np.int32)
    want = wanted_ranks(V)
    for i in range(M_FULL):
        if i == ROW_EQUAL:
            target[i] = 11 % V
        elif i in (ROW_LADDER_A, ROW_LADDER_B, ROW_LADDER_C):
            target[i] = cols[i - ROW_LADDER_A][LADDER_POS]
        else:
            target[i] = pick_target(lg[i], want[i % len(want)], delta[i])
    return {"x": x, "ln_w": ln_w, "Wb": Wb, "target": target, "lg": lg, "delta": delta, "maxabs": maxabs, "cols": cols, "split": split}


def random_rows(M):
    return np.setdiff1d(np.arange(M), PLANTED)


def fragile_rows(c):
    """random rows where two of float64's 17 best logits are closer than FRAGILE max(1, max |logit|)"""
    top = -np.sort(-c["lg"], axis=1)[:, :17]
    return (top[:, :-1] - top[:, 1:]).min(1) <= FRAGILE * np.maximum(1.0, c["maxabs"])


def seed_ok(c):
    if (c["target"] < 0).any():
        return False
    f = fragile_rows(c)
    return f[random_rows(33)].sum() == 0 and f[random_rows(M_FULL)].sum() <= 0.02 * len(random_rows(M_FULL))


@functools.lru_cache(maxsize=None)
def case(prec, K, V):
    c = build(prec, K, V, SEEDS[(prec, K, V)])
    assert (c["target"] >= 0).all(), "a row without an isolated target"
    assert seed_ok(c), "the row seed leaves float64 itself short of the 2 % rule"
    lg, t = c["lg"], c["target"]
    rows = np.arange(M_FULL)
    tl = lg[rows, t]
    mx = lg.max(1)
    lse = mx + np.log(np.exp(lg - mx[:, None]).sum(1))
    p = np.exp(lg - lse[:, None])
    ref = {"rank": (lg > tl[:, None]).sum(1), "lse": lse, "order": np.argsort(-lg, axis=1, kind="stable")[:, :16]}
    ref["H"] = -(p * (lg - lse[:, None])).sum(1)
    not_t = np.ones_like(lg, bool)
    not_t[rows, t] = False
    d2 = 2 * c["delta"][:, None]
    for tau in TAUS:
        z = lg / tau
        q = np.exp(z - z.max(1, keepdims=True))
        q /= q.sum(1, keepdims=True)
        ref[f"L{tau}"] = (q * (lg > tl[:, None] + d2)).sum(1)
        ref[f"U{tau}"] = (q * ((lg > tl[:, None] - d2) & not_t)).sum(1)
        iso = np.setdiff1d(rows, [ROW_EQUAL])
        assert np.array_equal(ref[f"L{tau}"][iso], ref[f"U{tau}"][iso])
    # the fp32 summation term of the entropy bar: a float32 restatement of the centred sum on the same logits
    v = lg.astype(np.float32)
    cm = v - v.max(1, keepdims=True)
    e = np.exp(cm)
    S = e.sum(1, dtype=np.float32)
    H32 = np.log(S) - (e * cm).sum(1, dtype=np.float32) / S
    v64 = v.astype(np.float64)
    m64 = v64.max(1, keepdims=True)
    S64 = np.exp(v64 - m64).sum(1)
    H64 = np.log(S64) - (np.exp(v64 - m64) * (v64 - m64)).sum(1) / S64
    ref["c"] = 4 * np.abs(H32.astype(np.float64) - H64).max()
    # the planted rows are what they are meant to be
    for k, row in enumerate((ROW_LADDER_A, ROW_LADDER_B, ROW_LADDER_C)):
        assert np.array_equal(ref["order"][row], c["cols"][k]) and ref["rank"][row] == LADDER_POS
        top = lg[row][ref["order"][row]]
        assert (top[:-1] - top[1:]).min() > 4 * c["delta"][row] and top[-1] - np.sort(lg[row])[-17] > 4 * c["delta"][row]
    for row in (ROW_FIRST, ROW_LAST, ROW_SPLIT):
        assert ref["H"][row] < 5e-4, (row, ref["H"][row])
    assert c["maxabs"][ROW_SCALE80] > 150
    c["ref"] = ref
    return c


def run(prec, K, V, x, ln_w, Wb, target, topk=16, tau=0.7):
    M = x.shape[0]
    x = np.ascontiguousarray(x, dtype=np.float32)
    target = np.ascontiguousarray(target, dtype=np.int32)
    rank = np.zeros(M, np.int32)
    mass, ent = np.zeros(M, np.float32), np.zeros(M, np.float32)
    tok = np.zeros((M, topk), np.int32)
    tlp = np.zeros((M, topk), np.float32)
    check(lib().umgen_dbg_head_detail(prec, M, K, V, fp(x), K, fp(ln_w), vp(Wb), target.ctypes.data_as(i32p), topk, tau, rank.ctypes.data_as(i32p),
                                      fp(mass), fp(ent), tok.ctypes.data_as(i32p), fp(tlp)))      # (a changed guard band is UMGEN_E_STATE)
    return {"rank": rank, "mass": mass, "entropy": ent, "tok": tok, "tlp": tlp}


@functools.lru_cache(maxsize=None)
def full_run(prec, K, V, tau):
    c = case(prec, K, V)
    return run(prec, K, V, c["x"], c["ln_w"], c["Wb"], c["target"], tau=tau)


def check_rows(got, c, rows, tau, tag):
    """every bar of the docstring on `rows` (indices into the case); returns per row whether the token list equals float64's"""
    rows = np.asarray(rows)
    ref, lg, delta = c["ref"], c["lg"][rows], c["delta"][rows]
    for k in ("mass", "entropy", "tlp"):
        assert np.isfinite(got[k]).all(), (tag, k)
    assert np.array_equal(got["rank"], ref["rank"][rows]), (tag, "rank", got["rank"], ref["rank"][rows])
    lo = ref[f"L{tau}"][rows] * np.exp(-2 * delta / tau) - 1e-6
    hi = ref[f"U{tau}"][rows] * np.exp(2 * delta / tau) + 1e-6
    print(f"{tag} mass_above: max |got - float64| = {np.abs(got['mass'] - ref[f'L{tau}'][rows]).max():.3g}")
    assert ((got["mass"] >= lo) & (got["mass"] <= hi)).all(), (tag, "mass", got["mass"], lo, hi)
    H = ref["H"][rows]
    err = np.abs(got["entropy"] - H)
    bar = 2 * delta * (1 + H) + ref["c"]
    print(f"{tag} entropy: max error {err.max():.3g}, max error / bar = {(err / bar).max():.3g} (c = {ref['c']:.3g})")
    assert (err <= bar).all(), (tag, "entropy", int(rows[(err / bar).argmax()]), float(err.max()))
    tok = got["tok"].astype(np.int64)
    assert ((tok >= 0) & (tok < lg.shape[1])).all(), tag
    assert all(len(set(r)) == 16 for r in tok.tolist()), (tag, "distinct")
    at = np.take_along_axis(lg, tok, 1)
    best = -np.sort(-lg, axis=1)[:, :16]
    perr = np.abs(at - best) / delta[:, None]
    print(f"{tag} top-16 logits by position: max |lg64[tok] - sorted64| / delta = {perr.max():.3g}")
    assert perr.max() <= 2, (tag, "positional", float(perr.max()))
    lerr = np.abs(got["tlp"] - (at - ref["lse"][rows][:, None])) / np.maximum(1.0, c["maxabs"][rows])[:, None]
    print(f"{tag} topk_logp: max error / bar = {lerr.max() / (2 * BAR):.3g}")
    assert lerr.max() <= 2 * BAR, (tag, "topk_logp", float(lerr.max()))
    return (tok == ref["order"][rows]).all(1)


@pytest.mark.parametrize("M", [1, 33, M_FULL])
@pytest.mark.parametrize("K,V", SHAPES)
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_head_detail_against_float64(prec, K, V, M):
    c = case(prec, K, V)
    tag = f"prec {prec} K {K} V {V} M {M}"
    if M == 1:
        # one row alone: the bars, and the same bits as the row gives inside the launch of 70
        full = full_run(prec, K, V, 0.7)
        for row in (ROW_ALONE, ROW_SCALE80, 0):
            got = run(prec, K, V, c["x"][row:row + 1], c["ln_w"], c["Wb"], c["target"][row:row + 1])
            check_rows(got, c, [row], 0.7, f"{tag} row {row}")
            for k in got:
                assert got[k].tobytes() == full[k][row:row + 1].tobytes(), (tag, row, k, got[k], full[k][row])
        return
    exact = first = None
    for tau in TAUS:
        got = full_run(prec, K, V, tau) if M == M_FULL else run(prec, K, V, c["x"][:M], c["ln_w"], c["Wb"], c["target"][:M], tau=tau)
        exact = check_rows(got, c, np.arange(M), tau, f"{tag} tau {tau}")
        if tau != TAUS[0]:      # only mass_above depends on the temperature
            for k in ("rank", "entropy", "tok", "tlp"):
                assert got[k].tobytes() == first[k].tobytes(), (tag, k)
        first = got
    rr = random_rows(M)
    print(f"{tag}: token lists equal float64's on {int(exact[rr].sum())} of {len(rr)} random rows")
    assert (~exact[rr]).sum() <= 0.02 * len(rr), (tag, int((~exact[rr]).sum()))
    # all-equal logits: nothing lies above, the entropy of the uniform distribution, the lowest indices win the ties
    assert got["rank"][ROW_EQUAL] == 0 and got["mass"][ROW_EQUAL] == 0.0
    assert abs(got["entropy"][ROW_EQUAL] - np.log(V)) <= 2 * BAR
    assert got["tok"][ROW_EQUAL].tolist() == list(range(16))
    assert np.abs(got["tlp"][ROW_EQUAL] + np.log(V)).max() <= 2 * BAR
    # decisive maxima at the ends of the vocabulary and on a split's first column
    for row, col in ((ROW_FIRST, 0), (ROW_LAST, V - 1), (ROW_SPLIT, c["split"])):
        assert got["entropy"][row] < 1e-3 and got["tok"][row, 0] == col, (tag, row)
    # the ladders: exactly the planted columns in planted order, whichever levels of the fold they meet in
    for k, row in enumerate((ROW_LADDER_A, ROW_LADDER_B, ROW_LADDER_C)):
        assert got["tok"][row].tolist() == c["cols"][k], (tag, "ladder", k, got["tok"][row])
        assert got["rank"][row] == LADDER_POS
    if M == 33:      # a shorter list is the head of the long one
        five = run(prec, K, V, c["x"][:M], c["ln_w"], c["Wb"], c["target"][:M], topk=5, tau=TAUS[-1])
        assert five["tok"].tobytes() == np.ascontiguousarray(got["tok"][:, :5]).tobytes()
        assert five["tlp"].tobytes() == np.ascontiguousarray(got["tlp"][:, :5]).tobytes()
        for k in ("rank", "mass", "entropy"):
            assert five[k].tobytes() == got[k].tobytes(), k


def test_unsupported_width_is_refused():
    x = np.zeros((1, 64), np.float32)
    W = np.zeros((32, 64), np.float32)
    t = np.zeros(1, np.int32)
    o = np.zeros(16, np.float32)
    a = np.zeros(16, np.int32)
    assert lib().umgen_dbg_head_detail(0, 1, 64, 32, fp(x), 64, fp(x[0]), vp(W), t.ctypes.data_as(i32p), 16, 1.0, a.ctypes.data_as(i32p), fp(o), fp(o),
                                       a.ctypes.data_as(i32p), fp(o)) == -5


@pytest.mark.parametrize("V", [48, 56, 1028])
def test_logits_detail_on_given_logits(V):
    """one wave per row on explicit fp32 logits: rank and top-K exact against float64 on the same logits (ties by the lower index), mass and entropy
    within 1e-5; columns past V (3e4 planted) are never read"""
    M, ld, tau = 9, 1100, 0.7
    rng = np.random.default_rng(V)
    lg = np.full((M, ld), 3e4, np.float32)
    lg[:, :V] = (3.0 * rng.standard_normal((M, V))).astype(np.float32)
    lg[1, :V] = np.round(lg[1, :V])                 # many exact ties
    lg[2, :V] = 0.25                                # all equal
    lg[3, :V] = 80.0 * rng.standard_normal(V)       # scale 80
    target = rng.integers(0, V, M).astype(np.int32)
    target[0] = int(lg[0, :V].argmax())
    rank = np.zeros(M, np.int32)
    mass, ent = np.zeros(M, np.float32), np.zeros(M, np.float32)
    tok = np.zeros((M, 16), np.int32)
    tlp = np.zeros((M, 16), np.float32)
    check(lib().umgen_dbg_logits_detail(M, V, fp(lg), ld, target.ctypes.data_as(i32p), 16, tau, rank.ctypes.data_as(i32p), fp(mass), fp(ent),
                                        tok.ctypes.data_as(i32p), fp(tlp)))
    v = lg[:, :V].astype(np.float64)
    tl = v[np.arange(M), target]
    mx = v.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(v - mx).sum(1))
    p = np.exp(v - lse[:, None])
    q = np.exp((v - mx) / tau)
    q /= q.sum(1, keepdims=True)
    assert np.array_equal(rank, (v > tl[:, None]).sum(1))
    assert rank[0] == 0 and mass[0] == 0.0
    assert np.array_equal(tok, np.argsort(-v, axis=1, kind="stable")[:, :16])
    assert np.abs(mass - (q * (v > tl[:, None])).sum(1)).max() <= 1e-5
    assert np.abs(ent + (p * (v - lse[:, None])).sum(1)).max() <= 1e-5
    at = np.take_along_axis(v, tok.astype(np.int64), 1) - lse[:, None]
    assert np.abs(tlp - at).max() <= 2 * BAR * max(1.0, float(np.abs(v).max()))
