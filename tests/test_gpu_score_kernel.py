"""The scoring head (csrc/score.hip) through its hook umgen_dbg_head_nll: LayerNorm + head + log-softmax at the target per row, against float64.

Inputs: rows from gpu_util.ln_input, weights N(0, 0.02) rounded to the operand type before either side sees them, plus planted rows --
all-equal logits, a row whose logits have scale 80, decisive maxima on column 0, on column V - 1 and on the first column of the second
vocabulary split.  The planted rows are spikes on feature dimensions (LayerNorm turns a spike of any height into ~sqrt(K) on its dimension) whose
weight column is zero but for the planted entries, or -- the scale-80 column -- meets the row mean in every other row, so the other rows keep
ordinary logits.

Bars: target logit and log-sum-exp |got - ref| <= 1e-4 max(1, |ref|) -- GEMV_BAR of tests/test_gpu_decode_layer.py, the bar of the head's decode-step
kernel on the same inputs and contract (fp32 LayerNorm output x weights as stored, fp32 accumulation); logp within 2e-4 max(1, max |logit| of the
row) (a difference of two such quantities); arg-max equal to float64's wherever the float64 top-2 gap exceeds twice the logit bar."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.gpu_util import bits16, check, fp, lib, ln_input, ref_ln, round16, vp

pytestmark = pytest.mark.gpu

BAR = 1e-4
M_FULL = 70
ROW_EQUAL, ROW_SCALE80, ROW_FIRST, ROW_LAST, ROW_SPLIT = 1, 2, 3, 4, 5     # planted rows (inside M = 33 as well)
ROW_ALONE = 37                                                             # the row the M = 1 case runs alone
SHAPES = [(96, 1028), (768, 8192), (768, 1028), (1536, 8192)]
ROW_SEED = 8      # (with 28 random rows at M = 33 the 2 % rule on exempt rows admits none: a seed whose float64 top-2 gaps all clear the bar)


@functools.lru_cache(maxsize=None)
def weights(K, V):
    rng = np.random.default_rng(1000 * K + V)
    W = (0.02 * rng.standard_normal((V, K))).astype(np.float32)
    split = lib().umgen_dbg_head_nll_split(V)
    assert 0 < split < V and split % 16 == 0
    d_first, d_last, d_split, d_80 = 3, K // 2 + 1, K - 2, 17
    for d, v in ((d_first, 0), (d_last, V - 1), (d_split, split)):
        W[:, d] = 0.0
        W[v, d] = 30.0 / np.sqrt(K)
    W[:, d_80] = (80.0 / np.sqrt(K)) * rng.standard_normal(V)
    return W, (d_first, d_last, d_split, d_80), split


@functools.lru_cache(maxsize=None)
def case(prec, K, V):
    W, dims, split = weights(K, V)
    Wr = W if prec == 0 else round16(W, prec)
    Wb = np.ascontiguousarray(Wr) if prec == 0 else bits16(W, prec)
    rng = np.random.default_rng(ROW_SEED + K + V)
    x = ln_input(rng, M_FULL, K)
    others = np.delete(np.arange(K), dims[3])
    x[:, dims[3]] = x[:, others].astype(np.float64).mean(1)      # the scale-80 column stays out of every other row: its feature sits on the row mean
    x[ROW_EQUAL] = 1.5
    for row, d in ((ROW_FIRST, dims[0]), (ROW_LAST, dims[1]), (ROW_SPLIT, dims[2]), (ROW_SCALE80, dims[3])):
        x[row] = (0.1 * rng.standard_normal(K)).astype(np.float32)
        x[row, d] = 1000.0
    ln_w = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    target = rng.integers(0, V, M_FULL).astype(np.int32)
    target[0], target[ROW_FIRST], target[ROW_LAST], target[M_FULL - 1], target[ROW_ALONE] = 0, 0, V - 1, V - 1, V - 1
    lg = ref_ln(x, ln_w) @ Wr.astype(np.float64).T
    mx = lg.max(1)
    srt = np.sort(lg, axis=1)
    ref = {"tl": lg[np.arange(M_FULL), target], "lse": mx + np.log(np.exp(lg - mx[:, None]).sum(1)), "argmax": lg.argmax(1),
           "gap": srt[:, -1] - srt[:, -2], "maxabs": np.abs(lg).max(1)}
    ref["logp"] = ref["tl"] - ref["lse"]
    return {"x": x, "ln_w": ln_w, "Wb": Wb, "target": target, "ref": ref, "split": split}


def run(prec, K, V, x, ln_w, Wb, target):
    M = x.shape[0]
    x = np.ascontiguousarray(x, dtype=np.float32)
    target = np.ascontiguousarray(target, dtype=np.int32)
    logp, lse, tl = (np.zeros(M, np.float32) for _ in range(3))
    am = np.zeros(M, np.int32)
    check(lib().umgen_dbg_head_nll(prec, M, K, V, fp(x), K, fp(ln_w), vp(Wb), target.ctypes.data_as(C.POINTER(C.c_int32)), fp(logp),
                                   am.ctypes.data_as(C.POINTER(C.c_int32)), fp(lse), fp(tl)))      # (a changed guard band is UMGEN_E_STATE)
    return {"logp": logp, "lse": lse, "tl": tl, "argmax": am}


@functools.lru_cache(maxsize=None)
def full_run(prec, K, V):
    c = case(prec, K, V)
    return run(prec, K, V, c["x"], c["ln_w"], c["Wb"], c["target"])


def check_rows(got, ref, rows, tag):
    rows = np.asarray(rows)
    for k in ("logp", "lse", "tl"):
        assert np.isfinite(got[k]).all(), (tag, k)
    for k in ("tl", "lse"):
        err = np.abs(got[k] - ref[k][rows]) / np.maximum(1.0, np.abs(ref[k][rows]))
        print(f"{tag} {k}: max error / bar = {err.max() / BAR:.3f}")
        assert err.max() <= BAR, (tag, k, int(rows[err.argmax()]), float(err.max()))
    err = np.abs(got["logp"] - ref["logp"][rows]) / np.maximum(1.0, ref["maxabs"][rows])
    print(f"{tag} logp: max error / bar = {err.max() / (2 * BAR):.3f}")
    assert err.max() <= 2 * BAR, (tag, "logp", int(rows[err.argmax()]), float(err.max()))
    decided = ref["gap"][rows] > 2 * BAR * np.maximum(1.0, ref["maxabs"][rows])
    assert np.array_equal(got["argmax"][decided], ref["argmax"][rows][decided]), tag
    return decided


@pytest.mark.parametrize("M", [1, 33, M_FULL])
@pytest.mark.parametrize("K,V", SHAPES)
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_head_nll_against_float64(prec, K, V, M):
    c = case(prec, K, V)
    ref = c["ref"]
    tag = f"prec {prec} K {K} V {V} M {M}"
    if M == 1:
        # one row alone: the bars, and the SAME BITS as the row gives inside the launch of 70 (nothing of a row's result depends on M or on
        # the rows it shares a launch with)
        full = full_run(prec, K, V)
        for row in (ROW_ALONE, ROW_SCALE80, 0):
            got = run(prec, K, V, c["x"][row:row + 1], c["ln_w"], c["Wb"], c["target"][row:row + 1])
            check_rows(got, ref, [row], f"{tag} row {row}")
            for k in got:
                assert got[k].tobytes() == full[k][row:row + 1].tobytes(), (tag, row, k, got[k], full[k][row])
        return
    got = full_run(prec, K, V) if M == M_FULL else run(prec, K, V, c["x"][:M], c["ln_w"], c["Wb"], c["target"][:M])
    decided = check_rows(got, ref, np.arange(M), tag)
    planted = [ROW_EQUAL, ROW_SCALE80, ROW_FIRST, ROW_LAST, ROW_SPLIT]
    random_rows = np.setdiff1d(np.arange(M), planted)
    assert (~decided[random_rows]).sum() <= 0.02 * len(random_rows), (tag, int((~decided[random_rows]).sum()))
    # all-equal logits: log p = -log V whatever the target, the lowest index wins the tie
    assert got["argmax"][ROW_EQUAL] == 0 and got["tl"][ROW_EQUAL] == 0.0
    assert abs(got["logp"][ROW_EQUAL] + np.log(V)) <= 2 * BAR
    # decisive maxima at the ends of the vocabulary and on a split's first column; a row whose running maximum keeps rising by tens
    assert got["argmax"][ROW_FIRST] == 0 and got["argmax"][ROW_LAST] == V - 1 and got["argmax"][ROW_SPLIT] == c["split"]
    assert ref["gap"][ROW_FIRST] > 10 and ref["gap"][ROW_LAST] > 10 and ref["gap"][ROW_SPLIT] > 10
    assert abs(got["logp"][ROW_FIRST]) <= 2 * BAR and abs(got["logp"][ROW_LAST]) <= 2 * BAR      # their targets are the maxima
    assert ref["maxabs"][ROW_SCALE80] > 150, ref["maxabs"][ROW_SCALE80]


def test_unsupported_width_is_refused():
    x = np.zeros((1, 64), np.float32)
    W = np.zeros((32, 64), np.float32)
    t = np.zeros(1, np.int32)
    o = np.zeros(1, np.float32)
    a = np.zeros(1, np.int32)
    i32p = C.POINTER(C.c_int32)
    assert lib().umgen_dbg_head_nll(0, 1, 64, 32, fp(x), 64, fp(x[0]), vp(W), t.ctypes.data_as(i32p), fp(o), a.ctypes.data_as(i32p), fp(o), fp(o)) == -5
