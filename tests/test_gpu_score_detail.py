"""umgen_score_detail on the engine (Engine.score(..., detail=True, topk=16)): rank, mass above, entropy and the 16 most likely tokens of every
scored position -- against float64 statistics of the same engine's teacher-forced trace rows, against the plain score call, across batch sizes,
around rollouts, and as the sampler's support on frames a rollout generated.

Bars.  fp32 against the trace: delta = 2e-3 is tests/test_gpu_score.py's fp32 bar for one-pass against step-by-step logits.  A logit error of delta
on both sides of a comparison moves the rank only across logits within 2 delta of the target's, a probability ratio by e^(2 delta / tau), the
log-sum-exp by delta and E_p(max - v) <= H by 2 delta H."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests.golden.make_full_width_golden import SCENE_ID, WEIGHT_SEED, config as width_config
from tests.golden.make_score_golden import TINY_SCENE, TINY_WEIGHT_SEED
from tests.test_gpu_score import golden_case, scenes
from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import Engine
from umgen_amd.score_stats import in_sampler_support
from umgen_amd.synth import synthetic_scene
from umgen_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
DELTA = 2e-3
TAU = 0.7
DETAIL = ("rank", "mass_above", "entropy", "topk_tokens", "topk_logp")
_engines = {}


def engine(width, precision, max_batch=1):
    key = (width, precision, max_batch)
    if key not in _engines:
        cfg = tiny_config() if width == "tiny" else width_config(width)
        e = Engine(cfg, precision=precision, max_batch=max_batch, max_cond_frames=4)
        e.load_state_dict(synthetic_state_dict(cfg, seed=TINY_WEIGHT_SEED if width == "tiny" else WEIGHT_SEED))
        e.finalize()
        _engines[key] = e
    return _engines[key]


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def vocab(e):
    return {"pose": e.cfg.pose_vocab_size, "map": e.cfg.map_vocab_size, "bbox3d": e.cfg.bbox3d_vocab_size, "image": e.cfg.img_vocab_size}


@pytest.mark.parametrize("width", ["tiny", "full_width"])
def test_fp32_detail_matches_float64_statistics_of_the_engines_own_trace(width):
    _, window, frame, _ = golden_case(width)
    e = engine(width, "fp32")
    res = e.score(window, frame, detail=True, topk=16, temperature=TAU)
    _, tr = e.frame(window, frame_idx=0, trace=True, forced=frame)
    traced = dict(pose=tr["ego_logits"], map=tr["logits_map"], bbox3d=tr["logits_bbox3d"], image=tr["logits_image"])
    for m in MOD_ORDER:
        lg = traced[m].astype(np.float64)
        S, V = lg.shape
        assert S == CONTENT_LEN[m] and res["rank"][m].shape == (S,) and res["rank"][m].dtype == np.int64
        assert res["topk_tokens"][m].shape == (S, 16) and res["topk_tokens"][m].dtype == np.int64 and res["topk_logp"][m].dtype == np.float32
        rows = np.arange(S)
        t = lg[rows, frame[m]][:, None]
        not_t = np.ones_like(lg, bool)
        not_t[rows, frame[m]] = False
        hi_set, lo_set = (lg > t - 2 * DELTA) & not_t, lg > t + 2 * DELTA
        rank = res["rank"][m]
        assert ((rank >= lo_set.sum(1)) & (rank <= hi_set.sum(1))).all(), (m, "rank")
        z = lg / TAU
        q = np.exp(z - z.max(1, keepdims=True))
        q /= q.sum(1, keepdims=True)
        lo = (q * lo_set).sum(1) * np.exp(-2 * DELTA / TAU) - 1e-6
        hi = (q * hi_set).sum(1) * np.exp(2 * DELTA / TAU) + 1e-6
        mass = res["mass_above"][m]
        assert ((mass >= lo) & (mass <= hi)).all(), (m, "mass_above")
        mx = lg.max(1, keepdims=True)
        lse = mx + np.log(np.exp(lg - mx).sum(1, keepdims=True))
        H = -(np.exp(lg - lse) * (lg - lse)).sum(1)
        err = np.abs(res["entropy"][m] - H) / (2 * DELTA * (1 + H))
        tok = res["topk_tokens"][m]
        n = min(16, V)
        assert all(len(set(r[:n])) == n for r in tok.tolist()), (m, "distinct")
        assert ((tok[:, :n] >= 0) & (tok[:, :n] < V)).all() and (tok[:, n:] == -1).all() and np.isneginf(res["topk_logp"][m][:, n:]).all()
        perr = np.abs(np.take_along_axis(lg, tok[:, :n], 1) - (-np.sort(-lg, axis=1)[:, :n])).max()
        print(f"{width} fp32 {m}: entropy max error / bar {err.max():.3g}; top-16 positional distance {perr:.3g} (bar {2 * DELTA}); "
              f"rank differs from the trace's at {int((rank != (lg > t).sum(1)).sum())} of {S} positions")
        assert err.max() <= 1.0, (m, "entropy", float(err.max()))
        assert perr <= 2 * DELTA, (m, "top-k", float(perr))


@pytest.mark.parametrize("width,precision", [("tiny", "fp32"), ("full_width", "bf16"), ("full_width", "fp16")])
def test_detail_is_consistent_with_the_plain_score(width, precision):
    _, window, frame, _ = golden_case(width)
    e = engine(width, precision)
    plain = e.score(window, frame)
    res = e.score(window, frame, detail=True, topk=16, temperature=TAU)
    assert set(res) == {"logp", "argmax", *DETAIL} and set(plain) == {"logp", "argmax"}
    V = vocab(e)
    for m in MOD_ORDER:
        assert res["logp"][m].tobytes() == plain["logp"][m].tobytes() and np.array_equal(res["argmax"][m], plain["argmax"][m]), m
        tok, tlp, rank, logp = res["topk_tokens"][m], res["topk_logp"][m], res["rank"][m], res["logp"][m]
        assert np.array_equal(tok[:, 0], res["argmax"][m]), m
        assert (tlp[:, :-1] >= tlp[:, 1:]).all(), m
        listed = np.flatnonzero((rank < 16) & np.array([len(set(r)) == 16 for r in tlp.tolist()]))
        print(f"{width} {precision} {m}: {listed.size} of {rank.size} targets are listed among the 16")
        assert np.array_equal(tok[listed, rank[listed]], np.asarray(frame[m])[listed]), m
        assert tlp[listed, rank[listed]].tobytes() == logp[listed].tobytes(), m
        mass, ent = res["mass_above"][m], res["entropy"][m]
        assert ((mass >= 0) & (mass <= 1)).all(), m
        assert (mass[rank == 0] == 0).all() and ((rank >= 0) & (rank < V[m])).all(), m
        assert ((ent >= 0) & (ent <= np.log(V[m]) + 1e-4)).all(), (m, float(ent.min()), float(ent.max()))
    # only mass_above depends on the temperature; a shorter list is the head of the long one
    other = e.score(window, frame, detail=True, topk=5, temperature=1.0)
    for m in MOD_ORDER:
        for k in ("rank", "entropy"):
            assert other[k][m].tobytes() == res[k][m].tobytes(), (k, m)
        assert np.array_equal(other["topk_tokens"][m], res["topk_tokens"][m][:, :5])
        assert other["topk_logp"][m].tobytes() == np.ascontiguousarray(res["topk_logp"][m][:, :5]).tobytes()
    assert not np.array_equal(other["mass_above"]["map"], res["mass_above"]["map"])
    few = e.score(window, frame, detail=("entropy",))
    assert set(few) == {"logp", "argmax", "entropy"} and few["entropy"]["image"].tobytes() == res["entropy"]["image"].tobytes()


@pytest.mark.parametrize("width,precision", [("full_width", "bf16"), ("tiny", "fp32")])
def test_a_batch_equals_its_one_scene_calls_bit_for_bit(width, precision):
    e = engine(width, precision, max_batch=3)
    window, frame = scenes(3)
    both = e.score(window, frame, detail=True, topk=16, temperature=TAU)
    for i in range(3):
        one = e.score({m: window[m][i] for m in MOD_ORDER}, {m: frame[m][i] for m in MOD_ORDER}, detail=True, topk=16, temperature=TAU)
        for kind in ("logp", "argmax", *DETAIL):
            for m in MOD_ORDER:
                assert both[kind][m].shape[:2] == (3, CONTENT_LEN[m])
                assert both[kind][m][i].tobytes() == one[kind][m].tobytes(), (kind, m, i)
    assert not np.array_equal(both["entropy"]["map"][0], both["entropy"]["map"][1])


def sampled(cfg):
    return dataclasses.replace(cfg, sample_method="topk", top_k=5, top_k_map=5, topk_image=16, rule_constrain=False)


def test_a_rollout_behind_a_detail_call_is_unchanged_and_the_tokens_lie_in_the_samplers_support():
    e = engine("tiny", "fp32")
    T_in, cf, nf = 2, 3, 2
    scene = synthetic_scene(TINY_SCENE + 40, n_frames=T_in)
    kw = dict(cond_frames=cf, input_cond_frames=T_in, seeds=[11], sampling=sampled(e.cfg))
    before = e.rollout(scene, nf, **kw)
    window, frame = scenes(1)
    a = e.score(window, frame, detail=True, topk=16, temperature=TAU)
    after = e.rollout(scene, nf, **kw)
    b = e.score(window, frame, detail=True, topk=16, temperature=TAU)
    for m in MOD_ORDER:
        np.testing.assert_array_equal(before[m], after[m], err_msg=m)
        for k in a:
            assert a[k][m].tobytes() == b[k][m].tobytes(), (k, m)
    # every generated map / image token was drawn from the top-k of its decode step's row: under the one-pass rows it lies inside that support up to
    # the one-pass / step-by-step logit distance (2e-3 on each of the two logits compared)
    for idx in range(nf):
        T_cur = T_in + idx
        w = {m: after[m][0, max(0, T_cur - cf):T_cur] for m in MOD_ORDER}
        gen = {m: after[m][0, T_cur] for m in MOD_ORDER}
        res = e.score(w, gen, topk=16)
        for m, k in (("map", 5), ("image", 16)):
            slack = res["logp"][m] - (res["topk_logp"][m][:, k - 1] - 2 * DELTA)
            inside = in_sampler_support(res["rank"][m], res["mass_above"][m], "topk", top_k=k)
            print(f"frame {idx} {m}: {int(inside.sum())} of {inside.size} tokens have rank < {k}; min logp - (k-th logp - 4e-3) = {slack.min():.3g}")
            assert (slack >= 0).all(), (idx, m, float(slack.min()))


def test_the_c_entry_point_refuses_bad_detail_arguments_and_takes_null_outputs():
    e = engine("tiny", "fp32")
    window, frame = scenes(1)
    ref = e.score(window, frame, detail=True, topk=4, temperature=TAU)
    p64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    toks = [np.ascontiguousarray(window[m], dtype=np.int64) for m in MOD_ORDER] + [np.ascontiguousarray(frame[m], dtype=np.int64) for m in MOD_ORDER]
    rank = np.zeros(CONTENT_LEN["map"], np.int32)
    tlp = np.zeros((CONTENT_LEN["image"], 4), np.float32)
    det = _lib.ScoreDetailOut(rank_map=rank.ctypes.data_as(C.POINTER(C.c_int32)), topk_logp_image=tlp.ctypes.data_as(C.POINTER(C.c_float)))

    def call(topk, temp, out, detail):
        return e.lib.umgen_score_detail(e._h, 1, 2, *[p64(a) for a in toks], topk, temp, out, detail)
    assert call(4, TAU, None, C.byref(det)) == 0      # no umgen_score_out, most detail pointers NULL
    assert np.array_equal(rank, ref["rank"]["map"][0]) and tlp.tobytes() == ref["topk_logp"]["image"][0].tobytes()
    for args in ((17, TAU), (-1, TAU), (4, 0.0), (4, -1.0), (4, float("nan")), (4, float("inf")), (0, TAU)):      # (0: a top-K pointer is set)
        assert call(*args, None, C.byref(det)) == -1, args
    assert call(4, TAU, None, None) == -1
    again = e.score(window, frame, detail=True, topk=4, temperature=TAU)      # the engine still answers the same
    assert all(again[k][m].tobytes() == ref[k][m].tobytes() for k in ref for m in MOD_ORDER)
