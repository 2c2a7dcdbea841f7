"""Constrained generation end to end (umgen_rollout_biased / umgen_frame_biased; Engine.rollout(logit_bias=..., return_logz=True),
Engine.frame(logit_bias=..., logz=True)) on the tiny config with synthetic weights, T = 2.

References (none measured on the code under test):
  * the parent's own call: without tables, and with all-zero tables, tokens, lp and every diagnostic have the bits of umgen_rollout_detail;
  * the oracle's sampler on the rows the SAME call traced plus the class row, with the position's rng_uniform: the returned token, whatever the
    precision and the decode path; lp against the float64 log-softmax of the traced row (1e-4 * max(1, |ref|)), logz against float64
    (1e-4 * (max(1, |lse64(w)|) + max(1, |lse64(v)|)));
  * the fan-out contract and the eager frame: bit equality."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle.umgen_oracle import DRAW_MAIN, rng_uniform
from tests.golden.make_score_golden import TINY_SCENE
from tests.test_gpu_frame_kernels import BOX_C0, IMG_C0, KSEQ, MAP_C0, Walk, sampler_params
from tests.test_gpu_rollout_logp import BAR, assert_same_tokens, close_engines, engine, sampled  # noqa: F401
from tests.test_gpu_score import log_softmax_at
from umgen_amd import _lib, constraints, scene_io
from umgen_amd.config import CONTENT_LEN, MOD_ORDER
from umgen_amd.engine import UMGenError
from umgen_amd.synth import synthetic_control, synthetic_scene

pytestmark = pytest.mark.gpu
NEG = np.float32(-np.inf)
K = 4
ROWS = {"pose": 3, "map": 1, "bbox3d": 11, "image": 1}


def vocab_of(cfg):
    return {"pose": cfg.pose_vocab_size, "map": cfg.map_vocab_size, "bbox3d": cfg.bbox3d_vocab_size, "image": cfg.img_vocab_size}


def zero_tables(cfg):
    return {m: np.zeros(constraints.table_shape(m, V), np.float32) for m, V in vocab_of(cfg).items()}


def random_tables(cfg, seed):
    """finite bias in [-3, 3] with about 30 % of every row banned"""
    rng = np.random.default_rng(seed)
    out = {}
    for m, V in vocab_of(cfg).items():
        t = rng.uniform(-3, 3, (ROWS[m], V)).astype(np.float32)
        t[rng.random((ROWS[m], V)) < 0.3] = NEG
        t[:, 0] = 0.0
        out[m] = t.reshape(constraints.table_shape(m, V))
    return out


def biased(v, r):
    with np.errstate(invalid="ignore"):
        w = (np.asarray(v, np.float32) + np.asarray(r, np.float32)).astype(np.float32)
    return np.where(np.isneginf(r), NEG, w).astype(np.float32)


def lse64(rows):
    v = np.asarray(rows, np.float64)
    m = v.max(-1, keepdims=True)
    return (m + np.log(np.exp(v - m).sum(-1, keepdims=True)))[..., 0]


def scenes_of(n, first=60):
    sc = [synthetic_scene(TINY_SCENE + first + i, n_frames=2) for i in range(n)]
    return {m: np.concatenate([s[m] for s in sc]) for m in MOD_ORDER}


def same_bits(a, b, what):
    for m in MOD_ORDER:
        assert a[m].tobytes() == b[m].tobytes(), f"{what}: {m}"


@pytest.mark.parametrize("precision,B,N,nf", [("fp32", 1, None, 2), ("fp32", 2, 2, 2), ("bf16", 1, None, 2), ("bf16", 2, 2, 2), ("bf16", 24, None, 1)])
def test_null_and_zero_tables_are_the_parents_call(precision, B, N, nf):
    """umgen_rollout_biased with bias = NULL and with all-zero tables against umgen_rollout_detail: tokens, lp, every diagnostic bit for bit; logz is
    +0.0 at every sampled position.  bf16 at 24 scenes runs the batched decode layer on its lanes."""
    e = engine("tiny", precision, max_batch=B * (N or 1))
    sc = scenes_of(B)
    seeds = list(range(31, 31 + B * (N or 1)))
    kw = dict(cond_frames=3, input_cond_frames=2, seeds=seeds, sampling=sampled(e.cfg), samples=N, return_logp=True, return_detail=True, topk=K)
    out, lp, det = e.rollout(sc, nf, **kw)
    if B == 24:
        assert e.timings()["decode_batched"] == 1 and e.timings()["decode_lanes"] >= 2
    for tables in (None, zero_tables(e.cfg)):
        o2, lp2, lz2, det2 = e.rollout(sc, nf, logit_bias=tables, return_logz=True, **kw)
        assert_same_tokens(out, o2, "tokens")
        same_bits(lp, lp2, "lp")
        for k in det:
            same_bits(det[k], det2[k], k)
        for m in MOD_ORDER:
            assert lz2[m].shape == lp[m].shape and not lz2[m].view(np.uint32).any(), f"logz of {m} is not +0.0 everywhere"


def sampler_args(cfg, m):
    """(k, p) the sampler of class m takes"""
    if m == "map":
        return cfg.top_k_map, cfg.p_map
    if m == "image":
        return cfg.topk_image, float(cfg.topk_image)
    return cfg.top_k, cfg.p


def position_of(m, k):
    """1-based scene position of content token k of class m (the RNG's position; the pose draws sit behind the scene)"""
    return {"pose": KSEQ + k, "map": MAP_C0 + k + 1, "bbox3d": BOX_C0 + k + 1, "image": IMG_C0 + k + 1}[m]


@pytest.mark.parametrize("method", ["topk", "top_p"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_replay_on_the_traced_rows(precision, method):
    """the rows come from the run itself: OracleUMGen.sample(traced row + r) with the position's uniform is the returned token at every position of
    every class; lp is on the traced row, logz its float64 value"""
    e = engine("tiny", precision)
    smp = sampled(e.cfg, sample_method=method, only_ar=True, p=0.6, p_map=0.3)
    tabs = random_tables(e.cfg, 5)
    window = {m: a[0] for m, a in scenes_of(1).items()}
    seed, frame_idx = 77, 1
    toks, tr = e.frame(window, frame_idx=frame_idx, seed=seed, sampling=smp, trace=True, logp=True, logz=True, logit_bias=tabs)
    rows = dict(pose=tr["ego_logits"], map=tr["logits_map"], bbox3d=tr["logits_bbox3d"], image=tr["logits_image"])
    wk = Walk(sampler_params(method=0 if method == "topk" else 1, top_k=smp.top_k, top_k_map=smp.top_k_map, topk_image=smp.topk_image, p=smp.p,
                             p_map=smp.p_map, temperature=smp.sfmx_temp))
    for m in MOD_ORDER:
        k, p = sampler_args(smp, m)
        t = tabs[m].reshape(ROWS[m], -1)
        r = np.stack([t[i % ROWS[m]] for i in range(CONTENT_LEN[m])])
        w = biased(rows[m], r)
        want = [wk.sample(torch.from_numpy(w[i]), k, p, rng_uniform(seed, frame_idx, position_of(m, i), DRAW_MAIN)) for i in range(CONTENT_LEN[m])]
        np.testing.assert_array_equal(toks[m], np.array(want), err_msg=f"{m}: not the oracle's draw on traced row + r")
        assert not np.isneginf(r[np.arange(CONTENT_LEN[m]), toks[m]]).any()
        ref = log_softmax_at(rows[m], toks[m])
        err = np.abs(tr["logp"][m].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        assert np.isfinite(tr["logp"][m]).all() and err.max() <= BAR, (m, float(err.max()))
        a, b = lse64(w), lse64(rows[m])
        ez = np.abs(tr["logz"][m].astype(np.float64) - (a - b))
        print(f"{precision} {method} {m}: lp err {err.max():.3g}, logz err {ez.max():.3g}")
        assert (ez <= BAR * (np.maximum(1, np.abs(a)) + np.maximum(1, np.abs(b)))).all(), (m, float(ez.max()))


def test_graph_path_equals_the_eager_frame():
    """fp32: the first frame of a biased rollout (step graphs) and the traced, eagerly launched frame on the same window, seed and tables"""
    e = engine("tiny", "fp32")
    smp = sampled(e.cfg)
    tabs = random_tables(e.cfg, 6)
    sc = scenes_of(1)
    out, lz = e.rollout(sc, 1, cond_frames=3, input_cond_frames=2, seeds=[9], sampling=smp, logit_bias=tabs, return_logz=True)
    toks, tr = e.frame({m: a[0] for m, a in sc.items()}, frame_idx=0, seed=9, sampling=smp, trace=True, logz=True, logit_bias=tabs)
    for m in MOD_ORDER:
        np.testing.assert_array_equal(out[m][0, 2], toks[m], err_msg=m)
        assert lz[m][0, 0].tobytes() == tr["logz"][m].tobytes(), m


def test_bans_end_to_end():
    """no pedestrians and a pose envelope over two frames in bf16 with the rule constraint on; then the same call with a controlled pose"""
    e = engine("tiny", "bf16")
    smp = dataclasses.replace(sampled(e.cfg), rule_constrain=True)
    val = scene_io.decode_ego_numpy(np.repeat(np.arange(1024)[:, None], 3, axis=1)).reshape(1024, 3)
    lim = [tuple(sorted((float(val[400, c]), float(val[640, c])))) for c in range(3)]
    tabs = constraints.merge(constraints.ban_categories(["pedestrian"]), constraints.pose_limits(dx=lim[0], dy=lim[1], dheading=lim[2]))
    assert np.isneginf(tabs["pose"]).any() and np.isneginf(tabs["bbox3d"][10, 1026])
    sc = scenes_of(1, first=70)
    kw = dict(cond_frames=3, input_cond_frames=2, seeds=[4], sampling=smp, logit_bias=tabs, return_logz=True)
    out, lz = e.rollout(sc, 2, **kw)
    assert not (out["bbox3d"][:, 2:, 10::11] == 1026).any(), "a pedestrian category token was generated"
    pose = out["pose"][0, 2:]
    assert not np.isneginf(tabs["pose"][np.arange(3)[None], pose]).any(), "a pose token outside the envelope was generated"
    for m in ("pose", "bbox3d"):
        assert np.isfinite(lz[m]).all() and (lz[m] <= 0).all(), m
    for m in ("map", "image"):
        assert not lz[m].view(np.uint32).any(), m
    ctl = synthetic_control(3, n_frames=2, slot=None)["pose"]
    ctl[:] = 5                                                        # far outside the envelope
    assert np.isneginf(tabs["pose"][:, 5]).all()
    out, lz = e.rollout(sc, 2, init_tokens={"pose": ctl}, **kw)
    np.testing.assert_array_equal(out["pose"][:, 2:], ctl)
    assert np.isnan(lz["pose"]).all() and np.isfinite(lz["bbox3d"]).all()
    assert not (out["bbox3d"][:, 2:, 10::11] == 1026).any()


def test_fan_branches_are_the_replicated_biased_rollout():
    e = engine("tiny", "fp32", max_batch=3)
    smp = sampled(e.cfg)
    tabs = random_tables(e.cfg, 8)
    sc = scenes_of(1)
    kw = dict(cond_frames=3, input_cond_frames=2, sampling=smp, logit_bias=tabs, return_logp=True, return_logz=True)
    fan, flp, flz = e.rollout(sc, 2, seeds=[1, 2, 3], samples=3, **kw)
    rep, rlp, rlz = e.rollout({m: np.repeat(a, 3, axis=0) for m, a in sc.items()}, 2, seeds=[1, 2, 3], **kw)
    for m in MOD_ORDER:
        np.testing.assert_array_equal(fan[m][0], rep[m], err_msg=m)
        assert flp[m][0].tobytes() == rlp[m].tobytes() and flz[m][0].tobytes() == rlz[m].tobytes(), m
    assert e.last_shared_slots == 1


def unchecked_bias(tables):
    """the tables as the C call takes them, without Engine._bias_args' own checks"""
    if tables is None:
        return None, None
    keep = {m: np.ascontiguousarray(t, np.float32) for m, t in tables.items()}
    return _lib.LogitBias(**{m: a.ctypes.data_as(C.POINTER(C.c_float)) for m, a in keep.items()}), keep


def test_refusals_leave_the_engine_usable():
    e = engine("tiny", "fp32")
    smp = sampled(e.cfg)
    sc = scenes_of(1)
    kw = dict(cond_frames=3, input_cond_frames=2, seeds=[2], sampling=smp)
    before = e.rollout(sc, 1, **kw)
    V = vocab_of(e.cfg)
    nan_t, inf_t, none_t, last_t = (zero_tables(e.cfg) for _ in range(4))
    nan_t["map"][17] = np.nan
    inf_t["pose"][2, 33] = np.inf
    none_t["image"][:] = NEG
    last_t["bbox3d"][4, :V["bbox3d"] - 1] = NEG
    ctl = {"bbox3d": synthetic_control(3, n_frames=1)["bbox3d"]}
    cases = [(nan_t, {}, ("map", "row 0", "index 17")), (inf_t, {}, ("pose", "row 2", "index 33")), (none_t, {}, ("image", "row 0", "index")),
             (last_t, dict(init_tokens=ctl, control_test=True), ("bbox3d", "row 4", f"index {V['bbox3d'] - 1}"))]
    e._bias_args = lambda call, lb: unchecked_bias(lb)      # (the C library's own refusal: the wrapper's checks come first otherwise)
    try:
        for tabs, extra, words in cases:
            with pytest.raises(UMGenError) as err:
                e.rollout(sc, 1, logit_bias=tabs, **kw, **extra)
            assert "rc=-1" in str(err.value) and all(w in str(err.value) for w in words), str(err.value)
            assert_same_tokens(e.rollout(sc, 1, **kw), before, "a plain rollout behind a refused call")
        # the row that control slots refuse is fine without them
        e.rollout(sc, 1, logit_bias=last_t, **kw)
    finally:
        del e._bias_args
    # ... and the wrapper refuses the same tables before the C call
    for tabs in (nan_t, inf_t, none_t):
        with pytest.raises(UMGenError):
            e.rollout(sc, 1, logit_bias=tabs, **kw)
