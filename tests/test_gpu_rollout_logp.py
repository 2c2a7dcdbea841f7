"""Log-likelihoods of GENERATED frames (umgen_rollout_logp / umgen_frame_logp; Engine.rollout(return_logp=True), Engine.frame(logp=True)): the
value block_logp (csrc/frame.hip) takes from the AR row of the very decode step that sampled the token, on every decode path.

References and bars (none of them measured on the code under test):
  * float64 log-softmax of the logit rows the SAME call traced, at the scored tokens: 1e-4 x max(1, |ref|), the bar tests/test_gpu_score_kernel.py
    holds fp32 target-logit / log-sum-exp arithmetic to (the traced row is the row the sampler read);
  * the CPU oracle's decode-step anchor of tests/golden/score_*.npz: fp32 2e-3, 16-bit 2 x dist_{bf16,fp16} -- tests/test_gpu_score.py's bars.  The
    16-bit bar is BORROWED: the fixture's distance is that of the one-pass CPU restatement, not of a step-by-step one;
  * Engine.score of the generated frame (one pass, other summation order): 2e-3 in fp32, frames without a blanked slot only.
Measured on an MI355X: see DESIGN.md section 5.11."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from tests.golden.make_full_width_golden import WEIGHT_SEED, config as width_config
from tests.golden.make_score_golden import TINY_SCENE, TINY_WEIGHT_SEED
from tests.test_gpu_decode_engine import make_batched
from tests.test_gpu_score import golden_case, log_softmax_at
from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.synth import synthetic_control, synthetic_given_map, synthetic_scene
from umgen_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
BAR = 1e-4                # against float64 on the traced rows
FP32_ANCHOR_BAR = 2e-3    # tests/test_gpu_score.py
SLOT_LEN, PAD = 11, 1027
_engines = {}


def config_of(width):
    return tiny_config() if width == "tiny" else width_config(width)


def sampled(cfg, **over):
    """the reference's top-k sampling (5 / 5 / 16) without the rule constraint, whatever the engine's own config says"""
    return dataclasses.replace(cfg, **{**dict(sample_method="topk", top_k=5, top_k_map=5, topk_image=16, rule_constrain=False), **over})


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def engine(width, precision, max_batch=1, overlap=None):
    """overlap="0": created with UMGEN_OVERLAP=0 -- no background TAR pass on a second stream, so given tokens take the one-pass prefix (the default
    of engines that run the decode engine; fp32 engines overlap by default and replay the given positions as decode steps)"""
    key = (width, precision, max_batch, overlap)
    if key not in _engines:
        cfg = config_of(width)
        with env(**({} if overlap is None else {"UMGEN_OVERLAP": overlap})):
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


def rel_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def traced_rows(tr):
    return dict(pose=tr["ego_logits"], map=tr["logits_map"], bbox3d=tr["logits_bbox3d"], image=tr["logits_image"])


def window_of(out, T_in, cond_frames, idx):
    """the window umgen_rollout hands frame idx: the last min(cond_frames, T_in + idx) frames before it"""
    T_cur = T_in + idx
    return {m: out[m][0, max(0, T_cur - cond_frames):T_cur] for m in MOD_ORDER}


def assert_same_tokens(a, b, what):
    for m in MOD_ORDER:
        np.testing.assert_array_equal(a[m], b[m], err_msg=f"{what}: {m}")


def forced_frame_errors(e, width):
    """frame(window, forced = the fixture's scored frame, trace, logp) -> per modality (error against float64 on the call's own traced rows,
    max |logp - decode-step anchor|)"""
    g, window, frame, _ = golden_case(width)
    toks, tr = e.frame(window, frame_idx=0, forced=frame, trace=True, logp=True)
    rows = traced_rows(tr)
    res = {}
    for m in MOD_ORDER:
        lp = tr["logp"][m]
        assert lp.shape == (CONTENT_LEN[m],) and lp.dtype == np.float32 and np.array_equal(toks[m], frame[m])
        assert np.isfinite(lp).all() and (lp <= 0).all(), m
        res[m] = (rel_err(lp, log_softmax_at(rows[m], frame[m])), float(np.abs(lp - g[f"logp_{m}"]).max()))
    return g, res


@pytest.mark.parametrize("width", ["tiny", "full_width"])
def test_fp32_forced_frame_is_a_step_by_step_score(width):
    g, res = forced_frame_errors(engine(width, "fp32"), width)
    for m, (d_rows, d_anchor) in res.items():
        print(f"{width} fp32 {m}: vs float64 on the traced rows {d_rows:.3g} (bar {BAR}), max |logp - anchor| {d_anchor:.3g} (bar {FP32_ANCHOR_BAR})")
    for m, (d_rows, d_anchor) in res.items():
        assert d_rows <= BAR, (m, d_rows)
        assert d_anchor <= FP32_ANCHOR_BAR, (m, d_anchor)


@pytest.mark.parametrize("width", ["full_width", "deep"])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_16bit_forced_frame_against_the_decode_step_anchor(width, precision):
    """Measured on an MI355X, max |logp - anchor| over the modalities (bar = 2 x the fixture's dist): full_width bf16 4.5e-3 (9.9e-3), deep bf16 5.2e-3
    (1.25e-2), full_width fp16 5.2e-4 (1.19e-3), deep fp16 7.0e-4 (1.84e-3); against float64 on the call's own traced rows <= 1.8e-7 everywhere."""
    g, res = forced_frame_errors(engine(width, precision), width)
    bar = 2.0 * float(g[f"dist_{precision}"])
    for m, (d_rows, d_anchor) in res.items():
        print(f"{width} {precision} {m}: vs float64 on the traced rows {d_rows:.3g} (bar {BAR}), max |logp - anchor| {d_anchor:.3g} (borrowed bar {bar:.3g})")
    for m, (d_rows, d_anchor) in res.items():
        assert d_rows <= BAR, (m, d_rows)
    worst = max(d for _, d in res.values())
    assert worst <= bar, (worst, bar)


@pytest.mark.parametrize("width,precision", [("tiny", "fp32"), ("full_width", "bf16"), ("full_width", "fp16")])
def test_a_rollout_reproduces_itself_under_forcing(width, precision):
    """three sampled frames, B = 1, default engine settings (16-bit: the decode engine, its background workers from frame 1 on).  Every frame, forced
    onto the tokens the rollout generated and traced eagerly, gives the rows whose float64 log-softmax at those tokens is the rollout's logp."""
    e = engine(width, precision)
    smp = sampled(e.cfg)
    T_in, cf, nf = (2, 3, 3) if precision == "fp32" else (3, 3, 3)      # fp32: the window grows, then slides; 16-bit: it slides (the workers' case)
    scene = synthetic_scene(TINY_SCENE + 40, n_frames=T_in)
    kw = dict(cond_frames=cf, input_cond_frames=T_in, seeds=[11], sampling=smp)
    before = e.rollout(scene, nf, **kw)
    out, logp = e.rollout(scene, nf, return_logp=True, **kw)
    tm = e.timings()
    after = e.rollout(scene, nf, **kw)
    assert_same_tokens(before, out, "return_logp changed the tokens")
    assert_same_tokens(after, out, "a rollout behind a return_logp rollout differs")
    if precision != "fp32":
        assert tm["decode_engine"] == 1 and tm["overlapped_frames"] >= 1, tm
    worst = 0.0
    for idx in range(nf):
        gen = {m: out[m][0, T_in + idx] for m in MOD_ORDER}
        toks, tr = e.frame(window_of(out, T_in, cf, idx), frame_idx=idx, seed=11, sampling=smp, forced=gen, trace=True)
        rows = traced_rows(tr)
        for m in MOD_ORDER:
            lp = logp[m][0, idx]
            assert logp[m].shape == (1, nf, CONTENT_LEN[m]) and logp[m].dtype == np.float32
            assert np.isfinite(lp).all() and (lp <= 0).all(), (idx, m)
            d = rel_err(lp, log_softmax_at(rows[m], gen[m]))
            worst = max(worst, d)
            assert d <= BAR, (idx, m, d)
    print(f"{width} {precision}: rollout logp vs float64 on the forced frames' traced rows, max {worst:.3g} (bar {BAR})")


def test_batched_layer_and_lanes():
    """33 scenes on the batched decode layer (3 lanes by default, 1 with UMGEN_DECODE_LANES=1): the values do not depend on the lane layout nor on
    the batch, and asking for them does not change a token"""
    cfg = tiny_config(n_embd=768, n_head=16, rule_constrain=False)
    sd = synthetic_state_dict(cfg, seed=21)
    B = 33
    scenes = [synthetic_scene(40 + i, n_frames=2) for i in range(B)]
    both_in = {m: np.concatenate([s[m] for s in scenes]) for m in MOD_ORDER}
    seeds = [100 + i for i in range(B)]
    kw = dict(cond_frames=3, input_cond_frames=2, sampling=sampled(cfg))
    res = {}
    for lanes in (None, "1"):
        with env(**({} if lanes is None else {"UMGEN_DECODE_LANES": lanes})):
            e = make_batched(cfg, sd, 1, max_batch=B)
        try:
            res[lanes] = e.rollout(both_in, 2, seeds=seeds, return_logp=True, **kw)
            t = e.timings()
            assert t["decode_batched"] == 1 and t["decode_lanes"] == (3 if lanes is None else 1), t
            if lanes is None:
                plain = e.rollout(both_in, 2, seeds=seeds, **kw)
                single = {i: e.rollout(scenes[i], 2, seeds=[seeds[i]], return_logp=True, **kw) for i in (0, 16, 32)}
        finally:
            e.close()
    assert_same_tokens(plain, res[None][0], "return_logp changed the tokens")
    assert_same_tokens(res["1"][0], res[None][0], "lanes")
    for m in MOD_ORDER:
        lp = res[None][1][m]
        assert lp.shape == (B, 2, CONTENT_LEN[m]) and np.isfinite(lp).all() and (lp <= 0).all(), m
        assert lp.tobytes() == res["1"][1][m].tobytes(), f"{m}: logp differs between 3 lanes and 1"
        for i, (toks, one) in single.items():
            np.testing.assert_array_equal(toks[m], res[None][0][m][i:i + 1], err_msg=f"scene {i} {m}")
            assert one[m].tobytes() == lp[i:i + 1].tobytes(), f"{m}: logp of scene {i} alone differs from the batch"


@pytest.mark.parametrize("prefix_pass", [True, False])
def test_nan_sits_exactly_on_the_positions_without_a_head(prefix_pass):
    """given map, given map + boxes, controlled pose, control_test with one controlled slot per scene (B = 2, two new frames); once with the given
    positions as one prefix pass (an engine without the second-stream overlap) and once replayed as fixed-token decode steps (UMGEN_PREFIX_PASS=0)"""
    with env(**({} if prefix_pass else {"UMGEN_PREFIX_PASS": "0"})):
        e = engine("tiny", "fp32", max_batch=2, overlap="0")
        B, nf = 2, 2
        scenes = [synthetic_scene(60 + i, n_frames=2) for i in range(B)]
        cat = lambda ds: {k: np.concatenate([d[k] for d in ds]) for k in ds[0]}      # noqa: E731
        gm = cat([synthetic_given_map(60 + i, n_frames=nf) for i in range(B)])
        gb = cat([{"bbox3d": synthetic_scene(960 + i, n_frames=nf)["bbox3d"]} for i in range(B)])
        ctl = cat([synthetic_control(60 + i, n_frames=nf, slot=2 + i) for i in range(B)])
        cases = {"given map": (dict(init_tokens=gm), {"map"}),
                 "given map + boxes": (dict(init_tokens={**gm, **gb}), {"map", "bbox3d"}),
                 "controlled pose": (dict(init_tokens={"pose": ctl["pose"]}), {"pose"}),
                 "control_test": (dict(init_tokens=ctl, control_test=True), {"pose"})}      # a controlled slot is RESAMPLED (TAR head), scored on the AR row
        for name, (kw, nan_mods) in cases.items():
            out, logp = e.rollout(cat(scenes), nf, cond_frames=3, input_cond_frames=2, seeds=[5, 6], sampling=sampled(e.cfg), return_logp=True, **kw)
            if name.startswith("given"):
                assert e.timings()["prefix_passes"] == (nf if prefix_pass else 0), (name, e.timings())
            for m in MOD_ORDER:
                lp = logp[m]
                assert lp.shape == (B, nf, CONTENT_LEN[m])
                if m in nan_mods:
                    assert np.isnan(lp).all(), (name, m)
                else:
                    assert np.isfinite(lp).all() and (lp <= 0).all(), (name, m)


def test_rule_constraint_keeps_the_drawn_tokens_values():
    """rule_constrain = 1 on a frame that blanks a slot: the tokens do not depend on logp, every sampled position is finite, and everything in front
    of the first slot that CAN have been blanked (returned all-pad, no object in the previous frame) agrees with Engine.score of the returned frame"""
    e = engine("tiny", "fp32")
    smp = sampled(e.cfg, rule_constrain=True)
    scene = synthetic_scene(TINY_SCENE + 41, n_frames=2)
    window = {m: scene[m][0] for m in MOD_ORDER}
    found = None
    for seed in range(6):
        toks, tr = e.frame(window, seed=seed, sampling=smp, trace=True, logp=True)
        if tr["counters"]["rule_blanked"] > 0:
            found = (seed, toks, tr)
            break
    if found is None:
        pytest.skip("no seed in 0..5 blanks a slot on this scene (the kernel-level test_blanked_slots_* is the binding check)")
    seed, toks, tr = found
    plain, _ = e.frame(window, seed=seed, sampling=smp)
    assert_same_tokens(plain, toks, "logp changed the tokens")
    for m in MOD_ORDER:
        assert np.isfinite(tr["logp"][m]).all() and (tr["logp"][m] <= 0).all(), m
    slots = toks["bbox3d"].reshape(-1, SLOT_LEN)
    prev_cat = window["bbox3d"][-1].reshape(-1, SLOT_LEN)[:, SLOT_LEN - 1]
    first = int(np.nonzero((slots == PAD).all(1) & (prev_cat == PAD))[0][0])
    sc = e.score(window, toks)["logp"]
    for m, n in (("pose", 3), ("map", 1024), ("bbox3d", first * SLOT_LEN)):
        d = float(np.abs(tr["logp"][m][:n] - sc[m][:n]).max()) if n else 0.0
        print(f"rule constraint, seed {seed}, {tr['counters']['rule_blanked']} slots blanked, first candidate slot {first}: {m}[:{n}] max |logp - score| {d:.3g}")
        assert d <= FP32_ANCHOR_BAR, (m, d)


def test_rollout_logp_agrees_with_score_of_the_generated_frames():
    e = engine("tiny", "fp32")
    T_in, cf, nf = 2, 3, 2
    scene = synthetic_scene(TINY_SCENE + 42, n_frames=T_in)
    out, logp = e.rollout(scene, nf, cond_frames=cf, input_cond_frames=T_in, seeds=[3], sampling=sampled(e.cfg), return_logp=True)
    for idx in range(nf):
        sc = e.score(window_of(out, T_in, cf, idx), {m: out[m][0, T_in + idx] for m in MOD_ORDER})["logp"]
        for m in MOD_ORDER:
            d = float(np.abs(logp[m][0, idx] - sc[m]).max())
            print(f"frame {idx} {m}: max |rollout logp - score| {d:.3g} (bar {FP32_ANCHOR_BAR})")
            assert d <= FP32_ANCHOR_BAR, (idx, m, d)


def raw_rollout_logp(e, scene, B, T_in, nf, lp):
    """umgen_rollout_logp itself, past the Python wrapper -> (rc, message, out tokens)"""
    i64p = C.POINTER(C.c_int64)
    arrs = [np.ascontiguousarray(scene[m], dtype=np.int64) for m in MOD_ORDER]
    outs = [np.zeros((B, T_in + nf, CONTENT_LEN[m]), np.int64) for m in MOD_ORDER]
    smp, keep = e._sampling(sampled(e.cfg), [9] * B)
    rc = e.lib.umgen_rollout_logp(e._h, B, T_in, nf, 3, *[a.ctypes.data_as(i64p) for a in arrs], 0, None, None, 0, None, None, C.byref(smp),
                                  *[o.ctypes.data_as(i64p) for o in outs], lp)
    del keep
    return rc, e.lib.umgen_last_error(e._h).decode(), dict(zip(MOD_ORDER, outs))


def test_argument_handling():
    e = engine("tiny", "fp32")
    scene = synthetic_scene(TINY_SCENE + 43, n_frames=2)
    kw = dict(cond_frames=3, input_cond_frames=2, seeds=[9], sampling=sampled(e.cfg))
    ref, ref_lp = e.rollout(scene, 1, return_logp=True, **kw)
    # a struct of NULL members, and no struct: the old entry point
    for lp in (C.byref(_lib.LogpOut()), None):
        rc, msg, out = raw_rollout_logp(e, scene, 1, 2, 1, lp)
        assert rc == 0, msg
        assert_same_tokens(out, ref, "all-NULL umgen_logp_out")
    # some members NULL
    only, keep = e._logp_out((1, 1))
    part = _lib.LogpOut(logp_bbox3d=keep.logp_bbox3d)
    rc, msg, out = raw_rollout_logp(e, scene, 1, 2, 1, C.byref(part))
    assert rc == 0 and only["bbox3d"].tobytes() == ref_lp["bbox3d"].tobytes() and np.isnan(only["map"]).all()
    # a refused call leaves the outputs alone and the engine usable
    two = {m: np.concatenate([scene[m], scene[m]]) for m in MOD_ORDER}
    sent, lp = e._logp_out((2, 1))
    for a in sent.values():
        a[:] = 7.0
    rc, msg, _ = raw_rollout_logp(e, two, 2, 2, 1, C.byref(lp))
    assert rc == -1 and "B=2" in msg and all((a == 7.0).all() for a in sent.values())
    with pytest.raises(UMGenError):
        e.rollout(two, 1, return_logp=True, **dict(kw, seeds=[9, 9]))
    # a score call between two return_logp rollouts changes neither
    e.score({m: scene[m][0] for m in MOD_ORDER}, {m: ref[m][0, 2] for m in MOD_ORDER})
    again, again_lp = e.rollout(scene, 1, return_logp=True, **kw)
    assert_same_tokens(again, ref, "behind a score call")
    for m in MOD_ORDER:
        assert again_lp[m].tobytes() == ref_lp[m].tobytes(), m
    # frame(logp=True) without trace / forced / given: a trace dict with "logp" alone
    toks, tr = e.frame({m: scene[m][0] for m in MOD_ORDER}, seed=9, sampling=sampled(e.cfg), logp=True)
    assert set(tr) == {"logp"} and all(tr["logp"][m].tobytes() == ref_lp[m][0, 0].tobytes() for m in MOD_ORDER)
    assert_same_tokens({m: toks[m][None, None] for m in MOD_ORDER}, {m: ref[m][:, 2:] for m in MOD_ORDER}, "frame vs rollout")
