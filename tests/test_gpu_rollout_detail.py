"""Diagnostics of GENERATED frames (umgen_rollout_detail / umgen_frame_detail; Engine.rollout(return_detail=True, topk=K), Engine.frame(detail=True)):
rank, mass_above, entropy and the K most likely tokens that block_detail (csrc/frame.hip) takes from the AR row of the very decode step that
sampled the token, on every decode path.

References and bars (none of them measured on the code under test):
  * float64 statistics of the logit rows the SAME call traced (or, for a rollout, of the same frames forced and traced eagerly), at the scored
    tokens: rank, the listed tokens and "is the token listed" exact; the rest inside the bars of tests/test_gpu_detail_kernel.py;
  * Engine.score(detail=True) of the same frame in fp32 (one pass, another summation order): entropy and topk_logp inside 2e-3 (tests/test_gpu_score.py's
    bar), rank equal wherever the call's own traced row has no other logit within 2e-3 of the token's; such positions are counted and may be at most
    1 % of 2199.  The frame is tests/golden/detail_tiny.npz (make_detail_golden.py says why the recorded frame of score_tiny.npz cannot serve).
Measured on an MI355X: see DESIGN.md section 5.17."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.golden.make_score_golden import TINY_SCENE
from tests.test_gpu_decode_engine import make, make_batched
from tests.test_gpu_detail_kernel import check_against_float64
from tests.test_gpu_rollout_logp import (FP32_ANCHOR_BAR, PAD, SLOT_LEN, assert_same_tokens, close_engines, config_of, engine, env, sampled,  # noqa: F401
                                         traced_rows, window_of)
from tests.test_gpu_score import golden_case
from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.score_stats import in_sampler_support
from umgen_amd.synth import synthetic_control, synthetic_given_map, synthetic_scene
from umgen_amd.weights import synthetic_state_dict
from tests.golden.make_full_width_golden import WEIGHT_SEED

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("rank", "mass_above", "entropy", "topk_tokens", "topk_logp")
K = 16


def as_kernel_names(det, m, at=()):
    """a detail dict's arrays of modality m (indexed by `at` in front of [S_mod]) under the names check_against_float64 reads"""
    return {"rank": det["rank"][m][at], "mass": det["mass_above"][m][at], "ent": det["entropy"][m][at], "tok": det["topk_tokens"][m][at],
            "tlp": det["topk_logp"][m][at]}


def assert_same_bits(a, b, what):
    for k in a:
        for m in a[k]:
            assert a[k][m].tobytes() == b[k][m].tobytes(), f"{what}: {k} {m}"


def check_frame_on_rows(tag, rows, tokens, det, logp, tau, at=()):
    """one frame's diagnostics against float64 on its rows; where the token is listed its topk_logp has logp's bits"""
    for m in MOD_ORDER:
        got = as_kernel_names(det, m, at)
        check_against_float64(f"{tag} {m}", rows[m], np.asarray(tokens[m]), tau, got)
        listed = got["tok"] == np.asarray(tokens[m])[:, None]
        lp = logp[m][at]
        for r in np.flatnonzero(listed.any(1)):
            assert got["tlp"][r, int(np.argmax(listed[r]))].tobytes() == lp[r].tobytes(), (tag, m, r)


@pytest.mark.parametrize("width,precision", [("tiny", "fp32"), ("full_width", "bf16"), ("full_width", "fp16")])
def test_a_forced_frame_against_float64_on_its_own_traced_rows(width, precision):
    e = engine(width, precision)
    _, window, frame, _ = golden_case(width)
    smp = sampled(e.cfg, sfmx_temp=0.7)
    toks, tr = e.frame(window, frame_idx=0, forced=frame, trace=True, logp=True, detail=True, topk=K, sampling=smp)
    assert tuple(tr["detail"]) == KEYS and all(np.array_equal(toks[m], frame[m]) for m in MOD_ORDER)
    for m in MOD_ORDER:
        assert tr["detail"]["rank"][m].shape == (CONTENT_LEN[m],) and tr["detail"]["topk_logp"][m].shape == (CONTENT_LEN[m], K)
    check_frame_on_rows(f"{width} {precision} forced", traced_rows(tr), frame, tr["detail"], tr["logp"], 0.7)
    # the same call without detail: the same logp bits
    _, tr2 = e.frame(window, frame_idx=0, forced=frame, trace=True, logp=True, sampling=smp)
    assert all(tr2["logp"][m].tobytes() == tr["logp"][m].tobytes() for m in MOD_ORDER)


def test_fp32_forced_frame_agrees_with_score_detail():
    e = engine("tiny", "fp32")
    _, window, _, _ = golden_case("tiny")
    g = np.load(os.path.join(GOLD, "detail_tiny.npz"))
    frame = {m: g[f"tok_{m}"].astype(np.int64) for m in MOD_ORDER}
    toks, tr = e.frame(window, frame_idx=0, forced=frame, trace=True, logp=True, detail=True, topk=K, sampling=sampled(e.cfg))
    sc = e.score(window, frame, detail=True, topk=K, temperature=1.0)
    rows = traced_rows(tr)
    excluded = 0
    for m in MOD_ORDER:
        d_ent = float(np.abs(tr["detail"]["entropy"][m] - sc["entropy"][m]).max())
        d_tlp = float(np.abs(tr["detail"]["topk_logp"][m] - sc["topk_logp"][m]).max())
        lg = rows[m].astype(np.float64)
        t = lg[np.arange(lg.shape[0]), frame[m]][:, None]
        near = ((np.abs(lg - t) <= FP32_ANCHOR_BAR).sum(1) - 1) > 0
        excluded += int(near.sum())
        same = tr["detail"]["rank"][m][~near] == sc["rank"][m][~near]
        print(f"{m}: entropy {d_ent:.3g}, topk_logp {d_tlp:.3g} (bar {FP32_ANCHOR_BAR}); {int(near.sum())} positions excluded, rank equal on {int(same.sum())} of {same.size}")
        assert d_ent <= FP32_ANCHOR_BAR and d_tlp <= FP32_ANCHOR_BAR, (m, d_ent, d_tlp)
        assert same.all(), (m, np.flatnonzero(~same)[:5])
    print(f"excluded {excluded} of 2199 (the oracle's rows: {int(g['near'])})")
    assert excluded <= 0.01 * 2199, excluded


def rollout_checks(e, scenes, seeds, T_in, cf, nf, tau=1.0, alone=True):
    """a sampled rollout with detail: tokens and logp have the bits of the call without detail; every frame's detail equals float64 on the rows of the
    same frame forced and traced eagerly; a scene alone has the bits it has in the batch; every map / image token lies inside its sampler's support"""
    B = len(scenes)
    smp = sampled(e.cfg, sfmx_temp=tau)
    both = {m: np.concatenate([s[m] for s in scenes]) for m in MOD_ORDER}
    kw = dict(cond_frames=cf, input_cond_frames=T_in, sampling=smp)
    plain, plain_lp = e.rollout(both, nf, seeds=seeds, return_logp=True, **kw)
    out, logp, det = e.rollout(both, nf, seeds=seeds, return_logp=True, return_detail=True, topk=K, **kw)
    tm = e.timings()
    bare, bare_det = e.rollout(both, nf, seeds=seeds, return_detail=True, topk=K, **kw)
    assert_same_tokens(plain, out, "return_detail changed the tokens")
    assert_same_tokens(bare, out, "return_detail without return_logp")
    assert_same_bits(det, bare_det, "detail with and without logp")
    for m in MOD_ORDER:
        assert logp[m].tobytes() == plain_lp[m].tobytes(), f"return_detail changed logp: {m}"
        assert det["rank"][m].shape == (B, nf, CONTENT_LEN[m]) and det["topk_tokens"][m].shape == (B, nf, CONTENT_LEN[m], K)
    for b in range(B):
        one = {m: out[m][b:b + 1] for m in MOD_ORDER}
        for idx in range(nf):
            gen = {m: out[m][b, T_in + idx] for m in MOD_ORDER}
            _, tr = e.frame(window_of(one, T_in, cf, idx), frame_idx=idx, seed=seeds[b], sampling=smp, forced=gen, trace=True)
            check_frame_on_rows(f"scene {b} frame {idx}", traced_rows(tr), gen, det, logp, tau, at=(b, idx))
        if alone and B > 1:
            o1, l1, d1 = e.rollout(scenes[b], nf, seeds=[seeds[b]], return_logp=True, return_detail=True, topk=K, **kw)
            assert_same_tokens(o1, one, f"scene {b} alone")
            assert_same_bits(d1, {k: {m: det[k][m][b:b + 1] for m in MOD_ORDER} for k in KEYS}, f"scene {b} alone differs from scene {b} of the batch")
    # the sampler's support, exact here: rank is counted on the row the sampler drew from
    assert in_sampler_support(det["rank"]["map"], det["mass_above"]["map"], "topk", top_k=smp.top_k_map).all()
    assert in_sampler_support(det["rank"]["image"], det["mass_above"]["image"], "topk", top_k=smp.topk_image).all()
    assert in_sampler_support(det["rank"]["pose"], det["mass_above"]["pose"], "topk", top_k=smp.top_k).all()
    return tm


def test_fp32_sampled_rollout_of_two_scenes():
    e = engine("tiny", "fp32", max_batch=2)
    rollout_checks(e, [synthetic_scene(TINY_SCENE + 50 + i, n_frames=2) for i in range(2)], [21, 22], 2, 3, 2, tau=0.7)


def test_fan_branches_are_the_replicated_rollout():
    e = engine("tiny", "fp32", max_batch=6)
    B, N, T_in, nf = 2, 3, 2, 2
    scenes = [synthetic_scene(TINY_SCENE + 60 + i, n_frames=T_in) for i in range(B)]
    both = {m: np.concatenate([s[m] for s in scenes]) for m in MOD_ORDER}
    rep = {m: np.repeat(both[m], N, axis=0) for m in MOD_ORDER}
    seeds = np.arange(B * N)
    kw = dict(cond_frames=3, input_cond_frames=T_in, sampling=sampled(e.cfg), return_logp=True, return_detail=True, topk=K)
    out, logp, det = e.rollout(both, nf, seeds=seeds.reshape(B, N), samples=N, **kw)
    assert e.last_shared_slots == T_in - 1
    r_out, r_logp, r_det = e.rollout(rep, nf, seeds=seeds, **kw)
    for m in MOD_ORDER:
        assert out[m].reshape(r_out[m].shape).tobytes() == r_out[m].tobytes() and logp[m].tobytes() == r_logp[m].tobytes(), m
        for k in KEYS:
            assert det[k][m].shape[:2] == (B, N) and det[k][m].tobytes() == r_det[k][m].tobytes(), (k, m)
            assert np.isfinite(det[k][m]).all() and (k not in ("rank", "topk_tokens") or (det[k][m] >= 0).all()), (k, m)


PATHS = {"five_launch": ("bf16", 2, lambda cfg, sd, B: make(cfg, sd, engine_on=False, max_batch=B)),
         "engine_with_workers": ("bf16", 1, lambda cfg, sd, B: new_engine(cfg, sd, "bf16", B, {})),
         "engine_without_workers": ("fp16", 1, lambda cfg, sd, B: new_engine(cfg, sd, "fp16", B, {"UMGEN_BG_ENGINE": "0"})),
         "batched_layer": ("fp16", 2, lambda cfg, sd, B: make_batched(cfg, sd, 1, max_batch=B, precision="fp16"))}


def new_engine(cfg, sd, precision, B, kv):
    with env(**kv):
        e = Engine(cfg, precision=precision, max_batch=B, max_cond_frames=4)
    e.load_state_dict(sd)
    e.finalize()
    return e


@pytest.mark.parametrize("path", sorted(PATHS))
def test_16bit_decode_paths(path):
    """the rollout checks on each 16-bit decode path at production width: three frames behind a full window of 3, so that the one-scene engine's later
    frames find their history pushed by the background workers"""
    precision, B, build = PATHS[path]
    cfg = config_of("full_width")
    e = build(cfg, synthetic_state_dict(cfg, seed=WEIGHT_SEED), B)
    try:
        tm = rollout_checks(e, [synthetic_scene(TINY_SCENE + 70 + i, n_frames=3) for i in range(B)], [31 + i for i in range(B)], 3, 3, 2, alone=(path == "batched_layer"))
    finally:
        e.close()
    if path == "five_launch":
        assert tm["decode_engine"] == 0 and tm["decode_batched"] == 0, tm
    elif path == "batched_layer":
        assert tm["decode_batched"] == 1, tm
    else:
        assert tm["decode_engine"] == 1 and (tm["overlapped_frames"] >= 1) == (path == "engine_with_workers"), tm


def is_fill(det, m, at=()):
    return ((det["rank"][m][at] == -1).all() and (det["topk_tokens"][m][at] == -1).all() and np.isnan(det["mass_above"][m][at]).all()
            and np.isnan(det["entropy"][m][at]).all() and np.isnan(det["topk_logp"][m][at]).all())


def is_written(det, m, at=()):
    return ((det["rank"][m][at] >= 0).all() and (det["topk_tokens"][m][at] >= 0).all() and np.isfinite(det["mass_above"][m][at]).all()
            and np.isfinite(det["entropy"][m][at]).all() and np.isfinite(det["topk_logp"][m][at]).all())


@pytest.mark.parametrize("prefix_pass", [True, False])
def test_given_and_controlled_positions_carry_the_fill(prefix_pass):
    """given map (one prefix pass, or replayed as fixed-token steps with UMGEN_PREFIX_PASS=0) and a controlled pose: -1 / NaN exactly where logp is NaN;
    everything behind the given prefix -- its first sampled position included -- against float64 on the traced rows"""
    with env(**({} if prefix_pass else {"UMGEN_PREFIX_PASS": "0"})):
        e = engine("tiny", "fp32", max_batch=2, overlap="0")
        smp = sampled(e.cfg)
        scene = synthetic_scene(60, n_frames=2)
        window = {m: scene[m][0] for m in MOD_ORDER}
        gm = synthetic_given_map(60, n_frames=1)["map"][0, 0]
        before = e.timings()["prefix_passes"]
        toks, tr = e.frame(window, seed=5, sampling=smp, given={"map": gm}, trace=True, logp=True, detail=True, topk=K)
        assert e.timings()["prefix_passes"] - before == (1 if prefix_pass else 0)
        det = tr["detail"]
        assert is_fill(det, "map") and np.isnan(tr["logp"]["map"]).all() and np.array_equal(toks["map"], gm)
        rows = traced_rows(tr)
        for m in ("pose", "bbox3d", "image"):
            assert is_written(det, m), m
            got = as_kernel_names(det, m)
            check_against_float64(f"given map, prefix pass {prefix_pass}: {m}", rows[m], toks[m], 1.0, got)
        # B = 2, two frames: given map + boxes, a controlled pose
        B, nf = 2, 2
        scenes = [synthetic_scene(60 + i, n_frames=2) for i in range(B)]
        cat = lambda ds: {k: np.concatenate([d[k] for d in ds]) for k in ds[0]}      # noqa: E731
        gmb = cat([synthetic_given_map(60 + i, n_frames=nf) for i in range(B)])
        gbb = cat([{"bbox3d": synthetic_scene(960 + i, n_frames=nf)["bbox3d"]} for i in range(B)])
        ctl = cat([synthetic_control(60 + i, n_frames=nf, slot=2 + i) for i in range(B)])
        for name, kw, fill in (("given map + boxes", dict(init_tokens={**gmb, **gbb}), {"map", "bbox3d"}),
                               ("controlled pose", dict(init_tokens={"pose": ctl["pose"]}), {"pose"})):
            out, logp, det = e.rollout(cat(scenes), nf, cond_frames=3, input_cond_frames=2, seeds=[5, 6], sampling=smp, return_logp=True,
                                       return_detail=True, topk=4, **kw)
            for m in MOD_ORDER:
                assert det["topk_logp"][m].shape == (B, nf, CONTENT_LEN[m], 4)
                assert (is_fill if m in fill else is_written)(det, m), (name, m)
                assert np.isnan(logp[m]).all() == (m in fill), (name, m)


def test_blanked_slot_keeps_the_diagnostics_of_the_drawn_tokens():
    """rule_constrain = 1 on a frame that blanks a slot: the returned tokens are pads, the 11 positions keep finite diagnostics, and at the slot's last
    position the listed token whose topk_logp has logp's bits -- the token that was drawn -- is not pad"""
    e = engine("tiny", "fp32")
    smp = sampled(e.cfg, rule_constrain=True)
    scene = synthetic_scene(TINY_SCENE + 41, n_frames=2)
    window = {m: scene[m][0] for m in MOD_ORDER}
    found = None
    for seed in range(12):
        toks, tr = e.frame(window, seed=seed, sampling=smp, trace=True, logp=True, detail=True, topk=K)
        if tr["counters"]["rule_blanked"] > 0:
            found = (seed, toks, tr)
            break
    assert found is not None, "no seed in 0..11 blanks a slot on this scene"
    seed, toks, tr = found
    plain, _ = e.frame(window, seed=seed, sampling=smp)
    assert_same_tokens(plain, toks, "detail changed the tokens")
    det, lp = tr["detail"], tr["logp"]["bbox3d"]
    assert is_written(det, "bbox3d")
    rows = tr["logits_bbox3d"]
    slots = toks["bbox3d"].reshape(-1, SLOT_LEN)
    blanked = 0
    for s in np.flatnonzero((slots == PAD).all(1)):
        at = s * SLOT_LEN + SLOT_LEN - 1
        hit = np.flatnonzero(det["topk_logp"]["bbox3d"][at].view(np.uint32) == lp[at:at + 1].view(np.uint32))
        drawn = int(det["topk_tokens"]["bbox3d"][at][hit[0]]) if len(hit) else PAD
        if drawn != PAD:      # the slot was complete when the rule looked at it: it was blanked
            blanked += 1
            assert det["rank"]["bbox3d"][at] == int((rows[at] > rows[at][drawn]).sum()) and det["rank"]["bbox3d"][at] != int((rows[at] > rows[at][PAD]).sum())
    print(f"seed {seed}: {tr['counters']['rule_blanked']} slots blanked, {blanked} recognised by their drawn category token")
    assert blanked == tr["counters"]["rule_blanked"]


def raw_rollout_detail(e, scene, topk, det, temperature=1.0):
    i64p = C.POINTER(C.c_int64)
    arrs = [np.ascontiguousarray(scene[m], dtype=np.int64) for m in MOD_ORDER]
    outs = [np.full((1, 3, CONTENT_LEN[m]), -7, np.int64) for m in MOD_ORDER]
    smp, keep = e._sampling(sampled(e.cfg, sfmx_temp=temperature), [9])
    rc = e.lib.umgen_rollout_detail(e._h, 1, 1, 2, 1, 3, *[a.ctypes.data_as(i64p) for a in arrs], 0, None, None, 0, None, None, C.byref(smp),
                                    *[o.ctypes.data_as(i64p) for o in outs], None, None, topk, det)
    del keep
    return rc, e.lib.umgen_last_error(e._h).decode(), dict(zip(MOD_ORDER, outs))


def test_argument_errors():
    e = engine("tiny", "fp32")
    scene = synthetic_scene(TINY_SCENE + 43, n_frames=2)
    kw = dict(cond_frames=3, input_cond_frames=2, seeds=[9], sampling=sampled(e.cfg))
    ref = e.rollout(scene, 1, **kw)
    bufs, det = Engine._gen_detail_out((1, 1), 4)
    frames_before = e.timings()["frames"]
    for what, args in (("topk 17", dict(topk=17, det=C.byref(det))), ("lists with topk 0", dict(topk=0, det=C.byref(det))),
                       ("temperature inf", dict(topk=4, det=C.byref(det), temperature=float("inf")))):
        rc, msg, out = raw_rollout_detail(e, scene, **args)
        assert rc == -1 and msg, what
        assert all((o == -7).all() for o in out.values()), f"{what}: something ran"
        assert all((bufs["rank"][m] == -1).all() and np.isnan(bufs["topk_logp"][m]).all() for m in MOD_ORDER), what
    # NULL and all-NULL structs are the plain call, whatever topk says
    for d in (None, C.byref(_lib.GenDetailOut())):
        rc, msg, out = raw_rollout_detail(e, scene, 17, d)
        assert rc == 0, msg
        assert_same_tokens(out, ref, "all-NULL umgen_gen_detail_out")
    # some members NULL
    part = _lib.GenDetailOut(rank_map=det.rank_map, topk_logp_image=det.topk_logp_image)
    rc, msg, out = raw_rollout_detail(e, scene, 4, C.byref(part))
    assert rc == 0 and (bufs["rank"]["map"] >= 0).all() and np.isfinite(bufs["topk_logp"]["image"]).all() and (bufs["rank"]["image"] == -1).all(), msg
    assert_same_tokens(out, ref, "partial struct")
    with pytest.raises(UMGenError):
        e.rollout(scene, 1, return_detail=True, topk=17, **kw)
    assert e.timings()["frames"] >= frames_before
