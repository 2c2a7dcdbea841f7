"""-m gpu: what a call leaves behind on a handle.  The host engine hands every stack pass its stream and workspaces and every decode step
its view of the per-scene buffers as arguments; nothing about where a call ran may survive it.  So the kinds of call in any order on one
handle give the tokens of a fresh handle, lanes of unequal size (a non-zero base offset, 2 and 1 scenes) give the one-stream bits of every
side output, and a profiled frame -- the per-call flags through their other branch -- gives the unprofiled tokens on every decode path."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from umgen_amd.config import MOD_ORDER, tiny_config
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.synth import synthetic_scene
from umgen_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

KNOBS = ("UMGEN_DECODE_ENGINE", "UMGEN_DECODE_BATCHED", "UMGEN_DECODE_LANES", "UMGEN_BG_ENGINE", "UMGEN_OVERLAP")


@contextmanager
def knobs(**env):
    """the engine reads its knobs when it is created: set for the with-block, every other knob unset, the caller's values put back"""
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update({f"UMGEN_{k}": str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


def make(cfg, sd, max_batch=1, **env):
    with knobs(**env):
        e = Engine(cfg, precision="bf16", max_batch=max_batch, max_cond_frames=4)
    e.load_state_dict(sd)
    e.finalize()
    return e


@pytest.fixture(scope="module")
def setup():
    cfg = tiny_config(n_embd=768, n_head=16, n_oar_layer=5, rule_constrain=False)     # (tests/test_gpu_decode_engine.py's)
    return cfg, synthetic_state_dict(cfg, seed=21)


def cat(scenes):
    return {m: np.concatenate([s[m] for s in scenes]) for m in MOD_ORDER}


@pytest.mark.parametrize("overlap", [False, True], ids=["engine", "second_stream"])
def test_call_kinds_in_any_order_leave_the_handle_as_they_found_it(setup, overlap):
    """Rollout R, a traced frame (eager launches), a score, a fan rollout, one hooked decode step on the handle's own path and a call refused at
    the ABI boundary, then R again: the second R equals the first and both equal R on a fresh handle.  Once on the XCD-resident engine, once on
    a handle with the background pass on a second stream (UMGEN_OVERLAP=1: five launches per layer)."""
    cfg, sd = setup
    env = {"OVERLAP": 1} if overlap else {}
    scene = synthetic_scene(31, n_frames=3)
    hist = {m: scene[m][:, :2] for m in MOD_ORDER}
    window = {m: scene[m][0, :2] for m in MOD_ORDER}
    R = lambda h: h.rollout(hist, 2, cond_frames=3, input_cond_frames=2, seeds=[11])  # noqa: E731
    h = make(cfg, sd, max_batch=4, **env)
    first = R(h)
    t = h.timings()
    path = 2 if t["decode_batched"] else t["decode_engine"]
    print(f"overlap {overlap}: decode path {path}, overlapped frames {t['overlapped_frames']} of {t['frames']}, bg_ms {t['bg_ms']:.3f}")
    # R's second frame pushes only its last slot through the stacks on either handle: behind the first frame's own passes (the growing window's
    # reuse) or behind the pass on the second stream, which alone books bg_ms
    assert path == (0 if overlap else 1) and t["overlapped_frames"] == 1 and (t["bg_ms"] > 0) == overlap, t
    h.frame(window, frame_idx=0, seed=3, trace=True)
    h.score(window, {m: scene[m][0, 2] for m in MOD_ORDER})
    h.rollout(hist, 1, cond_frames=3, input_cond_frames=2, samples=2, seeds=[[5, 6]])
    x = np.random.default_rng(1).standard_normal((1, cfg.n_embd)).astype(np.float32)
    assert np.isfinite(h.dbg_oar_step(x, 0, path)).all()
    bad = {m: hist[m].copy() for m in MOD_ORDER}
    bad["map"][0, 1, 7] = cfg.map_vocab_size
    with pytest.raises(UMGenError):
        h.rollout(bad, 1, cond_frames=3, input_cond_frames=2, seeds=[11])
    second = R(h)
    h.close()
    fresh = make(cfg, sd, max_batch=4, **env)
    ref = R(fresh)
    fresh.close()
    for m in MOD_ORDER:
        np.testing.assert_array_equal(second[m], first[m], err_msg=f"second R vs first, {m}")
        np.testing.assert_array_equal(first[m], ref[m], err_msg=f"R vs a fresh handle, {m}")


def test_a_biased_call_reads_no_set_index_an_earlier_plan_left(setup):
    """A call with one set of tables is the plan that puts every scene on set 0, and its samplers read the per-scene set index.  A planned rollout that leaves
    scene 0 on set 1 and scene 1 on no set, the biased call, a plain rollout and the biased call again, on one handle: both biased calls have the tokens and
    logz of the biased call on a fresh handle, bit for bit, and the plain rollout the tokens of a fresh handle's.  Two scenes and one new frame are the
    smallest case in which the index the plan leaves differs from "set 0 for everyone"."""
    from tests.test_gpu_rollout_bias import random_tables
    from umgen_amd import constraints
    cfg, sd = setup
    toks = cat([synthetic_scene(80 + i, n_frames=1) for i in range(2)])
    tabs, others = random_tables(cfg, 3), [random_tables(cfg, 4), random_tables(cfg, 5)]
    kw = dict(cond_frames=3, input_cond_frames=1, seeds=[21, 22])
    biased = lambda h: h.rollout(toks, 1, logit_bias=tabs, return_logz=True, **kw)  # noqa: E731
    h = make(cfg, sd, max_batch=2)
    planned = h.rollout(toks, 1, logit_bias=constraints.schedule(others, [1, -1]), return_logz=True, **kw)
    b = biased(h)
    c = h.rollout(toks, 1, **kw)
    d = biased(h)
    h.close()
    fresh = make(cfg, sd, max_batch=2)
    b_ref = biased(fresh)
    fresh.close()
    fresh = make(cfg, sd, max_batch=2)
    c_ref = fresh.rollout(toks, 1, **kw)
    fresh.close()
    assert any((planned[0][m] != b_ref[0][m]).any() for m in MOD_ORDER), "premise: the plan's sets generate other tokens than the call's one set"
    assert any((c_ref[m] != b_ref[0][m]).any() for m in MOD_ORDER), "premise: the tables change what is generated"
    for m in MOD_ORDER:
        for name, got in (("first", b), ("second", d)):
            np.testing.assert_array_equal(got[0][m], b_ref[0][m], err_msg=f"{name} biased call vs a fresh handle, tokens of {m}")
            assert got[1][m].tobytes() == b_ref[1][m].tobytes(), f"{name} biased call vs a fresh handle, logz of {m}"
        np.testing.assert_array_equal(c[m], c_ref[m], err_msg=f"plain rollout vs a fresh handle, {m}")


def test_uneven_lanes_give_the_one_stream_bits_of_every_side_output(setup):
    """3 scenes on 2 lanes are lanes of 2 and 1: the smallest batch in which a lane has a non-zero base offset and the lanes differ in size.  Tokens,
    logp and every diagnostic array of two frames equal the one-stream batched layer's, bit for bit."""
    cfg, sd = setup
    B = 3
    toks = cat([synthetic_scene(70 + i, n_frames=2) for i in range(B)])
    outs = {}
    for lanes in (2, 1):
        e = make(cfg, sd, max_batch=B, DECODE_BATCHED=1, DECODE_LANES=lanes)
        outs[lanes] = e.rollout(toks, 2, cond_frames=3, input_cond_frames=2, seeds=[500 + i for i in range(B)], return_logp=True, return_detail=True, topk=2)
        t = e.timings()
        e.close()
        assert t["decode_batched"] == 1 and t["decode_lanes"] == lanes, t
    (tok2, logp2, det2), (tok1, logp1, det1) = outs[2], outs[1]
    assert set(det2) == {"rank", "mass_above", "entropy", "topk_tokens", "topk_logp"}
    for m in MOD_ORDER:
        np.testing.assert_array_equal(tok2[m], tok1[m], err_msg=m)
        assert logp2[m].tobytes() == logp1[m].tobytes(), f"logp {m}"
        for k in det2:
            assert det2[k][m].dtype == det1[k][m].dtype and det2[k][m].tobytes() == det1[k][m].tobytes(), f"{k} {m}"


@pytest.mark.parametrize("path", ["launches", "engine", "batched_2_lanes"])
def test_profiled_frames_return_the_unprofiled_tokens(setup, path):
    """umgen_set_profiling takes the per-call flags through the other branch (eager steps timed one by one; lane 0's runs timed around their graph
    launches): same tokens on the same handle, one timed layer pass per decode step, and the stacks' GEMM / attention launches counted."""
    cfg, sd = setup
    if path == "launches":
        B, e = 1, make(cfg, sd, DECODE_ENGINE=0, DECODE_BATCHED=0)
    elif path == "engine":
        B, e = 1, make(cfg, sd, DECODE_ENGINE=1, DECODE_BATCHED=0, BG_ENGINE=0)
    else:
        B, e = 3, make(cfg, sd, max_batch=3, DECODE_BATCHED=1, DECODE_LANES=2)
    toks = cat([synthetic_scene(40 + i, n_frames=2) for i in range(B)])
    run = lambda: e.rollout(toks, 1, cond_frames=3, input_cond_frames=2, seeds=list(range(B)))  # noqa: E731
    plain = run()
    e.set_profiling(True)
    prof = run()
    e.set_profiling(False)
    t1 = e.timings()      # (of the last rollout: every rollout starts its timings afresh)
    e.close()
    d = {k: t1[k] for k in ("oar_steps", "layers_launches", "gemm_launches", "attn_launches")}
    print(f"{path}: {d}, engine {t1['decode_engine']} batched {t1['decode_batched']} lanes {t1['decode_lanes']}")
    assert (t1["decode_engine"], t1["decode_batched"], t1["decode_lanes"]) == {"launches": (0, 0, 0), "engine": (1, 0, 0), "batched_2_lanes": (0, 1, 2)}[path]
    for m in MOD_ORDER:
        np.testing.assert_array_equal(prof[m], plain[m], err_msg=m)
    assert d["oar_steps"] > 0 and d["layers_launches"] == d["oar_steps"], d
    assert d["gemm_launches"] > 0 and d["attn_launches"] > 0, d
