"""-m gpu: umgen_rollout_fan on the engine (Engine.rollout(samples=N)) -- N sampled futures per scene whose first frame runs the history once per
scene.  The yardstick everywhere is Engine.rollout(return_logp=True) on the inputs replicated N times on the SAME engine, compared with tobytes():
branch (b, s) must be scene b*N + s of that call, tokens and log-likelihoods, in every precision.

Cases: a window that slides at once and one that is full from the start; a window that grows (the slot caches must come out of the fan frame as the
replicated call leaves them: the later frames then push one slot per branch, counted in timings()["overlapped_frames"]); control and given tokens;
the fallbacks (one history frame, UMGEN_FAN_SHARE=0, N = 1); ordinary rollouts around a fan call; refused calls past the Python checks."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from tests.golden.make_full_width_golden import SCENE_ID, WEIGHT_SEED, config as width_config
from tests.golden.make_score_golden import TINY_WEIGHT_SEED
from umgen_amd import _lib
from umgen_amd.config import CONTENT_LEN, MOD_ORDER, tiny_config
from umgen_amd.engine import Engine, UMGenError
from umgen_amd.synth import synthetic_control, synthetic_given_map, synthetic_scene
from umgen_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
ENGINES = [("tiny", "fp32"), ("full_width", "bf16"), ("full_width", "fp16")]
_engines = {}


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


def engine(width, precision, overlap=None):
    """max_batch 6, max_cond_frames 4.  overlap="0": created with UMGEN_OVERLAP=0 -- an fp32 engine then grows its window in the foreground like the
    16-bit engines, which run the decode engine, do by default"""
    key = (width, precision, overlap)
    if key not in _engines:
        cfg = tiny_config() if width == "tiny" else width_config(width)
        with env(**({} if overlap is None else {"UMGEN_OVERLAP": overlap})):
            e = Engine(cfg, precision=precision, max_batch=6, max_cond_frames=4)
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


def sampled(cfg):
    """the reference's top-k sampling (5 / 5 / 16) without the rule constraint: the seeds matter"""
    return dataclasses.replace(cfg, sample_method="topk", top_k=5, top_k_map=5, topk_image=16, rule_constrain=False)


def scenes(B, T, scene0=SCENE_ID + 20):
    return {m: np.concatenate([synthetic_scene(scene0 + i, n_frames=T)[m] for i in range(B)]) for m in MOD_ORDER}


def rep(d, N):
    return None if d is None else {k: np.repeat(np.asarray(v), N, axis=0) for k, v in d.items()}


def both(e, sc, N, nf, cond, T_in, seeds, init=None, control_test=False):
    """(the fan call, the replicated call reshaped to the fan call's shapes), each (tokens, logp, overlapped_frames); shared_slots of the fan call"""
    seeds = np.asarray(seeds, dtype=np.uint64)
    B = sc["pose"].shape[0]
    kw = dict(cond_frames=cond, input_cond_frames=T_in, control_test=control_test, sampling=sampled(e.cfg), return_logp=True)
    r_out, r_lp = e.rollout(rep(sc, N), nf, init_tokens=rep(init, N), seeds=seeds.reshape(-1), **kw)
    r_ov = e.timings()["overlapped_frames"]
    f_out, f_lp = e.rollout(sc, nf, init_tokens=init, seeds=seeds.reshape(B, N), samples=N, **kw)
    f_ov, shared = e.timings()["overlapped_frames"], e.last_shared_slots
    r_out = {m: r_out[m].reshape(f_out[m].shape) for m in MOD_ORDER}
    r_lp = {m: r_lp[m].reshape(f_lp[m].shape) for m in MOD_ORDER}
    return (f_out, f_lp, f_ov), (r_out, r_lp, r_ov), shared


def same_bytes(fan, ref, what):
    for kind, a, b in (("tokens", fan[0], ref[0]), ("logp", fan[1], ref[1])):
        for m in MOD_ORDER:
            assert a[m].shape == b[m].shape and a[m].dtype == b[m].dtype, (what, kind, m, a[m].shape, b[m].shape)
            assert a[m].tobytes() == b[m].tobytes(), (what, kind, m, np.argwhere(a[m] != b[m])[:4].tolist())


@pytest.mark.parametrize("T_in,cond", [(4, 4), (2, 2)])
@pytest.mark.parametrize("width,precision", ENGINES)
def test_sliding_window_branches_have_the_bits_of_the_replicated_call(width, precision, T_in, cond):
    e = engine(width, precision)
    B, N, nf = 2, 3, 2
    sc = scenes(B, T_in)
    seeds = [[11, 12, 11], [13, 13, 14]]
    fan, ref, shared = both(e, sc, N, nf, cond, T_in, seeds)
    assert shared == min(T_in, cond) - 1
    same_bytes(fan, ref, f"{width} {precision} T_in {T_in}")
    out, lp = fan[0], fan[1]
    for m in MOD_ORDER:
        assert out[m].shape == (B, N, T_in + nf, CONTENT_LEN[m]) and lp[m].shape == (B, N, nf, CONTENT_LEN[m])
        assert np.array_equal(out[m][:, :, :T_in], np.repeat(sc[m][:, None], N, axis=1)), m      # the history comes back per branch
        assert np.isfinite(lp[m]).all() and (lp[m] <= 0).all(), m
        # equal seeds: the same future (the scene index does not enter the RNG)
        assert out[m][0, 0].tobytes() == out[m][0, 2].tobytes() and out[m][1, 0].tobytes() == out[m][1, 1].tobytes(), m
        assert lp[m][0, 0].tobytes() == lp[m][0, 2].tobytes() and lp[m][1, 0].tobytes() == lp[m][1, 1].tobytes(), m
    # distinct seeds: not the same future
    assert any(not np.array_equal(out[m][0, 0], out[m][0, 1]) for m in MOD_ORDER) and any(not np.array_equal(out[m][1, 1], out[m][1, 2]) for m in MOD_ORDER)


@pytest.mark.parametrize("width,precision,overlap", [(w, p, None) for w, p in ENGINES] + [("tiny", "fp32", "0")])
def test_growing_window_keeps_the_slot_cache_reuse(width, precision, overlap):
    e = engine(width, precision, overlap)
    fan, ref, shared = both(e, scenes(2, 2, SCENE_ID + 30), 3, 3, 4, 2, np.arange(21, 27))
    assert shared == 1
    same_bytes(fan, ref, f"{width} {precision} growing")
    print(f"growing window {width} {precision} overlap={overlap}: overlapped_frames fan {fan[2]} replicated {ref[2]}")
    # the frames behind the fan frame push one slot per branch exactly when the replicated call's do (without the spread: one frame fewer)
    assert fan[2] == ref[2]
    # engines that grow the window in the foreground (no second-stream overlap: created without it, or running the decode engine) reuse the caches in frames 2, 3
    if overlap == "0" or e.timings()["decode_engine"]:
        assert ref[2] == 2, "the replicated call itself does not reuse the slot caches on this engine"


def test_control_and_given_tokens_are_shared_by_a_scenes_branches():
    e = engine("tiny", "fp32")
    B, N, nf = 2, 3, 2
    sc = scenes(B, 2, SCENE_ID + 40)
    cat = lambda ds: {k: np.concatenate([d[k] for d in ds]) for k in ds[0]}      # noqa: E731
    gm = cat([synthetic_given_map(60 + i, n_frames=nf) for i in range(B)])
    gb = cat([{"bbox3d": synthetic_scene(960 + i, n_frames=nf)["bbox3d"]} for i in range(B)])
    ctl = cat([synthetic_control(60 + i, n_frames=nf, slot=2 + i) for i in range(B)])
    cases = {"control pose + boxes": (dict(init=ctl, control_test=True), {"pose"}),
             "given map": (dict(init=gm), {"map"}),
             "given map + boxes": (dict(init={**gm, **gb}), {"map", "bbox3d"})}
    for name, (kw, nan_mods) in cases.items():
        fan, ref, shared = both(e, sc, N, nf, 3, 2, np.arange(31, 37), **kw)
        assert shared == 1, name
        same_bytes(fan, ref, name)      # (NaN patterns included: bytes)
        for m in MOD_ORDER:
            assert np.isnan(fan[1][m]).all() if m in nan_mods else np.isfinite(fan[1][m]).all(), (name, m)
    # the given map is every branch's map
    assert np.array_equal(fan[0]["map"][:, :, 2:], np.repeat(gm["map"][:, None], N, axis=1))


def test_fallbacks_share_nothing_and_keep_the_bits():
    e = engine("tiny", "fp32")
    fan, ref, shared = both(e, scenes(2, 1, SCENE_ID + 50), 3, 2, 3, 1, np.arange(41, 47))      # one history frame: nothing to share
    assert shared == 0
    same_bytes(fan, ref, "T_in = 1")
    sc = scenes(2, 2, SCENE_ID + 52)
    on, ref, shared = both(e, sc, 3, 2, 3, 2, np.arange(41, 47))
    assert shared == 1
    with env(UMGEN_FAN_SHARE="0"):
        off, _, shared = both(e, sc, 3, 2, 3, 2, np.arange(41, 47))
    assert shared == 0
    same_bytes(off, ref, "UMGEN_FAN_SHARE=0")
    same_bytes(off, on, "UMGEN_FAN_SHARE=0 against the shared path")
    one, ref, shared = both(e, sc, 1, 2, 3, 2, [41, 42])
    assert shared == 0
    same_bytes(one, ref, "N = 1")
    plain = e.rollout(sc, 2, cond_frames=3, input_cond_frames=2, seeds=[41, 42], sampling=sampled(e.cfg))
    for m in MOD_ORDER:
        assert one[0][m][:, 0].tobytes() == plain[m].tobytes(), m


@pytest.mark.parametrize("width,precision", [("tiny", "fp32"), ("full_width", "bf16")])
def test_a_fan_call_leaves_rollouts_unchanged_and_repeats_itself(width, precision):
    e = engine(width, precision)
    sc = scenes(2, 2, SCENE_ID + 60)
    kw = dict(cond_frames=4, input_cond_frames=2, sampling=sampled(e.cfg))
    before = e.rollout(sc, 2, seeds=[5, 6], **kw)
    a = e.rollout(sc, 2, seeds=np.arange(6), samples=3, return_logp=True, **kw)
    after = e.rollout(sc, 2, seeds=[5, 6], **kw)
    b = e.rollout(sc, 2, seeds=np.arange(6), samples=3, return_logp=True, **kw)
    assert e.last_shared_slots == 1
    for m in MOD_ORDER:
        assert before[m].tobytes() == after[m].tobytes(), m
    same_bytes(a, b, "the call repeated")


def raw_call(e, sc, B, N, T_in, nf, out="make"):
    """umgen_rollout_fan itself, past the Python checks -> (rc, message, shared_slots)"""
    i64p = C.POINTER(C.c_int64)
    arrs = [np.ascontiguousarray(sc[m], dtype=np.int64) for m in MOD_ORDER]
    outs = [np.zeros((max(B * N, 1), T_in + nf, CONTENT_LEN[m]), np.int64) for m in MOD_ORDER]
    smp, keep = e._sampling(sampled(e.cfg), list(range(41, 41 + max(B * N, 1))))
    op = [None] * 4 if out is None else [o.ctypes.data_as(i64p) for o in outs]
    shared = C.c_int32(-1)
    rc = e.lib.umgen_rollout_fan(e._h, B, N, T_in, nf, 3, *[a.ctypes.data_as(i64p) for a in arrs], 0, None, None, 0, None, None, C.byref(smp), *op, None,
                                 C.byref(shared))
    del keep
    return rc, e.lib.umgen_last_error(e._h).decode(), dict(zip(MOD_ORDER, outs))


def test_refused_calls_leave_the_engine_usable():
    e = engine("tiny", "fp32")
    sc = scenes(2, 2, SCENE_ID + 52)
    ref = e.rollout(rep(sc, 3), 2, cond_frames=3, input_cond_frames=2, seeds=np.arange(41, 47), sampling=sampled(e.cfg))
    bad = dict(sc, image=sc["image"].copy())
    bad["image"][1, 1, 9] = 8192
    for what, args, needle in (("N = 0", (sc, 2, 0, 2, 2), "N=0"), ("B*N > max_batch", (sc, 2, 4, 2, 2), "B*N=8"),
                               ("NULL output", (sc, 2, 3, 2, 2, None), "null"), ("token >= vocab", (bad, 2, 3, 2, 2), "8192")):
        rc, msg, _ = raw_call(e, *args)
        assert rc == -1 and needle in msg, (what, rc, msg)
    # B = 2, N = 2, a map token outside the vocabulary in scene 1: the message names the index in the caller's [2][T_in][1024] array (not in a replicated
    # one, where scene 1 starts at item 2), and the call is refused before any device work: no frame is counted, nothing is written
    bad = dict(sc, map=sc["map"].copy())
    bad["map"][1, 1, 9] = e.cfg.map_vocab_size
    frames = e.timings()["frames"]
    rc, msg, out = raw_call(e, bad, 2, 2, 2, 2)
    assert rc == -1 and f"map token {e.cfg.map_vocab_size} at flat index {(1 * 2 + 1) * 1024 + 9} " in msg, (rc, msg)
    assert e.timings()["frames"] == frames and all(not out[m].any() for m in MOD_ORDER)
    with pytest.raises(UMGenError):
        e.rollout(sc, 2, cond_frames=3, input_cond_frames=2, samples=4)
    rc, msg, out = raw_call(e, sc, 2, 3, 2, 2)      # a NULL umgen_logp_out is fine
    assert rc == 0, msg
    for m in MOD_ORDER:
        assert out[m].tobytes() == ref[m].tobytes(), m
