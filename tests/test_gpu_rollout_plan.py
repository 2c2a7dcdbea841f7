"""Sampling plans end to end (umgen_rollout_planned; Engine.rollout(sampling=[...], logit_bias=constraints.schedule(...))) on the tiny config with
synthetic weights: 2 input frames, 2 - 3 new frames on a growing window, fp32 and bf16.

References (none measured on the code under test): the parent's own calls.  Scene / branch i of a planned call in new frame f has, bit for bit, the
tokens, lp, logz and diagnostics of branch i of the umgen_rollout_biased call on the same inputs and seeds that applies branch i's settings and table set
to everyone (include/umgen.h) -- the reference calls run at the same B * N, so on the same decode path."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests.test_gpu_rollout_bias import K, NEG, random_tables, same_bits, scenes_of
from tests.test_gpu_rollout_logp import close_engines, engine, sampled  # noqa: F401
from umgen_amd import _lib, constraints
from umgen_amd.config import CONTENT_LEN, MOD_ORDER
from umgen_amd.engine import UMGenError

pytestmark = pytest.mark.gpu
T_IN = 2


def settings_of(cfg):
    """four settings, no two alike: two top-k ladders, two nuclei; temperatures of their own"""
    return [sampled(cfg, top_k=3, top_k_map=4, topk_image=7, sfmx_temp=1.0),
            sampled(cfg, top_k=6, top_k_map=2, topk_image=11, sfmx_temp=0.7),
            sampled(cfg, sample_method="top_p", p=0.6, p_map=0.3, sfmx_temp=1.3),
            sampled(cfg, sample_method="top_p", p=0.25, p_map=0.8, sfmx_temp=0.9)]


def assert_branch(got, ref, i, what):
    """everything a call returned (tokens, lp, lz, diagnostics) for flat scene / branch i"""
    def groups(res):
        return [("tokens", res[0]), ("logp", res[1]), ("logz", res[2])] + sorted(res[3].items())

    for (key, a), (_, b) in zip(groups(got), groups(ref)):
        tail = 3 if key.startswith("topk_") else 2      # [.., frames, S_mod] (the lists: x topk) per branch
        for m in MOD_ORDER:
            x, y = a[m].reshape((-1,) + a[m].shape[-tail:]), b[m].reshape((-1,) + b[m].shape[-tail:])
            assert x[i].tobytes() == y[i].tobytes(), f"{what}: branch {i}: {key} of {m}"


def compare_with_uniform_calls(e, sc, nf, B, N, cfgs, sets, set_of):
    """the planned call against one umgen_rollout_biased call per distinct (settings, set): cfgs / set_of per flat branch"""
    BN = B * (N or 1)
    seeds = list(range(31, 31 + BN))
    kw = dict(cond_frames=4, input_cond_frames=T_IN, seeds=seeds, samples=N, return_logp=True, return_logz=True, return_detail=True, topk=K)
    got = e.rollout(sc, nf, sampling=cfgs, logit_bias=constraints.schedule(sets, np.asarray(set_of).reshape((B, N or 1))), **kw)
    moved = 0
    for pair in sorted({(cfgs.index(c), q) for c, q in zip(cfgs, set_of)}):
        ref = e.rollout(sc, nf, sampling=cfgs[pair[0]], logit_bias=None if pair[1] < 0 else sets[pair[1]], **kw)
        for i in range(BN):
            if (cfgs.index(cfgs[i]), set_of[i]) == pair:
                assert_branch(got, ref, i, f"settings {pair[0]} set {pair[1]}")
            else:
                moved += int(any((got[0][m].reshape(BN, -1)[i] != ref[0][m].reshape(BN, -1)[i]).any() for m in MOD_ORDER))
    assert moved > 0, "premise: the settings and sets of the plan change what the other branches generate"
    return got


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_branches_under_their_own_settings_and_sets(precision):
    """samples = 4: four different settings, two sets (and one branch without)"""
    e = engine("tiny", precision, max_batch=4)
    sets = [random_tables(e.cfg, 5), {"bbox3d": random_tables(e.cfg, 6)["bbox3d"], "pose": random_tables(e.cfg, 6)["pose"]}]
    got = compare_with_uniform_calls(e, scenes_of(1), 2, 1, 4, settings_of(e.cfg), sets, [0, 1, -1, 0])
    lz = got[2]
    assert not lz["map"][0, 1].view(np.uint32).any() and not lz["image"][0, 1].view(np.uint32).any(), "logz of a class without a table in the branch's set"
    assert all(not lz[m][0, 2].view(np.uint32).any() for m in MOD_ORDER), "logz of the branch without a set"
    assert (lz["bbox3d"][0, 1] != 0).any() and (lz["map"][0, 0] != 0).any()


def test_across_a_lane_boundary():
    """24 scenes in bf16: the batched decode layer on its lanes; settings and sets cycle with period 3, so every lane holds all of them"""
    B = 24
    e = engine("tiny", "bf16", max_batch=B)
    cfgs3 = settings_of(e.cfg)[:3]
    sets = [random_tables(e.cfg, 5), {"bbox3d": random_tables(e.cfg, 6)["bbox3d"], "pose": random_tables(e.cfg, 6)["pose"]}]
    compare_with_uniform_calls(e, scenes_of(B), 1, B, None, [cfgs3[i % 3] for i in range(B)], sets, [(i % 3) - 1 for i in range(B)])
    assert e.timings()["decode_batched"] == 1 and e.timings()["decode_lanes"] >= 2


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_uniform_plan_and_no_plan_are_the_unplanned_call(precision):
    e = engine("tiny", precision, max_batch=4)
    sc, smp, tabs = scenes_of(2), sampled(e.cfg), random_tables(e.cfg, 7)
    kw = dict(cond_frames=4, input_cond_frames=T_IN, seeds=[5, 6, 7, 8], samples=2, return_logp=True, return_logz=True, return_detail=True, topk=K)
    ref = e.rollout(sc, 2, sampling=smp, logit_bias=tabs, **kw)
    uniform = e.rollout(sc, 2, sampling=[dataclasses.replace(smp) for _ in range(4)], logit_bias=constraints.schedule([tabs], np.zeros((2, 2, 2), np.int64)), **kw)
    for i in range(4):
        assert_branch(uniform, ref, i, "uniform plan")
    plain = e.rollout(sc, 2, sampling=smp, **kw)
    i64p = C.POINTER(C.c_int64)
    arrs = [np.ascontiguousarray(sc[m], dtype=np.int64) for m in MOD_ORDER]
    outs = {m: np.zeros((2, 2, T_IN + 2, CONTENT_LEN[m]), np.int64) for m in MOD_ORDER}
    s, keep = e._sampling(smp, [5, 6, 7, 8])
    lp, lps = e._logp_out((2, 2, 2))
    rc = e.lib.umgen_rollout_planned(e._h, 2, 2, T_IN, 2, 4, *[a.ctypes.data_as(i64p) for a in arrs], 0, None, None, 0, None, None, C.byref(s),
                                     *[outs[m].ctypes.data_as(i64p) for m in MOD_ORDER], C.byref(lps), None, 0, None, None, None)
    assert rc == 0, e.lib.umgen_last_error(e._h).decode()
    same_bits(outs, plain[0], "plan = NULL: tokens")
    same_bits(lp, plain[1], "plan = NULL: lp")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_schedule_switches_sets_between_frames(precision):
    """set A in new frames < f0, set B from f0 on; B bans the pose-component-0 token the all-A call drew in frame f0"""
    e = engine("tiny", precision, max_batch=2)
    sc, smp, nf, f0 = scenes_of(2), sampled(e.cfg), 3, 1
    kw = dict(cond_frames=4, input_cond_frames=T_IN, seeds=[11, 12], sampling=smp, return_logp=True, return_logz=True)
    A = random_tables(e.cfg, 9)
    A["pose"] = np.where(np.isneginf(A["pose"]), NEG, np.float32(0)).astype(np.float32)      # bans alone: logz is the log of the allowed mass, <= 0
    all_a = e.rollout(sc, nf, logit_bias=A, **kw)
    drawn = [int(all_a[0]["pose"][b, T_IN + f0, 0]) for b in range(2)]
    B = constraints.merge(A, constraints.ban("pose", drawn, attr=0, vocab=e.cfg.pose_vocab_size))
    sch = constraints.per_frame([A] * f0 + [B] * (nf - f0))
    assert len(sch.sets) == 2
    got = e.rollout(sc, nf, logit_bias=sch, **kw)
    for part, ref in zip(got, all_a):
        for m in MOD_ORDER:
            lo = T_IN if part is got[0] else 0
            assert part[m][:, :lo + f0].tobytes() == ref[m][:, :lo + f0].tobytes(), f"frames before the switch: {m}"
    for b in range(2):
        tok = int(got[0]["pose"][b, T_IN + f0, 0])
        assert tok != drawn[b] and tok not in drawn and not np.isneginf(B["pose"][0, tok])
        assert got[2]["pose"][b, f0, 0] < 0, "logz of the pose position whose drawn token B bans"
    for m in MOD_ORDER:
        rows = B[m].reshape(constraints.ROWS[m], -1)
        t = got[0][m][:, T_IN + f0:]
        r = rows[np.arange(CONTENT_LEN[m]) % constraints.ROWS[m], t]
        assert not np.isneginf(r).any(), f"a token banned by set B was drawn in a frame >= f0: {m}"
    # the sets permuted in the pool, the index renumbered: the same bytes
    swapped = e.rollout(sc, nf, logit_bias=constraints.schedule([B, A], np.array([1] * f0 + [0] * (nf - f0)), axis="frame"), **kw)
    for x, y in zip(swapped, got):
        same_bits(x, y, "permuted sets")


def raw_planned(e, sc, B, N, nf, smp, plan, control=None):
    i64p = C.POINTER(C.c_int64)
    arrs = [np.ascontiguousarray(sc[m], dtype=np.int64) for m in MOD_ORDER]
    outs = [np.full((B * N, T_IN + nf, CONTENT_LEN[m]), -7, np.int64) for m in MOD_ORDER]
    cb = None if control is None else np.ascontiguousarray(control, dtype=np.int64)
    rc = e.lib.umgen_rollout_planned(e._h, B, N, T_IN, nf, 4, *[a.ctypes.data_as(i64p) for a in arrs], 0 if cb is None else 1, None,
                                     None if cb is None else cb.ctypes.data_as(i64p), int(cb is not None), None, None, C.byref(smp),
                                     *[o.ctypes.data_as(i64p) for o in outs], None, None, 0, None, C.byref(plan), None)
    assert all((o[:, T_IN:] == -7).all() for o in outs) or rc == 0, "a refused call wrote tokens"
    return rc, e.lib.umgen_last_error(e._h).decode()


def test_refusals_name_the_offender():
    e = engine("tiny", "fp32", max_batch=4)
    sc, B, N, nf = scenes_of(2), 2, 2, 2
    base, keep = e._sampling(sampled(e.cfg), [1, 2, 3, 4])
    fptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    good = random_tables(e.cfg, 3)
    hold = []

    def bias_struct(tabs):
        arrs = {m: np.ascontiguousarray(t, np.float32) for m, t in tabs.items()}
        hold.append(arrs)
        return _lib.LogitBias(**{m: fptr(a) for m, a in arrs.items()})

    def plan(per=None, sets=(), of=None, n_sets=None):
        p = _lib.SamplePlan()
        if per is not None:
            arr = (_lib.Sampling * len(per))(*per)
            hold.append(arr)
            p.per_scene = C.cast(arr, C.POINTER(_lib.Sampling))
        arr = (_lib.LogitBias * max(1, len(sets)))(*[bias_struct(t) for t in sets])
        hold.append(arr)
        p.bias_sets, p.n_bias_sets = C.cast(arr, C.POINTER(_lib.LogitBias)), len(sets) if n_sets is None else n_sets
        if of is not None:
            a = np.ascontiguousarray(of, np.int32)
            hold.append(a)
            p.bias_of = a.ctypes.data_as(C.POINTER(C.c_int32))
        return p

    def entry(**over):
        s = e._sampling(dataclasses.replace(sampled(e.cfg), **{k: v for k, v in over.items() if k not in ("method", "temperature")}), [])[0]
        for k in ("method", "temperature"):
            if k in over:
                setattr(s, k, over[k])
        s.seeds = None
        return s

    def refused(p, *parts, control=None):
        rc, msg = raw_planned(e, sc, B, N, nf, base, p, control)
        assert rc == -1 and all(x in msg for x in parts), (rc, msg, parts)

    ok = [entry() for _ in range(4)]
    refused(plan(per=ok[:2] + [entry(temperature=0.0)] + ok[3:]), "per_scene[2]", "temperature")
    refused(plan(per=ok[:3] + [entry(method=5)]), "per_scene[3]", "sample method 5")
    refused(plan(per=ok[:1] + [entry(top_k=17)] + ok[2:]), "per_scene[1]", "top-k")
    for flag in ("rule_constrain", "merage_ar_tar", "only_ar"):
        refused(plan(per=ok[:2] + [entry(**{flag: not getattr(sampled(e.cfg), flag)})] + ok[3:]), "per_scene[2]", "per call")
    refused(plan(n_sets=-1), "n_bias_sets=-1")
    refused(plan(sets=[good] * 17), "n_bias_sets=17")
    refused(plan(of=np.zeros((4, nf))), "n_bias_sets = 0")
    of = np.zeros((4, nf), np.int32)
    of[3, 1] = 2
    refused(plan(sets=[good, good], of=of), "scene 3", "frame 1", "is 2")
    of[3, 1] = -2
    refused(plan(sets=[good, good], of=of), "scene 3", "frame 1", "is -2")
    of[3, 1] = 0
    bad = {m: t.copy() for m, t in good.items()}
    bad["bbox3d"][4, 9] = np.nan
    refused(plan(sets=[good, bad], of=of), "bias set 1", "class bbox3d row 4 index 9 is NaN")      # (no scene uses set 1: still validated)
    bad["bbox3d"][4, 9] = 0.0
    bad["map"][:] = NEG
    refused(plan(sets=[good, bad], of=of), "bias set 1", "class map row 0 bans every token")
    # the control resample's masked index: refused in a set some scene uses, accepted in one nobody uses
    last = {"bbox3d": np.full((11, e.cfg.bbox3d_vocab_size), NEG, np.float32)}
    last["bbox3d"][:, -1] = 0.0
    ctl = np.full((B, 1, CONTENT_LEN["bbox3d"]), -1, np.int64)
    ctl[:, 0, :11] = sc["bbox3d"][:, -1, :11]
    of[1, 0] = 1
    refused(plan(sets=[good, last], of=of), "bias set 1", "allows only index", control=ctl)
    of[1, 0] = 0
    rc, msg = raw_planned(e, sc, B, N, nf, base, plan(sets=[good, last], of=of), ctl)
    assert rc == 0, msg
    del keep
    # the Python layer: lengths and shapes that do not fit the call
    kw = dict(cond_frames=4, input_cond_frames=T_IN, seeds=[1, 2, 3, 4], samples=2)
    with pytest.raises(UMGenError, match="sampling has 3 entries"):
        e.rollout(sc, nf, sampling=[sampled(e.cfg)] * 3, **kw)
    with pytest.raises(UMGenError, match="per call"):
        e.rollout(sc, nf, sampling=[sampled(e.cfg), sampled(e.cfg, only_ar=True)], **kw)
    with pytest.raises(UMGenError, match="scene axis"):
        e.rollout(sc, nf, sampling=sampled(e.cfg), logit_bias=constraints.schedule([good], np.zeros(3, np.int64)), **kw)
    with pytest.raises(UMGenError, match="frame axis"):
        e.rollout(sc, nf, sampling=sampled(e.cfg), logit_bias=constraints.schedule([good], np.zeros(nf + 1, np.int64), axis="frame"), **kw)
