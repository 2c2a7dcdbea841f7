"""Sampling plans inside the samplers (csrc/frame.hip), through umgen_dbg_token_steps_planned and umgen_dbg_sample_ego_planned: with OarState::plan
set, the block of scene b draws under its own SamplerParams (sp_of[b], bit 0) and under its own table set of the pool (bias_set_of[b], -1 = none, the
set's class bits in set_classes; bit 1) -- the AR row, both TAR resamples, logz and the diagnostics' temperature.

References (none measured on the code under test):
  * tokens, x_next, counters, boxes, step / epoch / done: the oracle's own walk (Steps.walk of tests/test_gpu_frame_kernels.py), run once per scene on
    that scene's rows alone with that scene's settings and tables (logits + r in float32, like tests/test_gpu_bias_kernel.py), counters summed;
  * lp: float64 log-softmax of the UNBIASED row at the drawn token, bar 1e-4 * max(1, |ref|) (BAR, tests/test_gpu_logp_kernel.py);
  * logz: float64 lse(w) - lse(v) against the scene's own table, bar BAR on each of the two log-sum-exps (tests/test_gpu_bias_kernel.py); exactly +0.0
    for a scene without a set and for a class without a table in the scene's set;
  * mass_above: float64 at the scene's own temperature, bar 1e-5 (ABS_BAR, tests/test_gpu_detail_kernel.py).
E = 96 like tests/test_gpu_bias_kernel.py, whose rows these are: ld columns per scene with 3e4 in every column past the position's vocabulary."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests.gpu_util import check, fp, lib
from tests.test_gpu_bias_kernel import NEG, RUNS, ZERO_BITS, BiasSteps, biased, lse64, random_table
from tests.test_gpu_detail_kernel import ABS_BAR, reference
from tests.test_gpu_frame_kernels import (DRAW_MAIN, IMG_BOS, IMG_C0, KSEQ, MAP_C0, MAP_EOS, OFF_BOX, PAD, TOK, Steps, Tables, Walk, at_box, frame_tokens,
                                          i32p, kind_of, nan32, rng_uniform, sampler_params, u64p)
from tests.test_gpu_logp_kernel import BAR, LogpSteps, is_nan_bits, slot_of
from tests.test_gpu_score import log_softmax_at
from umgen_amd._lib import DbgSamplerParams

pytestmark = pytest.mark.gpu
E = 96
CLASS_BIT = {0: 1, 1: 2, 2: 4, 3: 8}      # pose, map, bbox3d, image (kBiasPose ..)
OUT_KEYS = ("tokens", "x_next", "counters", "n_boxes", "boxes", "state", "logp", "logz", "rank", "mass", "ent", "tok", "tlp")


def params_array(sps):
    arr = (DbgSamplerParams * len(sps))()
    for i, sp in enumerate(sps):
        arr[i] = DbgSamplerParams(**sp)
    return arr


class PlanSteps(BiasSteps):
    """BiasSteps through umgen_dbg_token_steps_planned.  sp_of: a list of B settings dicts, or None (the switch's bit 0 off: self.sp for everyone);
    sets: a list of table sets {1: [n_map], 2: [11, n_box], 3: [n_img]} (a missing class: no table) with set_of [B] (-1: none), or set_of None (bit 1 off).
    walk: the oracle's walk scene by scene, each under its own settings and its own set."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.sp_of, self.sets, self.set_of = None, [], None

    def with_vocab(self, V):
        """map and image vocabularies of V codes: new tables, rows wide enough, tokens in range"""
        self.tb = Tables(self.E, dims=dict(n_map=V, n_img=V))
        self.V = {1: V, 2: self.tb.dims["n_box"], 3: V}
        self.ld = max(1100, V + 4)
        self.tokens = frame_tokens(self.rng, self.tb, self.B)
        return self

    def pool(self):
        d = self.tb.dims
        off = {0: 0, 1: 3 * d["n_pose"], 2: 3 * d["n_pose"] + d["n_map"], 3: 3 * d["n_pose"] + d["n_map"] + 11 * d["n_box"]}
        stride = off[3] + d["n_img"]
        pool = np.full((max(1, len(self.sets)), stride), np.nan, np.float32)      # (a class without a table is never read: NaN would show)
        classes = np.zeros(max(1, len(self.sets)), np.int32)
        for q, tabs in enumerate(self.sets):
            for k, t in tabs.items():
                t = np.ascontiguousarray(t, np.float32).reshape(-1)
                pool[q, off[k]:off[k] + t.size] = t
                classes[q] |= CLASS_BIT[k]
        return pool, classes

    def run(self, j0, j1, logits, want_logz=True):
        out = self.blank(j1 - j0)
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        assert logits.shape == (j1 - j0, self.B, self.ld)
        sp_of = None if self.sp_of is None else params_array(self.sp_of)
        pool, classes = self.pool()
        set_of = None if self.set_of is None else np.ascontiguousarray(self.set_of, np.int32)
        check(lib().umgen_dbg_token_steps_planned(self.tb.ref, C.byref(self.args(out, logits, j0, j1)), fp(out.logp), fp(out.logz) if want_logz else None,
                                                  self.topk, i32p(out.rank), fp(out.mass), fp(out.ent), i32p(out.tok), fp(out.tlp), sp_of,
                                                  None if set_of is None else fp(pool), len(self.sets), i32p(classes), None if set_of is None else i32p(set_of)))
        return out

    def scene_sp(self, b):
        return self.sp if self.sp_of is None else self.sp_of[b]

    def scene_bias(self, b):
        return {} if self.set_of is None or self.set_of[b] < 0 else self.sets[self.set_of[b]]

    def walk(self, j0, j1, logits):
        refs = []
        for b in range(self.B):
            s = Steps.scene(self, b)
            s.__class__ = BiasSteps
            s.sp, s.bias = self.scene_sp(b), self.scene_bias(b)
            refs.append(s.walk(j0, j1, np.ascontiguousarray(logits[:, b:b + 1])))
        cat = lambda k, axis=0: np.concatenate([getattr(r, k) for r in refs], axis=axis)      # noqa: E731
        return types.SimpleNamespace(tokens=cat("tokens"), drawn=cat("drawn"), x_next=cat("x_next", 1), counters=sum(r.counters for r in refs),
                                     boxes=[r.boxes[0] for r in refs], n_boxes=cat("n_boxes"))

    def check_plan(self, j0, j1, logits):
        """Steps.check (tokens, x_next, counters, boxes, state against the per-scene walks), then lp, logz and mass_above against float64"""
        got, ref = Steps.check(self, j0, j1, logits)
        for b in range(self.B):
            tabs, tau = self.scene_bias(b), self.scene_sp(b)["temperature"]
            for i, j in enumerate(range(j0, j1)):
                kind, at = kind_of(j, self.given_end), slot_of(j)
                if not kind:
                    continue
                v = logits[i, b, :self.V[kind]]
                tok = int(ref.drawn[b, at])
                want = float(log_softmax_at(v[None], np.array([tok]))[0])
                assert abs(float(got.logp[b, at]) - want) <= BAR * max(1.0, abs(want)), (b, j, float(got.logp[b, at]), want)
                t = tabs.get(kind)
                if t is None:
                    assert got.logz[b, at].view(np.uint32) == ZERO_BITS, f"scene {b} position {j}: logz without a table is not +0.0"
                else:
                    r = t[(j - at_box(0)) % 11] if kind == 2 else t
                    assert not np.isneginf(r[tok]), f"scene {b} drew token {tok}, banned by its own set, at position {j}"
                    lw, lv = float(lse64(biased(v, r))), float(lse64(v))
                    assert abs(float(got.logz[b, at]) - (lw - lv)) <= BAR * (max(1.0, abs(lw)) + max(1.0, abs(lv))), (b, j, float(got.logz[b, at]), lw - lv)
                m = reference(v[None], np.array([tok]), tau)["mass"][0]
                assert abs(float(got.mass[b, at]) - m) <= ABS_BAR, f"scene {b} position {j}: mass_above {got.mass[b, at]} vs {m} at the scene's temperature {tau}"
        sampled = np.array([slot_of(j) for j in range(j0, j1) if kind_of(j, self.given_end)], int)
        rest = np.setdiff1d(np.arange(TOK), sampled)
        assert is_nan_bits(got.logp[:, rest]).all() and is_nan_bits(got.logz[:, rest]).all(), "a position without a sampled step lost its NaN"
        return got, ref


def mixed_settings():
    """two top-k scenes and two nucleus scenes, no two alike"""
    return [sampler_params(method=0, top_k=3, top_k_map=4, topk_image=7, temperature=1.0),
            sampler_params(method=0, top_k=6, top_k_map=2, topk_image=11, temperature=0.7),
            sampler_params(method=1, p=0.6, p_map=0.3, temperature=1.3),
            sampler_params(method=1, p=0.25, p_map=0.8, temperature=0.9)]


# ---- 1. per-scene settings -------------------------------------------------------------------------------------------------------------------
def test_mixed_settings_equal_the_per_scene_walks():
    s = PlanSteps(E, 4)
    s.prev_box[:] = s.rng.integers(0, 1028, s.prev_box.shape)
    s.sp_of = mixed_settings()
    one = PlanSteps.__new__(PlanSteps)      # the same inputs under s.sp for every scene
    one.__dict__.update(s.__dict__)
    one.sp_of = None
    differ = 0
    for j0, j1 in RUNS:
        lg = s.random_logits(j0, j1)
        got, ref = s.check_plan(j0, j1, lg)
        differ += int((one.walk(j0, j1, lg).tokens != ref.tokens).sum())
    assert differ > 0, "premise: the walk under ONE set of settings for every scene differs from the per-scene walks"


# ---- 2. per-scene table sets -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1])
def test_scenes_on_their_own_sets(method):
    """scene 0 unbiased, scenes 1 and 3 on set 0 (all three classes), scene 2 on set 1 (a bbox3d table only)"""
    s = PlanSteps(E, 4, seed=2, method=method, top_k=3, top_k_map=4, topk_image=7, p=0.6, p_map=0.3)
    s.prev_box[:] = s.rng.integers(0, 1028, s.prev_box.shape)
    s.sets = [{1: random_table(s.rng, 1, s.V[1])[0], 2: random_table(s.rng, 11, s.V[2]), 3: random_table(s.rng, 1, s.V[3])[0]},
              {2: random_table(s.rng, 11, s.V[2])}]
    s.set_of = [-1, 0, 1, 0]
    other = {0: 0, 1: 0}      # draws of a scene on set q that the OTHER set bans
    for j0, j1 in RUNS:
        lg = s.random_logits(j0, j1)
        got, ref = s.check_plan(j0, j1, lg)
        for j in range(j0, j1):
            if kind_of(j, s.given_end) != 2:
                assert kind_of(j, s.given_end) == 0 or (got.logz[[0, 2], slot_of(j)].view(np.uint32) == ZERO_BITS).all()
                continue
            row, at = (j - at_box(0)) % 11, slot_of(j)
            assert got.logz[0, at].view(np.uint32) == ZERO_BITS
            for b, q in ((1, 0), (2, 1), (3, 0)):
                other[q] += int(np.isneginf(s.sets[1 - q][2][row, ref.drawn[b, at]]))
    assert other[0] > 0 and other[1] > 0, f"premise: the walks draw tokens that only the other set bans ({other})"


# ---- 3. the two TAR resamples read their own scene's row and table ----------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1])
def test_control_resample_under_two_sets(method):
    """test_control_resample_draws_from_the_biased_tar_row's construction in both scenes: the TAR peak on the masked column, the runner-up 77 banned by both
    sets; set 0 lifts 99, set 1 lifts 101"""
    s = PlanSteps(E, 2, rule_constrain=0, merge_ar_tar=0, method=method)
    s.use_control = 1
    s.control[:, 1] = 1
    s.logits_tar[:, 12] = 0
    s.logits_tar[:, 12, PAD] = 1e4
    s.logits_tar[:, 12, 77] = 50
    s.sets = [{2: random_table(s.rng, 11, s.V[2], keep=(5, 77, 99, 101))} for _ in range(2)]
    for q, lifted in enumerate((99, 101)):
        s.sets[q][2][12 % 11, 77] = NEG
        s.sets[q][2][12 % 11, lifted] = 60.0
    s.set_of = [0, 1]
    j0, j1 = at_box(8), at_box(23)
    got, ref = s.check_plan(j0, j1, s.peaked_logits(j0, j1, lambda b, j: 5))
    assert got.tokens[0, OFF_BOX + 12] == 99 and got.tokens[1, OFF_BOX + 12] == 101 and got.counters[1] == 22


@pytest.mark.parametrize("method", [0, 1])
def test_pad_avoid_resample_under_two_sets(method):
    """test_pad_avoid_resample_draws_from_the_biased_tar_row's construction: both sets ban the TAR peak 300; set 0 lifts 301, set 1 lifts 302"""
    s = PlanSteps(E, 2, rule_constrain=0, method=method)
    s.prev_box[0, 0:6] = [500, 1027, 3, 1027, 7, 1026]
    s.prev_box[1, 0:6] = 1027
    s.prev_box[1, 4] = 9
    s.logits_tar[:, 0:6] = 0
    s.logits_tar[:, 0:6, 300] = 1e4
    s.sets = [{2: random_table(s.rng, 11, s.V[2], keep=(PAD, 300, 301, 302))} for _ in range(2)]
    for q, lifted in enumerate((301, 302)):
        s.sets[q][2][0:6, 300] = NEG
        s.sets[q][2][0:6, lifted] = 50.0
    s.set_of = [0, 1]
    j0, j1 = at_box(0), at_box(6)
    got, ref = s.check_plan(j0, j1, s.peaked_logits(j0, j1, lambda b, j: PAD))
    assert got.counters[0] == 5 and not got.counters[1:6].any()
    assert list(got.tokens[0, OFF_BOX:OFF_BOX + 6]) == [301, PAD, 301, PAD, 301, 301] and got.tokens[1, OFF_BOX + 4] == 302


# ---- 4. a uniform plan is no plan -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1])
def test_uniform_plan_gives_the_bytes_of_the_unplanned_hooks(method):
    s = PlanSteps(E, 3, seed=1, method=method, top_k=3, top_k_map=4, topk_image=7, p=0.6, p_map=0.3)
    s.prev_box[:] = s.rng.integers(0, 1028, s.prev_box.shape)
    s.random_bias()
    for j0, j1 in RUNS:
        lg = s.random_logits(j0, j1)
        unplanned = BiasSteps.run(s, j0, j1, lg)                        # umgen_dbg_token_steps_biased_detail with self.bias
        s.sp_of, s.sets, s.set_of = [dict(s.sp)] * 3, [dict(s.bias)], [0, 0, 0]
        got = s.run(j0, j1, lg)
        for k in OUT_KEYS:
            assert getattr(got, k).tobytes() == getattr(unplanned, k).tobytes(), k
        s.sp_of, s.sets, s.set_of = None, [], None                      # the switch at 0
        plain = s.run_plain_detail(j0, j1, lg)
        got = s.run(j0, j1, lg, want_logz=False)
        for k in OUT_KEYS:
            assert getattr(got, k).tobytes() == getattr(plain, k).tobytes(), k


def test_one_set_without_the_steps_class_is_the_unbiased_step():
    """umgen_dbg_token_steps_biased with a bbox3d table alone is the plan of one set that has no map and no image table: on a two-step walk of map
    positions and one of image positions, tokens and x_next have the bytes of umgen_dbg_token_steps_logp on the same rows, and logz is +0.0"""
    s = PlanSteps(E, 1, seed=3, top_k=3, top_k_map=4, topk_image=7)
    box = np.ascontiguousarray(random_table(s.rng, 11, s.V[2]))
    for j0 in (MAP_C0, IMG_C0):
        lg = s.random_logits(j0, j0 + 2)
        plain = LogpSteps.run(s, j0, j0 + 2, lg)
        got = s.blank(2)
        check(lib().umgen_dbg_token_steps_biased(s.tb.ref, C.byref(s.args(got, lg, j0, j0 + 2)), fp(got.logp), None, fp(box), None, fp(got.logz)))
        for k in ("tokens", "x_next", "logp"):
            assert getattr(got, k).tobytes() == getattr(plain, k).tobytes(), (j0, k)
        at = [slot_of(j0), slot_of(j0 + 1)]
        assert (got.logz[0, at].view(np.uint32) == ZERO_BITS).all(), f"logz at positions {j0}, {j0 + 1}: a class without a table in the one set is not +0.0"
        assert is_nan_bits(np.delete(got.logz[0], at)).all(), "a position without a sampled step lost its NaN"


# ---- 5. edges: vocabularies, one scene, the last scene --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("V", [5, 1028, 8192])
def test_the_last_scene_alone_has_settings_and_a_table(V, Bn):
    """only scene Bn - 1 is on a set and has settings of its own: an index taken without the scene's offset, or applied to another scene, moves the
    tokens of the walk.  V = 5 / 8192: the map and image vocabularies; V = 1028: the bbox3d steps"""
    s = PlanSteps(E, Bn, seed=V, top_k=3, top_k_map=4, topk_image=7)
    if V != 1028:
        s.with_vocab(V)
    s.prev_box[:] = s.rng.integers(0, 1028, s.prev_box.shape)
    s.sp_of = [dict(s.sp) for _ in range(Bn)]
    s.sp_of[-1] = sampler_params(method=1, p=0.5, p_map=0.5, temperature=0.8)
    s.sets = [{}, {1: random_table(s.rng, 1, s.V[1])[0], 2: random_table(s.rng, 11, s.V[2]), 3: random_table(s.rng, 1, s.V[3])[0]}]
    s.set_of = [-1] * (Bn - 1) + [1]
    runs = (RUNS[1],) if V == 1028 else (RUNS[0], RUNS[2])
    for j0, j1 in runs:
        s.check_plan(j0, j1, s.random_logits(j0, j1))


# ---- 6. the ego sampler ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bn", [1, 3])
def test_sample_ego_planned(Bn):
    """per-scene temperature / method and per-scene pose tables, all three components; the last scene is the one on set 1, scene 0 (of 3) has no set"""
    V, frame = 1024, 5
    rng = np.random.default_rng(40 + Bn)
    sps = [sampler_params(method=b % 2, top_k=3 + b, p=0.3 + 0.2 * b, temperature=0.6 + 0.4 * b) for b in range(Bn)]
    lg = rng.standard_normal((Bn, 3, V), dtype=np.float32)
    seeds = rng.integers(0, 2 ** 63, Bn).astype(np.uint64)
    pool = np.stack([random_table(rng, 3, V), random_table(rng, 3, V)])
    classes = np.array([1, 1], np.int32)
    set_of = np.array(([-1, 0, 1] if Bn == 3 else [1]), np.int32)
    ref = np.zeros((Bn, 3), np.int32)
    for b in range(Bn):
        wk = Walk(sps[b])
        for q in range(3):
            w = lg[b, q] if set_of[b] < 0 else biased(lg[b, q], pool[set_of[b], q])
            ref[b, q] = wk.sample(torch.from_numpy(w.copy()), sps[b]["top_k"], sps[b]["p"], rng_uniform(int(seeds[b]), frame, KSEQ + q, DRAW_MAIN))
    out, logp, logz = np.zeros((Bn, 3), np.int32), nan32((Bn, TOK)), nan32((Bn, TOK))
    rank, mass, ent = np.full((Bn, TOK), -1, np.int32), nan32((Bn, TOK)), nan32((Bn, TOK))
    check(lib().umgen_dbg_sample_ego_planned(fp(lg), V, C.byref(DbgSamplerParams(**sampler_params())), u64p(seeds), frame, None, Bn, i32p(out), fp(logp),
                                             fp(logz), 0, i32p(rank), fp(mass), fp(ent), None, None, params_array(sps), fp(np.ascontiguousarray(pool)), 2,
                                             i32p(classes), i32p(set_of)))
    np.testing.assert_array_equal(out, ref)
    assert is_nan_bits(logp[:, 3:]).all() and is_nan_bits(logz[:, 3:]).all() and is_nan_bits(mass[:, 3:]).all() and (rank[:, 3:] == -1).all()
    for b in range(Bn):
        want = log_softmax_at(lg[b], out[b])
        assert (np.abs(logp[b, :3].astype(np.float64) - want) <= BAR * np.maximum(1.0, np.abs(want))).all()
        d = reference(lg[b], out[b], sps[b]["temperature"])      # the diagnostics on v, mass_above at the scene's own temperature
        assert (rank[b, :3] == d["rank"]).all() and np.abs(mass[b, :3] - d["mass"]).max() <= ABS_BAR and np.abs(ent[b, :3] - d["ent"]).max() <= ABS_BAR
        if Bn > 1:      # premise, on the references alone: another scene's temperature lies outside the bar wherever a token outranks the drawn one
            other = reference(lg[b], out[b], sps[(b + 1) % Bn]["temperature"])["mass"]
            assert np.abs(d["mass"] - other).max() > ABS_BAR or (d["rank"] == 0).all()
        if set_of[b] < 0:
            assert (logz[b, :3].view(np.uint32) == ZERO_BITS).all()
            continue
        tab = pool[set_of[b]]
        assert not np.isneginf(tab[np.arange(3), out[b]]).any()
        a, c = lse64(biased(lg[b], tab)), lse64(lg[b])
        assert (np.abs(logz[b, :3].astype(np.float64) - (a - c)) <= BAR * (np.maximum(1, np.abs(a)) + np.maximum(1, np.abs(c)))).all()
    # the switch at 0: the plain ego sampler's tokens
    plain, out0 = np.zeros((Bn, 3), np.int32), np.zeros((Bn, 3), np.int32)
    sp = DbgSamplerParams(**sps[0])
    check(lib().umgen_dbg_sample_ego(fp(lg), V, C.byref(sp), u64p(seeds), frame, None, Bn, i32p(plain)))
    check(lib().umgen_dbg_sample_ego_planned(fp(lg), V, C.byref(sp), u64p(seeds), frame, None, Bn, i32p(out0), None, None, 0, None, None, None, None, None,
                                             None, None, 0, None, None))
    np.testing.assert_array_equal(out0, plain)
