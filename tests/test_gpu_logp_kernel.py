"""block_logp inside the samplers (csrc/frame.hip), through umgen_dbg_token_steps_logp / umgen_dbg_sample_ego_logp: the token step with
OarState::want_logp = 1 writes log softmax(AR row over [0, V))[settled token] into SampleArgs::logp and changes nothing else.

Reference: float64 log-softmax of the very logit row the hook was handed (tests/test_gpu_score.py log_softmax_at).  Bar: |got - ref| <= 1e-4 x
max(1, |ref|), the bar tests/test_gpu_score_kernel.py holds the same fp32 target-logit / log-sum-exp arithmetic to.  The rows are Steps' own:
ld = 1100 columns per scene with 3e4 in every column past the position's vocabulary, so one column read past V moves the result by ~3e4.
Everything the existing token-step tests assert (tokens, x_next, counters, boxes, step / epoch / done against the oracle's walk) is asserted
again on the logp hook by Steps.check."""
import ctypes as C
import types

import numpy as np
import pytest

from tests.gpu_util import check, fp, lib
from tests.test_gpu_frame_kernels import (BOX_C0, IMG_BOS, IMG_C0, KSEQ, MAP_C0, MAP_EOS, OFF_BOX, OFF_IMG, OFF_MAP, PAD, TOK, Steps, Walk, at_box,
                                          frame_tokens, i32p, kind_of, nan32, object_tokens, sampler_params, scripted, u64p)
from tests.test_gpu_score import log_softmax_at
from umgen_amd._lib import DbgSamplerParams, DbgSteps

pytestmark = pytest.mark.gpu
BAR = 1e-4
STEP_WIDTHS = [96, 1536]


def slot_of(j):
    """index of decode position j in a [2199] frame buffer, or None for bos / eos / pose-prefix positions"""
    if MAP_C0 <= j < MAP_EOS:
        return OFF_MAP + j - MAP_C0
    if BOX_C0 <= j < BOX_C0 + 660:
        return OFF_BOX + j - BOX_C0
    if IMG_C0 <= j < IMG_C0 + 512:
        return OFF_IMG + j - IMG_C0
    return None


def is_nan_bits(a):
    return np.ascontiguousarray(a).view(np.uint32) == 0x7FC00000


class LogpSteps(Steps):
    """Steps whose run goes through umgen_dbg_token_steps_logp: out.logp [B, 2199] starts as NaN; walk also keeps the tokens the samplers
    settled on BEFORE the rule constraint (out.drawn)"""

    def run(self, j0, j1, logits):
        B, E, n = self.B, self.E, j1 - j0
        out = types.SimpleNamespace(tokens=self.tokens.copy(), x_next=np.zeros((n, B, E), np.float32), counters=np.zeros(8, np.int32),
                                    n_boxes=np.zeros(B, np.int32), boxes=np.zeros((B, 64, 10), np.float64), state=np.zeros((n, 3), np.uint32),
                                    logp=nan32((B, TOK)))
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        assert logits.shape == (n, B, self.ld)
        a = DbgSteps(cond=fp(self.cond), logits=fp(logits), logits_tar=fp(self.logits_tar), prev_box=i32p(self.prev_box),
                     control_slot=self.control.ctypes.data_as(C.POINTER(C.c_ubyte)), forced=None if self.forced is None else i32p(self.forced),
                     seeds=u64p(self.seeds), tokens=i32p(out.tokens), x_next=fp(out.x_next), counters=i32p(out.counters), n_boxes=i32p(out.n_boxes),
                     boxes=out.boxes.ctypes.data_as(C.POINTER(C.c_double)), state_log=out.state.ctypes.data_as(C.POINTER(C.c_uint32)),
                     sp=DbgSamplerParams(**self.sp), B=B, j0=j0, j1=j1, given_end=self.given_end, ld_logits=self.ld,
                     use_forced=int(self.forced is not None), use_control=self.use_control, frame_idx=self.frame_idx, epoch0=self.epoch0)
        check(lib().umgen_dbg_token_steps_logp(self.tb.ref, C.byref(a), fp(out.logp)))
        return out

    def scene(self, b):
        s = super().scene(b)
        s.__class__ = type(self)
        return s

    def walk(self, j0, j1, logits):
        """the oracle's walk; the first argument of every _rule call is the token the samplers settled on at that position"""
        calls = []
        rule = Walk._rule

        def recording(wk, tok, inferred, dec, prev, pos):
            calls.append((pos - 1, int(tok)))
            return rule(wk, tok, inferred, dec, prev, pos)
        Walk._rule = recording
        try:
            ref = super().walk(j0, j1, logits)
        finally:
            Walk._rule = rule
        ref.drawn = ref.tokens.copy()
        if calls:            # scene after scene, every bbox3d position of [j0, j1) once
            per = len(calls) // self.B
            assert per * self.B == len(calls)
            for b in range(self.B):
                for j, tok in calls[b * per:(b + 1) * per]:
                    ref.drawn[b, slot_of(j)] = tok
        return ref

    def check_logp(self, j0, j1, logits):
        """Steps.check on the logp hook, then logp against float64 on the same rows -> (hook outputs, walk, float64 reference [B, 2199])"""
        got, ref = self.check(j0, j1, logits)
        want = np.full((self.B, TOK), np.nan)
        for i, j in enumerate(range(j0, j1)):
            kind = kind_of(j, self.given_end)
            if kind:
                at = slot_of(j)
                scored = self.forced[:, at] if self.forced is not None else ref.drawn[:, at]
                want[:, at] = log_softmax_at(logits[i, :, :self.V[kind]], scored)
        wrote = ~np.isnan(want)
        assert is_nan_bits(got.logp[~wrote]).all(), "a position without a sampled step lost the NaN it was handed"
        err = np.abs(got.logp[wrote].astype(np.float64) - want[wrote]) / np.maximum(1.0, np.abs(want[wrote]))
        print(f"E={self.E} B={self.B} steps [{j0}, {j1}): {int(wrote.sum())} values, max err {err.max():.3g} (bar {BAR})")
        assert np.isfinite(got.logp[wrote]).all() and err.max() <= BAR, float(err.max())
        return got, ref, want


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("E", STEP_WIDTHS)
def test_random_rows_over_every_kind_of_position(E, method):
    """top-k and top-p on N(0, 1) rows, B = 3, runs that cross bos / eos between the map, the bbox3d and the image section"""
    s = LogpSteps(E, 3, method=method, top_k=3, top_k_map=4, topk_image=7, p=0.6, p_map=0.3)
    s.prev_box[:] = s.rng.integers(0, 1028, s.prev_box.shape)
    for j0, j1 in ((0, MAP_C0 + 6), (MAP_EOS - 3, at_box(13)), (IMG_BOS - 4, IMG_C0 + 6)):
        s.check_logp(j0, j1, s.random_logits(j0, j1))


@pytest.mark.parametrize("E", STEP_WIDTHS)
def test_given_positions_keep_their_nan(E):
    """with the map given (given_end behind the map's eos) its positions are fixed-token steps: nothing is written there"""
    s = LogpSteps(E, 2, rule_constrain=0)
    s.given_end = MAP_EOS + 1
    j0, j1 = MAP_EOS - 4, at_box(5)
    got, _, want = s.check_logp(j0, j1, s.random_logits(j0, j1))
    assert np.isnan(want[:, OFF_MAP:OFF_BOX]).all() and not np.isnan(want[:, OFF_BOX:OFF_BOX + 5]).any()


@pytest.mark.parametrize("E", STEP_WIDTHS)
def test_resampled_tokens_are_scored_on_the_ar_row(E):
    """pad-avoid, control, and control-then-pad-avoid resamples draw from logits_tar; the value is the AR row's (the inputs of the existing
    test_step_pad_avoid / _control_resample / _control_then_pad_avoid)"""
    s = LogpSteps(E, 2, rule_constrain=0)
    s.prev_box[0, 0:6] = [500, 1027, 3, 1027, 7, 1026]
    s.prev_box[1, 0:6] = 1027
    s.prev_box[1, 4] = 9
    j0, j1 = at_box(0), at_box(6)
    got, ref, want = s.check_logp(j0, j1, s.peaked_logits(j0, j1, lambda b, j: PAD))
    assert got.counters[0] == 5
    moved = ref.drawn[:, OFF_BOX:OFF_BOX + 6] != PAD             # resampled away from the AR peak: scored ~ -1e4 on the AR row, not ~ 0
    assert moved.sum() == 5 and (got.logp[:, OFF_BOX:OFF_BOX + 6][moved] <= -9e3).all() and (got.logp[:, OFF_BOX:OFF_BOX + 6][~moved] == 0).all()

    s = LogpSteps(E, 2, rule_constrain=0, merge_ar_tar=0)
    s.use_control = 1
    s.control[0, 1] = 1
    s.control[1, 0] = 1
    s.logits_tar[0, 12] = 0
    s.logits_tar[0, 12, PAD] = 1e4
    s.logits_tar[0, 12, 77] = 50
    j0, j1 = at_box(8), at_box(23)
    got, ref, want = s.check_logp(j0, j1, s.peaked_logits(j0, j1, lambda b, j: 5))
    assert got.counters[1] == 13 and got.tokens[0, OFF_BOX + 12] == 77 and got.logp[0, OFF_BOX + 12] <= -9e3

    s = LogpSteps(E, 1, n_box=1030, rule_constrain=0)
    s.use_control = 1
    s.control[0, 0] = 1
    s.prev_box[0, 3] = 400
    s.logits_tar[0, 3] = 0
    s.logits_tar[0, 3, 1029] = 1e4
    s.logits_tar[0, 3, PAD] = 5e3
    got, ref, want = s.check_logp(at_box(3), at_box(4), s.peaked_logits(at_box(3), at_box(4), lambda b, j: 8))
    assert got.counters[1] == 1 and got.counters[0] == 1 and got.tokens[0, OFF_BOX + 3] == 1029 and got.logp[0, OFF_BOX + 3] <= -9e3


@pytest.mark.parametrize("E", STEP_WIDTHS)
def test_blanked_slots_return_pad_and_keep_the_drawn_tokens_values(E):
    """the inputs of test_step_rule_constraint and test_step_rule_more_than_30_boxes: a blanked slot's 11 tokens come back as pad, its 11 values
    are those of the tokens that were drawn (the walk's pre-rule tokens) -- on peaked rows exactly 0, where pad itself would score ~ -1e4"""
    cross, far, free = object_tokens(2.0, 0.0), object_tokens(63.5, 0.0), object_tokens(-30.0, 20.0)
    j0, j1 = at_box(0), at_box(44)
    s = LogpSteps(E, 3)
    s.prev_box[1, 11:22] = 5
    got, ref, want = s.check_logp(j0, j1, s.peaked_logits(j0, j1, scripted([free, cross, far, cross])))
    assert got.counters[4] == 6
    blank = (got.tokens[:, OFF_BOX:OFF_BOX + 44] == PAD) & (ref.drawn[:, OFF_BOX:OFF_BOX + 44] != PAD)
    assert blank.sum() == 6 * 11 and (got.logp[:, OFF_BOX:OFF_BOX + 44] == 0).all()

    objs = [object_tokens(x, y) for y in (-30.0, -15.0, 15.0, 30.0) for x in (-48.0, -36.0, -24.0, -12.0, 12.0, 24.0, 36.0, 48.0)]
    s = LogpSteps(E, 1)
    j0, j1 = at_box(0), at_box(11 * 34)
    got, ref, want = s.check_logp(j0, j1, s.peaked_logits(j0, j1, scripted(objs)))
    assert got.counters[4] >= 2 and (got.logp[0, OFF_BOX:OFF_BOX + 11 * 34] == 0).all()


@pytest.mark.parametrize("E", STEP_WIDTHS)
def test_forced_steps_carry_the_forced_tokens_value(E):
    """the inputs of test_step_teacher_forcing_skips_the_rule; peaked rows: exactly 0 at the peak, finite and <= -9e3 when forced elsewhere"""
    s = LogpSteps(E, 2)
    s.forced = frame_tokens(s.rng, s.tb, 2)
    cross = object_tokens(2.0, 0.0)
    s.forced[0, OFF_BOX:OFF_BOX + 11] = cross
    j0, j1 = at_box(0), at_box(22)
    got, ref, want = s.check_logp(j0, j1, s.peaked_logits(j0, j1, scripted([cross, cross])))
    assert got.counters[5] > 0
    lp = got.logp[:, OFF_BOX:OFF_BOX + 22]
    at_peak = np.array([[s.forced[b, OFF_BOX + k] == scripted([cross, cross])(b, BOX_C0 + k) for k in range(22)] for b in range(2)])
    assert at_peak[0, :11].all() and (lp[at_peak] == 0).all()
    assert (~at_peak).sum() > 0 and np.isfinite(lp).all() and (lp[~at_peak] <= -9e3).all()


@pytest.mark.parametrize("B", [3, 8])
def test_a_scene_alone_gives_the_bits_it_gives_in_the_batch(B):
    s = LogpSteps(96, B, seed=B)
    s.prev_box[:] = s.rng.integers(0, 1028, (B, 660))
    s.use_control = 1
    s.control[:] = s.rng.integers(0, 2, s.control.shape)
    for j0, j1 in ((MAP_EOS - 2, at_box(24)), (IMG_BOS - 4, IMG_C0 + 3)):
        lg = s.random_logits(j0, j1)
        got = s.run(j0, j1, lg)
        for b in range(B):
            one = s.scene(b).run(j0, j1, lg[:, b:b + 1])
            assert one.logp[0].tobytes() == got.logp[b].tobytes(), f"logp of scene {b} alone differs from scene {b} of the batch"
            np.testing.assert_array_equal(one.tokens[0], got.tokens[b])


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [1024, 1028])
def test_sample_ego_logp(V, B, method):
    """the ego sampler's three rows per scene ([3 B][V], no padding: the next row starts right behind column V - 1); sampled and forced"""
    frame = 5
    rng = np.random.default_rng(V + B + method)
    sp = sampler_params(method=method, top_k=4, p=0.5)
    lg = (3.0 * rng.standard_normal((B, 3, V))).astype(np.float32)
    seeds = rng.integers(0, 2 ** 63, B).astype(np.uint64)
    plain, out = np.zeros((B, 3), np.int32), np.zeros((B, 3), np.int32)
    check(lib().umgen_dbg_sample_ego(fp(lg), V, C.byref(DbgSamplerParams(**sp)), u64p(seeds), frame, None, B, i32p(plain)))
    forced = rng.integers(0, V, (B, TOK)).astype(np.int32)
    for f in (None, forced):
        logp = nan32((B, TOK))
        check(lib().umgen_dbg_sample_ego_logp(fp(lg), V, C.byref(DbgSamplerParams(**sp)), u64p(seeds), frame, None if f is None else i32p(f), B,
                                              i32p(out), fp(logp)))
        np.testing.assert_array_equal(out, plain if f is None else f[:, :3])
        want = log_softmax_at(lg.reshape(B * 3, V), out.reshape(-1)).reshape(B, 3)
        err = np.abs(logp[:, :3].astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
        print(f"ego V={V} B={B} method={method} forced={f is not None}: max err {err.max():.3g}")
        assert err.max() <= BAR and is_nan_bits(logp[:, 3:]).all()
    assert KSEQ == 2207
