"""Constrained sampling inside the samplers (csrc/frame.hip), through umgen_dbg_token_steps_biased(_detail), umgen_dbg_sample_ego_biased and
umgen_dbg_sample_biased: with a table for the step's class in the call's one set, every sampler of a step draws from w = v + r -- the AR row, and the
head_tar_bbox3d row inside the control and pad-avoid resamples -- while lp and the diagnostics stay on v, and want_logz adds lse(w) - lse(v).

References (none measured on the code under test):
  * tokens, x_next, counters, boxes, step / epoch / done: the oracle's own sample / _sample_bbox / _rule walk (Steps.check) handed logits + r and
    logits_tar + r, formed here in float32 (one add, round to nearest; -inf where r is -inf);
  * lp: float64 log-softmax of the UNBIASED row at the drawn token, bar 1e-4 * max(1, |ref|) (tests/test_gpu_logp_kernel.py);
  * logz: float64 lse(w) - lse(v), bar 1e-4 * (max(1, |lse64(w)|) + max(1, |lse64(v)|)): that bar on each of the two log-sum-exps.
The rows are Steps' own: ld = 1100 columns per scene with 3e4 in every column past the position's vocabulary."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests.gpu_util import check, fp, lib
from oracle.umgen_oracle import exp_det
from tests.test_gpu_frame_kernels import (DRAW_MAIN, IMG_BOS, IMG_C0, KSEQ, MAP_C0, MAP_EOS, OFF_BOX, PAD, TOK, Walk, at_box, i32p, kind_of, nan32,
                                          object_tokens, rng_uniform, sampler_params, scripted, u64p)
from tests.test_gpu_logp_kernel import BAR, LogpSteps, is_nan_bits, slot_of
from tests.test_gpu_score import log_softmax_at
from umgen_amd._lib import DbgSamplerParams, DbgSteps

pytestmark = pytest.mark.gpu
E, B = 96, 3
NEG = np.float32(-np.inf)
ZERO_BITS = 0x00000000


def biased(v, r):
    """w = v + r in float32, -inf where r is -inf"""
    with np.errstate(invalid="ignore"):
        w = (np.asarray(v, np.float32) + np.asarray(r, np.float32)).astype(np.float32)
    return np.where(np.isneginf(r), NEG, w).astype(np.float32)


def lse64(rows):
    v = np.asarray(rows, np.float64)
    m = v.max(-1, keepdims=True)
    return (m + np.log(np.exp(v - m).sum(-1, keepdims=True)))[..., 0]


def random_table(rng, rows, V, keep=()):
    """finite bias in [-3, 3], about 30 % of every row banned; the tokens of `keep` stay allowed (bias 0)"""
    t = rng.uniform(-3.0, 3.0, (rows, V)).astype(np.float32)
    t[rng.random((rows, V)) < 0.3] = NEG
    for k in keep:
        t[:, k] = 0.0
    for r in range(rows):
        if np.isneginf(t[r]).all():
            t[r, 0] = 0.0
    return t


class BiasSteps(LogpSteps):
    """LogpSteps through umgen_dbg_token_steps_biased_detail with the tables self.bias = {1: [n_map], 2: [11, n_box], 3: [n_img]} (a missing class: no
    table); the walk is the oracle's on logits + r and logits_tar + r.  out gains logz [B, 2199] (handed over as NaN) and the diagnostics"""
    topk = 4

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bias = {}

    def random_bias(self, keep_box=()):
        self.bias = {1: random_table(self.rng, 1, self.V[1])[0], 2: random_table(self.rng, 11, self.V[2], keep_box), 3: random_table(self.rng, 1, self.V[3])[0]}

    def row_bias(self, j):
        """the class row of decode position j, or None"""
        kind = kind_of(j, self.given_end)
        t = self.bias.get(kind)
        if t is None:
            return None
        return t[(j - at_box(0)) % 11] if kind == 2 else t

    def args(self, out, logits, j0, j1):
        return DbgSteps(cond=fp(self.cond), logits=fp(logits), logits_tar=fp(self.logits_tar), prev_box=i32p(self.prev_box),
                        control_slot=self.control.ctypes.data_as(C.POINTER(C.c_ubyte)), forced=None if self.forced is None else i32p(self.forced),
                        seeds=u64p(self.seeds), tokens=i32p(out.tokens), x_next=fp(out.x_next), counters=i32p(out.counters), n_boxes=i32p(out.n_boxes),
                        boxes=out.boxes.ctypes.data_as(C.POINTER(C.c_double)), state_log=out.state.ctypes.data_as(C.POINTER(C.c_uint32)),
                        sp=DbgSamplerParams(**self.sp), B=self.B, j0=j0, j1=j1, given_end=self.given_end, ld_logits=self.ld,
                        use_forced=int(self.forced is not None), use_control=self.use_control, frame_idx=self.frame_idx, epoch0=self.epoch0)

    def blank(self, n):
        Bn, K = self.B, self.topk
        return types.SimpleNamespace(tokens=self.tokens.copy(), x_next=np.zeros((n, Bn, self.E), np.float32), counters=np.zeros(8, np.int32),
                                     n_boxes=np.zeros(Bn, np.int32), boxes=np.zeros((Bn, 64, 10), np.float64), state=np.zeros((n, 3), np.uint32),
                                     logp=nan32((Bn, TOK)), logz=nan32((Bn, TOK)), rank=np.full((Bn, TOK), -1, np.int32), mass=nan32((Bn, TOK)),
                                     ent=nan32((Bn, TOK)), tok=np.full((Bn, TOK, K), -1, np.int32), tlp=nan32((Bn, TOK, K)))

    def run(self, j0, j1, logits):
        out = self.blank(j1 - j0)
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        assert logits.shape == (j1 - j0, self.B, self.ld)
        tabs = [None if self.bias.get(k) is None else np.ascontiguousarray(self.bias[k], np.float32) for k in (1, 2, 3)]
        check(lib().umgen_dbg_token_steps_biased_detail(self.tb.ref, C.byref(self.args(out, logits, j0, j1)), fp(out.logp),
                                                        *[None if t is None else fp(t) for t in tabs], fp(out.logz), self.topk, i32p(out.rank),
                                                        fp(out.mass), fp(out.ent), i32p(out.tok), fp(out.tlp)))
        return out

    def run_plain_detail(self, j0, j1, logits):
        """the same input through the parent's umgen_dbg_token_steps_detail"""
        out = self.blank(j1 - j0)
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        check(lib().umgen_dbg_token_steps_detail(self.tb.ref, C.byref(self.args(out, logits, j0, j1)), fp(out.logp), self.topk, i32p(out.rank),
                                                 fp(out.mass), fp(out.ent), i32p(out.tok), fp(out.tlp)))
        return out

    def walk(self, j0, j1, logits):
        """the oracle's walk on the rows w: logits + r per position, logits_tar + r per bbox3d position"""
        lw = np.array(logits, np.float32)
        tar = self.logits_tar
        tw = tar.copy()
        for i, j in enumerate(range(j0, j1)):
            r = self.row_bias(j)
            if r is not None:
                lw[i, :, :r.shape[0]] = biased(lw[i, :, :r.shape[0]], r)
        if self.bias.get(2) is not None:
            for k in range(tw.shape[1]):
                tw[:, k] = biased(tar[:, k], self.bias[2][k % 11])
        self.logits_tar = tw
        try:
            return super().walk(j0, j1, lw)
        finally:
            self.logits_tar = tar

    def check_bias(self, j0, j1, logits):
        """Steps.check (tokens, x_next, counters, boxes, state against the walk on w), lp against float64 on v, logz against float64"""
        got, ref, want = self.check_logp(j0, j1, logits)      # (check_logp's reference is the UNBIASED row `logits` at the walk's drawn token)
        wz = np.full((self.B, TOK), np.nan)
        tol = np.zeros((self.B, TOK))
        exact0 = np.zeros((self.B, TOK), bool)
        for i, j in enumerate(range(j0, j1)):
            kind = kind_of(j, self.given_end)
            if not kind:
                continue
            at, v, r = slot_of(j), logits[i, :, :self.V[kind]], self.row_bias(j)
            if r is None or not np.any(r):
                wz[:, at], exact0[:, at] = 0.0, True
                continue
            a, b = lse64(biased(v, r)), lse64(v)
            wz[:, at], tol[:, at] = a - b, BAR * (np.maximum(1.0, np.abs(a)) + np.maximum(1.0, np.abs(b)))
        wrote = ~np.isnan(wz)
        assert is_nan_bits(got.logz[~wrote]).all(), "a position without a sampled step lost the NaN logz it was handed"
        assert (got.logz[exact0].view(np.uint32) == ZERO_BITS).all(), "logz of a class without a table (or an all-zero table) is not +0.0"
        err = np.abs(got.logz[wrote].astype(np.float64) - wz[wrote])
        print(f"logz: {int(wrote.sum())} values, max err {err.max():.3g}, smallest bar {tol[wrote & ~exact0].min() if (wrote & ~exact0).any() else 0:.3g}")
        assert np.isfinite(got.logz[wrote]).all() and (err <= tol[wrote]).all(), float(err.max())
        # every drawn token is allowed
        for i, j in enumerate(range(j0, j1)):
            r = self.row_bias(j)
            if r is not None and self.forced is None:
                assert not np.isneginf(r[ref.drawn[:, slot_of(j)]]).any(), f"a banned token was drawn at position {j}"
        return got, ref


RUNS = ((0, MAP_C0 + 6), (MAP_EOS - 3, at_box(13)), (IMG_BOS - 4, IMG_C0 + 6))


@pytest.mark.parametrize("method", [0, 1])
def test_biased_steps_equal_the_oracle_walk_on_w(method):
    """random rows, random tables with ~30 % bans, runs across map -> bbox3d -> image; lp on v (the bias makes a kernel that scored w fail); logz"""
    s = BiasSteps(E, B, method=method, top_k=3, top_k_map=4, topk_image=7, p=0.6, p_map=0.3)
    s.prev_box[:] = s.rng.integers(0, 1028, s.prev_box.shape)
    s.random_bias()
    for j0, j1 in RUNS:
        s.check_bias(j0, j1, s.random_logits(j0, j1))


@pytest.mark.parametrize("method", [0, 1])
def test_zero_tables_and_missing_tables_change_nothing(method):
    """all-zero tables, and no tables at all, give the bytes of umgen_dbg_token_steps_detail: tokens, x_next, counters, boxes, logp, every diagnostic;
    logz is +0.0 at every sampled position"""
    s = BiasSteps(E, B, seed=1, method=method, top_k=3, top_k_map=4, topk_image=7, p=0.6, p_map=0.3)
    s.prev_box[:] = s.rng.integers(0, 1028, s.prev_box.shape)
    for j0, j1 in RUNS:
        lg = s.random_logits(j0, j1)
        plain = s.run_plain_detail(j0, j1, lg)
        for tabs in ({1: np.zeros(s.V[1], np.float32), 2: np.zeros((11, s.V[2]), np.float32), 3: np.zeros(s.V[3], np.float32)}, {}):
            s.bias = tabs
            got = s.run(j0, j1, lg)
            for k in ("tokens", "x_next", "counters", "n_boxes", "boxes", "state", "logp", "rank", "mass", "ent", "tok", "tlp"):
                assert getattr(got, k).tobytes() == getattr(plain, k).tobytes(), (k, bool(tabs))
            sampled = np.array([slot_of(j) for j in range(j0, j1) if kind_of(j, s.given_end)], int)
            assert (got.logz[:, sampled].view(np.uint32) == ZERO_BITS).all()
            rest = np.setdiff1d(np.arange(TOK), sampled)
            assert is_nan_bits(got.logz[:, rest]).all()


@pytest.mark.parametrize("method", [0, 1])
def test_control_resample_draws_from_the_biased_tar_row(method):
    """test_step_control_resample's construction: the TAR peak sits on the masked column V - 1, the runner-up 77 would win; the table bans 77 at that
    attribute and lifts 99: the control draw yields 99"""
    s = BiasSteps(E, 2, rule_constrain=0, merge_ar_tar=0, method=method)
    s.use_control = 1
    s.control[0, 1] = 1
    s.control[1, 0] = 1
    s.logits_tar[0, 12] = 0
    s.logits_tar[0, 12, PAD] = 1e4
    s.logits_tar[0, 12, 77] = 50
    s.random_bias(keep_box=(5, 77, 99))
    j0, j1 = at_box(8), at_box(23)
    lg = s.peaked_logits(j0, j1, lambda b, j: 5)
    s.bias[2][:, 5] = 0.0
    unb = s.run_plain_detail(j0, j1, lg)
    assert unb.tokens[0, OFF_BOX + 12] == 77
    s.bias[2][12 % 11, 77] = NEG
    s.bias[2][12 % 11, 99] = 60.0
    got, ref = s.check_bias(j0, j1, lg)
    assert got.counters[1] == 11 + 2 and got.tokens[0, OFF_BOX + 12] == 99


@pytest.mark.parametrize("method", [0, 1])
def test_pad_avoid_resample_draws_from_the_biased_tar_row(method):
    """test_step_pad_avoid's construction: AR says pad, the previous frame had an object; the TAR row peaks on 300, which the table bans at that
    attribute while lifting 301: the pad-avoid draw yields 301"""
    s = BiasSteps(E, 2, rule_constrain=0, method=method)
    s.prev_box[0, 0:6] = [500, 1027, 3, 1027, 7, 1026]
    s.prev_box[1, 0:6] = 1027
    s.prev_box[1, 4] = 9
    s.logits_tar[:, 0:6] = 0
    s.logits_tar[:, 0:6, 300] = 1e4
    s.random_bias(keep_box=(PAD, 300, 301))
    j0, j1 = at_box(0), at_box(6)
    lg = s.peaked_logits(j0, j1, lambda b, j: PAD)
    unb = s.run_plain_detail(j0, j1, lg)
    assert unb.counters[0] == 5 and unb.tokens[0, OFF_BOX] == 300
    s.bias[2][0:6, 300] = NEG
    s.bias[2][0:6, 301] = 50.0
    got, ref = s.check_bias(j0, j1, lg)
    assert got.counters[0] == 5 and not got.counters[1:6].any()
    assert list(got.tokens[0, OFF_BOX:OFF_BOX + 6]) == [301, PAD, 301, PAD, 301, 301] and got.tokens[1, OFF_BOX + 4] == 301


def test_rule_constraint_blanks_to_pad_whatever_the_tables_say():
    """test_step_rule_constraint's scene under tables that ban pad in every row: no draw yields pad, the blank still writes it (a non-draw), lp and logz
    keep the values of the tokens that were drawn"""
    cross, far, free = object_tokens(2.0, 0.0), object_tokens(63.5, 0.0), object_tokens(-30.0, 20.0)
    j0, j1 = at_box(0), at_box(44)
    s = BiasSteps(E, 3)
    s.prev_box[1, 11:22] = 5
    s.random_bias(keep_box=sorted(set(cross + far + free)))
    s.bias[2][:, PAD] = NEG
    lg = s.peaked_logits(j0, j1, scripted([free, cross, far, cross]))
    got, ref = s.check_bias(j0, j1, lg)
    assert np.all(got.tokens[0, OFF_BOX + 11:OFF_BOX + 22] == PAD) and list(got.counters[2:5]) == [12, 7, 6]


# ---- the sampler's edges -------------------------------------------------------------------------------------------------------------------
def expected_token(wk, w, k, p, u):
    """OracleUMGen.sample on w where its walk finds a hit -- a banned token can only come out of its no-hit fallback -- else the last allowed entry in
    walk order: ascending index among the kept set (top-k), descending probability with ties by index inside the nucleus (top-p)"""
    tok = wk.sample(torch.from_numpy(w.copy()), k, p, u)
    if w[tok] > NEG:
        return tok
    if wk.cfg.sample_method == "topk":
        return int(np.flatnonzero(w > NEG)[-1])
    assert p >= 1.0                                      # (a nucleus below 1 ends on an entry of positive probability)
    z = w / np.float32(wk.cfg.sfmx_temp)
    pr = exp_det(z - z.max())
    pr = pr / np.cumsum(pr, dtype=np.float32)[-1]
    order = np.argsort(-pr, kind="stable")               # the oracle's walk order: descending probability, ties by ascending index
    return int([i for i in order if w[i] > NEG][-1])


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("V", [5, 1028, 8192])
def test_bans_at_the_samplers_edges(V, k, method):
    rng = np.random.default_rng(V + 10 * k + method)
    us = np.array([0.0, 0.5, 1.0 - 2.0 ** -24], np.float32)
    rows = []      # (v, r, mask_idx, p)

    def table(allowed):
        r = np.full(V, NEG, np.float32)
        r[np.asarray(allowed)] = rng.uniform(-3, 3, len(allowed)).astype(np.float32)
        return r
    v = rng.standard_normal(V).astype(np.float32)
    rows.append((v, table([V // 2]), -1, 0.7))                                                     # exactly one allowed token
    rows.append((v, table([0]), V - 1, 0.7))                                                       # ... with the mask on another index
    few = rng.choice(V, size=max(1, min(V - 1, k) - 1), replace=False)
    rows.append((v, table(few), -1, 0.7))                                                          # fewer allowed tokens than k
    rows.append((v, table(np.setdiff1d(few, [V - 1]) if len(few) > 1 else [0]), V - 1, 0.7))       # ... together with mask_idx = V - 1
    r = np.where(rng.random(V) < 0.3, NEG, np.float32(0)).astype(np.float32)                       # the k-th largest w ties with others
    r[:min(V, 3)] = 0
    t = rng.standard_normal(V).astype(np.float32)
    ties = rng.choice(np.flatnonzero(r == 0), size=min(int((r == 0).sum()), k + 2), replace=False)
    t[ties] = 4.0
    rows.append((t, r, -1, 0.7))
    rows.append((t, r, V - 1, 0.7))
    r = np.where(rng.random(V) < 0.3, NEG, rng.uniform(-3, 3, V)).astype(np.float32)               # ~30 % bans; p = 16: the image head's nucleus keeps everything
    r[0] = 0
    rows.append((v, r, -1, 16.0))
    rows.append((v, np.where(np.arange(V) == V - 1, np.float32(0), r).astype(np.float32), V - 1, 16.0))
    rows.append((v, table([V - 2 if V > 1 else 0]), -1, 16.0))
    wk = Walk(sampler_params(method=method))
    for p in sorted({row[3] for row in rows}):
        for mask in sorted({row[2] for row in rows if row[3] == p}):
            grp = [row for row in rows if row[3] == p and row[2] == mask]
            lg = np.ascontiguousarray(np.repeat(np.stack([g[0] for g in grp]), len(us), axis=0))
            bs = np.ascontiguousarray(np.repeat(np.stack([g[1] for g in grp]), len(us), axis=0))
            uu = np.ascontiguousarray(np.tile(us, len(grp)))
            out = np.full(len(uu), -1, np.int32)
            check(lib().umgen_dbg_sample_biased(method, fp(lg), fp(bs), len(uu), V, k, p, 1.0, mask, fp(uu), i32p(out)))
            for i in range(len(uu)):
                w = biased(lg[i], bs[i])
                if mask >= 0:
                    w[mask] = NEG
                assert w[out[i]] > NEG, f"row {i}: token {out[i]} is banned or masked (V={V} k={k} p={p} mask={mask} u={uu[i]})"
                want = expected_token(wk, w, k, p, np.float32(uu[i]))
                assert out[i] == want, f"row {i}: {out[i]} != {want} (V={V} k={k} p={p} mask={mask} u={uu[i]})"


# ---- the ego sampler -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("Bn", [1, 3])
def test_sample_ego_biased(Bn, method):
    V, frame = 1024, 5
    rng = np.random.default_rng(Bn + 7 * method)
    sp = sampler_params(method=method, top_k=4, p=0.5)
    lg = rng.standard_normal((Bn, 3, V), dtype=np.float32)
    seeds = rng.integers(0, 2 ** 63, Bn).astype(np.uint64)
    tab = random_table(rng, 3, V)
    wk = Walk(sp)
    ref = np.array([[wk.sample(torch.from_numpy(biased(lg[b, q], tab[q])), sp["top_k"], sp["p"], rng_uniform(int(seeds[b]), frame, KSEQ + q, DRAW_MAIN))
                     for q in range(3)] for b in range(Bn)], np.int32)
    for table in (tab, np.zeros((3, V), np.float32), None):
        out, logp, logz = np.zeros((Bn, 3), np.int32), nan32((Bn, TOK)), nan32((Bn, TOK))
        check(lib().umgen_dbg_sample_ego_biased(fp(lg), V, C.byref(DbgSamplerParams(**sp)), u64p(seeds), frame, None, Bn, i32p(out),
                                                None if table is None else fp(np.ascontiguousarray(table)), fp(logp), fp(logz)))
        assert is_nan_bits(logp[:, 3:]).all() and is_nan_bits(logz[:, 3:]).all()
        if table is tab:
            np.testing.assert_array_equal(out, ref)
            assert not np.isneginf(tab[np.arange(3)[None], out]).any()
            a, b = lse64(biased(lg, tab[None])), lse64(lg)
            err = np.abs(logz[:, :3].astype(np.float64) - (a - b))
            assert (err <= BAR * (np.maximum(1, np.abs(a)) + np.maximum(1, np.abs(b)))).all(), float(err.max())
        else:
            plain = np.zeros((Bn, 3), np.int32)
            check(lib().umgen_dbg_sample_ego(fp(lg), V, C.byref(DbgSamplerParams(**sp)), u64p(seeds), frame, None, Bn, i32p(plain)))
            np.testing.assert_array_equal(out, plain)
            assert (logz[:, :3].view(np.uint32) == ZERO_BITS).all()
        want = log_softmax_at(lg.reshape(Bn * 3, V), out.reshape(-1)).reshape(Bn, 3)      # lp on v
        err = np.abs(logp[:, :3].astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
        assert err.max() <= BAR, float(err.max())
