"""block_detail inside the samplers (csrc/frame.hip), through umgen_dbg_token_steps_detail / umgen_dbg_sample_ego_detail: a sampled step with
OarState::want_detail = 1 writes rank, mass_above, entropy and the detail_topk most likely tokens of the row it drew from into SampleArgs::detail
and changes nothing else.

Yardstick: float64 numpy on the very fp32 rows handed to the hook.  The rows are the fp32 bits, so rank (np.sum(row[:V] > row[tok])), the listed
tokens (a stable descending sort of row[:V]) and "is the settled token listed" are EXACT, without a tolerance.  The other three carry the bars the
existing tests hold the same quantities to on given fp32 logits:
  topk_logp             |got - ref| <= 1e-4 max(1, |ref|)   BAR of tests/test_gpu_logp_kernel.py: it is block_logp's value, formed the same way
  entropy, mass_above   |got - ref| <= 1e-5                 test_logits_detail_on_given_logits in tests/test_gpu_score_detail_kernel.py
Rows are ld columns per scene with 3e4 in every column past the position's vocabulary (Steps.mark_past_vocab): one column read past V changes the
maximum, and with it every output.  The ego hook's rows lie back to back ([3 B][V]), so a read past V meets the next row.

Shapes: V = 5 (< K: -1 / -inf fill), 48 and 56 (the tables' own map / image vocabularies), 257 (one thread with two columns), 1028 inside
1100-column rows (the bbox3d positions), 8192 (all 32 columns of every thread).  Each case carries the planted rows that fit its V."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from tests.gpu_util import check, fp, lib
from tests.test_gpu_frame_kernels import (BOX_C0, IMG_C0, MAP_C0, MAP_EOS, OFF_BOX, OFF_IMG, OFF_MAP, PAD, TOK, Tables, at_box, frame_tokens, i32p, nan32,
                                          object_tokens, sampler_params, scripted, u64p)
from tests.test_gpu_logp_kernel import BAR, LogpSteps, is_nan_bits, slot_of
from umgen_amd._lib import DbgSamplerParams, DbgSteps

pytestmark = pytest.mark.gpu
ABS_BAR = 1e-5                      # entropy and mass_above on given fp32 logits (tests/test_gpu_score_detail_kernel.py)
KMAX = 16
E = 96
STRADDLE = (0, 63, 64, 255, 256, 511, 512)            # lane, wave and register boundaries of the 256-thread block
ONE_THREAD = tuple(7 + 256 * i for i in range(16))    # 16 columns of thread 7
SPREAD = tuple(64 * i + (5 * i + 3) % 64 for i in range(16))   # 16 columns in 16 different (wave, lane) places: waves 0..3 four times over
# V -> (kind of position, first position, table sizes, columns per row)
CASES = {5: (1, MAP_C0, dict(n_map=5), 1100), 48: (1, MAP_C0, {}, 1100), 56: (3, IMG_C0, {}, 1100), 257: (1, MAP_C0, dict(n_map=257), 1100),
         1028: (2, BOX_C0, {}, 1100), 8192: (1, MAP_C0, dict(n_map=8192), 8192)}


@functools.lru_cache(maxsize=None)
def tables_for(V):
    return Tables(E, dims=dict(n_box=1028, **CASES[V][2]))


class DetailSteps(LogpSteps):
    """LogpSteps through umgen_dbg_token_steps_detail: out gains rank, mass, ent [B, 2199] and tok, tlp [B, 2199, topk], handed over as -1 / NaN"""
    topk = KMAX

    def __init__(self, V, B, seed=0, **sp):
        super().__init__(E, B, seed=seed, **sp)
        self.tb = tables_for(V)
        self.V = {1: self.tb.dims["n_map"], 2: self.tb.dims["n_box"], 3: self.tb.dims["n_img"]}
        self.kind, self.j0, _, self.ld = CASES[V]
        assert self.V[self.kind] == V
        self.tokens = frame_tokens(self.rng, self.tb, B)

    def args(self, out, logits, j0, j1):
        return DbgSteps(cond=fp(self.cond), logits=fp(logits), logits_tar=fp(self.logits_tar), prev_box=i32p(self.prev_box),
                        control_slot=self.control.ctypes.data_as(C.POINTER(C.c_ubyte)), forced=None if self.forced is None else i32p(self.forced),
                        seeds=u64p(self.seeds), tokens=i32p(out.tokens), x_next=fp(out.x_next), counters=i32p(out.counters), n_boxes=i32p(out.n_boxes),
                        boxes=out.boxes.ctypes.data_as(C.POINTER(C.c_double)), state_log=out.state.ctypes.data_as(C.POINTER(C.c_uint32)),
                        sp=DbgSamplerParams(**self.sp), B=self.B, j0=j0, j1=j1, given_end=self.given_end, ld_logits=self.ld,
                        use_forced=int(self.forced is not None), use_control=self.use_control, frame_idx=self.frame_idx, epoch0=self.epoch0)

    def blank(self, n):
        B = self.B
        return types.SimpleNamespace(tokens=self.tokens.copy(), x_next=np.zeros((n, B, self.E), np.float32), counters=np.zeros(8, np.int32),
                                     n_boxes=np.zeros(B, np.int32), boxes=np.zeros((B, 64, 10), np.float64), state=np.zeros((n, 3), np.uint32),
                                     logp=nan32((B, TOK)))

    def run(self, j0, j1, logits):
        B, K = self.B, self.topk
        out = self.blank(j1 - j0)
        out.rank, out.mass, out.ent = np.full((B, TOK), -1, np.int32), nan32((B, TOK)), nan32((B, TOK))
        out.tok, out.tlp = np.full((B, TOK, K), -1, np.int32), nan32((B, TOK, K))
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        assert logits.shape == (j1 - j0, B, self.ld)
        a = self.args(out, logits, j0, j1)
        check(lib().umgen_dbg_token_steps_detail(self.tb.ref, C.byref(a), fp(out.logp), K, i32p(out.rank), fp(out.mass), fp(out.ent),
                                                 i32p(out.tok) if K else None, fp(out.tlp) if K else None))      # (a changed guard band is UMGEN_E_STATE)
        return out

    def run_logp(self, j0, j1, logits):
        """the same input through umgen_dbg_token_steps_logp"""
        out = self.blank(j1 - j0)
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        check(lib().umgen_dbg_token_steps_logp(self.tb.ref, C.byref(self.args(out, logits, j0, j1)), fp(out.logp)))
        return out


def reference(rows, tok, tau):
    """float64 statistics of fp32 rows [R, V] at tokens tok [R] -> dict of [R] / [R, 16] arrays (lists padded with -1 / -inf past V)"""
    R, V = rows.shape
    v = rows.astype(np.float64)
    t = v[np.arange(R), tok][:, None]
    c = v - v.max(1, keepdims=True)
    e = np.exp(c)
    S = e.sum(1)
    z = np.exp(c / tau)
    order = np.argsort(-rows, axis=1, kind="stable")[:, :KMAX]
    tlp = np.take_along_axis(c, order, 1) - np.log(S)[:, None]
    pad = KMAX - order.shape[1]
    return {"rank": (rows > rows[np.arange(R), tok][:, None]).sum(1), "mass": (z * (v > t)).sum(1) / z.sum(1), "ent": np.log(S) - (e * c).sum(1) / S,
            "tok": np.pad(order, ((0, 0), (0, pad)), constant_values=-1), "tlp": np.pad(tlp, ((0, 0), (0, pad)), constant_values=-np.inf)}


def planted_rows(V, rng):
    """[(name, row [V], target)]: the planted rows that fit V, then random rows whose targets sit at float64 ranks 0, 1, 4, V // 2 and V - 1"""
    out = []
    out.append(("equal", np.full(V, 0.25, np.float32), 11 % V))
    r = np.zeros(V, np.float32)
    r[V // 3] = 1e4
    out.append(("peaked", r, V // 3))
    out.append(("scale80", (80.0 * rng.standard_normal(V)).astype(np.float32), int(rng.integers(0, V))))
    r = np.round(2.0 * rng.standard_normal(V)).astype(np.float32)                  # many exact ties, the target among them
    r[0] = r[V - 1] = r[V // 2]
    out.append(("tied", r, V // 2))
    cols = [c for c in STRADDLE if c < V]
    if len(cols) > 1:
        r = rng.standard_normal(V).astype(np.float32)
        r[cols] = 9.0
        out.append(("straddle", r, cols[len(cols) // 2]))
    for name, cols in (("one_thread", ONE_THREAD), ("spread", SPREAD)):
        if max(cols) < V:
            r = rng.standard_normal(V).astype(np.float32)
            order = rng.permutation(16)                                            # planted maxima, descending in a scrambled column order
            r[np.array(cols)[order]] = 30.0 - np.arange(16)
            out.append((name, r, int(np.array(cols)[order][7])))
    for i, want in enumerate((0, 1, 4, V // 2, V - 1)):
        r = (3.0 * rng.standard_normal(V)).astype(np.float32)
        out.append((f"random{i}", r, int(np.argsort(-r, kind="stable")[min(want, V - 1)])))
    return out


@functools.lru_cache(maxsize=None)
def case(V, B, forced, method, tau):
    """One hook run per (V, B, forced, method, tau): the planted rows, row r at step r // B of scene r % B -> (steps, logits, hook outputs, rows, targets)"""
    s = DetailSteps(V, B, seed=V, method=method, temperature=tau, top_k=3, top_k_map=4, topk_image=7, p=0.6, p_map=0.3, rule_constrain=0)
    rng = np.random.default_rng(1000 + V)
    rows = planted_rows(V, rng)
    while len(rows) % B:
        rows.append((f"fill{len(rows)}", (3.0 * rng.standard_normal(V)).astype(np.float32), int(rng.integers(0, V))))
    n = len(rows) // B
    lg = np.full((n, B, s.ld), 3e4, np.float32)
    for r, (_, row, _) in enumerate(rows):
        lg[r // B, r % B, :V] = row
    if forced:
        s.forced = frame_tokens(s.rng, s.tb, B)
        for r, (_, _, tgt) in enumerate(rows):
            s.forced[r % B, slot_of(s.j0 + r // B)] = tgt
    got = s.run(s.j0, s.j0 + n, lg)
    return s, lg, got, rows


def gather(s, got, n_rows, key):
    """hook output `key` of row r (step r // B of scene r % B) -> [R, ...]"""
    a = getattr(got, key)
    return np.stack([a[r % s.B, slot_of(s.j0 + r // s.B)] for r in range(n_rows)])


def check_against_float64(tag, rows, tok, tau, got, K=KMAX):
    """got: dict of [R] / [R, K] arrays.  Exact: rank, the listed tokens.  Bars: the docstring's.  Returns the largest distances."""
    ref = reference(rows, tok, tau)
    assert np.array_equal(got["rank"], ref["rank"]), (tag, "rank", got["rank"], ref["rank"])
    assert np.array_equal(got["tok"], ref["tok"][:, :K]), (tag, "topk_tok", got["tok"], ref["tok"][:, :K])
    d_mass = np.abs(got["mass"].astype(np.float64) - ref["mass"]).max()
    d_ent = np.abs(got["ent"].astype(np.float64) - ref["ent"]).max()
    want = ref["tlp"][:, :K]
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got["tlp"]), ~fin), (tag, "-inf exactly past the vocabulary")
    d_tlp = (np.abs(got["tlp"].astype(np.float64)[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))).max() if fin.any() else 0.0
    print(f"{tag}: {len(rows)} rows, mass_above {d_mass:.3g}, entropy {d_ent:.3g} (bar {ABS_BAR}); topk_logp {d_tlp:.3g} (bar {BAR})")
    assert np.isfinite(got["mass"]).all() and np.isfinite(got["ent"]).all(), tag
    assert d_mass <= ABS_BAR and d_ent <= ABS_BAR and d_tlp <= BAR, (tag, d_mass, d_ent, d_tlp)
    return d_mass, d_ent, d_tlp


@pytest.mark.parametrize("forced", [True, False])
@pytest.mark.parametrize("method,tau", [(0, 0.7), (1, 1.0)])
@pytest.mark.parametrize("V", sorted(CASES))
def test_detail_against_float64(V, method, tau, forced):
    B = 3
    s, lg, got, rows = case(V, B, forced, method, tau)
    R = len(rows)
    mat = np.stack([r for _, r, _ in rows])
    settled = gather(s, got, R, "tokens")
    if forced:
        assert np.array_equal(settled, [t for _, _, t in rows])
    out = {k: gather(s, got, R, k) for k in ("rank", "mass", "ent", "tok", "tlp")}
    check_against_float64(f"V {V} method {method} tau {tau} forced {forced}", mat, settled, tau, out)
    logp = gather(s, got, R, "logp")
    # where the settled token is listed its entry has the bits of the step's logp
    listed = out["tok"] == settled[:, None]
    for r in np.flatnonzero(listed.any(1)):
        k = int(np.argmax(listed[r]))
        assert out["tlp"][r, k].tobytes() == logp[r].tobytes(), (V, rows[r][0], out["tlp"][r, k], logp[r])
    ref_listed = (reference(mat, settled, tau)["tok"] == settled[:, None]).any(1)
    assert np.array_equal(listed.any(1), ref_listed), "is the settled token listed"
    if not forced and method == 0:
        # the main draw of the top-k sampler lies inside its support on the row it drew from: exact here
        k_of = {1: s.sp["top_k_map"], 2: s.sp["top_k"], 3: s.sp["topk_image"]}[s.kind]
        assert (out["rank"] < k_of).all(), (V, out["rank"])
    # every slot no sampled step reached keeps what it was handed
    wrote = np.zeros((B, TOK), bool)
    for r in range(R):
        wrote[r % B, slot_of(s.j0 + r // B)] = True
    assert (got.rank[~wrote] == -1).all() and (got.tok[~wrote] == -1).all()
    assert is_nan_bits(got.mass[~wrote]).all() and is_nan_bits(got.ent[~wrote]).all() and is_nan_bits(got.tlp[~wrote]).all()
    # tokens, x_next, counters, boxes, step state and logp: bit-equal to the _logp hook on the same input
    plain = s.run_logp(s.j0, s.j0 + R // B, lg)
    for k in ("tokens", "x_next", "counters", "n_boxes", "boxes", "state", "logp"):
        assert getattr(got, k).tobytes() == getattr(plain, k).tobytes(), (V, k)


@pytest.mark.parametrize("V", sorted(CASES))
def test_planted_rows(V):
    s, lg, got, rows = case(V, 3, True, 0, 0.7)
    R = len(rows)
    out = {k: gather(s, got, R, k) for k in ("rank", "mass", "ent", "tok", "tlp")}
    at = {name: r for r, (name, _, _) in enumerate(rows)}
    K = min(KMAX, V)
    r = at["equal"]      # nothing above, the uniform distribution's entropy, the lowest indices win the ties
    assert out["rank"][r] == 0 and out["mass"][r] == 0.0 and abs(out["ent"][r] - np.log(V)) <= ABS_BAR
    assert out["tok"][r, :K].tolist() == list(range(K)) and (out["tok"][r, K:] == -1).all() and np.isneginf(out["tlp"][r, K:]).all()
    r = at["peaked"]     # all mass on the target
    assert out["rank"][r] == 0 and out["mass"][r] == 0.0 and out["ent"][r] == 0.0 and out["tok"][r, 0] == rows[r][2] and out["tlp"][r, 0] == 0.0
    r = at["scale80"]    # the centred entropy does not cancel at logits of scale 80
    assert np.abs(rows[r][1]).max() > (100 if V >= 48 else 40) and np.isfinite(out["ent"][r]) and 0.0 <= out["ent"][r] < 3.0
    r = at["tied"]       # ties are not counted
    row, tgt = rows[r][1], rows[r][2]
    assert (row == row[tgt]).sum() > 1 and out["rank"][r] == (row > row[tgt]).sum()
    if "straddle" in at:      # equal maxima across lane, wave and register boundaries come back in ascending index order
        r = at["straddle"]
        cols = [c for c in STRADDLE if c < V]
        assert out["tok"][r, :len(cols)].tolist() == cols and out["rank"][r] == 0
    for name, cols in (("one_thread", ONE_THREAD), ("spread", SPREAD)):
        if name in at:        # 16 distinct planted maxima: all in one thread's registers, or in 16 places across the waves
            r = at[name]
            row = rows[r][1]
            assert sorted(out["tok"][r].tolist()) == sorted(cols) and (np.diff(row[out["tok"][r]]) == -1).all() and out["rank"][r] == 7
    assert ("one_thread" in at) == (V == 8192) and ("spread" in at) == (V >= 1028) and ("straddle" in at) == (V >= 64)


@pytest.mark.parametrize("V", [5, 257, 1028])
def test_shorter_lists_are_heads_and_scenes_do_not_depend_on_the_batch(V):
    s, lg, got, rows = case(V, 3, True, 0, 0.7)
    n = len(rows) // 3
    for K in (0, 1, 5):
        s.topk = K
        short = s.run(s.j0, s.j0 + n, lg)
        s.topk = KMAX
        for k in ("rank", "mass", "ent", "logp", "tokens", "x_next"):
            assert getattr(short, k).tobytes() == getattr(got, k).tobytes(), (V, K, k)
        assert short.tok.tobytes() == np.ascontiguousarray(got.tok[:, :, :K]).tobytes(), (V, K)
        assert short.tlp.tobytes() == np.ascontiguousarray(got.tlp[:, :, :K]).tobytes(), (V, K)
    for b in range(3):       # B = 1: the bits of the same rows inside B = 3
        one = s.scene(b).run(s.j0, s.j0 + n, lg[:, b:b + 1])
        for k in ("rank", "mass", "ent", "tok", "tlp", "logp", "tokens"):
            assert getattr(one, k)[0].tobytes() == getattr(got, k)[b].tobytes(), (V, b, k)


def test_given_positions_keep_the_fill():
    """with the map given its positions are fixed-token steps: nothing is written there; the first bbox3d steps behind them are"""
    s = DetailSteps(1028, 2, rule_constrain=0)
    s.given_end = MAP_EOS + 1
    j0, j1 = MAP_EOS - 4, at_box(5)
    lg = s.random_logits(j0, j1)
    got = s.run(j0, j1, lg)
    m = slice(OFF_MAP, OFF_BOX)
    assert (got.rank[:, m] == -1).all() and (got.tok[:, m] == -1).all() and is_nan_bits(got.mass[:, m]).all() and is_nan_bits(got.ent[:, m]).all()
    assert is_nan_bits(got.tlp[:, m]).all() and is_nan_bits(got.logp[:, m]).all()
    b5 = slice(OFF_BOX, OFF_BOX + 5)
    rows = np.stack([lg[at_box(k) - j0, b, :1028] for b in range(2) for k in range(5)])
    out = {k: getattr(got, k)[:, b5].reshape((10,) + getattr(got, k).shape[2:]) for k in ("rank", "mass", "ent", "tok", "tlp")}
    check_against_float64("behind a given map", rows, got.tokens[:, b5].reshape(-1), 1.0, out)
    assert (got.rank[:, OFF_BOX + 5:] == -1).all()


def test_blanked_slots_keep_the_diagnostics_of_the_drawn_tokens():
    """the inputs of test_step_rule_constraint (tests/test_gpu_logp_kernel.py likewise): a blanked slot's 11 tokens come back as pad, its diagnostics are
    those of the tokens that were drawn -- on peaked rows rank 0, entropy 0, the drawn token listed first with logp's bits (0), where pad would rank 1"""
    cross, far, free = object_tokens(2.0, 0.0), object_tokens(63.5, 0.0), object_tokens(-30.0, 20.0)
    j0, j1 = at_box(0), at_box(44)
    s = DetailSteps(1028, 3)
    s.prev_box[1, 11:22] = 5
    lg = s.peaked_logits(j0, j1, scripted([free, cross, far, cross]))
    got, ref = s.run(j0, j1, lg), s.walk(j0, j1, lg)
    np.testing.assert_array_equal(got.tokens, ref.tokens)
    sl = slice(OFF_BOX, OFF_BOX + 44)
    blank = (got.tokens[:, sl] == PAD) & (ref.drawn[:, sl] != PAD)
    assert got.counters[4] == 6 and blank.sum() == 6 * 11
    assert (got.rank[:, sl] == 0).all() and (got.ent[:, sl] == 0).all() and (got.mass[:, sl] == 0).all()
    assert np.array_equal(got.tok[:, sl, 0], ref.drawn[:, sl]) and (got.tlp[:, sl, 0] == 0).all() and (got.logp[:, sl] == 0).all()


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [5, 1024, 1028])
def test_sample_ego_detail(V, B, method):
    """the ego sampler's rows ([3 B][V] back to back) with the planted rows that fit, sampled and forced; K = 16 and its heads"""
    tau, frame = 0.7, 5
    rng = np.random.default_rng(V + B + method)
    sp = DbgSamplerParams(**sampler_params(method=method, top_k=4, p=0.5, temperature=tau))
    planted = planted_rows(V, rng)
    pick = rng.permutation(len(planted))[:3 * B] if len(planted) >= 3 * B else np.arange(3 * B) % len(planted)
    mat = np.stack([planted[i][1] for i in pick])
    seeds = rng.integers(0, 2 ** 63, B).astype(np.uint64)
    forced = rng.integers(0, V, (B, TOK)).astype(np.int32)
    forced[:, :3] = np.array([planted[i][2] for i in pick]).reshape(B, 3)
    plain, plain_lp = np.zeros((B, 3), np.int32), nan32((B, TOK))
    for f in (None, forced):
        fptr = None if f is None else i32p(f)
        check(lib().umgen_dbg_sample_ego_logp(fp(mat), V, C.byref(sp), u64p(seeds), frame, fptr, B, i32p(plain), fp(plain_lp)))
        first = None
        for K in (16, 5, 1, 0):
            out, logp = np.zeros((B, 3), np.int32), nan32((B, TOK))
            rank, mass, ent = np.full((B, TOK), -1, np.int32), nan32((B, TOK)), nan32((B, TOK))
            tok, tlp = np.full((B, TOK, K), -1, np.int32), nan32((B, TOK, K))
            check(lib().umgen_dbg_sample_ego_detail(fp(mat), V, C.byref(sp), u64p(seeds), frame, fptr, B, i32p(out), fp(logp), K, i32p(rank), fp(mass),
                                                    fp(ent), i32p(tok) if K else None, fp(tlp) if K else None))
            assert out.tobytes() == plain.tobytes() and logp.tobytes() == plain_lp.tobytes()
            assert (rank[:, 3:] == -1).all() and is_nan_bits(mass[:, 3:]).all() and is_nan_bits(ent[:, 3:]).all()
            assert (tok[:, 3:] == -1).all() and is_nan_bits(tlp[:, 3:]).all()
            got = {"rank": rank[:, :3].reshape(-1), "mass": mass[:, :3].reshape(-1), "ent": ent[:, :3].reshape(-1), "tok": tok[:, :3].reshape(3 * B, K),
                   "tlp": tlp[:, :3].reshape(3 * B, K)}
            if K == 16:
                first = got
                check_against_float64(f"ego V {V} B {B} method {method} forced {f is not None}", mat, out.reshape(-1), tau, got)
                listed = got["tok"] == out.reshape(-1)[:, None]
                for r in np.flatnonzero(listed.any(1)):
                    assert got["tlp"][r, int(np.argmax(listed[r]))].tobytes() == logp[:, :3].reshape(-1)[r].tobytes()
                if f is None and method == 0:
                    assert (got["rank"] < 4).all()
            else:
                for k in ("rank", "mass", "ent"):
                    assert got[k].tobytes() == first[k].tobytes(), (K, k)
                assert got["tok"].tobytes() == np.ascontiguousarray(first["tok"][:, :K]).tobytes()
                assert got["tlp"].tobytes() == np.ascontiguousarray(first["tlp"][:, :K]).tobytes()
        if B == 3 and f is not None:      # a scene alone: the bits it has inside the batch
            for b in range(B):
                o1, l1 = np.zeros((1, 3), np.int32), nan32((1, TOK))
                r1, m1, e1, t1, p1 = np.full((1, TOK), -1, np.int32), nan32((1, TOK)), nan32((1, TOK)), np.full((1, TOK, 16), -1, np.int32), nan32((1, TOK, 16))
                check(lib().umgen_dbg_sample_ego_detail(fp(np.ascontiguousarray(mat[3 * b:3 * b + 3])), V, C.byref(sp), u64p(seeds[b:b + 1]), frame,
                                                        i32p(np.ascontiguousarray(f[b:b + 1])), 1, i32p(o1), fp(l1), 16, i32p(r1), fp(m1), fp(e1), i32p(t1), fp(p1)))
                sl = slice(3 * b, 3 * b + 3)
                assert r1[0, :3].tobytes() == first["rank"][sl].tobytes() and m1[0, :3].tobytes() == first["mass"][sl].tobytes()
                assert e1[0, :3].tobytes() == first["ent"][sl].tobytes() and t1[0, :3].tobytes() == first["tok"][sl].tobytes()
                assert p1[0, :3].tobytes() == first["tlp"][sl].tobytes()


def test_hooks_refuse_bad_detail_arguments():
    s = DetailSteps(48, 1)
    lg = s.random_logits(s.j0, s.j0 + 1)
    out = s.blank(1)
    a = s.args(out, lg, s.j0, s.j0 + 1)
    r, f, t, p = np.full((1, TOK), -1, np.int32), nan32((1, TOK)), np.full((1, TOK, 16), -1, np.int32), nan32((1, TOK, 16))
    call = lib().umgen_dbg_token_steps_detail
    assert call(s.tb.ref, C.byref(a), fp(out.logp), 17, i32p(r), fp(f), fp(f), i32p(t), fp(p)) == -1
    assert call(s.tb.ref, C.byref(a), fp(out.logp), -1, i32p(r), fp(f), fp(f), i32p(t), fp(p)) == -1
    assert call(s.tb.ref, C.byref(a), fp(out.logp), 4, i32p(r), fp(f), fp(f), None, fp(p)) == -1
    assert call(s.tb.ref, C.byref(a), fp(out.logp), 4, None, fp(f), fp(f), i32p(t), fp(p)) == -1
