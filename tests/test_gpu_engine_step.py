"""One decode step of the two persistent decode engines -- oar_engine_kernel (umgen_amd/csrc/oar_engine.hip, XCD-resident, E = 768) and
oar_engine_wide_kernel (oar_engine_wide.hip, chip-wide, E = 1536) -- against an fp64 restatement of the whole BlockOAR stack, through the hooks
umgen_dbg_oar_step (one step on a live handle, on the path that is asked for or not at all), umgen_dbg_oar_cache (reads / writes K/V cache rows)
and umgen_dbg_oar_epoch (moves the hand-off tag epoch forward).  Every test needs a GPU except the two at the end of the file.

Reference: stack_ref chains layer_ref of tests/test_gpu_decode_layer.py over the layers in fp64 on the engine's own operands -- weights as
stored (the state dict holds the already rounded values, so the engine's rounding is the identity), the K/V history as stored, the new K/V
row of every layer as the engine stored it (downloaded after the step and checked to be within 1 ulp + bar of its fp64 value).  Values must
satisfy |got - ref| <= bar * max(1, |ref|).  The same case through the five-launch layer form (use_engine 0) must meet LAYER_BAR on every
layer's new row and n_layers x LAYER_BAR on x (every layer adds at most its own bar; a layer passes a perturbation of x on with gain ~1 through
the residual): reference, weights and cache layout are right independently of the engines.

The preloaded history is shaped per (scene, head, layer) from the fp64 query of that layer, pattern (h + b + l) % 5: 0 the newest cached key
dominates the softmax, 1 a key on a seam of the engine's key partition dominates (xcd_seam / wide_seam / rows_seam restate the partition), 2 every cached
score equal, 3 random, 4 every cached key ~20 nats below the new token's own key (which the engines take from the q|k|v exchange, not from
the cache).  Row L starts as NaN bits, rows (L, L + 64] hold 7.0: the engines load them (clamped at the last cache row) and must mask them.
Every preloaded row but row L must come back bit for bit.

Positions: XCD_POS / WIDE_POS, derived from the partitions (see xcd_partition / wide_partition): empty halves / quarters / waves, one-key
halves / quarters, the wave span's 16 -> 32 step, exactly 3 register buffers against the first refill (767 / 769), exactly the 5 passes in
flight against the first round trip (1919 / 1921), the last position of a frame, the last cache row.

Fixed arithmetic (bit for bit on x and the new rows): a scene inside a batch == the scene alone; 8 / 4 / 2 / 1 groups per layer chain
(UMGEN_DEBUG_ENGINE_D); the 4-group kernel instance with background workers == the 8-group one; the tag-epoch wrap (drain, clear the granule
buffers, restart at tag 16) leaves a step's result unchanged although it runs on the tags the handle's first step used -- at step level on
every schedule and in the middle of a rollout.

Largest relative error of x against stack_ref over all cases, measured on an MI355X (bf16 | fp16), the five-launch path's distance on the
same cases, and the bars -- 3 x measured rounded up to one digit, and never above 1e-4 (a tenth of what the rollout tests allow: above it a
dropped key at L = 2206, 1 / 2207 of a head's weight, would fit under the bar):
  XCD-resident engine, 12 layers   4.5e-5 | 2.6e-6   ENGINE_BAR 1e-4 | 8e-6   five launches per layer 2.7e-6 | 3.1e-6 (bar 12 x LAYER_BAR)
  chip-wide engine, 4 layers       1.5e-6 | 1.6e-6   WIDE_BAR   5e-6 | 5e-6   five launches per layer 2.0e-6 | 1.7e-6 (bar 4 x LAYER_BAR)
  batched decode layer, 4 layers (use_engine 2; families rows, E = 768, and rows96, E = 96; the cases and tests are in tests/test_gpu_batched_step.py):
    rows                           2.8e-5 | 3.9e-6   ROWS_STEP_BAR 9e-5 | 2e-5   five launches per layer 1.7e-6 | 1.4e-6 (bar 4 x LAYER_BAR)
    rows96                         1.8e-5 | 3.6e-6   ROWS_STEP_BAR 6e-5 | 2e-5
  In bf16 the batched layer feeds all four GEMMs of a layer with hi + lo pairs (2^-17 per activation, decode_batched.hip split8), like the XCD-resident
  engine's MLP below; 1.4e-5 .. 2.8e-5 over all cases whatever L or B is.  Its wrong references at (1, 2206): a key dropped from the all-equal heads
  1.8e-3 | 1.7e-3, no lo part 1.5e-2 | 1.7e-3 (asserted to be >= 4 x the bar on the CPU, test_bar_sees_a_dropped_key_and_a_lost_lo_part).
FINDING: in bf16 the XCD-resident engine is 17 x further from fp64 than the five-launch path and than its own fp16 instantiation, and 3 x its
measured error (1.4e-4) is above 1e-4, so the bar stays at the cap, 2.2 x measured.  The error is the MLP's: c_fc and the mlp c_proj run on the
matrix cores with the fp32 activation split into hi + lo parts of the operand type (oar_engine.hip ln_split / split16), which keeps 16 mantissa
bits in bf16 (2^-17 relative per activation) against 22 in fp16.  Evidence: the same kernel in fp16 and the chip-wide engine in bf16 (fp32
activations) are at 2e-6 or below; a reference that drops the lo part altogether (LayerNorm output rounded to bf16, 2^-9) is 1.4e-2 away, and
1.4e-2 x 2^-8 = 5.5e-5 is what is measured; the error does not depend on L or on the schedule (2.3e-5 .. 4.5e-5 over all cases).  It is the
engine's documented design precision, not a lost key: the deliberately wrong references (a key dropped from the all-equal heads at L = 2206:
2.4e-3 | 2.3e-3 on the XCD engine, 1.5e-3 | 1.5e-3 on the chip-wide one; no lo part: >= 1.0e-2 | 1.3e-3 and >= 7.0e-3 | 8.3e-4 at every L)
are far outside every bar.
"""
import contextlib
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests.gpu_util import NAN16, SCALE_QK, ref_ln
from tests.test_gpu_decode_layer import LAYER_BAR, LMAX, check_kv_row, layer_params, layer_ref, rel_err, store, stored
from umgen_amd.config import MOD_ORDER, tiny_config
from umgen_amd.weights import expected_keys, synth_tensor

PRECS = [1, 2]                                        # bf16, fp16: fp32 has no engine
PREC_NAME = {1: "bf16", 2: "fp16"}
ENGINE_BAR = {1: 1e-4, 2: 8e-6}
WIDE_BAR = {1: 5e-6, 2: 5e-6}
XCD_POS = [0, 1, 15, 16, 32, 255, 256, 257, 767, 769, 1100, 2206, 2303]
WIDE_POS = [0, 1, 15, 16, 63, 64, 65, 1100, 1919, 1921, 2206, 2303]
# (scenes, position) on the 33-scene handle: every position at 1 and 2 scenes, every scene count at one position (<= 257 above 4 scenes: a case
# uploads megabytes).  5 and 9 split the shared tail layers unevenly, 23 is the largest default engine batch, 33 runs as rounds with a one-scene last round
MANY_B = [(1, 2206), (2, 2303), (3, 1100), (4, 769), (5, 257), (8, 256), (9, 255), (23, 32), (33, 16)]
MANY_CASES = sorted({(B, L) for B in (1, 2) for L in XCD_POS} | set(MANY_B))
WIDE_CASES = sorted({(1, L) for L in WIDE_POS} | {(2, 64), (2, 1919), (2, 2303)})
GUARD = 64                                            # finite rows preloaded behind row L
EPOCH_WRAP = 0xE0000000                               # engine_frame.hip / engine_decode.hip: an epoch above it drains, clears and restarts at tag 16
# the batched decode layer (tests/test_gpu_batched_step.py): no cached key, one, a full lane-group row and one past it, exactly one pass round and a
# second that holds the token's own key alone, exactly one flight batch, a second with the own key alone and one more, the middle of a frame, the last
# position of a frame, the last cache row
ROWS_POS = [0, 1, 15, 16, 63, 64, 65, 255, 256, 257, 1100, 2206, 2303]
# every position at 1 and 2 scenes; each of the four column-block instantiations full and ragged (L <= 257: a case uploads B x layers cache blocks)
ROWS_B = [(15, 65), (16, 256), (17, 257), (32, 64), (33, 63), (48, 16), (49, 15), (64, 65)]
ROWS_CASES = sorted({(B, L) for B in (1, 2) for L in ROWS_POS} | set(ROWS_B))
ROWS96_CASES = [(B, L) for B in (1, 17) for L in (0, 64, 257)]    # K = 96: three k-steps, waves 3 .. 7 of rows_mfma_kernel idle in the E-wide GEMMs
ROWS_STEP_BAR = {"rows": {1: 9e-5, 2: 2e-5}, "rows96": {1: 6e-5, 2: 2e-5}}      # on x and on the new rows (the table in the file header)

FAMILY = {"xcd": types.SimpleNamespace(E=768, H=16, layers=12, use=1), "wide": types.SimpleNamespace(E=1536, H=32, layers=4, use=3),
          # 4 layers: the first reads rows_to_frag's output, two read the previous ROWS_RESID's fragment copy, the last one's copy only the head would read
          "rows": types.SimpleNamespace(E=768, H=16, layers=4, use=2), "rows96": types.SimpleNamespace(E=96, H=2, layers=4, use=2)}
CASES = {"xcd": MANY_CASES, "wide": WIDE_CASES, "rows": ROWS_CASES, "rows96": ROWS96_CASES}


# ---------------------------------------------------------------------------------------------------------------------------
# the engines' key partitions, restated (oar_engine.hip "attention geometry of this CU", oar_engine_wide.hip "attention geometry of this rank")
# ---------------------------------------------------------------------------------------------------------------------------
def up16(n):
    return (n + 15) & ~15


def xcd_partition(L):
    """[(k_lo, k_hi)] of the 2 halves x 8 waves over the L + 1 keys (cached 0 .. L - 1 and the token's own); k_lo >= k_hi: a wave without keys"""
    nk = L + 1
    n0 = min(nk, up16((nk + 1) >> 1))
    out = []
    for ka, kb in ((0, n0), (n0, nk)):
        span = up16((kb - ka + 7) // 8)
        out += [(ka + w * span, min(kb, ka + w * span + span)) for w in range(8)]
    return n0, out


def wide_partition(L):
    """[(k_lo, k_hi)] of the 4 quarters x 6 compute waves"""
    nk = L + 1
    spn = up16((nk + 3) // 4)
    span = up16((spn + 5) // 6)
    return spn, [(sp * spn + w * span, min(nk, (sp + 1) * spn, sp * spn + w * span + span)) for sp in range(4) for w in range(6)]


def seam(cands, L):
    """the first of the candidate keys that is a cached key, key L - 1 when none is"""
    return next((k for k in cands if 0 <= k < L), L - 1)


def xcd_seam(L, b, h, l):
    """scene b alternates: last key of the first half, first of the second, a wave's first key, a wave's last key (the wave by head and layer)"""
    n0, waves = xcd_partition(L)
    live = [w for w in waves if w[0] < w[1]]
    lo, hi = live[(h + 3 * l) % len(live)]
    return seam([[n0 - 1], [n0], [lo, n0 - 1], [hi - 1, n0]][b % 4], L)


def wide_seam(L, b, h, l):
    spn, waves = wide_partition(L)
    live = [w for w in waves if w[0] < w[1]]
    lo, hi = live[(h + 3 * l) % len(live)]
    q = 1 + (h + l) % 3
    return seam([[q * spn - 1, spn - 1], [q * spn, spn], [lo, spn - 1], [hi - 1, spn]][b % 4], L)


def rows_partition(L):
    """attn_decode_batched_kernel (decode_batched.hip) over the L + 1 keys: key k is lane group k % 16 of wave (k // 16) % 4 in pass k // 64, and
    a wave requests 4 passes (a flight batch, 256 keys) before it uses the first; loads past the last key clamp to the token's own row.
    -> (flight batches, [(k_lo, k_hi)] of the 16-key wave passes that are requested, index 4 * pass + wave; k_lo >= k_hi: only clamped loads)"""
    nk = L + 1
    nflight = (((nk + 63) // 64) + 3) // 4
    return nflight, [(16 * (w + 4 * p), min(nk, 16 * (w + 4 * p) + 16)) for p in range(4 * nflight) for w in range(4)]


def rows_seam(L, b, h, l):
    """the scene (with the head's and the layer's turn among the seam heads) picks the edge: the last / first key of a 16-key wave pass, of a 64-key
    pass round, of a 256-key flight batch (which pass, round or batch: by head and layer), key 0"""
    nflight, passes = rows_partition(L)
    live = [p for p in passes if p[0] < p[1]]
    lo, hi = live[(h + 3 * l) % len(live)]
    r = (h + 3 * l) % ((L + 64) // 64)                 # a pass round with keys
    f = (h + 3 * l) % nflight
    return seam([[hi - 1, 15], [lo, 16], [64 * r + 63, 63], [64 * r, 64], [256 * f + 255, 255], [256 * f, 256], [0]][(b + h // 5 + 2 * l) % 7], L)


SEAM = {"xcd": xcd_seam, "wide": wide_seam, "rows": rows_seam, "rows96": rows_seam}


# ---------------------------------------------------------------------------------------------------------------------------
# operands: weights, state dict, shaped K/V history
# ---------------------------------------------------------------------------------------------------------------------------
def params(fam, prec):
    f = FAMILY[fam]
    return [layer_params(prec, f.E, 1000 * (l + 1) + f.E + prec)[1] for l in range(f.layers)]


def config(fam, **over):
    f = FAMILY[fam]
    return tiny_config(n_embd=f.E, n_head=f.H, n_oar_layer=f.layers, rule_constrain=False, **over).greedy()


def oar_entries(P, i):
    key = f"transformer.OAR.{i}"
    return {f"{key}.ln_1.weight": P["ln_a"], f"{key}.ln_2.weight": P["ln_b"],
            f"{key}.temporal_attn.c_attn.weight": P["Wqkv"], f"{key}.temporal_attn.c_attn.bias": P["bqkv"],
            f"{key}.temporal_attn.c_proj.weight": P["Wo"], f"{key}.temporal_attn.c_proj.bias": P["bo"],
            f"{key}.mlp.c_fc.weight": P["Wfc"], f"{key}.mlp.c_proj.weight": P["Wproj"]}


def state_items(fam, prec, **over):
    """synthetic_state_dict(cfg) with the BlockOAR entries replaced by the layers' values as stored (fp32 holds them exactly), one tensor at a time"""
    oar = {}
    for i, P in enumerate(params(fam, prec)):
        oar.update(oar_entries(P, i))
    for key, shape in expected_keys(config(fam, **over)).items():
        yield key, (oar[key].astype(np.float32) if key in oar else synth_tensor(key, shape, 3))


@functools.lru_cache(maxsize=None)
def base_rows(prec, H):
    """random K/V rows [2][H][LMAX][48] rounded to the cache type: (bits, values); a (scene, layer) history is a rotation of them"""
    rng = np.random.default_rng(77 + H)
    bits, val = store(rng.standard_normal((2, H, LMAX, 48), dtype=np.float32), prec)
    return bits, val.astype(np.float32)


def pattern(b, h, l):
    return (h + b + l) % 5


def shape_history(fam, prec, kbits, q, k_own, L, b, l):
    """In place on the K bits [H][>= L][48] of scene b, layer l: the patterns of the file header, built from the layer's fp64 query q [H][48]
    and the token's own key as stored k_own [H][48]"""
    if L == 0:
        return
    H = q.shape[0]
    for h in range(H):
        pat = pattern(b, h, l)
        if pat == 3:
            continue
        if pat == 2:
            kbits[h, :L] = kbits[h, :1]
            continue
        qn = np.linalg.norm(q[h])
        u = q[h] / qn
        if pat == 4:
            rows = slice(0, L)
            nats = float(q[h] @ k_own[h]) * SCALE_QK - 20.0         # the cached scores: random (sd ~1) around own score - 20
        else:
            key = L - 1 if pat == 0 else SEAM[fam](L, b, h, l)
            rows = slice(key, key + 1)
            nats = 25.0
        kbits[h, rows] = store(stored(kbits[h, rows], prec) + nats / (qn * SCALE_QK) * u, prec)[0]


def check_premises(fam, scores, L, l):
    """scores [B][H][L + 1] of layer l (the reference's own): the patterns are there"""
    if L == 0:
        return
    B, H = scores.shape[:2]
    for b in range(B):
        for h in range(H):
            pat, s = pattern(b, h, l), scores[b, h]
            if pat == 2:
                assert np.ptp(s[:L]) == 0, f"layer {l} scene {b} head {h}: the cached scores are not all equal"
            elif pat != 3:
                key = {0: L - 1, 1: SEAM[fam](L, b, h, l), 4: L}[pat]
                assert s.argmax() == key, f"layer {l} scene {b} head {h} pattern {pat}: key {key} does not dominate (arg max {s.argmax()})"
                if pat == 4:
                    assert s[:L].max() < s[L] - 10, f"layer {l} scene {b} head {h}: a cached key within 10 nats of the own key"


def stack_ref(x0, P, caches, new_rows, prec, L):
    """fp64 stack at position L: x0 [B][E]; P the layers' values as stored; caches[l] bits [B][2][H][n][48] (rows < L: the history);
    new_rows[l] bits [B][2][H][48] of row L as stored.  -> (x out, [l] the new K/V rows before rounding [B][2][H][48], [l] scores [B][H][L + 1])"""
    x = x0.astype(np.float64)
    kv_refs, scores = [], []
    for l, Pl in enumerate(P):
        hv = stored(np.ascontiguousarray(caches[l][:, :, :, :L]), prec)
        new = stored(np.ascontiguousarray(new_rows[l]), prec)
        x, q, kv = layer_ref(x, Pl, hv[:, 0], hv[:, 1], new[:, 0], new[:, 1])
        B, H = hv.shape[0], hv.shape[2]
        K = np.concatenate([hv[:, 0], new[:, 0][:, :, None]], axis=2)
        scores.append(np.einsum("bhd,bhnd->bhn", q.reshape(B, H, 48), K) * SCALE_QK)
        kv_refs.append(kv)
    return x, kv_refs, scores


def step_input(rng, B, E):
    return (rng.uniform(0.5, 2.0, (B, 1)) * rng.standard_normal((B, E)) + rng.uniform(-1, 1, (B, 1))).astype(np.float32)


@functools.lru_cache(maxsize=3)
def plan(fam, prec, B, L, guard=GUARD):
    """One case, on the CPU: x0 [B][E], and per layer the cache rows [B][2][H][n][48] to preload (n = rows 0 .. min(L + guard, LMAX - 1)): the
    history shaped from the layer's own fp64 query, NaN bits in row L, 7.0 behind it.  The chain uses the reference's own rounding of the new
    rows; the premises of the patterns are asserted on it (and again on the final reference of a GPU case)."""
    f = FAMILY[fam]
    E, H = f.E, f.H
    P = params(fam, prec)
    rng = np.random.default_rng(L + 10000 * B + prec)
    x0 = step_input(rng, B, E)
    n = min(L + guard, LMAX - 1) + 1
    bbits, _ = base_rows(prec, H)
    seven = store(np.full(1, 7.0), prec)[0][0]
    x = x0.astype(np.float64)
    caches = []
    for l, Pl in enumerate(P):
        qkv = ref_ln(x, Pl["ln_a"]) @ Pl["Wqkv"].T + Pl["bqkv"]
        q = qkv[:, :E].reshape(B, H, 48)
        new_bits, new_val = store(qkv[:, E:].reshape(B, 2, H, 48), prec)
        c = np.empty((B, 2, H, n, 48), np.uint16)
        for b in range(B):
            idx = (np.arange(L) + 131 * l + 17 * b) % LMAX
            c[b, :, :, :L] = bbits[:, :, idx]
            shape_history(fam, prec, c[b, 0], q[b], new_val[b, 0], L, b, l)
        c[:, :, :, L] = NAN16[prec]
        c[:, :, :, L + 1:] = seven
        hv = stored(np.ascontiguousarray(c[:, :, :, :L]), prec)
        K = np.concatenate([hv[:, 0], new_val[:, 0][:, :, None]], axis=2)
        check_premises(fam, np.einsum("bhd,bhnd->bhn", q, K) * SCALE_QK, L, l)
        x, _, _ = layer_ref(x, Pl, hv[:, 0], hv[:, 1], new_val[:, 0], new_val[:, 1])
        caches.append(c)
    return types.SimpleNamespace(fam=fam, prec=prec, B=B, L=L, n=n, x0=x0, caches=caches)


def sub_plan(pl, b):
    """scene b of a case as a one-scene case"""
    return types.SimpleNamespace(fam=pl.fam, prec=pl.prec, B=1, L=pl.L, n=pl.n, x0=pl.x0[b:b + 1], caches=[c[b:b + 1] for c in pl.caches])


# ---------------------------------------------------------------------------------------------------------------------------
# handles
# ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def env(**kv):
    """engine-creation switches are read from the environment at umgen_create, UMGEN_DEBUG_ENGINE_D at every step"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def create(which, prec, max_batch=None, max_cond_frames=4, **over):
    """many: the XCD-resident engine for every batch size up to 33 (8 groups; 12 layers: the production tail sharing, 4 tail layers on two groups
    each; UMGEN_BG_ENGINE=0 keeps a fresh one-scene handle of this kind on 8 groups); one: one scene per call, so the kernel instance with background
    workers on 4 groups; wide: the chip-wide engine for up to two scenes; rows / rows96: the batched decode layer for every batch size
    (UMGEN_DECODE_BATCHED=1) up to 64 / 17 scenes; rows5: the rows family's layers as five launches per layer for up to 17 scenes.
    max_cond_frames / over (tiny_config fields): a longer window (tests/test_gpu_bg_pass.py)"""
    from umgen_amd.engine import Engine
    fam = {"wide": "wide", "rows": "rows", "rows96": "rows96", "rows5": "rows"}.get(which, "xcd")
    switches = {"many": dict(UMGEN_DECODE_BATCHED=0, UMGEN_BG_ENGINE=0), "one": {}, "wide": dict(UMGEN_DECODE_WIDE=2),
                "rows": dict(UMGEN_DECODE_BATCHED=1), "rows96": dict(UMGEN_DECODE_BATCHED=1), "rows5": dict(UMGEN_DECODE_BATCHED=0, UMGEN_BG_ENGINE=0)}[which]
    with env(**switches):
        e = Engine(config(fam, **over), precision=PREC_NAME[prec],
                   max_batch=max_batch or {"many": 33, "one": 1, "wide": 2, "rows": 64, "rows96": 17, "rows5": 17}[which], max_cond_frames=max_cond_frames)
    e.load_state_dict(state_items(fam, prec, **over))
    e.finalize()
    e.fam, e.prec = fam, prec
    return e


def handles_fixture(which):
    """module-scoped: prec -> the handle of that precision, created on first use; used for nothing but single steps"""
    @pytest.fixture(scope="module")
    def fx():
        made = {}

        def get(prec):
            if prec not in made:
                made[prec] = create(which, prec)
            return made[prec]
        yield get
        for e in made.values():
            e.close()
    return fx


many = handles_fixture("many")
one = handles_fixture("one")
wide = handles_fixture("wide")


# ---------------------------------------------------------------------------------------------------------------------------
# one step on the GPU
# ---------------------------------------------------------------------------------------------------------------------------
def preload(e, pl, rows=None):
    """rows None: every preloaded row; else (row0, n) of them"""
    r0, nr = rows or (0, pl.n)
    for l, c in enumerate(pl.caches):
        for b in range(pl.B):
            e.dbg_oar_cache_put(l, b, r0, c[b][:, :, r0:r0 + nr])


def download(e, pl):
    return [np.stack([e.dbg_oar_cache_get(l, b, 0, pl.n) for b in range(pl.B)]) for l in range(len(pl.caches))]


def run_step(e, pl, use, x=None, L=None, load=True):
    """-> (x out [B][E], per layer the cache rows [B][2][H][n][48] behind the step)"""
    if load:
        preload(e, pl)
    out = e.dbg_oar_step(pl.x0 if x is None else x, pl.L if L is None else L, use)
    return out, download(e, pl)


def new_rows(got, L):
    return [np.ascontiguousarray(g[:, :, :, L]) for g in got]


def check_step(pl, before, x0, L, out, got, row_bar, premises):
    """Everything of one step but the bar on x: rows other than L unchanged, the new rows within 1 ulp + row_bar of fp64, finite x.
    before: the cache rows in front of the step.  -> relative error of x"""
    for l, (g, c) in enumerate(zip(got, before)):
        np.testing.assert_array_equal(np.delete(g, L, axis=3), np.delete(c, L, axis=3), err_msg=f"layer {l}: a cache row other than {L} changed")
    new = new_rows(got, L)
    ref_x, kv_refs, scores = stack_ref(x0, params(pl.fam, pl.prec), before, new, pl.prec, L)
    for l, (n_, r) in enumerate(zip(new, kv_refs)):
        try:
            check_kv_row(n_, r, pl.prec, row_bar)
        except AssertionError as err:
            raise AssertionError(f"layer {l}: {err}") from None
    if premises:
        for l, s in enumerate(scores):
            check_premises(pl.fam, s, L, l)
    assert np.all(np.isfinite(out)), "non-finite x (an empty partial weighed in? a masked row?)"
    return rel_err(out, ref_x)


def step_case(e, pl, bar):
    """The case on the engine and on five launches per layer, both against stack_ref; -> (engine's x out, its new rows)"""
    use = FAMILY[pl.fam].use
    out, got = run_step(e, pl, use)
    err = check_step(pl, pl.caches, pl.x0, pl.L, out, got, bar, True)
    preload(e, pl, (pl.L, 1))                                       # (every other row came back bit for bit)
    out5, got5 = run_step(e, pl, 0, load=False)
    err5 = check_step(pl, pl.caches, pl.x0, pl.L, out5, got5, LAYER_BAR, False)
    print(f"ENGSTEP {pl.fam} {PREC_NAME[pl.prec]} B={pl.B} L={pl.L}: engine {err:.3e} (bar {bar:.1e}), five launches {err5:.3e}")
    bar5 = len(pl.caches) * LAYER_BAR
    assert err5 <= bar5, f"five launches per layer: max error {err5:.3e} > {bar5:.1e}"
    assert err <= bar, f"max error {err:.3e} > bar {bar:.1e}"
    return out, new_rows(got, pl.L)


def same_bits(a, b, what):
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32), err_msg=f"{what}: x differs")
    for l, (ra, rb) in enumerate(zip(a[1], b[1])):
        np.testing.assert_array_equal(ra, rb, err_msg=f"{what}: the new K/V row of layer {l} differs")


def engine_only(e, pl, **kw):
    out, got = run_step(e, pl, FAMILY[pl.fam].use, **kw)
    return out, new_rows(got, pl.L)


@pytest.mark.gpu
@pytest.mark.parametrize("B,L", MANY_CASES)
@pytest.mark.parametrize("prec", PRECS)
def test_xcd_engine_step(many, prec, B, L):
    """8 groups per scene (B = 1), 4 (2), disjoint group sets (3, 4), the systolic schedule with shared tail layers (5 .. 23), rounds (33)"""
    step_case(many(prec), plan("xcd", prec, B, L), ENGINE_BAR[prec])


@pytest.mark.gpu
@pytest.mark.parametrize("L", XCD_POS)
@pytest.mark.parametrize("prec", PRECS)
def test_xcd_engine_step_with_background_workers(one, many, prec, L):
    """the kernel instance of engines for one scene per call (4 groups, the other XCDs' workgroups poll an empty op queue): against fp64, and bit
    for bit what the 8-group instance computes"""
    pl = plan("xcd", prec, 1, L)
    res = step_case(one(prec), pl, ENGINE_BAR[prec])
    same_bits(engine_only(many(prec), pl), res, "4 groups with background workers against 8 groups")


@pytest.mark.gpu
@pytest.mark.parametrize("B,L", WIDE_CASES)
@pytest.mark.parametrize("prec", PRECS)
def test_wide_engine_step(wide, prec, B, L):
    step_case(wide(prec), plan("wide", prec, B, L), WIDE_BAR[prec])


# ---------------------------------------------------------------------------------------------------------------------------
# fixed arithmetic: the schedule never changes a bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,L", MANY_B[1:])
@pytest.mark.parametrize("prec", PRECS)
def test_xcd_scene_in_a_batch_equals_the_scene_alone(many, prec, B, L):
    """scenes 0, the last, and the two around the middle (the tail layers' two groups take half the batch each)"""
    e, pl = many(prec), plan("xcd", prec, B, L)
    out, rows = engine_only(e, pl)
    for b in sorted({0, (B - 1) // 2, (B + 1) // 2, B - 1}):
        same_bits(engine_only(e, sub_plan(pl, b)), (out[b:b + 1], [r[b:b + 1] for r in rows]), f"scene {b} of {B}")


@pytest.mark.gpu
@pytest.mark.parametrize("L", [15, 257, 2206])
@pytest.mark.parametrize("prec", PRECS)
def test_xcd_groups_per_scene_do_not_change_a_bit(many, prec, L):
    """UMGEN_DEBUG_ENGINE_D (read at every step): the layers of one scene chained over 8, 4, 2 groups or kept on 1 (the in-group x edge)"""
    e, pl = many(prec), plan("xcd", prec, 1, L)
    res = {}
    for D in (8, 4, 2, 1):
        with env(UMGEN_DEBUG_ENGINE_D=D):
            res[D] = engine_only(e, pl)
    for D in (4, 2, 1):
        same_bits(res[D], res[8], f"{D} groups per scene against 8")


@pytest.mark.gpu
@pytest.mark.parametrize("L", [64, 1919, 2303])
@pytest.mark.parametrize("prec", PRECS)
def test_wide_scene_of_two_equals_the_scene_alone(wide, prec, L):
    e, pl = wide(prec), plan("wide", prec, 2, L)
    out, rows = engine_only(e, pl)
    same_bits(engine_only(e, sub_plan(pl, 1)), (out[1:], [r[1:] for r in rows]), "scene 1 of 2")


# ---------------------------------------------------------------------------------------------------------------------------
# carry-over: each path reads the rows the other wrote
# ---------------------------------------------------------------------------------------------------------------------------
def carry_over(e, fam, prec, B, L0, bar):
    pl = plan(fam, prec, B, L0)
    rng = np.random.default_rng(L0 + prec)
    preload(e, pl)
    before = [c.copy() for c in pl.caches]
    for t in range(4):
        use = FAMILY[fam].use if t % 2 == 0 else 0
        x = pl.x0 if t == 0 else step_input(rng, B, FAMILY[fam].E)
        out, got = run_step(e, pl, use, x=x, L=L0 + t, load=False)
        err = check_step(pl, before, x, L0 + t, out, got, bar if use else LAYER_BAR, t == 0)
        print(f"ENGSTEP carry-over {fam} {PREC_NAME[prec]} B={B} L={L0 + t} ({'engine' if use else 'five launches'}): {err:.3e}")
        lim = bar if use else len(pl.caches) * LAYER_BAR
        assert err <= lim, f"step {t} at L = {L0 + t} ({'engine' if use else 'five launches'}): max error {err:.3e} > {lim:.1e}"
        before = got


@pytest.mark.gpu
@pytest.mark.parametrize("L0", [14, 254])
@pytest.mark.parametrize("prec", PRECS)
def test_xcd_steps_carry_over(many, prec, L0):
    """four consecutive steps without a new preload, engine and five-launch steps alternating: rows 14 .. 17 fill the first half and open the
    second, 254 .. 257 cross the wave span's 16 -> 32 step"""
    carry_over(many(prec), "xcd", prec, 2, L0, ENGINE_BAR[prec])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_wide_steps_carry_over(wide, prec):
    carry_over(wide(prec), "wide", prec, 2, 62, WIDE_BAR[prec])


# ---------------------------------------------------------------------------------------------------------------------------
# the tag-epoch wrap
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which,B,L", [("many", 1, 257), ("many", 2, 257), ("many", 5, 257), ("many", 33, 16), ("one", 1, 257), ("wide", 2, 65)])
@pytest.mark.parametrize("prec", PRECS)
def test_epoch_wrap_reuses_the_first_steps_tags(which, prec, B, L):
    """A fresh handle's first step uses tags 16 ...; behind the wrap another step uses the very same tags with other data.  Whatever survived of
    the first step's granules (the buffers are cleared, a group's L2 may keep plain-stored copies) must not be taken for the new step's."""
    e = create(which, prec, max_batch=B)
    try:
        pl = plan(e.fam, prec, B, L)
        xb = step_input(np.random.default_rng(5), B, FAMILY[e.fam].E)
        engine_only(e, pl)                                           # x = A on the handle's first tags
        ref = engine_only(e, pl, x=xb)
        e.dbg_oar_epoch(EPOCH_WRAP + 1)
        with pytest.raises(Exception, match="below the current"):
            e.dbg_oar_epoch(16)
        same_bits(engine_only(e, pl, x=xb), ref, "the step behind the wrap")
        same_bits(engine_only(e, pl, x=xb), ref, "the second step behind the wrap")
        e.dbg_oar_epoch(1 << 20)                                     # (forward only: accepted because the wrap restarted the epoch at 16)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 8])
def test_epoch_wrap_in_the_middle_of_a_rollout(B):
    """Three frames: frame 0 starts just below the threshold, so frame 1 wraps -- with a background pass in flight at one scene per call (the
    workers run inside the decode launches), on the systolic schedule at 8.  Same tokens as a handle whose epoch was left alone."""
    from umgen_amd.engine import Engine
    from umgen_amd.synth import synthetic_scene
    from umgen_amd.weights import synthetic_state_dict
    cfg = tiny_config(n_embd=768, n_head=16, n_oar_layer=5, rule_constrain=False)
    sd = synthetic_state_dict(cfg, seed=21)
    scenes = [synthetic_scene(40 + i, n_frames=2) for i in range(B)]
    toks = {m: np.concatenate([s[m] for s in scenes]) for m in MOD_ORDER}
    outs = []
    for epoch in (None, EPOCH_WRAP - 100):
        e = Engine(cfg, precision="bf16", max_batch=B, max_cond_frames=4)
        e.load_state_dict(sd)
        e.finalize()
        if epoch is not None:
            e.dbg_oar_epoch(epoch)
        outs.append(e.rollout(toks, 3, cond_frames=3, input_cond_frames=2, seeds=[100 + i for i in range(B)]))
        if epoch is not None:
            e.dbg_oar_epoch(EPOCH_WRAP // 2)                         # (forward only: accepted because frame 1 restarted the epoch at 16)
        t = e.timings()
        e.close()
        assert t["decode_engine"] == 1 and (B > 1 or t["overlapped_frames"] == 2), t
    for m in MOD_ORDER:
        np.testing.assert_array_equal(outs[1][m], outs[0][m], err_msg=m)


@pytest.mark.gpu
def test_step_hook_refuses_a_path_the_step_would_not_take():
    """umgen_dbg_oar_step never runs another path than the one asked for: 24 scenes take the batched decode layer by default, so neither
    the engine nor five launches per layer, and 23 do not, so not the batched layer (use_engine 2); no chip-wide engine at E = 768; the cache
    hook checks its ranges; with UMGEN_DECODE_BATCHED=0 no batch size takes the batched layer; fp32 has no 16-bit path at all"""
    from umgen_amd.engine import Engine, UMGenError
    from umgen_amd.weights import synthetic_state_dict
    cfg = tiny_config(n_embd=768, n_head=16, rule_constrain=False)
    e = Engine(cfg, precision="bf16", max_batch=24, max_cond_frames=4)
    e.load_state_dict(synthetic_state_dict(cfg, seed=1))
    e.finalize()
    x = np.zeros((24, 768), np.float32)
    try:
        for use in (1, 0):
            with pytest.raises(UMGenError, match="batched decode layer"):
                e.dbg_oar_step(x, 0, use)
        with pytest.raises(UMGenError, match="chip-wide"):
            e.dbg_oar_step(x[:1], 0, 3)
        e.dbg_oar_step(x[:23], 0, 1)
        with pytest.raises(UMGenError, match="do not take the batched decode layer"):
            e.dbg_oar_step(x[:23], 0, 2)
        out, frag = e.dbg_oar_step(x, 0, 2, return_frag=True)
        assert np.all(np.isfinite(out)) and np.array_equal(out.view(np.uint32), frag.view(np.uint32))
        with pytest.raises(UMGenError, match="use_engine 2"):            # no other path keeps a fragment-major copy of x
            e.dbg_oar_step(x[:23], 0, 1, return_frag=True)
        for layer, scene, row0, n in ((2, 0, 0, 1), (0, 24, 0, 1), (0, 0, -1, 1), (0, 0, 0, 0), (0, 0, LMAX - 1, 2)):
            with pytest.raises(UMGenError):
                e.dbg_oar_cache_get(layer, scene, row0, n)
        rows = (np.arange(2 * 16 * 3 * 48) % 65536).astype(np.uint16).reshape(2, 16, 3, 48)
        e.dbg_oar_cache_put(1, 23, LMAX - 3, rows)
        np.testing.assert_array_equal(e.dbg_oar_cache_get(1, 23, LMAX - 3, 3), rows)
        assert not e.dbg_oar_cache_get(1, 22, LMAX - 3, 3).any() and not e.dbg_oar_cache_get(1, 23, LMAX - 6, 3).any()
    finally:
        e.close()
    # UMGEN_DECODE_BATCHED=0: no batch size takes the batched decode layer; fp32 has neither engines nor the batched layer
    with env(UMGEN_DECODE_BATCHED=0):
        e = Engine(cfg, precision="bf16", max_batch=24, max_cond_frames=4)
    e32 = Engine(tiny_config(rule_constrain=False), precision="fp32", max_batch=1, max_cond_frames=2)
    try:
        e.load_state_dict(synthetic_state_dict(cfg, seed=1))
        e.finalize()
        for B in (1, 23, 24):
            with pytest.raises(UMGenError, match="do not take the batched decode layer"):
                e.dbg_oar_step(x[:B], 0, 2)
        e.dbg_oar_step(x, 0, 0)
        e32.load_state_dict(synthetic_state_dict(tiny_config(rule_constrain=False), seed=1))
        e32.finalize()
        with pytest.raises(UMGenError, match="16-bit engines only"):
            e32.dbg_oar_step(np.zeros((1, 96), np.float32), 0, 2)
    finally:
        e.close()
        e32.close()


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the reference's referee, and the premises of every case
# ---------------------------------------------------------------------------------------------------------------------------
def test_stack_restatement_matches_oracle():
    """stack_ref over two layers is the oracle's BlockOAR chained (OracleUMGen._block_oar, bf16_engine) up to the oracle's fp32 arithmetic"""
    from oracle.umgen_oracle import OracleUMGen
    prec, E, B, pos = 1, 96, 3, 70
    H = E // 48
    P = [layer_params(prec, E, 4242 + i)[1] for i in range(2)]
    sd = {}
    for i, Pl in enumerate(P):
        sd.update(oar_entries(Pl, i))
    oracle = OracleUMGen(types.SimpleNamespace(n_embd=E, n_head=H), {k: v.astype(np.float32) for k, v in sd.items()}, weight_dtype="bf16_engine")
    rng = np.random.default_rng(6)
    x0 = step_input(rng, B, E)
    caches = [store(rng.standard_normal((B, 2, H, pos, 48)).astype(np.float32), prec)[0] for _ in P]
    x, new = torch.from_numpy(x0)[:, None], []
    with torch.no_grad():
        for i, c in enumerate(caches):
            hv = stored(c, prec).astype(np.float32)
            kt, vt = (torch.from_numpy(np.ascontiguousarray(hv[:, j].transpose(0, 2, 1, 3).reshape(B, pos, E))) for j in (0, 1))
            x, (k, v) = oracle._block_oar(x, f"transformer.OAR.{i}", (kt, vt))
            new.append(store(np.stack([k[:, -1].numpy().reshape(B, H, 48), v[:, -1].numpy().reshape(B, H, 48)], 1), prec)[0])
    ref_x, kv_refs, _ = stack_ref(x0, P, caches, new, prec, pos)
    for n_, r in zip(new, kv_refs):
        check_kv_row(n_, r, prec, 1e-5)
    err = rel_err(x[:, 0].numpy(), ref_x)
    assert err <= 2e-6, f"restatement vs oracle: {err:.3e}"


def rows_partition_claims():
    """what the comment at ROWS_POS says of rows_partition, and rows_seam's keys: cached keys on the edge that the scene's turn names"""
    def live(L):
        return [p for p in rows_partition(L)[1] if p[0] < p[1]]
    assert live(0) == [(0, 1)] and live(1) == [(0, 2)]                              # the own key alone | one cached key
    assert live(15) == [(0, 16)] and live(16) == [(0, 16), (16, 17)]                # a full lane-group row | one key past it
    assert len(live(63)) == 4 and live(63)[-1] == (48, 64)                          # exactly one pass round
    assert live(64)[4:] == [(64, 65)] and live(65)[4:] == [(64, 66)]                # the second round: the own key alone | with one cached key
    assert rows_partition(255)[0] == 1 and len(live(255)) == 16 and live(255)[-1] == (240, 256)     # exactly one flight batch
    assert rows_partition(256)[0] == 2 and live(256)[16:] == [(256, 257)]           # the second flight batch: the own key alone
    assert rows_partition(257)[0] == 2 and live(257)[16:] == [(256, 258)]
    assert [rows_partition(L)[0] for L in (1100, 2206, 2303)] == [5, 9, 9]
    assert len(live(2303)) == 144 == len(rows_partition(2303)[1]) and live(2303)[-1] == (2288, LMAX)        # the last cache row fills the last flight batch
    for L in ROWS_POS:
        nflight, passes = rows_partition(L)
        assert len(passes) == 16 * nflight and all(passes[k // 16][0] <= k < passes[k // 16][1] for k in range(L + 1))
        assert sum(hi - lo for lo, hi in live(L)) == L + 1
    residue = [(16, 15), (16, 0), (64, 63), (64, 0), (256, 255), (256, 0), (1 << 30, 0)]        # by edge kind: k % 16 == 15, ...
    for L in ROWS_POS[1:]:
        edges = {k for lo, hi in live(L) for k in (lo, hi - 1)} | {L - 1}
        for b in range(7):
            for h in range(16):
                for l in range(4):
                    k = rows_seam(L, b, h, l)
                    mod, r = residue[(b + h // 5 + 2 * l) % 7]
                    assert k in edges and 0 <= k < L and (k % mod == r or k == L - 1), (L, b, h, l, k)
    # at one scene the seam heads of the four layers take every kind of edge, and at L = 2206 none of them falls back to key L - 1
    assert {(h // 5 + 2 * l) % 7 for l in range(4) for h in range(16) if pattern(0, h, l) == 1} == set(range(7))
    assert all(rows_seam(2206, 0, h, l) != 2205 for l in range(4) for h in range(16) if pattern(0, h, l) == 1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("fam", ["xcd", "wide", "rows", "rows96"])
def test_case_premises_hold_on_the_reference(fam, prec):
    """every case's patterns (dominant newest / seam / own key, all-equal scores) are there in the reference's own scores, the seam keys are
    cached keys on a boundary of the partition, and the position lists hit what the file header says of the partitions"""
    for B, L in CASES[fam]:
        plan(fam, prec, B, L)                          # (asserts the premises)
    plan.cache_clear()
    if fam in ("rows", "rows96"):
        rows_partition_claims()
        return
    n0, w = xcd_partition(15)
    assert n0 == 16 and all(lo >= hi for lo, hi in w[8:])                           # empty second half
    assert [xcd_partition(L)[1][8] for L in (16, 32)] == [(16, 17), (32, 33)]       # one-key second half: the token's own
    assert [xcd_partition(L)[1][1][0] for L in (255, 256)] == [16, 32] and xcd_partition(256)[1][5][0] >= 144   # span 16 -> 32, waves without keys
    assert xcd_partition(767)[1][0] == (0, 48) and xcd_partition(769)[1][0] == (0, 64)                       # 3 buffers of 16 | a refill
    spn, w = wide_partition(15)
    assert spn == 16 and all(lo >= hi for lo, hi in w[1:])                          # one wave has keys
    assert wide_partition(64)[1][12] == (64, 65) and all(lo >= hi for lo, hi in wide_partition(64)[1][18:])  # one-key quarter, empty quarter
    assert wide_partition(1919)[1][0] == (0, 80) and wide_partition(1921)[1][0] == (0, 96)                   # 5 passes in flight | a sixth
    for L in sorted(set(XCD_POS + WIDE_POS) - {0}):
        for f_, part in (("xcd", xcd_partition), ("wide", wide_partition)):
            edges = {k for lo, hi in part(L)[1] if lo < hi for k in (lo, hi - 1)} | {L - 1}
            for b in range(4):
                for h in range(4):
                    assert SEAM[f_](L, b, h, 0) in edges and 0 <= SEAM[f_](L, b, h, 0) < L
