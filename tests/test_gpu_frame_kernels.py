"""Frame assembly around the decode layers, one kernel family at a time through the hooks umgen_dbg_embed_warp / _layernorm / _cond_rows /
_first_input / _ego_queries / _prefix_rows / _prefix_kv_to_cache / _token_steps / _sample_ego.  Each hook launches the product's own launcher
(launch_embed_stack + launch_warp_map as run_stack does, launch_layernorm<T>, launch_cond_rows, launch_first_input, launch_ego_queries,
launch_prefix_rows, launch_prefix_kv_to_cache<T>, launch_fixed_token / launch_sample_token as enqueue_step does, launch_sample_ego) on tables
that are hook inputs (small vocabularies, not a loaded model).  Outputs start as NaN and carry guard bands (the hooks return an error when a
band changed).  Every test needs a GPU except the two CPU checks of the references themselves (restatement vs oracle, fp32 vs fp64 warp).

What is bit-equal (asserted on integer views): every embedding row that is not a warped map row, mapfeat, first input, ego queries, prefix
rows, the K/V move, x_next of every token step, the decoded boxes (fp64).  Tokens, counters 0-5, n_boxes, step / epoch / done are integers.
What carries a bar: |got - ref64| <= bar * max(1, |ref64|).

Largest errors measured on an MI355X over all cases, the reference's own error where the bar comes from it, and the bars:
  map warp, X map rows                 kernel 1.75e-5 | torch fp32 CPU (grid_sample and the three adds in fp32) against fp64 1.43e-5 | WARP_BAR 5.7e-5
  map warp, warped_last                kernel 1.48e-5 | torch fp32 CPU affine_grid + grid_sample alone against fp64 1.19e-5        | WARP_BAR_O 4.7e-5
                                       each bar = 4 x the fp32 reference's distance on the pose cases (test_warp_bars_are_four_times_the_fp32_reference)
  LayerNorm -> fp32 | bf16 | fp16      1.3e-5 | 9.5e-6 | 8.9e-6 (16-bit: beyond 1 ulp of the type)     LN_BAR 1e-4 = GEMV_BAR: the same fp32
  conditioning rows                    1.2e-5                                                          LayerNorm on the same row distribution
The wholly-outside share of the warped cells is 0.15 at (10 m, 4 m, 1 rad), 0.14 at -pi / 4 and 1.0 / 1.0 / 0.75 / 0.97 in the `far` group.
"""
import ctypes as C
import functools
import types
from collections import Counter

import numpy as np
import pytest
import torch

from oracle.umgen_oracle import DRAW_MAIN, OracleUMGen, rng_uniform
from tests.gpu_util import bf16_bits, bf16_round, check, fp, from_bits, lib, vp
from tests.test_gpu_decode_layer import GEMV_BAR, NAN16, NAN32, ln_input, nan_array, raw, ref_ln, rel_err, store, stored, ulp16
from umgen_amd._lib import DbgSamplerParams, DbgSteps, DbgTables

KSEQ, NMAP, NBOX, NIMG, NPOSE, TOK = 2207, 1024, 660, 512, 3, 2199
OFF_MAP, OFF_BOX, OFF_IMG = 3, 1027, 1687
POSE_EOS, MAP_BOS, MAP_C0, MAP_EOS, BOX_BOS, BOX_C0, BOX_EOS, IMG_BOS, IMG_C0, IMG_EOS = 4, 5, 6, 1030, 1031, 1032, 1692, 1693, 1694, 2206
AUX = {0: 0, 4: 1, 5: 2, 1030: 3, 1031: 4, 1692: 5, 1693: 6, 2206: 7}        # bos / eos position -> axe row
STACK_EGO, STACK_MAP, STACK_BOX, STACK_TAR = 0, 1, 2, 3
STACK_LEN = {STACK_EGO: 2207, STACK_MAP: 1031, STACK_BOX: 1693, STACK_TAR: 2207}
SLOTS, SLOT_LEN, PAD = 60, 11, 1027
EPOCH_PER_STEP = 16384
WIDTHS = [96, 768, 1536]
PRECS = [0, 1, 2]
# On the pose cases below torch's fp32 CPU affine_grid + grid_sample is 1.19e-5 from its fp64 self (the warp `o` alone: the bar of warped_last), and
# 1.43e-5 once the three fp32 adds ((o + f) + spe) + tpe of a map row are made in fp32 too (the bar of the X map rows).  Each bar is 4 x its figure
# (test_warp_bars_are_four_times_the_fp32_reference measures both and holds the bars to that); the kernel evaluates sin / cos and the base grid
# differently, each a few ulp on coordinates scaled by 16
WARP_BAR = 5.7e-5            # X map rows
WARP_BAR_O = 4.7e-5          # warped_last
LN_BAR = GEMV_BAR            # the LayerNorm arithmetic and the row distribution gemv_ln_kernel is held to (rows with |mean| / sd = 80: fp32 mean)

i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))        # noqa: E731
u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))       # noqa: E731


def nan32(shape):
    return np.full(shape, NAN32, np.uint32).view(np.float32)


def assert_bits(got, ref, msg):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref, dtype=np.float32).view(np.uint32), err_msg=msg)


def all_nan(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint32) == NAN32))


# ---------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------
class Tables:
    """embedding tables as hook inputs: fp32 arrays, bf16 bits, and the float32 values of the bf16 tables"""
    DIMS = dict(n_tpe=6, n_pose=40, n_map=48, n_box=1028, n_img=56, n_posi=1030)

    def __init__(self, E, arrays=None, dims=None, seed=0):
        self.E = E
        d = dict(self.DIMS, **(dims or {}))
        self.dims = d
        if arrays is None:
            rng = np.random.default_rng(1000 + E + seed)
            f = lambda n: rng.standard_normal((n, E), dtype=np.float32)             # noqa: E731
            arrays = dict(egoe=f(3), axe=f(8), be=f(d["n_box"]), tpe=f(d["n_tpe"]), spe=f(KSEQ), gmap=f(d["n_map"]), gimg=f(d["n_img"]),
                          fouier_pe=bf16_bits(f(d["n_pose"])), posi=bf16_bits(f(d["n_posi"])), grid_posi=bf16_bits(f(NMAP)))
        for k, v in arrays.items():
            setattr(self, k, np.ascontiguousarray(v))
        for k in ("fouier_pe", "posi", "grid_posi"):
            setattr(self, k + "_f", from_bits(getattr(self, k)))
        self.c = DbgTables(E=E, **d)
        for k in ("egoe", "axe", "be", "tpe", "spe", "gmap", "gimg"):
            assert getattr(self, k).dtype == np.float32
            setattr(self.c, k, fp(getattr(self, k)))
        for k in ("fouier_pe", "posi", "grid_posi"):
            assert getattr(self, k).dtype == np.uint16
            setattr(self.c, k, getattr(self, k).ctypes.data_as(C.POINTER(C.c_uint16)))

    @property
    def ref(self):
        return C.byref(self.c)


@functools.lru_cache(maxsize=None)
def tables(E, n_box=1028):
    return Tables(E, dims=dict(n_box=n_box))


def random_tokens(rng, tb, B, T):
    """window tokens [B][T][..] with distinct content in every slot; the first two tokens of every bbox3d slot index posi"""
    d = tb.dims
    return dict(pose=rng.integers(0, d["n_pose"], (B, T, NPOSE)).astype(np.int32), map=rng.integers(0, d["n_map"], (B, T, NMAP)).astype(np.int32),
                box=rng.integers(0, min(d["n_box"], d["n_posi"]), (B, T, NBOX)).astype(np.int32), img=rng.integers(0, d["n_img"], (B, T, NIMG)).astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. embedding + map warp
# ---------------------------------------------------------------------------------------------------------------------------
def embed_ref(tb, stack, toks, t0, T):
    """fp32 restatement of embed_stack_row for slots t0 .. t0 + T - 1 of toks [B][Tf][..], adding in the kernel's (= the reference's) order.
    -> X [B][T][SS][E] with the map rows of the TAR stacks left at 0 (the warp finishes them) and mapfeat [B][T][1024][E]"""
    SS, E = STACK_LEN[stack], tb.E
    sl = slice(t0, t0 + T)
    B = toks["pose"].shape[0]
    emb = np.zeros((B, T, SS, E), np.float32)
    for s, a in AUX.items():
        if s < SS:
            emb[:, :, s] = tb.axe[a]
    emb[:, :, 1:4] = tb.fouier_pe_f[toks["pose"][:, sl]]
    gm = tb.gmap[toks["map"][:, sl]]
    mapfeat = gm + tb.grid_posi_f if stack == STACK_TAR else gm
    if stack == STACK_EGO:
        emb[:, :, MAP_C0:MAP_EOS] = gm
    if SS > BOX_EOS:
        bt = toks["box"][:, sl]
        first = bt.reshape(B, T, SLOTS, SLOT_LEN)
        pe = bf16_round(tb.posi_f[first[..., 0]] + tb.posi_f[first[..., 1]])          # bf16 + bf16 -> bf16
        emb[:, :, BOX_C0:BOX_EOS] = tb.be[bt] + np.repeat(pe, SLOT_LEN, axis=2)
    if SS > IMG_EOS:
        emb[:, :, IMG_C0:IMG_EOS] = tb.gimg[toks["img"][:, sl]]
    X = (emb + tb.spe[:SS]) + tb.tpe[sl][None, :, None, :]
    if stack != STACK_EGO:
        X[:, :, MAP_C0:MAP_EOS] = 0
    return X, mapfeat.astype(np.float32)


def warp_ref(mapfeat, pd, dtype):
    """affine_transform on mapfeat [B][T][1024][E] by pose_diff [B][T][3]: the oracle's own _affine (affine_grid + grid_sample, bilinear, zeros,
    align_corners=False, theta as umgen_oracle.py builds it) in dtype"""
    with torch.no_grad():
        return OracleUMGen._affine(None, torch.from_numpy(mapfeat).to(dtype), torch.from_numpy(pd).to(dtype)).numpy()


def map_rows_ref(tb, o, mapfeat, t0, T, dtype):
    """((o + f) + spe) + tpe in dtype"""
    spe = tb.spe[MAP_C0:MAP_EOS].astype(dtype)
    tpe = tb.tpe[t0:t0 + T].astype(dtype)[None, :, None, :]
    return ((o + mapfeat.astype(dtype)) + spe) + tpe


POSES = {
    "zero": [(0, 0, 0)],
    "bins": [(10, 4, 1), (-10, -4, -1), (9.99, 0, 0), (0, 3.99, 0), (0, 0, 0.999)],
    "cell": [(4, 0, 0), (0, 4, 0), (-4, -4, 0), (8, -8, 0), (2, 2, 0)],
    "rot": [(0, 0, np.pi / 2), (0, 0, np.pi), (0, 0, -np.pi / 4), (3, -1, 0.3)],
    "far": [(130, 0, 0), (0, -200, 0), (64, 64, 0), (127.9, 0, 0)],
}
ALL_POSES = [p for g in POSES.values() for p in g]                                  # 19
GROUP_MIX = [POSES["bins"][0], POSES["cell"][4], POSES["rot"][3], POSES["far"][3], POSES["far"][2], POSES["rot"][2], POSES["zero"][0],
             POSES["cell"][0], POSES["bins"][1], POSES["far"][0]]                   # a small window still sees all four groups


def embed_warp_call(tb, stack, toks, B, T, Tf, t0, pd, want_last):
    SS, E = STACK_LEN[stack], tb.E
    X, mf, wl = np.zeros((B, T, SS, E), np.float32), np.zeros((B, T, NMAP, E), np.float32), np.zeros((B, NMAP, E), np.float32)
    check(lib().umgen_dbg_embed_warp(stack, tb.ref, i32p(toks["pose"]), i32p(toks["map"]), i32p(toks["box"]), i32p(toks["img"]), B, T, Tf, t0, fp(pd),
                                     int(want_last), fp(X), fp(mf), fp(wl)))
    return X, mf, wl


def embed_warp_case(stack, E, B, T, Tf, t0, poses, want_last=True):
    """one pass through the hook with everything checked, the two bars of the warp included; -> (error of the X map rows, error of warped_last,
    share of wholly-outside cells per slot [B][T])"""
    tb = tables(E)
    rng = np.random.default_rng(17 * E + 5 * stack + 1000 * B + 100 * T + 10 * Tf + t0)
    toks = random_tokens(rng, tb, B, Tf)
    pd = np.array([poses[i % len(poses)] for i in range(B * Tf)], np.float32).reshape(B, Tf, 3)
    X, mf, wl = embed_warp_call(tb, stack, toks, B, T, Tf, t0, pd, want_last)
    Xr, mfr = embed_ref(tb, stack, toks, t0, T)
    not_map = np.ones(STACK_LEN[stack], bool)
    if stack != STACK_EGO:
        not_map[MAP_C0:MAP_EOS] = False
    assert_bits(X[:, :, not_map], Xr[:, :, not_map], "an embedding row differs from the fp32 restatement")
    if stack == STACK_EGO:
        assert all_nan(mf) and all_nan(wl), "the ego stack wrote mapfeat / warped_last"
        return 0.0, 0.0, None
    assert_bits(mf, mfr, "mapfeat differs from gmap[tok] (+ grid_posi in the TAR stack)")
    pdw = np.ascontiguousarray(pd[:, t0:t0 + T])
    o64 = warp_ref(mf, pdw, torch.float64)
    ref = map_rows_ref(tb, o64, mf, t0, T, np.float64)
    got = X[:, :, MAP_C0:MAP_EOS]
    assert np.all(np.isfinite(got)), "non-finite map row"
    err = rel_err(got, ref)
    # the zero-padding rule: where the fp64 warp is exactly 0 the kernel's is 0 too, so the row is (f + spe) + tpe bit for bit
    zero = o64 == 0
    plain = map_rows_ref(tb, np.zeros_like(mf), mf, t0, T, np.float32)
    bad = zero & (got.view(np.uint32) != plain.view(np.uint32))
    assert not bad.any(), f"{int(bad.sum())} elements are not (0 + f + spe) + tpe where the fp64 warp is exactly 0"
    err_o = 0.0
    if want_last and t0 + T == Tf:
        assert np.all(np.isfinite(wl)), "warped_last has unwritten elements"
        err_o = rel_err(wl, o64[:, -1])
        assert not np.any(wl.view(np.uint32)[o64[:, -1] == 0]), "warped_last is not +0 where the fp64 warp is exactly 0"
    else:
        assert all_nan(wl), "warped_last was written by a pass that does not hold the last slot (or was not asked for it)"
    print(f"warp error: map rows {err:.3e}, warped_last {err_o:.3e}")
    assert err <= WARP_BAR, f"map rows: warp error {err:.3e} > bar {WARP_BAR}"
    assert err_o <= WARP_BAR_O, f"warped_last: warp error {err_o:.3e} > bar {WARP_BAR_O}"
    return err, err_o, zero.all(-1).mean(-1)


WINDOWS = [(1, 1, 1, 0), (2, 3, 3, 0), (2, 2, 5, 3), (2, 2, 5, 1)]
STACKS = (STACK_EGO, STACK_MAP, STACK_BOX, STACK_TAR)


@pytest.mark.gpu
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("stack", STACKS)
def test_embed_warp_windows(stack, E, window):
    """tokens, tpe row and pose_diff row of slot t0 + t; warped_last from slot Tfull - 1 of both scenes when the pass holds it, untouched otherwise"""
    B, T, Tf, t0 = window
    embed_warp_case(stack, E, B, T, Tf, t0, GROUP_MIX[t0:] + GROUP_MIX[:t0])


@pytest.mark.gpu
@pytest.mark.parametrize("stack", [STACK_MAP, STACK_BOX, STACK_TAR])
def test_warp_pose_cases(stack):
    """every pose case in a slot of its own (4 scenes x 5 slots, the 20th slot repeats the first): bin ends of the ego tokeniser, whole- and half-cell shifts,
    rotations, and motions that push (almost) everything off the grid"""
    _, _, outside = embed_warp_case(stack, 96, 4, 5, 5, 0, ALL_POSES)
    outside = outside.reshape(-1)
    print(f"wholly-outside share per pose {np.round(outside, 3)}")
    check_outside_shares(dict(zip(ALL_POSES, outside)))


OUTSIDE_SHARE = {(130, 0, 0): (1.0, 1.0), (0, -200, 0): (1.0, 1.0), (64, 64, 0): (0.7, 0.8), (127.9, 0, 0): (0.9, 1.0), (10, 4, 1): (0.1, 0.2), (0, 0, 0): (0.0, 0.0)}


def check_outside_shares(share):
    """the share of wholly-outside cells (fp64 warp exactly 0 over the whole cell) of the poses whose share is known"""
    for pose, (lo, hi) in OUTSIDE_SHARE.items():
        if pose in share:
            assert lo <= share[pose] <= hi, (pose, share[pose])


# the pose cases at the wide embeddings, one group per pass (two scenes, the last slot of the pass repeats the group's first pose where the group is odd)
@pytest.mark.gpu
@pytest.mark.parametrize("group", ["zero+bins", "cell", "rot", "far"])
@pytest.mark.parametrize("E", [768, 1536])
@pytest.mark.parametrize("stack", [STACK_MAP, STACK_BOX, STACK_TAR])
def test_warp_pose_cases_wide(stack, E, group):
    poses = [p for g in group.split("+") for p in POSES[g]]
    T = (len(poses) + 1) // 2
    _, _, outside = embed_warp_case(stack, E, 2, T, T, 0, poses)
    check_outside_shares(dict(zip(poses, outside.reshape(-1))))


@pytest.mark.gpu
@pytest.mark.parametrize("E", WIDTHS)
def test_warp_without_warped_last(E):
    """the BOX / TAR stacks hand no warped_last to the launcher (run_stack): the pass holds the last slot and still must not write it"""
    embed_warp_case(STACK_BOX, E, 1, 1, 2, 1, GROUP_MIX[1:], want_last=False)      # slot 1: (3, -1, 0.3)


def fp32_reference_distance():
    """torch's own fp32 CPU affine_grid + grid_sample against its fp64 self on the pose cases (the cases and features of test_warp_pose_cases):
    -> (the map rows ((o + f) + spe) + tpe with the adds in fp32 too, the warp o alone)"""
    tb = tables(96)
    rows, alone = 0.0, 0.0
    for stack in (STACK_MAP, STACK_TAR):
        rng = np.random.default_rng(17 * 96 + 5 * stack + 1000 * 4 + 100 * 5 + 10 * 5)
        toks = random_tokens(rng, tb, 4, 5)
        pd = np.array([ALL_POSES[i % len(ALL_POSES)] for i in range(20)], np.float32).reshape(4, 5, 3)
        _, mf = embed_ref(tb, stack, toks, 0, 5)
        o64, o32 = warp_ref(mf, pd, torch.float64), warp_ref(mf, pd, torch.float32)
        alone = max(alone, rel_err(o32, o64))
        rows = max(rows, alone, rel_err(map_rows_ref(tb, o32, mf, 0, 5, np.float32), map_rows_ref(tb, o64, mf, 0, 5, np.float64)))
    return rows, alone


def test_warp_bars_are_four_times_the_fp32_reference():
    """CPU: each bar of the warp is at most 4 x the distance of torch's fp32 result from the fp64 reference on the same cases (measured: map rows
    1.43e-5, the warp alone 1.19e-5)"""
    rows, alone = fp32_reference_distance()
    print(f"torch fp32 CPU vs fp64: map rows {rows:.3e} (bar {WARP_BAR}), grid_sample alone {alone:.3e} (bar {WARP_BAR_O})")
    assert WARP_BAR <= 4 * rows, f"WARP_BAR {WARP_BAR} is wider than 4 x the fp32 reference's own error {rows:.3e}"
    assert WARP_BAR_O <= 4 * alone, f"WARP_BAR_O {WARP_BAR_O} is wider than 4 x the fp32 reference's own error {alone:.3e}"


def test_embed_restatement_matches_oracle():
    """CPU: embed_ref is what OracleUMGen feeds into _run_stack (forward_ego_net, forward_tar of the three stacks) for the tiny config, bit for
    bit on every row that is not a warped map row; mapfeat is the oracle's map embedding."""
    from umgen_amd.config import tiny_config
    from umgen_amd.synth import synthetic_scene
    from umgen_amd.weights import synthetic_state_dict
    cfg = tiny_config()
    oracle = OracleUMGen(cfg, synthetic_state_dict(cfg, seed=11))
    T = 3
    scene = synthetic_scene(5, n_frames=T)
    tokens = {m: torch.as_tensor(np.asarray(scene[m]), dtype=torch.long)[:, :T] for m in ("pose", "map", "bbox3d", "image")}
    w = oracle.w
    with torch.no_grad():
        gmap = oracle._gmlp(torch.arange(cfg.map_vocab_size), "map").numpy()
        gimg = oracle._gmlp(torch.arange(cfg.img_vocab_size), "img").numpy()
    bits = lambda t: t.view(torch.int16).numpy().view(np.uint16)                      # noqa: E731
    g = lambda k: w[f"transformer.{k}.weight"].numpy()                                # noqa: E731
    arrays = dict(egoe=g("egoe"), axe=g("axe"), be=g("be"), tpe=g("tpe"), spe=g("spe"), gmap=gmap, gimg=gimg, fouier_pe=bits(oracle.fouier_pe),
                  posi=bits(oracle.posi), grid_posi=bits(oracle.grid_posi))
    tb = Tables(cfg.n_embd, arrays, dict(n_tpe=g("tpe").shape[0], n_pose=1024, n_map=cfg.map_vocab_size, n_box=cfg.bbox3d_vocab_size,
                                         n_img=cfg.img_vocab_size, n_posi=1030))
    toks = dict(pose=tokens["pose"].numpy().astype(np.int32), map=tokens["map"].numpy().astype(np.int32), box=tokens["bbox3d"].numpy().astype(np.int32),
                img=tokens["image"].numpy().astype(np.int32))
    seen = []
    oracle._run_stack = lambda x, name, n, ln: (seen.append((name, x.numpy().copy())), x)[1]
    with torch.no_grad():
        oracle.forward_ego_net(tokens)
        for s in ("map_tar", "box_tar", "TAR"):
            oracle.forward_tar(tokens, s)
    assert [n for n, _ in seen] == ["ego_tar", "map_tar", "box_tar", "TAR"]
    for stack, (name, x) in zip((STACK_EGO, STACK_MAP, STACK_BOX, STACK_TAR), seen):
        Xr, mfr = embed_ref(tb, stack, toks, 0, T)
        keep = np.ones(STACK_LEN[stack], bool)
        if stack != STACK_EGO:
            keep[MAP_C0:MAP_EOS] = False
        assert_bits(Xr[:, :, keep], x[:, :, keep], f"{name}: embed_ref differs from the oracle's stack input")
        if stack != STACK_EGO:      # the warped rows: the oracle's fp32 warp of the restated mapfeat, added in the restated order
            from oracle.umgen_oracle import decode_pose_values
            o32 = warp_ref(mfr, decode_pose_values(toks["pose"]), torch.float32)
            assert_bits(map_rows_ref(tb, o32, mfr, 0, T, np.float32), x[:, :, MAP_C0:MAP_EOS], f"{name}: map rows differ from the oracle's stack input")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm, conditioning rows, first input, ego queries
# ---------------------------------------------------------------------------------------------------------------------------
def ln_call(prec, x, stride, n_rows, E, w, extra=5):
    out = np.zeros((n_rows + extra, E), np.float32 if prec == 0 else np.uint16)
    check(lib().umgen_dbg_layernorm(prec, fp(x), stride, n_rows, E, fp(w), vp(out), n_rows + extra))
    tail = out[n_rows:]
    assert np.all(tail.view(np.uint32) == NAN32) if prec == 0 else np.all(tail == NAN16[prec]), "a row >= n_rows was written"
    return out[:n_rows]


def ln_check(prec, got, ref):
    """-> the fp32 error, or the 16-bit error beyond 1 ulp of the type, relative to max(1, |ref|)"""
    v = stored(got, prec)
    assert np.all(np.isfinite(v)), "non-finite LayerNorm output"
    slack = 0.0 if prec == 0 else ulp16(ref, prec)
    return float(((np.abs(v - ref) - slack) / np.maximum(1.0, np.abs(ref))).max())


def special_rows(rng, E):
    const = np.full(E, 2.5, np.float32)                                     # variance 0: rstd = 1 / sqrt(1e-5), output exactly 0
    big = (1e4 * rng.standard_normal(E)).astype(np.float32)                 # magnitude 1e4
    return const, big


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 2207, 8193])
@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("prec", PRECS)
def test_layernorm(prec, E, pad, n_rows):
    rng = np.random.default_rng(E + 7 * n_rows + pad + prec)
    stride = E + pad
    w = (1 + 0.2 * rng.standard_normal(E)).astype(np.float32)
    const, big = special_rows(rng, E)
    rows = ln_input(rng, n_rows, E)                                        # both extremes of the distribution in rows 0 and n_rows - 1
    if n_rows == 1:
        batches, const_rows = [rows, const[None], big[None]], [None, 0, None]          # three one-row launches
    else:
        special = rows.copy()
        special[0], special[-1] = const, big                                # a second launch of n_rows rows: constant row first, 1e4 row last
        batches, const_rows = [rows, special], [None, 0]
    worst = 0.0
    for rows, ci in zip(batches, const_rows):
        x = np.full((rows.shape[0], stride), np.nan, np.float32)           # the columns between the rows are never read
        x[:, :E] = rows
        got = ln_call(prec, x, stride, rows.shape[0], E, w)
        ref = ref_ln(rows, w)
        if ci is not None:
            assert not np.any(stored(got[ci], prec)), "the constant row is not exactly 0"
        worst = max(worst, ln_check(prec, got, ref))
    print(f"layernorm prec {prec} error {worst:.3e}")
    assert worst <= LN_BAR, f"LayerNorm error {worst:.3e} (beyond 1 ulp of the output type) > bar {LN_BAR}"


COND_ROWS = {STACK_MAP: np.arange(MAP_BOS, MAP_EOS + 1), STACK_BOX: np.arange(BOX_BOS, BOX_EOS + 1),
             STACK_TAR: np.concatenate([np.arange(0, 5), np.arange(IMG_BOS, IMG_EOS + 1)])}


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("E", WIDTHS)
def test_cond_rows(E, B, T):
    """each stack alone writes exactly its rows, from slot T - 1 (the earlier slots are NaN), the warped-map prior on rows 6 .. 1029 of the MAP stack only;
    then the three launches in the product's order into one buffer: no NaN left, every row its owner's"""
    rng = np.random.default_rng(E + 10 * B + T)
    wl = rng.standard_normal((B, NMAP, E), dtype=np.float32)
    alone, worst = {}, 0.0
    both = nan32((B, KSEQ, E))
    ops = {}
    for stack in (STACK_MAP, STACK_BOX, STACK_TAR):
        SS = STACK_LEN[stack]
        X = nan32((B, T, SS, E))
        X[:, T - 1] = ln_input(rng, B * SS, E).reshape(B, SS, E)
        lw = (1 + 0.2 * rng.standard_normal(E)).astype(np.float32)
        ops[stack] = (X, lw)
        cond = nan32((B, KSEQ, E))
        check(lib().umgen_dbg_cond_rows(stack, B, T, E, fp(X), fp(lw), fp(wl), fp(cond)))     # (warped_last handed to every stack: only MAP may use it)
        rows = COND_ROWS[stack]
        others = np.setdiff1d(np.arange(KSEQ), rows)
        assert all_nan(cond[:, others]), f"stack {stack} wrote a row that is not its own"
        ref = ref_ln(X[:, T - 1, rows].reshape(-1, E), lw).reshape(B, len(rows), E)
        if stack == STACK_MAP:
            ref[:, 1:1 + NMAP] += wl.astype(np.float64)
        got = cond[:, rows]
        assert np.all(np.isfinite(got)), f"stack {stack} left one of its rows unwritten"
        worst = max(worst, rel_err(got, ref))
        alone[stack] = got.copy()
    for stack in (STACK_MAP, STACK_BOX, STACK_TAR):                                           # engine.hip umgen_frame's order
        X, lw = ops[stack]
        check(lib().umgen_dbg_cond_rows(stack, B, T, E, fp(X), fp(lw), fp(wl) if stack == STACK_MAP else None, fp(both)))
    assert np.all(np.isfinite(both)), "a conditioning row is left unwritten by the three launches"
    for stack, got in alone.items():
        assert_bits(both[:, COND_ROWS[stack]], got, f"rows of stack {stack} changed in the combined buffer")
    print(f"cond rows error {worst:.3e}")
    assert worst <= LN_BAR, f"conditioning-row error {worst:.3e} > bar {LN_BAR}"


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("E", WIDTHS)
def test_first_input_and_ego_queries(E, B):
    tb = tables(E)
    rng = np.random.default_rng(E + B)
    cond = rng.standard_normal((B, KSEQ, E), dtype=np.float32)
    row = rng.standard_normal(E, dtype=np.float32)
    x = np.zeros((B, E), np.float32)
    check(lib().umgen_dbg_first_input(B, E, fp(row), fp(cond), fp(x)))
    assert_bits(x, row + cond[:, 0], "first input differs from row + cond[b][0]")
    for T in (1, 4, tb.dims["n_tpe"]):
        q = np.zeros((B, 3, E), np.float32)
        check(lib().umgen_dbg_ego_queries(tb.ref, B, T, fp(q)))
        assert_bits(q, np.broadcast_to((tb.egoe + tb.spe[:3]) + tb.tpe[T - 1], (B, 3, E)), f"ego queries differ from (egoe + spe) + tpe[{T - 1}]")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the given-token prefix: rows and the K/V move (the causal attention is tested next to test_attn_spatial in test_gpu_kernels.py)
# ---------------------------------------------------------------------------------------------------------------------------
def frame_tokens(rng, tb, B):
    d = tb.dims
    t = np.empty((B, TOK), np.int32)
    t[:, :OFF_MAP] = rng.integers(0, d["n_pose"], (B, NPOSE))
    t[:, OFF_MAP:OFF_BOX] = rng.integers(0, d["n_map"], (B, NMAP))
    t[:, OFF_BOX:OFF_IMG] = rng.integers(0, d["n_box"], (B, NBOX))
    t[:, OFF_IMG:] = rng.integers(0, d["n_img"], (B, NIMG))
    return t


def token_embedding(tb, toks, jp):
    """embedding of the (given) token at scene position jp of every scene: what fixed_token_kernel / prefix_rows_kernel feed back [B][E]"""
    if jp in AUX:
        return np.broadcast_to(tb.axe[AUX[jp]], (toks.shape[0], tb.E))
    if jp < POSE_EOS:
        return tb.fouier_pe_f[toks[:, jp - 1]]
    if jp < MAP_EOS:
        return tb.gmap[toks[:, OFF_MAP + jp - MAP_C0]]
    if jp < BOX_EOS:
        return tb.be[toks[:, OFF_BOX + jp - BOX_C0]]
    return tb.gimg[toks[:, OFF_IMG + jp - IMG_C0]]


# 1031 = kMapEos + 1 and 1693 = kBoxEos + 1 are what umgen_frame passes for a given map / a given map + boxes (given_end, engine.hip)
@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 5, 6, 7, 1031, 1032, 1693, 1694])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("E", WIDTHS)
def test_prefix_rows(E, B, P):
    tb = tables(E)
    rng = np.random.default_rng(E + 3 * B + P)
    cond = rng.standard_normal((B, KSEQ, E), dtype=np.float32)
    tske = rng.standard_normal(E, dtype=np.float32)
    toks = frame_tokens(rng, tb, B)
    X, xl = np.zeros((B, P - 1, E), np.float32), np.zeros((B, E), np.float32)
    check(lib().umgen_dbg_prefix_rows(tb.ref, fp(tske), fp(cond), i32p(toks), B, P, fp(X), fp(xl)))
    ref = np.empty((B, P, E), np.float32)
    ref[:, 0] = tske + cond[:, 0]
    for j in range(1, P):
        ref[:, j] = token_embedding(tb, toks, j - 1) + cond[:, j]
    assert_bits(X, ref[:, :P - 1], "a prefix row differs from emb(token at j - 1) + cond[j]")
    assert_bits(xl, ref[:, P - 1], "x_last is not row P - 1")


@pytest.mark.gpu
@pytest.mark.parametrize("S,S_pad,Lmax", [(1, 64, 8), (70, 128, 130), (129, 192, 129), (1030, 1088, 2304)])
@pytest.mark.parametrize("H", [2, 16, 32])
@pytest.mark.parametrize("prec", PRECS)
def test_prefix_kv_to_cache(prec, H, S, S_pad, Lmax):
    """pure movement: k rows and V^T columns < S land in rows < S of the scene's cache; rows >= S, the q half and the pad columns never do"""
    B, E = 2, H * 48
    if S > 1000 and H > 2:
        Lmax = S + 3                                   # the long prefix at the wide heads: a shorter cache, the same rows
    rng = np.random.default_rng(H + S + prec)
    dt = np.float32 if prec == 0 else np.uint16
    qk = store(rng.standard_normal((B, S, 2 * E), dtype=np.float32), prec)[0]
    vt = store(rng.standard_normal((B, H, 48, S_pad), dtype=np.float32), prec)[0]
    cache = np.zeros((B, 2, H, Lmax, 48), dt)
    check(lib().umgen_dbg_prefix_kv_to_cache(prec, vp(qk), vp(vt), B, S, S_pad, H, Lmax, vp(cache)))
    ref = nan_array((B, 2, H, Lmax, 48), prec)
    ref[:, 0, :, :S] = qk[:, :, E:].reshape(B, S, H, 48).transpose(0, 2, 1, 3)
    ref[:, 1, :, :S] = vt[:, :, :, :S].transpose(0, 1, 3, 2)
    np.testing.assert_array_equal(raw(cache), raw(ref))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the token step
# ---------------------------------------------------------------------------------------------------------------------------
def sampler_params(**over):
    d = dict(method=0, top_k=5, top_k_map=5, topk_image=16, p=0.4, p_map=0.4, temperature=1.0, rule_constrain=1, merge_ar_tar=1, only_ar=0)
    d.update(over)
    return d


class Walk:
    """The oracle's own sampler, bbox3d branch and rule constraint (unbound OracleUMGen methods) on given logits: head_tar_bbox3d on the
    conditioning row is the logits_tar row of the position"""
    sample = OracleUMGen.sample
    _sample_bbox = OracleUMGen._sample_bbox
    _rule = OracleUMGen._rule

    def __init__(self, sp):
        self.cfg = types.SimpleNamespace(sample_method="topk" if sp["method"] == 0 else "top_p", sfmx_temp=sp["temperature"], top_k=sp["top_k"],
                                         p=sp["p"], top_k_map=sp["top_k_map"], p_map=sp["p_map"], topk_image=sp["topk_image"],
                                         merage_ar_tar=bool(sp["merge_ar_tar"]), only_ar=bool(sp["only_ar"]), rule_constrain=bool(sp["rule_constrain"]))
        self.w = None
        self.counts = Counter()
        self.lt = None

    def _count(self, k):
        self.counts[k] += 1

    def _lin(self, x, name, bias=True):
        assert name == "transformer.head_tar_bbox3d"
        return torch.from_numpy(self.lt.copy())


def kind_of(j, given_end):
    if j < given_end:
        return 0
    return 1 if MAP_C0 <= j < MAP_EOS else 2 if BOX_C0 <= j < BOX_EOS else 3 if IMG_C0 <= j < IMG_EOS else 0


class Steps:
    """inputs of umgen_dbg_token_steps for B scenes (every field can be edited before run / walk)"""

    def __init__(self, E, B, seed=0, n_box=1028, **sp):
        self.tb, self.E, self.B = tables(E, n_box), E, B
        rng = self.rng = np.random.default_rng(E + 100 * B + seed)
        self.V = {1: self.tb.dims["n_map"], 2: self.tb.dims["n_box"], 3: self.tb.dims["n_img"]}
        self.ld = 1100
        self.cond = rng.standard_normal((B, KSEQ, E), dtype=np.float32)
        self.logits_tar = rng.standard_normal((B, NBOX, self.V[2]), dtype=np.float32)
        self.prev_box = np.full((B, NBOX), PAD, np.int32)
        self.control = np.zeros((B, SLOTS), np.uint8)
        self.tokens = frame_tokens(rng, self.tb, B)
        self.forced = None
        self.seeds = rng.integers(0, 2 ** 63, B).astype(np.uint64)
        self.sp = sampler_params(**sp)
        self.use_control, self.frame_idx, self.given_end, self.epoch0 = 0, 3, POSE_EOS + 1, 7 * EPOCH_PER_STEP

    def random_logits(self, j0, j1):
        lg = self.rng.standard_normal((j1 - j0, self.B, self.ld), dtype=np.float32)
        self.mark_past_vocab(lg, j0)
        return lg

    def mark_past_vocab(self, lg, j0):
        for i in range(lg.shape[0]):            # columns past the position's vocabulary would win every draw if the sampler read them
            k = kind_of(j0 + i, self.given_end)
            if k:
                lg[i, :, self.V[k]:] = 3e4

    def peaked_logits(self, j0, j1, peak):
        """all mass on token peak(b, j): 1e4 above the rest, every other exp underflows to 0"""
        lg = np.zeros((j1 - j0, self.B, self.ld), np.float32)
        for i in range(j1 - j0):
            for b in range(self.B):
                lg[i, b, peak(b, j0 + i)] = 1e4
        self.mark_past_vocab(lg, j0)
        return lg

    def scene(self, b):
        """scene b alone"""
        s = Steps.__new__(Steps)
        s.__dict__.update(self.__dict__)
        s.B = 1
        for k in ("cond", "logits_tar", "prev_box", "control", "tokens", "seeds"):
            setattr(s, k, np.ascontiguousarray(getattr(self, k)[b:b + 1]))
        s.forced = None if self.forced is None else np.ascontiguousarray(self.forced[b:b + 1])
        return s

    def run(self, j0, j1, logits):
        B, E, n = self.B, self.E, j1 - j0
        out = types.SimpleNamespace(tokens=self.tokens.copy(), x_next=np.zeros((n, B, E), np.float32), counters=np.zeros(8, np.int32),
                                    n_boxes=np.zeros(B, np.int32), boxes=np.zeros((B, 64, 10), np.float64), state=np.zeros((n, 3), np.uint32))
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        assert logits.shape == (n, B, self.ld)
        a = DbgSteps(cond=fp(self.cond), logits=fp(logits), logits_tar=fp(self.logits_tar), prev_box=i32p(self.prev_box),
                     control_slot=self.control.ctypes.data_as(C.POINTER(C.c_ubyte)), forced=None if self.forced is None else i32p(self.forced),
                     seeds=u64p(self.seeds), tokens=i32p(out.tokens), x_next=fp(out.x_next), counters=i32p(out.counters), n_boxes=i32p(out.n_boxes),
                     boxes=out.boxes.ctypes.data_as(C.POINTER(C.c_double)), state_log=out.state.ctypes.data_as(C.POINTER(C.c_uint32)),
                     sp=DbgSamplerParams(**self.sp), B=B, j0=j0, j1=j1, given_end=self.given_end, ld_logits=self.ld,
                     use_forced=int(self.forced is not None), use_control=self.use_control, frame_idx=self.frame_idx, epoch0=self.epoch0)
        check(lib().umgen_dbg_token_steps(self.tb.ref, C.byref(a)))
        return out

    def walk(self, j0, j1, logits):
        """the oracle's walk over the same steps -> tokens, x_next, counters[6], n_boxes, boxes (list per scene).  sample, _sample_bbox, _rule and
        rng_uniform are the oracle's own code, called as _oar calls them; counter 5 (sampled != forced) has no counterpart in the oracle and is
        restated here: the token the oracle's samplers gave, compared with the forced one before it is overwritten"""
        B, tb = self.B, self.tb
        toks = self.tokens.copy()
        x_next = np.zeros((j1 - j0, B, self.E), np.float32)
        counters = np.zeros(6, np.int64)
        decoded = []
        for b in range(B):
            wk = Walk(self.sp)
            seed = int(self.seeds[b])
            slots = np.nonzero(self.control[b])[0] if self.use_control else None
            dec = []
            for i, j in enumerate(range(j0, j1)):
                kind, pos = kind_of(j, self.given_end), j + 1
                if kind == 0:
                    emb = token_embedding(tb, toks[b:b + 1], j)[0]
                else:
                    lg = torch.from_numpy(logits[i, b, :self.V[kind]].copy())
                    u = rng_uniform(seed, self.frame_idx, pos, DRAW_MAIN)
                    if kind == 1:
                        tok, at = wk.sample(lg, wk.cfg.top_k_map, wk.cfg.p_map, u), OFF_MAP + j - MAP_C0
                    elif kind == 3:
                        tok, at = wk.sample(lg, wk.cfg.topk_image, float(wk.cfg.topk_image), u), OFF_IMG + j - IMG_C0
                    else:
                        k = j - BOX_C0
                        at = OFF_BOX + k
                        wk.lt = self.logits_tar[b, k]
                        tok = wk._sample_bbox(lg, None, pos, self.prev_box[b], slots, seed, self.frame_idx, u)
                        if self.forced is None and wk.cfg.rule_constrain:
                            inferred = [int(t) for t in toks[b, OFF_BOX:at]]
                            tok = wk._rule(tok, inferred, dec, int(self.prev_box[b, pos - 1033]), pos)
                            toks[b, OFF_BOX:at] = inferred
                    if self.forced is not None:
                        counters[5] += int(tok != self.forced[b, at])
                        tok = int(self.forced[b, at])
                    toks[b, at] = tok
                    emb = {1: tb.gmap, 2: tb.be, 3: tb.gimg}[kind][tok]
                x_next[i, b] = emb + self.cond[b, j + 1]
            c = wk.counts
            counters[:5] += [c["pad_avoid"], c["control_resample"], c["rule_checked"], c["rule_collision"], c["rule_blanked"]]
            decoded.append(dec)
        return types.SimpleNamespace(tokens=toks, x_next=x_next, counters=counters, boxes=decoded, n_boxes=np.array([len(d) for d in decoded]))

    def check(self, j0, j1, logits):
        """hook == walk; -> (hook outputs, walk)"""
        got, ref = self.run(j0, j1, logits), self.walk(j0, j1, logits)
        np.testing.assert_array_equal(got.tokens, ref.tokens, err_msg="tokens differ from the oracle walk")
        np.testing.assert_array_equal(got.counters[:6], ref.counters, err_msg="event counters differ from the oracle walk")
        assert got.counters[6] == 0 and got.counters[7] == 0
        np.testing.assert_array_equal(got.n_boxes, ref.n_boxes, err_msg="n_boxes differs from the oracle walk")
        for b, dec in enumerate(ref.boxes):
            if dec:
                np.testing.assert_array_equal(got.boxes[b, :len(dec)].view(np.uint64), np.array(dec, np.float64).view(np.uint64),
                                              err_msg=f"decoded boxes of scene {b} differ bitwise")
        assert_bits(got.x_next, ref.x_next, "x_next differs from emb[token] + cond[b][j + 1]")
        n = j1 - j0
        np.testing.assert_array_equal(got.state[:, 0], np.arange(j0 + 1, j1 + 1), err_msg="step does not advance by 1 per launch")
        np.testing.assert_array_equal(got.state[:, 1], (self.epoch0 + EPOCH_PER_STEP * np.arange(1, n + 1)).astype(np.uint32), err_msg="epoch advance")
        assert not got.state[:, 2].any(), "done is not back at 0"
        return got, ref


def at_box(k):
    return BOX_C0 + k


STEP_WIDTHS = [96, 1536]


@pytest.mark.gpu
@pytest.mark.parametrize("E", STEP_WIDTHS)
def test_step_pad_avoid(E):
    """AR says pad, the previous frame had an object there: resample from logits_tar with the pad-avoid draw; no resample where prev is pad"""
    s = Steps(E, 2, rule_constrain=0)
    s.prev_box[0, 0:6] = [500, 1027, 3, 1027, 7, 1026]
    s.prev_box[1, 0:6] = 1027
    s.prev_box[1, 4] = 9
    got, ref = s.check(at_box(0), at_box(6), s.peaked_logits(at_box(0), at_box(6), lambda b, j: PAD))
    assert got.counters[0] == 5 and not got.counters[1:6].any()
    assert np.all(got.tokens[1, OFF_BOX:OFF_BOX + 4] == PAD)


@pytest.mark.gpu
@pytest.mark.parametrize("E", STEP_WIDTHS + [768])
def test_step_control_resample(E):
    """a controlled slot resamples from logits_tar with column V - 1 masked (the TAR peak sits ON V - 1 at one position: the mask decides) and the
    control draw; the category token of the last slot has object_id 60 and must not read control_slot[b][60] (= the next scene's slot 0)"""
    s = Steps(E, 2, rule_constrain=0, merge_ar_tar=0)
    s.use_control = 1
    s.control[0, 1] = 1            # object_id of position k is (k + 1) // 11: slot 1 covers k = 10 .. 20
    s.control[1, 0] = 1            # scene 1's slot 0 lies where control_slot[0][60] would be read
    s.logits_tar[0, 12] = 0
    s.logits_tar[0, 12, PAD] = 1e4
    s.logits_tar[0, 12, 77] = 50   # the runner-up the mask hands the draw to
    j0, j1 = at_box(8), at_box(23)
    got, ref = s.check(j0, j1, s.peaked_logits(j0, j1, lambda b, j: 5))
    assert got.counters[1] == 11 + 2 and got.tokens[0, OFF_BOX + 12] == 77       # scene 0: k = 10 .. 20; scene 1: k = 8, 9
    j0, j1 = at_box(655), at_box(660)
    got, ref = s.check(j0, j1, s.peaked_logits(j0, j1, lambda b, j: 6))
    assert got.counters[1] == 0 and np.all(got.tokens[:, OFF_BOX + 655:OFF_BOX + 660] == 6)


@pytest.mark.gpu
@pytest.mark.parametrize("E", STEP_WIDTHS)
def test_step_control_then_pad_avoid(E):
    """the control resample yields pad (the runner-up behind the masked column), the previous frame had an object: pad-avoid fires on top"""
    # with the product's vocabulary of 1028 the masked column V - 1 IS the pad token, so a control resample cannot yield pad; a vocabulary of
    # 1030 (mask on 1029) lets pad be the runner-up and shows the order of the two resamples
    s = Steps(E, 1, n_box=1030, rule_constrain=0)
    s.use_control = 1
    s.control[0, 0] = 1
    s.prev_box[0, 3] = 400
    s.logits_tar[0, 3] = 0
    s.logits_tar[0, 3, 1029] = 1e4          # masked in the control draw, the winner of the pad-avoid draw
    s.logits_tar[0, 3, PAD] = 5e3           # the runner-up: the control draw yields pad
    got, ref = s.check(at_box(3), at_box(4), s.peaked_logits(at_box(3), at_box(4), lambda b, j: 8))
    assert got.counters[1] == 1 and got.counters[0] == 1 and got.tokens[0, OFF_BOX + 3] == 1029


def object_tokens(x, y, length=4.0, width=2.0, yaw=0.0):
    """the 11 tokens of an object whose decoded centre / size / yaw are close to the arguments (bin centres), category 1024"""
    from umgen_amd.config import BBOX_RANGE
    vals = [x, y, 0.0, length, width, 1.5, yaw, 0.0, 0.0, 0.0]
    t = [int(np.clip(round((v - lo) / (hi - lo) * 1023 + 0.5), 1, 1023)) for v, (lo, hi) in zip(vals, BBOX_RANGE)]
    return t + [1024]


def scripted(objs):
    """peak(b, j) for a bbox3d section whose slot i holds objs[i] (11 tokens), pad behind them"""
    flat = [t for o in objs for t in o]
    return lambda b, j: flat[j - BOX_C0] if j - BOX_C0 < len(flat) else PAD


@pytest.mark.gpu
@pytest.mark.parametrize("E", STEP_WIDTHS)
def test_step_rule_constraint(E):
    """(a) a new-born box across the ego box is blanked with the 10 tokens before it; (b) the same box with an object in prev_box is kept;
    (c) a box with x >= 63 is ignored by the collision filter"""
    cross = object_tokens(2.0, 0.0)                     # x in [0, 4]: crosses the ego box's front edge at 2.588
    far = object_tokens(63.5, 0.0)                       # filtered out: cannot collide, and does not become the query box
    free = object_tokens(-30.0, 20.0)
    j0, j1 = at_box(0), at_box(44)
    s = Steps(E, 3)
    s.prev_box[1, 11:22] = 5                             # scene 1: slot 1 existed in the previous frame
    peak = scripted([free, cross, far, cross])
    got, ref = s.check(j0, j1, s.peaked_logits(j0, j1, peak))
    # scenes 0 and 2: both `cross` objects are new-born and collide -> blanked; `far` is filtered out, the query box is `free`: kept.
    # scene 1: the first `cross` is kept (not new-born); behind it `far` is filtered out, so the query box is that `cross` -- a collision, and the
    # new-born `far` is blanked (the reference tests the last box that SURVIVES the filter, misc.py:591-630)
    assert np.all(got.tokens[0, OFF_BOX + 11:OFF_BOX + 22] == PAD) and np.all(got.tokens[:, OFF_BOX + 33:OFF_BOX + 44] == PAD)
    assert list(got.tokens[1, OFF_BOX + 11:OFF_BOX + 22]) == cross
    assert list(got.tokens[0, OFF_BOX + 22:OFF_BOX + 33]) == far and np.all(got.tokens[1, OFF_BOX + 22:OFF_BOX + 33] == PAD)
    assert list(got.n_boxes) == [3, 3, 3] and list(got.counters[2:5]) == [12, 7, 6]


@pytest.mark.gpu
@pytest.mark.parametrize("E", STEP_WIDTHS)
def test_step_rule_more_than_30_boxes(E):
    """32 new-born objects that collide with nothing: from the point where the box list (the ego box counts) would exceed 30 every further one is blanked"""
    objs = [object_tokens(x, y) for y in (-30.0, -15.0, 15.0, 30.0) for x in (-48.0, -36.0, -24.0, -12.0, 12.0, 24.0, 36.0, 48.0)]
    s = Steps(E, 1)
    j0, j1 = at_box(0), at_box(11 * 34)
    got, ref = s.check(j0, j1, s.peaked_logits(j0, j1, scripted(objs)))
    assert ref.counters[3] == 0 and ref.counters[4] >= 2 and got.n_boxes[0] == 30
    kept = [bool(np.all(got.tokens[0, OFF_BOX + 11 * i:OFF_BOX + 11 * i + 11] != PAD)) for i in range(32)]
    assert kept == [i < sum(kept) for i in range(32)] and sum(kept) == 32 - int(ref.counters[4])


@pytest.mark.gpu
@pytest.mark.parametrize("E", STEP_WIDTHS)
def test_step_teacher_forcing_skips_the_rule(E):
    """under use_forced the rule constraint is skipped and counter 5 counts sampled != forced"""
    s = Steps(E, 2)
    s.forced = frame_tokens(s.rng, s.tb, 2)
    cross = object_tokens(2.0, 0.0)
    s.forced[0, OFF_BOX:OFF_BOX + 11] = cross
    j0, j1 = at_box(0), at_box(22)
    got, ref = s.check(j0, j1, s.peaked_logits(j0, j1, scripted([cross, cross])))
    assert got.counters[2] == 0 and got.counters[4] == 0 and got.counters[5] == ref.counters[5] > 0 and not got.n_boxes.any()
    np.testing.assert_array_equal(got.tokens[:, OFF_BOX:OFF_BOX + 22], s.forced[:, OFF_BOX:OFF_BOX + 22])


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("E", [96, 768])
def test_step_map_and_image_heads(E, method):
    """map positions draw with top_k_map / p_map, image positions with topk_image; in top-p mode the image head gets p = topk_image (keeps all)"""
    s = Steps(E, 2, method=method, top_k=2, top_k_map=3, topk_image=7, p=0.6, p_map=0.3)
    for j0, j1 in ((MAP_C0, MAP_C0 + 12), (MAP_EOS - 3, MAP_EOS + 2), (IMG_BOS, IMG_C0 + 12), (IMG_EOS - 6, IMG_EOS)):
        s.check(j0, j1, s.random_logits(j0, j1))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 8])
def test_step_batch(B):
    """step / epoch / done per launch at several scene counts (one block per scene; the last to arrive advances the state) on ordinary N(0, 1)
    logits over every kind of position, and scene b of the batch == scene b alone"""
    s = Steps(96, B, seed=B)
    s.prev_box[:] = s.rng.integers(0, 1028, (B, NBOX))
    s.use_control = 1
    s.control[:] = s.rng.integers(0, 2, (B, SLOTS))
    for j0, j1 in ((0, 9), (MAP_EOS - 2, at_box(24)), (BOX_EOS - 4, IMG_C0 + 3)):
        lg = s.random_logits(j0, j1)
        got, _ = s.check(j0, j1, lg)
        for b in range(B):
            one = s.scene(b).run(j0, j1, lg[:, b:b + 1])
            np.testing.assert_array_equal(one.tokens[0], got.tokens[b], err_msg=f"scene {b} alone differs from scene {b} of the batch")
            assert_bits(one.x_next[:, 0], got.x_next[:, b], f"x_next of scene {b} alone differs")


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
def test_sample_ego(B, method):
    """three draws per scene at positions 2207 + jq with the scene's seed; forced pose tokens override"""
    V, frame = 1024, 5
    rng = np.random.default_rng(B + method)
    sp = sampler_params(method=method, top_k=4, p=0.5)
    lg = rng.standard_normal((B, 3, V), dtype=np.float32)
    seeds = rng.integers(0, 2 ** 63, B).astype(np.uint64)
    wk = Walk(sp)
    ref = np.array([[wk.sample(torch.from_numpy(lg[b, q]), sp["top_k"], sp["p"], rng_uniform(int(seeds[b]), frame, KSEQ + q, DRAW_MAIN)) for q in range(3)]
                    for b in range(B)], np.int32)
    out = np.zeros((B, 3), np.int32)
    check(lib().umgen_dbg_sample_ego(fp(lg), V, C.byref(DbgSamplerParams(**sp)), u64p(seeds), frame, None, B, i32p(out)))
    np.testing.assert_array_equal(out, ref)
    forced = rng.integers(0, 1000, (B, TOK)).astype(np.int32)
    check(lib().umgen_dbg_sample_ego(fp(lg), V, C.byref(DbgSamplerParams(**sp)), u64p(seeds), frame, i32p(forced), B, i32p(out)))
    np.testing.assert_array_equal(out, forced[:, :3])
