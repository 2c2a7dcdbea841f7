"""One decode step of the batched decode layer (umgen_amd/csrc/decode_batched.hip: rows_to_frag, then per layer rows_mfma_kernel QKV,
attn_decode_batched_kernel, rows_mfma_kernel RESID, GELU, RESID) as the handle runs it -- oar_layers of engine_decode.hip through the hook
umgen_dbg_oar_step with use_engine 2 -- against the fp64 restatement of the whole BlockOAR stack of tests/test_gpu_engine_step.py, whose
machinery (plan, stack_ref, check_step, same_bits, the family and seam registries, the bars and their header table) this file uses.  Every
test needs a GPU except the last one.

What a step on the live handle adds to the kernel tests (tests/test_gpu_decode_kernels.py): the weights as engine_weights.hip stored them, the K/V
cache at its real [layer][scene][2][H][Lmax][48] strides on a 64-scene handle, the position read from the device OarState, rows_to_frag in front of
the first layer, the fragment-major hand-offs between the launches and the layers, the attention launch reading row L that the q|k|v launch wrote in
the same stream, and the fragment-major copy of x behind the last layer, which is what the head's launch streams (umgen_dbg_oar_step_frag hands it
back): it must equal the row-major x bit for bit.

Families (FAMILY): rows, E = 768, 4 layers, on a handle for 64 scenes; rows96, E = 96 (three k-steps: waves 3 .. 7 of rows_mfma_kernel have no
work in the E-wide GEMMs), for 17 scenes.  Both handles are created with UMGEN_DECODE_BATCHED=1, so every batch size takes the path.  Key patterns as
in the engines' step tests, the seam key (pattern 1) on an edge of rows_partition: rows_seam.  The hook refuses use_engine 0 on such a handle, so the
five-launch cross-check of the reference runs the same plans on a handle of the same layers with UMGEN_DECODE_BATCHED=0.

Fixed arithmetic (bit for bit on x, the new rows and the fragment copy): a scene inside a batch == the scene alone across column-block edges
and kernel instantiations (NB, RT, JB differ between 1, 17, 33 and 64 scenes); whatever earlier steps left in the fragment columns past the batch
does not matter.
"""
import numpy as np
import pytest

from tests.gpu_util import SCALE_QK, gelu64, ref_ln, round16
from tests.test_gpu_decode_layer import LAYER_BAR, rel_err, store, stored
from tests.test_gpu_engine_step import (FAMILY, PREC_NAME, PRECS, ROWS96_CASES, ROWS_CASES, ROWS_STEP_BAR, check_step, create, download, handles_fixture,
                                        new_rows, params, pattern, plan, preload, run_step, same_bits, stack_ref, step_input, sub_plan)

rows = handles_fixture("rows")
rows96 = handles_fixture("rows96")
five = handles_fixture("rows5")


def batched_step(e, pl, x=None, L=None, load=True):
    """-> (x out [B][E], the fragment-major copy of x as rows [B][E], per layer the cache rows [B][2][H][n][48] behind the step)"""
    if load:
        preload(e, pl)
    out, frag = e.dbg_oar_step(pl.x0 if x is None else x, pl.L if L is None else L, 2, return_frag=True)
    return out, frag, download(e, pl)


def frag_is_x(out, frag, what=""):
    np.testing.assert_array_equal(frag.view(np.uint32), out.view(np.uint32), err_msg=f"{what}the fragment-major copy of x (the head's input) differs from x")


def rows_case(e, pl):
    bar = ROWS_STEP_BAR[pl.fam][pl.prec]
    out, frag, got = batched_step(e, pl)
    err = check_step(pl, pl.caches, pl.x0, pl.L, out, got, bar, True)
    print(f"ENGSTEP {pl.fam} {PREC_NAME[pl.prec]} B={pl.B} L={pl.L}: batched layer {err:.3e} (bar {bar:.1e})")
    frag_is_x(out, frag)
    assert err <= bar, f"max error {err:.3e} > bar {bar:.1e}"


def batched_only(e, pl, **kw):
    """-> ((x out, the new rows), the fragment copy)"""
    out, frag, got = batched_step(e, pl, **kw)
    return (out, new_rows(got, pl.L)), frag


def same_step(a, b, what):
    same_bits(a[0], b[0], what)
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32), err_msg=f"{what}: the fragment-major copy of x differs")


@pytest.mark.gpu
@pytest.mark.parametrize("B,L", ROWS_CASES)
@pytest.mark.parametrize("prec", PRECS)
def test_batched_layer_step(rows, prec, B, L):
    """1 .. 4 column blocks of 16 scenes, full and ragged (15 | 16 | 17, 32 | 33, 48 | 49, 64), every position of ROWS_POS at 1 and 2 scenes"""
    rows_case(rows(prec), plan("rows", prec, B, L))


@pytest.mark.gpu
@pytest.mark.parametrize("B,L", ROWS96_CASES)
@pytest.mark.parametrize("prec", PRECS)
def test_batched_layer_step_at_three_k_steps(rows96, prec, B, L):
    rows_case(rows96(prec), plan("rows96", prec, B, L))


@pytest.mark.gpu
@pytest.mark.parametrize("B,L", [(1, 2206), (2, 257), (17, 257)])
@pytest.mark.parametrize("prec", PRECS)
def test_rows_plans_on_five_launches_per_layer(five, prec, B, L):
    """the reference with the batched layer's seams is right independently of the path under test"""
    e, pl = five(prec), plan("rows", prec, B, L)
    out, got = run_step(e, pl, 0)
    err = check_step(pl, pl.caches, pl.x0, L, out, got, LAYER_BAR, True)
    bar = len(pl.caches) * LAYER_BAR
    print(f"ENGSTEP rows {PREC_NAME[prec]} B={B} L={L}: five launches {err:.3e} (bar {bar:.1e})")
    assert err <= bar, f"five launches per layer: max error {err:.3e} > {bar:.1e}"


# ---------------------------------------------------------------------------------------------------------------------------
# fixed arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,L", [(17, 257), (33, 63), (64, 65)])
@pytest.mark.parametrize("prec", PRECS)
def test_scene_in_a_batch_equals_the_scene_alone(rows, prec, B, L):
    """scenes 0, 15 | 16 (a column-block edge) and the last: 2, 3 and 4 column blocks against 1 (other NB, RT, JB of rows_mfma_kernel)"""
    e, pl = rows(prec), plan("rows", prec, B, L)
    (out, nrows), frag = batched_only(e, pl)
    for b in sorted({0, 15, 16, B - 1}):
        same_step(batched_only(e, sub_plan(pl, b)), ((out[b:b + 1], [r[b:b + 1] for r in nrows]), frag[b:b + 1]), f"scene {b} of {B}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_stale_fragment_columns_do_not_matter(rows, prec):
    """17 scenes multiply 2 column blocks: columns 17 .. 31 of the fragment buffers are computed on what a 64-scene step with |x| ~ 1e30 left there,
    and never stored.  Same bits as on a handle (for 17 scenes: other cache strides) that has run nothing else."""
    pl = plan("rows", prec, 17, 257)
    fresh = create("rows", prec, max_batch=17)
    try:
        ref = batched_only(fresh, pl)
    finally:
        fresh.close()
    e = rows(prec)
    rng = np.random.default_rng(3)
    big = (1e30 * rng.uniform(0.5, 2.0, (64, 1)) * rng.standard_normal((64, FAMILY["rows"].E))).astype(np.float32)
    out, frag = e.dbg_oar_step(big, pl.L, 2, return_frag=True)
    assert np.abs(frag[17:]).min() > 1e20, "the 64-scene step left nothing large in the fragment columns"
    same_step(batched_only(e, pl), ref, "17 scenes behind a 64-scene step against a fresh handle")


# ---------------------------------------------------------------------------------------------------------------------------
# carry-over: each step's attention reads the rows that the previous steps' q|k|v launches wrote through the handle's strides
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L0", [62, 254])
@pytest.mark.parametrize("prec", PRECS)
def test_batched_steps_carry_over(rows, prec, L0):
    """four consecutive steps without a new preload: rows 62 .. 65 cross the first pass round, 254 .. 257 the first flight batch"""
    e, B, bar = rows(prec), 2, ROWS_STEP_BAR["rows"][prec]
    pl = plan("rows", prec, B, L0)
    rng = np.random.default_rng(L0 + prec)
    preload(e, pl)
    before = [c.copy() for c in pl.caches]
    for t in range(4):
        x = pl.x0 if t == 0 else step_input(rng, B, FAMILY["rows"].E)
        out, frag, got = batched_step(e, pl, x=x, L=L0 + t, load=False)
        err = check_step(pl, before, x, L0 + t, out, got, bar, t == 0)
        print(f"ENGSTEP carry-over rows {PREC_NAME[prec]} B={B} L={L0 + t}: {err:.3e}")
        frag_is_x(out, frag, f"step {t}: ")
        assert err <= bar, f"step {t} at L = {L0 + t}: max error {err:.3e} > {bar:.1e}"
        before = got


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the bar sees what it is for
# ---------------------------------------------------------------------------------------------------------------------------
def chain(pl, drop=False, round_act=False):
    """The fp64 stack on a plan with the reference's own rounding of the new rows -> (x out, [l] the new rows' bits).  drop: one cached key (the
    middle one) masked out of every all-equal (pattern 2) head; round_act: the activations entering the four GEMMs of every layer rounded to the
    16-bit type (a lost lo part of the hi + lo split)."""
    prec, L = pl.prec, pl.L
    r16 = (lambda a: round16(a, prec).astype(np.float64)) if round_act else (lambda a: a)
    x, bits = pl.x0.astype(np.float64), []
    for l, (P, c) in enumerate(zip(params(pl.fam, prec), pl.caches)):
        B, E = x.shape
        H = E // 48
        hv = stored(np.ascontiguousarray(c[:, :, :, :L]), prec)
        qkv = r16(ref_ln(x, P["ln_a"])) @ P["Wqkv"].T + P["bqkv"]
        nb, new = store(qkv[:, E:].reshape(B, 2, H, 48), prec)
        K, V = (np.concatenate([hv[:, j], new[:, j][:, :, None]], axis=2) for j in (0, 1))
        s = np.einsum("bhd,bhnd->bhn", qkv[:, :E].reshape(B, H, 48), K) * SCALE_QK
        if drop:
            for b in range(B):
                for h in range(H):
                    if pattern(b, h, l) == 2:
                        s[b, h, L // 2] = -np.inf
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        x1 = x + r16(np.einsum("bhn,bhnd->bhd", p, V).reshape(B, E)) @ P["Wo"].T + P["bo"]
        x = x1 + r16(gelu64(r16(ref_ln(x1, P["ln_b"])) @ P["Wfc"].T)) @ P["Wproj"].T
        bits.append(nb)
    return x, bits


@pytest.mark.parametrize("prec", PRECS)
def test_bar_sees_a_dropped_key_and_a_lost_lo_part(prec):
    """A condition on the inputs of (1, 2206), not a measurement: a reference that drops one cached key of 2206 from every all-equal head, and one
    that loses the lo part of every GEMM's activations, are each at least 4 x the bar away from stack_ref in the measure the bar is applied in.
    Distances (bf16 | fp16): dropped key 1.8e-3 | 1.7e-3, no lo part 1.5e-2 | 1.7e-3."""
    pl = plan("rows", prec, 1, 2206)
    x, bits = chain(pl)
    ref = stack_ref(pl.x0, params("rows", prec), pl.caches, bits, prec, pl.L)[0]
    assert rel_err(x, ref) <= 1e-12, "chain does not restate stack_ref"
    assert sum(pattern(0, h, l) == 2 for l in range(4) for h in range(16)) >= 12
    bar = ROWS_STEP_BAR["rows"][prec]
    for what, wrong in (("one cached key dropped from the all-equal heads", chain(pl, drop=True)[0]), ("no lo part", chain(pl, round_act=True)[0])):
        d = rel_err(wrong, ref)
        print(f"ENGSTEP rows {PREC_NAME[prec]} wrong reference, {what}: {d:.3e} (bar {bar:.1e})")
        assert d >= 4 * bar, f"{what}: {d:.3e} from stack_ref, less than 4 x the bar {bar:.1e}"
