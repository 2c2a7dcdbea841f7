"""-m gpu: the slot-indexed forms of three frame kernels that umgen_score_clip launches, through the hooks umgen_dbg_cond_rows_slots /
umgen_dbg_embed_warp_slots / umgen_dbg_ego_queries_slots, at E = 96.  Each is held bit for bit to the existing hook called on the window cut at the
item's slot -- what umgen_score launches for that window -- and the conditioning rows also to a float64 LayerNorm + warped-map sum within the bar
tests/test_gpu_frame_kernels.py states for conditioning rows (LN_BAR: |got - ref64| <= bar * max(1, |ref64|))."""
import numpy as np
import pytest

from tests.gpu_util import check, fp, lib
from tests.test_gpu_decode_layer import ln_input, ref_ln, rel_err
from tests.test_gpu_frame_kernels import (COND_ROWS, GROUP_MIX, KSEQ, LN_BAR, NMAP, STACK_BOX, STACK_LEN, STACK_MAP, STACK_TAR, all_nan, assert_bits,
                                          embed_warp_call, i32p, nan32, random_tokens, tables)

pytestmark = pytest.mark.gpu
E = 96


def test_cond_rows_slots_have_the_bits_of_the_window_cut_at_the_slot():
    """B = 2, T = 3; items: a first, a middle and a last slot, and scene 1 twice"""
    B, T = 2, 3
    items = np.array([[0, 0], [1, 1], [0, 2], [1, 2], [1, 1]], np.int32)
    rng = np.random.default_rng(5)
    wa = rng.standard_normal((B, T, NMAP, E), dtype=np.float32)
    worst = 0.0
    for stack in (STACK_MAP, STACK_BOX, STACK_TAR):
        SS = STACK_LEN[stack]
        X = ln_input(rng, B * T * SS, E).reshape(B, T, SS, E)
        lw = (1 + 0.2 * rng.standard_normal(E)).astype(np.float32)
        cond_all = nan32((len(items), KSEQ, E))
        check(lib().umgen_dbg_cond_rows_slots(stack, B, T, E, fp(X), fp(lw), fp(wa) if stack == STACK_MAP else None, i32p(items), len(items), fp(cond_all)))
        rows = COND_ROWS[stack]
        assert all_nan(cond_all[:, np.setdiff1d(np.arange(KSEQ), rows)]), f"stack {stack} wrote a row that is not its own"
        for i, (b, t) in enumerate(items.tolist()):
            Xc = np.ascontiguousarray(X[:, :t + 1])      # the window cut to T = t + 1: its last slot is slot t
            wl = np.ascontiguousarray(wa[:, t])
            cond = nan32((B, KSEQ, E))
            check(lib().umgen_dbg_cond_rows(stack, B, t + 1, E, fp(Xc), fp(lw), fp(wl) if stack == STACK_MAP else None, fp(cond)))
            assert_bits(cond_all[i], cond[b], f"stack {stack} item {i} = (scene {b}, slot {t}) differs from the cut window's rows")
            ref = ref_ln(X[b, t, rows], lw)
            if stack == STACK_MAP:
                ref[1:1 + NMAP] += wa[b, t].astype(np.float64)
            worst = max(worst, rel_err(cond_all[i][rows], ref))
    print(f"cond rows (slots) error {worst:.3e}")
    assert worst <= LN_BAR, f"conditioning-row error {worst:.3e} > bar {LN_BAR}"


@pytest.mark.parametrize("stack", [STACK_MAP, STACK_BOX, STACK_TAR])
def test_warped_map_of_every_slot_is_the_last_slot_of_the_cut_window(stack):
    B, T = 2, 3
    tb = tables(E)
    rng = np.random.default_rng(40 + stack)
    toks = random_tokens(rng, tb, B, T)
    pd = np.array([GROUP_MIX[i % len(GROUP_MIX)] for i in range(B * T)], np.float32).reshape(B, T, 3)
    X0, mf0, wl0 = embed_warp_call(tb, stack, toks, B, T, T, 0, pd, True)
    SS = STACK_LEN[stack]
    X, mf, wl = np.zeros((B, T, SS, E), np.float32), np.zeros((B, T, NMAP, E), np.float32), np.zeros((B, NMAP, E), np.float32)
    wa = np.zeros((B, T, NMAP, E), np.float32)
    check(lib().umgen_dbg_embed_warp_slots(stack, tb.ref, i32p(toks["pose"]), i32p(toks["map"]), i32p(toks["box"]), i32p(toks["img"]), B, T, T, 0, fp(pd), 1,
                                           fp(X), fp(mf), fp(wl), fp(wa)))
    assert_bits(X, X0, "X changed with the new output")
    assert_bits(mf, mf0, "mapfeat changed with the new output")
    assert_bits(wl, wl0, "warped_last changed with the new output")
    assert np.all(np.isfinite(wa)), "a slot's warped map is left unwritten"
    for t in range(T):
        cut = {k: np.ascontiguousarray(v[:, :t + 1]) for k, v in toks.items()}
        _, _, wlt = embed_warp_call(tb, stack, cut, B, t + 1, t + 1, 0, np.ascontiguousarray(pd[:, :t + 1]), True)
        assert_bits(wa[:, t], wlt, f"warped_all[:, {t}] differs from warped_last of the window cut to {t + 1} slots")


def test_ego_queries_take_their_items_window_length():
    tb = tables(E)
    item_T = np.array([3, 1, 6, 3, 2], np.int32)      # (n_tpe = 6)
    q = np.zeros((len(item_T), 3, E), np.float32)
    check(lib().umgen_dbg_ego_queries_slots(tb.ref, len(item_T), i32p(item_T), fp(q)))
    for i, Ti in enumerate(item_T.tolist()):
        one = np.zeros((1, 3, E), np.float32)
        check(lib().umgen_dbg_ego_queries(tb.ref, 1, Ti, fp(one)))
        assert_bits(q[i], one[0], f"item {i}: the queries of window length {Ti}")
    assert lib().umgen_dbg_ego_queries_slots(tb.ref, 1, i32p(np.array([7], np.int32)), fp(q)) == -1      # past the tpe table: refused, nothing launched
