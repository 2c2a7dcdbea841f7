"""The float64 restatement of the VQ decoder / encoder (tests/vq_ref.py) is pinned here, on the CPU, before any GPU test leans on it:
against the committed goldens (recorded from the reference's own classes), against the imported reference in float64 at the six
configurations of tests/test_gpu_vq_shapes.py (skipped where the reference is absent), and the input conditions those GPU tests rely on
(the margin cap of the code test must hold for the committed raster seeds by the restatement alone)."""
import os

import numpy as np
import pytest
import torch

from tests import vq_ref
from tests.golden.make_vq_golden import SEED, SMALL
from tests.golden.refimport import reference_available
from umgen_amd.vq import decoder_keys, encoder_keys, synth_vq_raster, synth_vq_tensor

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# 3 x the measured max |decode(float64) - golden out|, rounded up to one digit (measured: small_map 6.55e-6, small_image 1.01e-5; outputs reach 2.3 / 2.7)
DECODE_BARS = {"small_map": 2e-5, "small_image": 4e-5}


@pytest.mark.parametrize("name", list(SMALL))
def test_encode_equals_the_float64_goldens(name):
    """Both sides float64, only summation order can differ: rows to 1e-9; codes and runner-up equal wherever the recorded margin exceeds 1e-9."""
    cfg = SMALL[name]
    g = np.load(os.path.join(GOLD, f"vqenc_{name}.npz"))
    sd = {k: synth_vq_tensor(k, shape, SEED) for k, shape in encoder_keys(cfg).items()}
    codes, z, second, margin = vq_ref.encode(cfg, sd, synth_vq_raster(cfg, g["codes"].shape[0], int(g["seed"])), torch.float64)
    assert z.dtype == np.float64 and z.shape == g["z64"].shape
    assert float(np.abs(z - g["z64"]).max()) <= 1e-9
    clear = g["margin"] > 1e-9
    assert clear.mean() > 0.99
    np.testing.assert_array_equal(codes[clear], g["codes64"].astype(np.int64)[clear])
    np.testing.assert_array_equal(codes[clear], g["codes"].astype(np.int64)[clear])
    np.testing.assert_array_equal(second[clear], g["second64"].astype(np.int64)[clear])
    assert float(np.abs(margin - g["margin"]).max()) <= 1e-9


@pytest.mark.parametrize("name", list(SMALL))
def test_decode_is_within_fp32_of_the_goldens(name):
    """The goldens hold the reference's fp32 output, so the distance is the reference's own fp32 error.  Measured on the CPU:
    small_map 6.55e-6, small_image 1.01e-5 (the restatement's own float32-vs-float64 distance on the same inputs: 7.3e-6 and 8.0e-6).
    The bar is 3 x that, rounded up to one digit; anything above 5e-5 would mean a wrong restatement."""
    cfg = SMALL[name]
    g = np.load(os.path.join(GOLD, f"vq_{name}.npz"))
    sd = {k: synth_vq_tensor(k, shape, SEED) for k, shape in decoder_keys(cfg).items()}
    out = vq_ref.decode(cfg, sd, g["codes"].astype(np.int64), torch.float64)
    assert out.dtype == np.float64 and out.shape == g["out"].shape
    d = float(np.abs(out - g["out"]).max())
    print(f"{name}: max |decode(float64) - golden| = {d:.3e}, bar {DECODE_BARS[name]:.0e}")
    assert DECODE_BARS[name] <= 5e-5
    assert d <= DECODE_BARS[name]


def test_argmin_codes_on_a_direct_statement():
    rng = np.random.default_rng(4)
    cb = rng.standard_normal((7, 4))
    cb[5] = cb[2]                                          # an exact tie: the first wins, the runner-up is its twin at margin 0
    z = np.concatenate([cb[[2, 6]] * 1.0, rng.standard_normal((3, 4))])
    codes, second, margin = vq_ref.argmin_codes(z.reshape(1, 5, 4), cb)
    assert codes.shape == second.shape == margin.shape == (1, 5)
    d = ((z[:, None, :] - cb[None]) ** 2).sum(-1)
    order = np.argsort(d, axis=1, kind="stable")
    np.testing.assert_array_equal(codes[0], order[:, 0])
    np.testing.assert_array_equal(second[0, 1:], order[1:, 1])
    assert codes[0, 0] == 2 and second[0, 0] == 5 and margin[0, 0] == 0.0
    np.testing.assert_allclose(margin[0], np.sort(d, axis=1)[:, 1] - np.sort(d, axis=1)[:, 0], atol=1e-12)
    one = vq_ref.argmin_codes(z, cb[:1])
    assert not one[0].any() and (one[1] == -1).all() and np.isinf(one[2]).all()


@pytest.mark.parametrize("name", list(vq_ref.CONFIGS))
def test_the_committed_seeds_keep_the_code_test_meaningful(name):
    """The code test of tests/test_gpu_vq_shapes.py exempts positions whose float64 margin lies under code_threshold(err32_z) from equality.
    At most 2 % of a case may lie there (none where a case has fewer than 50 positions), by the restatement alone: a later change of
    seed cannot silently exempt everything.  The forced codes 0 and n_embed - 1 are in the decoder's input."""
    cfg = vq_ref.CONFIGS[name]
    r = vq_ref.restated(name)
    thr = vq_ref.code_threshold(r["err32_z"])
    under = r["margin"] < thr
    print(f"{name}: err32_z {r['err32_z']:.2e}, threshold {thr:.2e}, {int(under.sum())} of {under.size} positions under it, err32_out {r['err32_out']:.2e}")
    assert cfg["post_quant_pad"] == (cfg["post_quant_ks"] - 1) // 2
    assert r["x"].shape[:2] == (vq_ref.N_FRAMES, cfg["in_channels"]) and r["codes_in"].shape == (vq_ref.N_FRAMES,) + tuple(cfg["token_hw"])
    assert all(h * w < 200 for h, w in [(cfg["token_hw"][0] << lv, cfg["token_hw"][1] << lv) for lv in range(len(cfg["ch_mult"]))])
    assert max(cfg["ch_mult"]) * cfg["ch"] < 200
    assert under.mean() <= 0.02 and (under.size >= 50 or not under.any())
    assert 0 in r["codes_in"] and cfg["n_embed"] - 1 in r["codes_in"]
    assert 0.0 < r["err32_z"] < 1e-4 and 0.0 < r["err32_out"] < 1e-4            # fp32's own error on rows / outputs of unit scale
    np.testing.assert_allclose(np.linalg.norm(r["z64"], axis=-1), 1.0, atol=1e-12)


@pytest.mark.skipif(not reference_available(), reason="upstream reference not present (build-container only)")
@pytest.mark.parametrize("name", list(vq_ref.CONFIGS))
def test_restatement_equals_the_reference_in_float64(name):
    """The reference's own NormVQModel in float64 on the same weights and inputs: outputs and rows to 1e-9, codes equal."""
    from tests.golden.make_vq_encode_golden import reference_model as ref_encoder
    from tests.golden.make_vq_golden import reference_model as ref_decoder
    assert vq_ref.WEIGHT_SEED == SEED                     # the generators' reference models load synth_vq_tensor(.., SEED)
    cfg = vq_ref.CONFIGS[name]
    r = vq_ref.restated(name)
    with torch.no_grad():
        out = ref_decoder(cfg).double().decode_code(torch.from_numpy(np.array(r["codes_in"]))).numpy()
    assert out.shape == r["out64"].shape
    assert float(np.abs(out - r["out64"]).max()) <= 1e-9
    m = ref_encoder(cfg).double()
    with torch.no_grad():                                 # (the generator's rows_and_codes, without its top-2: single_token has one code)
        h = m.quant_conv(m.encoder(torch.from_numpy(np.array(r["x"])).double()))
        codes = m.quantize(h)[2].numpy()
        z = torch.nn.functional.normalize(h.permute(0, 2, 3, 1), p=2, dim=-1).numpy()
    assert z.shape == r["z64"].shape
    assert float(np.abs(z - r["z64"]).max()) <= 1e-9
    np.testing.assert_array_equal(codes, r["codes64"])
