"""Host side of the VQ encoders (umgen_amd/vq.py): key lists against the reference's own state dict, the test-raster recipe, the
``quantized`` helper, and -- on a box without a GPU -- the loud failure of VQEncoder (no CPU fallback)."""
import os
import sys

import numpy as np
import pytest

from tests.golden.make_vq_golden import FULL, SMALL
from tests.golden.refimport import REFERENCE_ROOT, reference_available
from umgen_amd.vq import IMAGE_VQ, MAP_VQ, VQEncoder, VQError, decoder_keys, encoder_keys, quantized, synth_vq_raster

CASES = {**SMALL, **FULL}


@pytest.mark.skipif(not reference_available(), reason="upstream reference not present (build-container only)")
@pytest.mark.parametrize("name", list(CASES))
def test_encoder_keys_are_the_reference_state_dict(name):
    sys.path.insert(0, REFERENCE_ROOT)
    from projects.tokenizer.vq_model import NormVQModel
    cfg = CASES[name]
    dd = dict(double_z=False, z_channels=cfg["z_channels"], resolution=cfg["resolution"], in_channels=cfg["out_ch"], out_ch=cfg["out_ch"],
              ch=cfg["ch"], ch_mult=list(cfg["ch_mult"]), num_res_blocks=cfg["num_res_blocks"], attn_resolutions=list(cfg["attn_resolutions"]), dropout=0.0)
    m = NormVQModel(n_embed=cfg["n_embed"], embed_dim=cfg["embed_dim"], ddconfig=dd, stride=cfg["post_quant_ks"], padding=cfg["post_quant_pad"], ckpt_path=None)
    ref = [(k, tuple(v.shape)) for k, v in m.state_dict().items()
           if k.startswith(("encoder.", "quant_conv.")) or k == "quantize.embedding.weight"]
    assert list(encoder_keys(cfg).items()) == ref
    assert set(encoder_keys(cfg)) & set(decoder_keys(cfg)) == {"quantize.embedding.weight"}


def test_encoder_keys_shape_without_the_reference():
    """What holds with or without the reference at hand: disjoint from the decoder's keys but for the codebook, in_channels honoured."""
    for cfg in CASES.values():
        keys = encoder_keys(cfg)
        assert set(keys) & set(decoder_keys(cfg)) == {"quantize.embedding.weight"}
        assert all(k.startswith(("encoder.", "quant_conv.")) or k == "quantize.embedding.weight" for k in keys)
        assert keys["encoder.conv_in.weight"] == (cfg["ch"], cfg["out_ch"], 3, 3)
        assert keys["quant_conv.weight"] == (cfg["embed_dim"], cfg["z_channels"], 1, 1)
    assert encoder_keys(dict(MAP_VQ, in_channels=7))["encoder.conv_in.weight"] == (128, 7, 3, 3)
    assert "encoder.down.4.attn.1.q.weight" in encoder_keys(IMAGE_VQ) and "encoder.down.3.downsample.conv.bias" in encoder_keys(IMAGE_VQ)
    assert not any(".attn." in k and ".down." in k for k in encoder_keys(MAP_VQ))       # the map encoder has no in-level attention
    assert "encoder.down.3.downsample.conv.weight" not in encoder_keys(MAP_VQ)           # no Downsample on the last level


@pytest.mark.parametrize("name", list(CASES))
def test_synth_vq_raster(name):
    cfg = CASES[name]
    L = len(cfg["ch_mult"])
    a = synth_vq_raster(cfg, 2, 11)
    assert a.dtype == np.float32 and a.shape == (2, cfg["out_ch"], cfg["token_hw"][0] << (L - 1), cfg["token_hw"][1] << (L - 1))
    assert a.tobytes() == synth_vq_raster(cfg, 2, 11).tobytes() and a.tobytes() != synth_vq_raster(cfg, 2, 12).tobytes()
    assert a.min() >= -1.0 and a.max() <= 1.0
    u = (a.astype(np.float64) + 1.0) * 127.5
    np.testing.assert_allclose(u, np.round(u), atol=1e-4)
    assert np.array_equal((np.round(u) / 127.5 - 1.0).astype(np.float32), a)
    assert a.std() > 0.3 and len(np.unique(a)) > 100


def test_quantized_against_a_direct_statement():
    rng = np.random.default_rng(2)
    cb = rng.standard_normal((6, 4)).astype(np.float32)
    codes = rng.integers(0, 6, size=(2, 3, 5))
    z = rng.standard_normal((2, 3, 5, 4)).astype(np.float32)
    z_q, loss = quantized(codes, z, cb)
    assert z_q.shape == (2, 4, 3, 5) and z_q.dtype == np.float32
    tot = 0.0
    for n in range(2):
        for y in range(3):
            for x in range(5):
                assert np.array_equal(z_q[n, :, y, x], cb[codes[n, y, x]])
                tot += float(((cb[codes[n, y, x]].astype(np.float64) - z[n, y, x]) ** 2).sum())
    assert abs(float(loss) - tot / z.size) < 1e-6


def test_encoder_has_no_cpu_fallback():
    """Like the engine's test in test_host.py: without a GPU the constructor fails loudly."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the constructor succeeds here")
    with pytest.raises(VQError):
        VQEncoder(SMALL["small_map"])
