"""-m gpu: the VQ encoders (csrc/vqenc.hip through the C ABI) against rows and codes recorded from the
reference's own NormVQModel.encode (tests/golden/make_vq_encode_golden.py) on the same seeded weights and rasters.

fp32 throughout.  The bar on the pre-quantisation rows is set by the reference itself: Z_BAR = 10 x z_err32, the reference's own
fp32-vs-float64 distance stored in each golden (1.0e-5 - 1.3e-5).  The two fp32 sides differ only in summation order (one k-ascending
fmaf chain up to K = 4608 here, blocked sums in torch's CPU convolution) and in expf / GroupNorm-statistics implementations, a small
single-digit factor over the reference's own error; a wrong padding, a transposed kernel or a missed bias moves z by 1e-2 and more.

Measured on an MI355X, max |z_gpu - z64| against Z_BAR:
  small_map    1.9e-6  (Z_BAR 1.01e-5)      small_image  1.8e-6  (Z_BAR 1.24e-5)
  full_map     3.6e-6  (Z_BAR 1.25e-5)      full_image   5.4e-6  (Z_BAR 1.31e-5)
and every code equal to the reference's in all four cases (0.0 - 0.4 % of the positions lie under the margin threshold of
test_codes_match_reference, 1.6e-4 - 2.1e-4; none of them flipped).
"""
import os

import numpy as np
import pytest

from tests.golden.make_vq_golden import FULL, SEED, SMALL
from umgen_amd.vq import (Imagetokenizer, Maptokenizer, VQDecoder, VQEncoder, VQError, decoder_keys, encoder_keys, quantized,
                          synth_vq_raster, synth_vq_tensor)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = {**SMALL, **FULL}


def weights(cfg, keys=encoder_keys):
    return {k: synth_vq_tensor(k, shape, SEED) for k, shape in keys(cfg).items()}


def make(cfg, sd=None):
    e = VQEncoder(cfg)
    sd = dict(weights(cfg) if sd is None else sd)
    sd["decoder.conv_in.weight"] = np.zeros((4, 4, 3, 3), np.float32)      # present in real checkpoints, not read by the encode path
    missing, unexpected = e.load_state_dict(sd)
    assert not missing and unexpected == ["decoder.conv_in.weight"]
    return e


_runs = {}


def run(name):
    """One encode per case and session: (golden, codes, z, codebook)."""
    if name not in _runs:
        g = np.load(os.path.join(GOLD, f"vqenc_{name}.npz"))
        cfg = CASES[name]
        e = make(cfg)
        x = synth_vq_raster(cfg, g["codes"].shape[0], int(g["seed"]))
        codes, z = e.encode(x, return_z=True)
        e.close()
        assert codes.shape == g["codes"].shape and codes.dtype == np.int64 and z.shape == g["z64"].shape and z.dtype == np.float32
        _runs[name] = (g, codes, z, synth_vq_tensor("quantize.embedding.weight", (cfg["n_embed"], cfg["embed_dim"]), SEED))
    return _runs[name]


@pytest.mark.parametrize("name", list(CASES))
def test_rows_match_reference(name):
    """Pre-quantisation rows: max |z_gpu - z64| <= 10 x the reference's own fp32-vs-float64 distance."""
    g, _, z, _ = run(name)
    z_bar = 10.0 * float(g["z_err32"])
    err = float(np.abs(z.astype(np.float64) - g["z64"]).max())
    print(f"{name}: max |z_gpu - z64| = {err:.3e}, Z_BAR = {z_bar:.3e}, reference fp32 vs float64 = {float(g['z_err32']):.3e}")
    assert err <= z_bar


@pytest.mark.parametrize("name", list(CASES))
def test_codes_match_reference(name):
    """eps_row = 4 Z_BAR bounds the l2 distance of a row (16 channels) from the reference's; each of two distances then moves by at most
    2 eps_row |e_n| (|e_n| = 1), so the arg-min can differ only where the recorded margin is under 4 eps_row + 1e-6.  Everywhere
    else the codes are the reference's; under the threshold they are its best or second-best; and the threshold may exempt at most
    2 % of a case."""
    g, codes, _, _ = run(name)
    thr = 4.0 * (4.0 * 10.0 * float(g["z_err32"])) + 1e-6
    close = g["margin"] < thr
    diff = codes != g["codes"].astype(np.int64)
    print(f"{name}: threshold {thr:.3e}, {100.0 * close.mean():.2f} % of positions under it, {int(diff.sum())} codes differ from the reference "
          f"({int((diff & ~close).sum())} of them at or above the threshold)")
    assert close.mean() <= 0.02
    assert not (diff & ~close).any()
    assert np.all((codes == g["codes"]) | (codes == g["second64"]))


def host_argmin(z, codebook):
    """float64 three-term distances from the GPU's own rows: arg-min and the margin to the runner-up."""
    zf = z.reshape(-1, z.shape[-1]).astype(np.float64)
    w = codebook.astype(np.float64)
    d = (zf ** 2).sum(1, keepdims=True) + (w ** 2).sum(1)[None] - 2.0 * zf @ w.T
    best = d.argmin(1)
    two = np.partition(d, 1, axis=1)[:, :2]
    return best, two[:, 1] - two[:, 0]


@pytest.mark.parametrize("name", list(CASES))
def test_quantiser_is_the_exact_argmin_of_its_own_rows(name):
    _, codes, z, codebook = run(name)
    best, margin = host_argmin(z, codebook)
    clear = margin > 1e-6
    print(f"{name}: {100.0 * (~clear).mean():.2f} % of positions within 1e-6, {int((codes.reshape(-1) != best).sum())} codes differ from the float64 arg-min")
    assert (~clear).mean() < 0.005
    np.testing.assert_array_equal(codes.reshape(-1)[clear], best[clear])
    np.testing.assert_allclose(np.linalg.norm(z.astype(np.float64), axis=-1), 1.0, atol=1e-6)


def test_quantiser_breaks_exact_ties_towards_the_lower_index():
    """A codebook whose rows come in identical pairs (n and n + 32): every position's two best distances are bit-equal, the lower
    index must win like torch.argmin -- also across lanes of the wave reduction and across codebook orders."""
    cfg = SMALL["small_image"]
    sd = weights(cfg)
    cb = sd["quantize.embedding.weight"].copy()
    cb[32:] = cb[:32]
    for perm in (np.arange(64), np.arange(64)[::-1].copy()):
        sd["quantize.embedding.weight"] = np.ascontiguousarray(cb[perm])
        e = make(cfg, sd)
        codes, z = e.encode(synth_vq_raster(cfg, 2, 5), return_z=True)
        e.close()
        best, _ = host_argmin(z, cb[perm])          # numpy's argmin: the first of the equal minima in float64 as well
        twin = np.array([int(np.flatnonzero((cb[perm] == cb[perm][c]).all(1))[0]) for c in codes.reshape(-1)])
        np.testing.assert_array_equal(codes.reshape(-1), twin)        # the lower index of its identical pair
        assert (codes.reshape(-1) == best).mean() > 0.99              # and that pair is the nearest one
        assert len(np.unique(codes)) > 8


def test_frames_are_independent():
    cfg = SMALL["small_image"]
    e = make(cfg)
    x = synth_vq_raster(cfg, 3, 23)
    codes, z = e.encode(x, return_z=True)
    for i in range(3):
        ci, zi = e.encode(x[i:i + 1], return_z=True)
        np.testing.assert_array_equal(ci[0], codes[i])
        assert zi[0].tobytes() == z[i].tobytes()
    assert np.array_equal(e.encode(x), codes)
    e.close()


@pytest.mark.parametrize("name", ["small_map", "small_image"])
def test_round_trip_through_decoder_and_encoder(name):
    """Interop / workspace test: a decoder and an encoder handle alive together on one device (no equality is expected with
    synthetic weights)."""
    cfg = CASES[name]
    d = VQDecoder(cfg)
    d.load_state_dict(weights(cfg, decoder_keys))
    e = make(cfg)
    codes = np.random.default_rng(9).integers(0, cfg["n_embed"], size=(2,) + tuple(cfg["token_hw"]))
    img = d.decode_code(codes)
    back, z = e.encode(img, return_z=True)
    again = d.decode_code(back)
    assert back.shape == codes.shape and back.dtype == np.int64 and back.min() >= 0 and back.max() < cfg["n_embed"]
    assert again.shape == img.shape and np.isfinite(again).all()
    np.testing.assert_array_equal(d.decode_code(codes), img)          # the decoder's workspace is its own
    z_q, loss = e.quantized(back, z)
    assert z_q.shape == (2, cfg["embed_dim"]) + tuple(cfg["token_hw"]) and 0.0 <= float(loss) < 4.0 / cfg["embed_dim"]
    d.close()
    e.close()


def test_wrappers_and_errors(tmp_path):
    """Maptokenizer / Imagetokenizer on the rollout's token layout; malformed inputs fail loudly."""
    cfg = SMALL["small_image"]
    sd = weights(cfg)
    tok = Imagetokenizer(sd, cfg=cfg)
    x = synth_vq_raster(cfg, 3, 31)
    toks = tok.encode_images(x)
    assert toks.shape == (3, 8 * 16) and toks.dtype == np.int64
    np.testing.assert_array_equal(toks, tok.enc.encode(x).reshape(3, -1))
    u8 = np.round((np.moveaxis(x, 1, -1).astype(np.float64) + 1.0) * 127.5).astype(np.uint8)
    np.testing.assert_array_equal(tok.encode_images(u8), toks)            # the rasters lie on the uint8 grid
    with pytest.raises(VQError, match="shape"):
        tok.enc.encode(np.zeros((1, 3, 32, 32), np.float32))
    bad = x.copy()
    bad[1, 2, 5, 7] = np.nan
    with pytest.raises(VQError, match="finite"):
        tok.enc.encode(bad)
    bare = VQEncoder(cfg)
    with pytest.raises(VQError, match="finalize"):
        bare.encode(x[:1])
    with pytest.raises(VQError, match="dim 1"):
        bare.load_state_dict({"encoder.conv_in.weight": np.zeros((32, 4, 3, 3), np.float32)})
    bare.close()
    mcfg = SMALL["small_map"]
    mtok = Maptokenizer(weights(mcfg), cfg=mcfg)
    mx = synth_vq_raster(mcfg, 2, 37)
    mt = mtok.encode_maps(mx)
    assert mt.shape == (2, 256) and mt.min() >= 0 and mt.max() < mcfg["n_embed"]
    # a checkpoint path that holds both halves of the model: decoder keys are reported as unexpected, not an error
    import torch
    both = {**weights(mcfg), **weights(mcfg, decoder_keys)}
    sdm = {k: torch.from_numpy(v) for k, v in both.items()}
    torch.save({"state_dict": sdm}, tmp_path / "map_vq.pt")
    np.testing.assert_array_equal(Maptokenizer(str(tmp_path / "map_vq.pt"), cfg=mcfg).encode_maps(mx), mt)
    enc = VQEncoder(mcfg)
    missing, unexpected = enc.load_state_dict(both)
    enc.close()
    assert not missing and sorted(unexpected) == sorted(k for k in decoder_keys(mcfg) if k != "quantize.embedding.weight")
    del sdm["encoder.conv_out.bias"]
    with pytest.raises(VQError, match="lacks 1 encoder"):
        Maptokenizer(sdm, cfg=mcfg)
