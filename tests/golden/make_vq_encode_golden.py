"""Golden vectors of the VQ encoders, recorded from the REFERENCE's own classes:

    python tests/golden/make_vq_encode_golden.py [small] [full]      ->  tests/golden/vqenc_<case>.npz

imports the reference's projects/tokenizer/vq_model.py the way make_vq_golden.py does, builds NormVQModel for the four cases of
that file, loads the build's deterministic synthetic tensors (umgen_amd/vq.py: synth_vq_tensor) for every ``encoder.*`` /
``quant_conv.*`` key and the codebook, marks the codebook as initialised (no k-means init runs) and encodes
``synth_vq_raster(cfg, n, SEED + len(name))`` (2 frames small, 1 frame full) twice on the CPU: in fp32 (the reference as it runs)
and in float64 (``.double()``: the same model, the yardstick of the fp32 error).  Data only is stored:
  seed      the raster seed (weights: SEED of make_vq_golden.py)
  codes     the reference's fp32 codes [n, h, w]                     (asserted equal to codes64 here)
  z64       the float64 l2-normalised rows [n, h, w, embed_dim]
  codes64   the float64 arg-min
  second64  the float64 runner-up code per position
  margin    second-smallest minus smallest float64 distance per position
  z_err32   max |z_fp32 - z64| of the reference against itself (the tests' bar is 10 x this)

Recorded run (16 CPU threads):
  case         positions  z_err32   codes fp32 == fp64  margin < 1e-4  < 4e-4   < 1e-3   median margin
  small_map    512        1.0e-06   all                 0.0 %          0.0 %    0.0 %    0.100
  small_image  256        1.2e-06   all                 0.0 %          0.8 %    1.2 %    0.099
  full_image   512        1.3e-06   all                 0.0 %          0.2 %    1.0 %    0.048
  full_map     1024       1.2e-06   all                 0.2 %          0.4 %    1.0 %    0.051
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.golden.make_vq_golden import FULL, REF, SEED, SMALL  # noqa: E402
from umgen_amd.vq import encoder_keys, synth_vq_raster, synth_vq_tensor  # noqa: E402


def reference_model(cfg):
    import torch
    sys.path.insert(0, REF)
    from projects.tokenizer.vq_model import NormVQModel
    in_ch = cfg.get("in_channels", cfg["out_ch"])
    dd = dict(double_z=False, z_channels=cfg["z_channels"], resolution=cfg["resolution"], in_channels=in_ch, out_ch=cfg["out_ch"],
              ch=cfg["ch"], ch_mult=list(cfg["ch_mult"]), num_res_blocks=cfg["num_res_blocks"], attn_resolutions=list(cfg["attn_resolutions"]), dropout=0.0)
    m = NormVQModel(n_embed=cfg["n_embed"], embed_dim=cfg["embed_dim"], ddconfig=dd, stride=cfg["post_quant_ks"], padding=cfg["post_quant_pad"],
                    ckpt_path=None).eval()
    sd = {k: torch.from_numpy(synth_vq_tensor(k, shape, SEED)) for k, shape in encoder_keys(cfg).items()}
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all(k.startswith(("decoder.", "post_quant_conv.", "quantize.")) for k in res.missing_keys), res.missing_keys
    m.quantize.embedding.initted.data.copy_(torch.Tensor([True]))       # no k-means init (EmbeddingEMA.init_embed_)
    return m


def rows_and_codes(m, x):
    """The normalised rows the reference's quantiser searches on, its codes, and the two smallest distances with their codes."""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        h = m.quant_conv(m.encoder(x))
        _, _, idx = m.quantize(h)
        z = F.normalize(h.permute(0, 2, 3, 1), p=2, dim=-1)
        zf = z.reshape(-1, z.shape[-1])
        w = m.quantize.embedding.weight
        d = zf.pow(2).sum(dim=1, keepdim=True) + w.pow(2).sum(dim=1) - 2 * torch.einsum("bd,nd->bn", zf, w)
        two = torch.topk(d, 2, dim=1, largest=False)
    return z.numpy(), idx.numpy(), two.values.numpy(), two.indices.numpy()


def main(names):
    import torch
    for name in names:
        cfg = {**SMALL, **FULL}[name]
        n = 2 if name in SMALL else 1
        seed = SEED + len(name)
        x = torch.from_numpy(synth_vq_raster(cfg, n, seed))
        m = reference_model(cfg)
        t0 = time.time()
        z32, codes32, _, _ = rows_and_codes(m, x)
        t1 = time.time()
        z64, codes64, two_d, two_i = rows_and_codes(m.double(), x.double())
        assert codes32.shape == (n,) + tuple(cfg["token_hw"])
        assert np.array_equal(codes32, codes64), f"{name}: the reference's fp32 and float64 codes differ"
        assert np.array_equal(codes64.reshape(-1), two_i[:, 0])
        margin = (two_d[:, 1] - two_d[:, 0]).reshape(codes64.shape)
        z_err32 = float(np.abs(z32.astype(np.float64) - z64).max())
        print(f"  {name:<12} {margin.size:<10d} {z_err32:.1e}   all                 {100 * (margin < 1e-4).mean():.1f} %          "
              f"{100 * (margin < 4e-4).mean():.1f} %    {100 * (margin < 1e-3).mean():.1f} %    {np.median(margin):.3f}     "
              f"({t1 - t0:.1f} s fp32, {time.time() - t1:.1f} s float64)")
        path = os.path.join(ROOT, "tests", "golden", f"vqenc_{name}.npz")
        np.savez_compressed(path, seed=np.int32(seed), codes=codes32.astype(np.int16), z64=z64, codes64=codes64.astype(np.int16),
                            second64=two_i[:, 1].reshape(codes64.shape).astype(np.int16), margin=margin, z_err32=np.float64(z_err32))
        print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    sel = sys.argv[1:] or ["small", "full"]
    main([k for k in SMALL if "small" in sel] + [k for k in FULL if "full" in sel])
