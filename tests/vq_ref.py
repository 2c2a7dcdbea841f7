"""A float64 restatement of the VQ decoder and encoder (umgen_amd/vq.py, csrc/vqdec.hip, csrc/vqenc.hip) in torch.nn.functional on the CPU:
the yardstick of the GPU tests at configurations no recording exists for (tests/test_gpu_vq_shapes.py), pinned itself by
tests/test_vq_ref.py against the committed goldens and, where the reference is at hand, against the reference's own classes in float64.

Written from the description of the arithmetic, on the state dicts of ``decoder_keys`` / ``encoder_keys`` / ``synth_vq_tensor``:
  conv2d;  GroupNorm(32 groups, eps 1e-6, affine);  swish x * sigmoid(x);  single-head attention over the H * W positions with C^-0.5 scaling;
  nearest 2x upsampling followed by a 3 x 3 convolution;  Downsample = zero pad of 1 on the right and bottom, then a 3 x 3 stride-2
  convolution without padding;  quantiser z / max(|z|, 1e-12), then the first arg-min of |z|^2 + |e|^2 - 2 z.e.
``dtype`` is torch.float64 (the reference value) or torch.float32 (only to measure fp32's own distance from float64).
"""
import numpy as np
import torch
import torch.nn.functional as F


class _Net:
    """the state dict in one dtype, and the layers by key prefix"""

    def __init__(self, sd, dtype):
        self.dtype = dtype
        self.sd = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(v))).to(dtype) for k, v in sd.items()}

    def has(self, k):
        return k + ".weight" in self.sd

    def conv(self, k, x, stride=1, padding=0):
        return F.conv2d(x, self.sd[k + ".weight"], self.sd[k + ".bias"], stride=stride, padding=padding)

    def norm(self, k, x, swish=False):
        y = F.group_norm(x, 32, self.sd[k + ".weight"], self.sd[k + ".bias"], eps=1e-6)
        return y * torch.sigmoid(y) if swish else y

    def res(self, k, x):
        h = self.conv(k + ".conv1", self.norm(k + ".norm1", x, swish=True), padding=1)
        h = self.conv(k + ".conv2", self.norm(k + ".norm2", h, swish=True), padding=1)
        if self.has(k + ".nin_shortcut"):
            x = self.conv(k + ".nin_shortcut", x)
        return x + h

    def attn(self, k, x):
        b, c, hh, ww = x.shape
        h = self.norm(k + ".norm", x)
        q = self.conv(k + ".q", h).reshape(b, c, hh * ww).transpose(1, 2)          # [b, position, c]
        kk = self.conv(k + ".k", h).reshape(b, c, hh * ww).transpose(1, 2)
        v = self.conv(k + ".v", h).reshape(b, c, hh * ww).transpose(1, 2)
        w = torch.softmax((q @ kk.transpose(1, 2)) * (float(c) ** -0.5), dim=-1)    # [b, query, key]
        o = (w @ v).transpose(1, 2).reshape(b, c, hh, ww)
        return x + self.conv(k + ".proj_out", o)


def decode(cfg, sd, codes, dtype=torch.float64):
    """codes [n, h, w] -> rasters [n, out_ch, H, W] (numpy, in ``dtype``)"""
    net = _Net(sd, dtype)
    L = len(cfg["ch_mult"])
    with torch.no_grad():
        z = net.sd["quantize.embedding.weight"][torch.from_numpy(np.asarray(codes, dtype=np.int64))].permute(0, 3, 1, 2)
        h = net.conv("post_quant_conv", z, padding=cfg["post_quant_pad"])
        h = net.conv("decoder.conv_in", h, padding=1)
        h = net.res("decoder.mid.block_1", h)
        h = net.attn("decoder.mid.attn_1", h)
        h = net.res("decoder.mid.block_2", h)
        for lv in reversed(range(L)):
            for b in range(cfg["num_res_blocks"] + 1):
                h = net.res(f"decoder.up.{lv}.block.{b}", h)
                if net.has(f"decoder.up.{lv}.attn.{b}.norm"):
                    h = net.attn(f"decoder.up.{lv}.attn.{b}", h)
            if lv != 0:
                h = net.conv(f"decoder.up.{lv}.upsample.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"), padding=1)
        h = net.conv("decoder.conv_out", net.norm("decoder.norm_out", h, swish=True), padding=1)
    return h.numpy()


def _two_best(z, codebook):
    """z [P, D], codebook [N, D] (float64 tensors) -> best code, runner-up code (-1 if N == 1), margin (inf if N == 1)"""
    d = (z ** 2).sum(1, keepdim=True) + (codebook ** 2).sum(1)[None] - 2.0 * z @ codebook.T
    best = torch.argmin(d, dim=1)                      # the first of equal minima
    if codebook.shape[0] == 1:
        return best.numpy(), np.full(best.shape, -1, np.int64), np.full(best.shape, np.inf)
    rest = d.clone()
    rest[torch.arange(d.shape[0]), best] = float("inf")
    second = torch.argmin(rest, dim=1)
    margin = rest.gather(1, second[:, None])[:, 0] - d.gather(1, best[:, None])[:, 0]
    return best.numpy(), second.numpy(), margin.numpy()


def argmin_codes(z, codebook):
    """The quantiser on rows z [..., D] as they are (not normalised here) in float64: (codes, runner-up codes, float64 margin between the two
    smallest distances), each of shape z.shape[:-1]."""
    z = np.asarray(z, dtype=np.float64)
    best, second, margin = _two_best(torch.from_numpy(z.reshape(-1, z.shape[-1])), torch.from_numpy(np.asarray(codebook, dtype=np.float64)))
    return best.reshape(z.shape[:-1]), second.reshape(z.shape[:-1]), margin.reshape(z.shape[:-1])


def encode(cfg, sd, x, dtype=torch.float64):
    """rasters x [n, in_channels, H, W] -> (codes [n, h, w], normalised rows z [n, h, w, embed_dim], runner-up codes [n, h, w], margin [n, h, w]):
    the arg-min, the runner-up and the margin between their distances are taken in float64 on the rows computed in ``dtype``."""
    net = _Net(sd, dtype)
    L = len(cfg["ch_mult"])
    with torch.no_grad():
        h = net.conv("encoder.conv_in", torch.from_numpy(np.asarray(x)).to(dtype), padding=1)
        for lv in range(L):
            for b in range(cfg["num_res_blocks"]):
                h = net.res(f"encoder.down.{lv}.block.{b}", h)
                if net.has(f"encoder.down.{lv}.attn.{b}.norm"):
                    h = net.attn(f"encoder.down.{lv}.attn.{b}", h)
            if lv != L - 1:
                h = net.conv(f"encoder.down.{lv}.downsample.conv", F.pad(h, (0, 1, 0, 1)), stride=2)
        h = net.res("encoder.mid.block_1", h)
        h = net.attn("encoder.mid.attn_1", h)
        h = net.res("encoder.mid.block_2", h)
        h = net.conv("encoder.conv_out", net.norm("encoder.norm_out", h, swish=True), padding=1)
        h = net.conv("quant_conv", h).permute(0, 2, 3, 1)
        z = h / torch.linalg.vector_norm(h, dim=-1, keepdim=True).clamp_min(1e-12)
        best, second, margin = _two_best(z.reshape(-1, z.shape[-1]).double(), net.sd["quantize.embedding.weight"].double())
    shp = tuple(z.shape[:-1])
    return best.reshape(shp), z.numpy(), second.reshape(shp), margin.reshape(shp)


# ---- the configurations of tests/test_gpu_vq_shapes.py (and of the restatement-vs-reference check in tests/test_vq_ref.py) ------------------------
def _cfg(ch, ch_mult, nrb, res, attn, thw, z, d, n, cin, cout, ks):
    return dict(n_embed=n, embed_dim=d, z_channels=z, resolution=res, in_channels=cin, out_ch=cout, ch=ch, ch_mult=ch_mult, num_res_blocks=nrb,
                attn_resolutions=attn, post_quant_ks=ks, post_quant_pad=(ks - 1) // 2, token_hw=thw)


CONFIGS = {
    # no resampling; C = 32 attention in-level and mid over n = 15; D = 4; N = 64 + 1
    "one_level": _cfg(32, (1,), 1, 8, (8,), (3, 5), 4, 4, 65, 1, 1, 3),
    # GroupNorm with 3 and 6 channels per group; C = 192 attention over 35; quantiser tile 256 with a partial tile of 44
    "wide_groups": _cfg(96, (1, 2), 1, 16, (), (5, 7), 8, 32, 300, 2, 7, 1),
    # attention at every level (96 / 24 / 6 positions): the finest level sets the attention workspace; D = 64 (tile 128, third tile partial)
    "attn_everywhere": _cfg(32, (1, 1, 2), 2, 32, (32, 16, 8), (2, 3), 12, 64, 300, 5, 5, 1),
    # the widest level is the finest; nin_shortcut 96 -> 32 and 32 -> 64; tile 512, third tile of 76 rows
    "shrinking_widths": _cfg(32, (3, 1, 2), 1, 32, (), (1, 2), 16, 16, 1100, 3, 3, 3),
    # attention over 1 and 4 positions; every 3 x 3 tap but the centre is padding at the coarse level; one code; 3 res blocks; 7 -> 8 pad lanes
    "single_token": _cfg(32, (1, 2), 3, 16, (16,), (1, 1), 4, 4, 1, 7, 7, 3),
    # n = 99: softmax lane loop with a ragged tail, odd K in the P.V GEMM; N = 128 + 1
    "ninety_nine": _cfg(64, (1,), 2, 8, (), (9, 11), 4, 16, 129, 3, 3, 1),
}
WEIGHT_SEED = 17
# raster seeds chosen so that the restatement alone meets the margin condition of the code test with room to spare: the smallest margin is 5 x
# the threshold or more in every case (test_vq_ref.py asserts the condition itself)
RASTER_SEEDS = {"one_level": 101, "wide_groups": 203, "attn_everywhere": 201, "shrinking_widths": 104, "single_token": 105, "ninety_nine": 106}
N_FRAMES = 2


def code_threshold(err32_z):
    """test_codes_match_reference's rule: the arg-min can differ only where the margin is under 4 x (4 x Z_BAR) + 1e-6, Z_BAR = 10 x err32"""
    return 4.0 * (4.0 * 10.0 * err32_z) + 1e-6


def weights(cfg, keys):
    from umgen_amd.vq import synth_vq_tensor
    return {k: synth_vq_tensor(k, shape, WEIGHT_SEED) for k, shape in keys(cfg).items()}


def shape_codes(name):
    """random codes [N_FRAMES, h, w] with code 0 and code n_embed - 1 both forced in"""
    cfg = CONFIGS[name]
    rng = np.random.default_rng(RASTER_SEEDS[name])
    codes = rng.integers(0, cfg["n_embed"], size=(N_FRAMES,) + tuple(cfg["token_hw"]), dtype=np.int64)
    codes.reshape(-1)[0] = 0
    codes.reshape(-1)[-1] = cfg["n_embed"] - 1
    return codes


_restated = {}


def restated(name):
    """One restatement per configuration and session, left unchanged: dict of the inputs (codes_in, x), the float64 values (out64; codes64, z64,
    second64, margin) and fp32's own distances from them (err32_out, err32_z)."""
    if name not in _restated:
        from umgen_amd.vq import decoder_keys, encoder_keys, synth_vq_raster
        cfg = CONFIGS[name]
        r = {"codes_in": shape_codes(name), "x": synth_vq_raster(cfg, N_FRAMES, RASTER_SEEDS[name])}
        sd_d, sd_e = weights(cfg, decoder_keys), weights(cfg, encoder_keys)
        r["out64"] = decode(cfg, sd_d, r["codes_in"], torch.float64)
        r["err32_out"] = float(np.abs(decode(cfg, sd_d, r["codes_in"], torch.float32).astype(np.float64) - r["out64"]).max())
        r["codes64"], r["z64"], r["second64"], r["margin"] = encode(cfg, sd_e, r["x"], torch.float64)
        r["err32_z"] = float(np.abs(encode(cfg, sd_e, r["x"], torch.float32)[1].astype(np.float64) - r["z64"]).max())
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _restated[name] = r
    return _restated[name]
