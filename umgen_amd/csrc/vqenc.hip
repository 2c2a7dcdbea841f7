// VQ encoders on the GPU: map / image rasters to the tokens the rollout conditions on, the mirror image
// of vqdec.hip.  Replaces, value for value in fp32:
//   NormVQModelTokenizer.encode / NormVQModel.encode          projects/tokenizer/vq_tokenizer.py:25-47, vq_model.py:80-85
//   Encoder.forward (conv_in, down levels, mid blocks, norm_out, conv_out)   projects/tokenizer/vq_modules.py:179-290
//   Downsample (pad right 1 / bottom 1, 3 x 3 stride 2)                      vq_modules.py:43-60
//   quant_conv + NormEMAVectorQuantizer.forward (l2norm, arg-min of the three-term distance)   quantize.py:19-20, 414-429
// The eval-mode side effect of the reference's quantiser (the cluster_size usage EMA, quantize.py:435-439) is statistics only and is
// not reproduced.
//
// Layout and arithmetic (channels-last fp32 activations, every convolution one fp32 GEMM of this library) and the blocks shared with
// the decoder are in vq_common.h.  The NCHW ingest, the stride-2 im2col of Downsample and the quantiser used here are kept there too, beside their launchers.
#include "vq_common.h"

namespace {

struct Level { std::vector<Res> block; std::vector<Attn> attn; Conv down; bool has_down = false; };

}  // namespace

struct umgen_vqenc : Ctx {
    umgen_vq_config cfg{};
    int in_ch = 0, in_pad = 0;     // channels of the raster; the same rounded up to a multiple of 4 (zero lanes)
    float* emb = nullptr; bool emb_loaded = false;
    float* e2 = nullptr;           // |e_n|^2
    Conv conv_in, conv_out, quant_conv;
    std::vector<Level> down;       // index = i_level (0 = finest), like Encoder.down
    Res mid1, mid2;
    Attn mid_attn;
    Norm norm_out;
    float* d_in = nullptr;         // one frame [in_ch][H][W]
    long long* d_codes = nullptr;
    float* d_z = nullptr;          // normalised rows of one frame
    int in_h = 0, in_w = 0;
};

extern "C" {

const char* umgen_vqenc_last_error(const umgen_vqenc* e) { return e ? e->err.c_str() : "null encoder"; }

int umgen_vqenc_create(const umgen_vq_config* cfg, int32_t in_channels, umgen_vqenc** out) {
    if (!cfg || !out) return UMGEN_E_INVALID;
    *out = nullptr;
    umgen_vqenc* e = new umgen_vqenc();
    *out = e;
    e->cfg = *cfg;
    if (cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->num_res_blocks < 1 || cfg->ch < 32 || cfg->ch % 32 != 0)
        return e->fail(UMGEN_E_INVALID, "levels %d / res blocks %d / ch %d", cfg->n_levels, cfg->num_res_blocks, cfg->ch);
    if (in_channels < 1 || cfg->token_h < 1 || cfg->token_w < 1 || cfg->n_embed < 1)
        return e->fail(UMGEN_E_INVALID, "in_channels %d / token grid %d x %d / n_embed %d", in_channels, cfg->token_h, cfg->token_w, cfg->n_embed);
    if (cfg->embed_dim % 4 != 0 || cfg->z_channels % 4 != 0) return e->fail(UMGEN_E_UNSUPPORTED, "embed_dim and z_channels must be multiples of 4");
    if (cfg->embed_dim > kQuantMaxD) return e->fail(UMGEN_E_UNSUPPORTED, "embed_dim %d (the quantiser holds at most %d)", cfg->embed_dim, kQuantMaxD);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return e->fail(UMGEN_E_HIP, "no HIP device visible: libumgen_hip has no CPU fallback");
    VQCHK(e, hipSetDevice(cfg->device));
    VQCHK(e, gemm256_prepare());   // per device (the encoder's convolutions are this library's GEMMs)
    VQCHK(e, hipStreamCreate(&e->stream));
    const int L = cfg->n_levels;
    e->in_ch = in_channels;
    e->in_pad = (in_channels + 3) & ~3;
    // every Downsample halves an even grid: H = token_h << (L - 1) guarantees that by construction; refuse what would overflow an int
    if ((long)cfg->token_h << (L - 1) > 1 << 14 || (long)cfg->token_w << (L - 1) > 1 << 14)
        return e->fail(UMGEN_E_UNSUPPORTED, "raster of %ld x %ld pixels", (long)cfg->token_h << (L - 1), (long)cfg->token_w << (L - 1));
    e->in_h = cfg->token_h << (L - 1);
    e->in_w = cfg->token_w << (L - 1);
    // Encoder.__init__ (vq_modules.py:180-261), then quant_conv (vq_model.py:50) and the codebook
    if (int rc = reg_conv(e, "encoder.conv_in", e->conv_in, e->in_pad, cfg->ch, 3, 1, in_channels)) return rc;
    e->down.resize(L);
    int curr_res = cfg->resolution, block_in = cfg->ch, max_c = cfg->ch;
    size_t act = (size_t)e->in_h * e->in_w * std::max(e->in_pad, cfg->ch), colsz = (size_t)e->in_h * e->in_w * 9 * e->in_pad;
    long n_att = 0;
    {
        int H = e->in_h, W = e->in_w;
        for (int lv = 0; lv < L; ++lv) {
            Level& d = e->down[lv];
            const int block_out = cfg->ch * cfg->ch_mult[lv];
            bool at = false;
            for (int a = 0; a < cfg->n_attn_res; ++a) at = at || cfg->attn_resolutions[a] == curr_res;
            d.block.resize(cfg->num_res_blocks);
            if (at) d.attn.resize(cfg->num_res_blocks);
            act = std::max(act, (size_t)H * W * std::max(block_in, block_out));
            colsz = std::max(colsz, (size_t)H * W * 9 * std::max(block_in, block_out));
            for (int b = 0; b < cfg->num_res_blocks; ++b) {
                if (int rc = reg_res(e, "encoder.down." + std::to_string(lv) + ".block." + std::to_string(b), d.block[b], block_in, block_out)) return rc;
                block_in = block_out;
                if (at) { if (int rc = reg_attn(e, "encoder.down." + std::to_string(lv) + ".attn." + std::to_string(b), d.attn[b], block_in)) return rc; }
            }
            if (at) n_att = std::max(n_att, (long)H * W);
            max_c = std::max(max_c, block_out);
            if (lv != L - 1) {
                if (H % 2 || W % 2) return e->fail(UMGEN_E_UNSUPPORTED, "level %d is %d x %d: Downsample needs an even grid", lv, H, W);
                d.has_down = true;
                if (int rc = reg_conv(e, "encoder.down." + std::to_string(lv) + ".downsample.conv", d.down, block_in, block_in, 3, 0)) return rc;
                curr_res /= 2;
                H /= 2; W /= 2;
            }
        }
        n_att = std::max(n_att, (long)H * W);      // the mid block always has one
        act = std::max(act, (size_t)H * W * std::max(block_in, std::max(cfg->z_channels, cfg->embed_dim)));
    }
    if (int rc = reg_res(e, "encoder.mid.block_1", e->mid1, block_in, block_in)) return rc;
    if (int rc = reg_attn(e, "encoder.mid.attn_1", e->mid_attn, block_in)) return rc;
    if (int rc = reg_res(e, "encoder.mid.block_2", e->mid2, block_in, block_in)) return rc;
    if (int rc = reg_norm(e, "encoder.norm_out", e->norm_out, block_in)) return rc;
    if (int rc = reg_conv(e, "encoder.conv_out", e->conv_out, block_in, cfg->z_channels, 3, 1)) return rc;
    if (int rc = reg_conv(e, "quant_conv", e->quant_conv, cfg->z_channels, cfg->embed_dim, 1, 0)) return rc;
    if (int rc = vq_alloc(e, &e->emb, (size_t)cfg->n_embed * cfg->embed_dim)) return rc;
    e->slots["quantize.embedding.weight"] = Ctx::Slot{e->emb, {cfg->n_embed, cfg->embed_dim}, nullptr, &e->emb_loaded};
    if (int rc = vq_alloc(e, &e->e2, (size_t)cfg->n_embed)) return rc;
    // workspace for one frame: the largest H * W * C products over the levels
    for (float** p : {&e->x, &e->h, &e->t}) { if (int rc = vq_alloc(e, p, act)) return rc; }
    if (int rc = vq_alloc(e, &e->col, colsz)) return rc;
    if (int rc = vq_alloc(e, &e->stats, 64)) return rc;
    if (n_att > 16384) return e->fail(UMGEN_E_UNSUPPORTED, "attention over %ld positions (scores would need %ld MB)", n_att, n_att * n_att * 4 >> 20);
    if (int rc = vq_alloc(e, &e->scores, (size_t)n_att * attn_ld(n_att))) return rc;
    for (float** p : {&e->q, &e->k, &e->vt}) { if (int rc = vq_alloc(e, p, (size_t)attn_ld(n_att) * max_c)) return rc; }
    const size_t n_tok = (size_t)cfg->token_h * cfg->token_w;
    if (int rc = vq_alloc(e, &e->d_in, (size_t)in_channels * e->in_h * e->in_w)) return rc;
    if (int rc = vq_alloc(e, &e->d_z, n_tok * cfg->embed_dim)) return rc;
    VQCHK(e, hipMalloc(reinterpret_cast<void**>(&e->d_codes), n_tok * sizeof(long long)));
    e->allocs.push_back(e->d_codes);
    return UMGEN_OK;
}

int umgen_vqenc_load_tensor(umgen_vqenc* e, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
    if (!e || !key || !data) return UMGEN_E_INVALID;
    return load_slot(e, key, data, shape, ndim);      // 1: decoder.*, post_quant_conv.*, EMA buffers: not read by the encode path
}

int umgen_vqenc_finalize(umgen_vqenc* e) {
    if (!e) return UMGEN_E_INVALID;
    if (int rc = check_slots(e, "encoder")) return rc;
    VQCHK(e, hipSetDevice(e->cfg.device));
    launch_code_norms(e->stream, e->emb, e->cfg.n_embed, e->cfg.embed_dim, e->e2);
    VQCHK(e, hipStreamSynchronize(e->stream));
    VQCHK(e, hipGetLastError());
    e->finalized = true;
    return UMGEN_OK;
}

// x [n][in_ch][H][W] -> codes [n][token_h][token_w] (and z [n][token_h][token_w][embed_dim], the rows the search ran on)
int umgen_vqenc_encode(umgen_vqenc* e, int32_t n, const float* x, int64_t* codes, float* z) {
    if (!e || !x || !codes || n < 0) return UMGEN_E_INVALID;
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_vqenc_finalize has not been called");
    const umgen_vq_config& cfg = e->cfg;
    const int L = cfg.n_levels;
    const long n_tok = (long)cfg.token_h * cfg.token_w;
    const long n_in = (long)e->in_ch * e->in_h * e->in_w;
    for (long i = 0; i < (long)n * n_in; ++i)
        if (!std::isfinite(x[i])) return e->fail(UMGEN_E_INVALID, "input value at flat index %ld is not finite", i);
    VQCHK(e, hipSetDevice(cfg.device));
    for (int f = 0; f < n; ++f) {
        int H = e->in_h, W = e->in_w;
        VQCHK(e, hipMemcpyAsync(e->d_in, x + (long)f * n_in, n_in * sizeof(float), hipMemcpyHostToDevice, e->stream));
        launch_from_nchw(e->stream, e->d_in, (long)H * W, e->in_ch, e->in_pad, e->h);
        conv(e, e->conv_in, e->h, H, W, e->x, false);                      // Encoder.forward
        for (int lv = 0; lv < L; ++lv) {
            const Level& d = e->down[lv];
            for (int b = 0; b < cfg.num_res_blocks; ++b) {
                res_block(e, d.block[b], H, W);
                if (!d.attn.empty()) attn_block(e, d.attn[b], H, W);
            }
            if (d.has_down) {
                const int C = d.down.cin;
                launch_im2col_s2(e->stream, e->x, H, W, C, e->col);
                H /= 2; W /= 2;
                conv_gemm(e, d.down, e->col, 9 * C, (long)H * W, e->t, false);
                std::swap(e->x, e->t);
            }
        }
        res_block(e, e->mid1, H, W);
        attn_block(e, e->mid_attn, H, W);
        res_block(e, e->mid2, H, W);
        group_norm(e, e->norm_out, e->x, (long)H * W, true, e->h);
        conv(e, e->conv_out, e->h, H, W, e->t, false);
        conv(e, e->quant_conv, e->t, H, W, e->h, false);                   // NormVQModel.encode: quant_conv
        launch_quantize(e->stream, e->h, e->quant_conv.cout_pad, e->emb, e->e2, cfg.n_embed, cfg.embed_dim, n_tok, e->d_codes, e->d_z);
        VQCHK(e, hipMemcpyAsync(codes + (long)f * n_tok, e->d_codes, n_tok * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
        if (z) VQCHK(e, hipMemcpyAsync(z + (long)f * n_tok * cfg.embed_dim, e->d_z, n_tok * cfg.embed_dim * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        VQCHK(e, hipStreamSynchronize(e->stream));     // once per frame: the frame's buffers are reused by the next one
    }
    VQCHK(e, hipGetLastError());
    return UMGEN_OK;
}

int umgen_vqenc_destroy(umgen_vqenc* e) {
    if (!e) return UMGEN_OK;
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    for (void* p : e->allocs) (void)hipFree(p);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return UMGEN_OK;
}

}  // extern "C"
