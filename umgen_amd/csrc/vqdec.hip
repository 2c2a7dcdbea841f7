// VQ decoders on the GPU: the map VQ-VAE and image VQGAN decoders that turn the rollout's map / image
// tokens back into rasters.  Replaces, value for value in fp32:
//   NormVQModel.decode_code / indices_to_quant + decode      projects/tokenizer/vq_model.py:88-103, 126-150
//   Decoder.forward (conv_in, mid blocks, up levels, norm_out, conv_out)   projects/tokenizer/vq_modules.py:293-415
//   ResnetBlock / AttnBlock / Upsample / Normalize / nonlinearity           vq_modules.py:14-40, 63-176
// as called by Mapdecoder.decode_maps / Imagedecoder.decode_images (projects/tools/decode_map.py:110-183).
//
// Layout and arithmetic (channels-last fp32 activations, every convolution one fp32 GEMM of this library) and the blocks shared with
// the encoder (vqenc.hip) are in vq_common.h.
#include "vq_common.h"

namespace {

// z[p][c] = embedding[code[p]][c]
__global__ void vq_embed_kernel(const long long* __restrict__ codes, const float* __restrict__ emb, int C, long n_px, float* __restrict__ z) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px * C) return;
    const long p = i / C;
    z[i] = emb[codes[p] * C + (i % C)];
}

struct Level { std::vector<Res> block; std::vector<Attn> attn; Conv up; bool has_up = false; };

}  // namespace

struct umgen_vq : Ctx {
    umgen_vq_config cfg{};
    float* emb = nullptr; bool emb_loaded = false;
    Conv post_quant, conv_in, conv_out;
    Res mid1, mid2;
    Attn mid_attn;
    std::vector<Level> up;     // index = i_level (0 = finest), like Decoder.up
    Norm norm_out;
    long long* d_codes = nullptr;
    float* d_out = nullptr;
    int out_h = 0, out_w = 0;
};

extern "C" {

const char* umgen_vq_last_error(const umgen_vq* e) { return e ? e->err.c_str() : "null decoder"; }

int umgen_vq_create(const umgen_vq_config* cfg, umgen_vq** out) {
    if (!cfg || !out) return UMGEN_E_INVALID;
    *out = nullptr;
    umgen_vq* e = new umgen_vq();
    *out = e;
    e->cfg = *cfg;
    if (cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->num_res_blocks < 1 || cfg->ch < 32 || cfg->ch % 32 != 0)
        return e->fail(UMGEN_E_INVALID, "levels %d / res blocks %d / ch %d", cfg->n_levels, cfg->num_res_blocks, cfg->ch);
    if (cfg->embed_dim % 4 != 0 || cfg->z_channels % 4 != 0) return e->fail(UMGEN_E_UNSUPPORTED, "embed_dim and z_channels must be multiples of 4");
    if (cfg->post_quant_ks != 1 && cfg->post_quant_ks != 3) return e->fail(UMGEN_E_UNSUPPORTED, "post_quant_conv kernel size 1 or 3");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return e->fail(UMGEN_E_HIP, "no HIP device visible: libumgen_hip has no CPU fallback");
    VQCHK(e, hipSetDevice(cfg->device));
    VQCHK(e, gemm256_prepare());   // per device (the decoder's convolutions are this library's GEMMs)
    VQCHK(e, hipStreamCreate(&e->stream));
    const int L = cfg->n_levels;
    // Decoder.__init__ (vq_modules.py:294-383)
    int block_in = cfg->ch * cfg->ch_mult[L - 1];
    int curr_res = cfg->resolution >> (L - 1);
    if (int rc = vq_alloc(e, &e->emb, (size_t)cfg->n_embed * cfg->embed_dim)) return rc;
    e->slots["quantize.embedding.weight"] = Ctx::Slot{e->emb, {cfg->n_embed, cfg->embed_dim}, nullptr, &e->emb_loaded};
    if (int rc = reg_conv(e, "post_quant_conv", e->post_quant, cfg->embed_dim, cfg->z_channels, cfg->post_quant_ks, cfg->post_quant_pad)) return rc;
    if (int rc = reg_conv(e, "decoder.conv_in", e->conv_in, cfg->z_channels, block_in, 3, 1)) return rc;
    if (int rc = reg_res(e, "decoder.mid.block_1", e->mid1, block_in, block_in)) return rc;
    if (int rc = reg_attn(e, "decoder.mid.attn_1", e->mid_attn, block_in)) return rc;
    if (int rc = reg_res(e, "decoder.mid.block_2", e->mid2, block_in, block_in)) return rc;
    e->up.resize(L);
    int max_c = block_in;
    for (int lv = L - 1; lv >= 0; --lv) {
        Level& u = e->up[lv];
        const int block_out = cfg->ch * cfg->ch_mult[lv];
        bool at = false;
        for (int a = 0; a < cfg->n_attn_res; ++a) at = at || cfg->attn_resolutions[a] == curr_res;
        u.block.resize(cfg->num_res_blocks + 1);
        if (at) u.attn.resize(cfg->num_res_blocks + 1);
        for (int b = 0; b <= cfg->num_res_blocks; ++b) {
            const std::string key = "decoder.up." + std::to_string(lv) + ".block." + std::to_string(b);
            if (int rc = reg_res(e, key, u.block[b], block_in, block_out)) return rc;
            block_in = block_out;
            if (at) { if (int rc = reg_attn(e, "decoder.up." + std::to_string(lv) + ".attn." + std::to_string(b), u.attn[b], block_in)) return rc; }
        }
        max_c = std::max(max_c, block_out);
        if (lv != 0) {
            u.has_up = true;
            if (int rc = reg_conv(e, "decoder.up." + std::to_string(lv) + ".upsample.conv", u.up, block_in, block_in, 3, 1)) return rc;
            curr_res *= 2;
        }
    }
    if (int rc = reg_norm(e, "decoder.norm_out", e->norm_out, block_in)) return rc;
    if (int rc = reg_conv(e, "decoder.conv_out", e->conv_out, block_in, cfg->out_ch, 3, 1)) return rc;
    // workspace for one frame at the finest level (the largest H * W * C products)
    e->out_h = cfg->token_h << (L - 1);
    e->out_w = cfg->token_w << (L - 1);
    size_t act = 0, colsz = 0;
    {
        int c_in = cfg->ch * cfg->ch_mult[L - 1], H = cfg->token_h, W = cfg->token_w;
        act = std::max(act, (size_t)H * W * std::max(c_in, std::max(cfg->embed_dim, cfg->z_channels)));
        colsz = std::max(colsz, (size_t)H * W * 9 * std::max(c_in, std::max(cfg->embed_dim, cfg->z_channels)));
        for (int lv = L - 1; lv >= 0; --lv) {
            const int c_out = cfg->ch * cfg->ch_mult[lv];
            act = std::max(act, (size_t)H * W * std::max(c_in, c_out));
            colsz = std::max(colsz, (size_t)H * W * 9 * std::max(c_in, c_out));
            c_in = c_out;
            if (lv != 0) {
                H *= 2; W *= 2;
                act = std::max(act, (size_t)H * W * c_in);
                colsz = std::max(colsz, (size_t)H * W * 9 * c_in);
            }
        }
    }
    for (float** p : {&e->x, &e->h, &e->t}) { if (int rc = vq_alloc(e, p, act)) return rc; }
    if (int rc = vq_alloc(e, &e->col, colsz)) return rc;
    if (int rc = vq_alloc(e, &e->stats, 64)) return rc;
    // attention workspaces: the positions of the coarsest level (attention only exists where curr_res is in attn_resolutions; the
    // mid block always has one): bounded by token_h * token_w * 4^(levels with attention) -- allocate for the finest attention level
    {
        long n_att = (long)cfg->token_h * cfg->token_w;
        int res = cfg->resolution >> (L - 1);
        long n = n_att;
        for (int lv = L - 1; lv >= 0; --lv) {
            for (int a = 0; a < cfg->n_attn_res; ++a)
                if (cfg->attn_resolutions[a] == res) n_att = std::max(n_att, n);
            if (lv != 0) { res *= 2; n *= 4; }
        }
        if (n_att > 16384) return e->fail(UMGEN_E_UNSUPPORTED, "attention over %ld positions (scores would need %ld MB)", n_att, n_att * n_att * 4 >> 20);
        if (int rc = vq_alloc(e, &e->scores, (size_t)n_att * attn_ld(n_att))) return rc;
        for (float** p : {&e->q, &e->k, &e->vt}) { if (int rc = vq_alloc(e, p, (size_t)attn_ld(n_att) * max_c)) return rc; }
    }
    VQCHK(e, hipMalloc(reinterpret_cast<void**>(&e->d_codes), (size_t)cfg->token_h * cfg->token_w * sizeof(long long)));
    e->allocs.push_back(e->d_codes);
    if (int rc = vq_alloc(e, &e->d_out, (size_t)cfg->out_ch * e->out_h * e->out_w)) return rc;
    return UMGEN_OK;
}

int umgen_vq_load_tensor(umgen_vq* e, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
    if (!e || !key || !data) return UMGEN_E_INVALID;
    return load_slot(e, key, data, shape, ndim);      // 1: encoder.*, quant_conv.*, EMA buffers: not read by the decode path
}

int umgen_vq_finalize(umgen_vq* e) {
    if (!e) return UMGEN_E_INVALID;
    if (int rc = check_slots(e, "decoder")) return rc;
    e->finalized = true;
    return UMGEN_OK;
}

// codes [n][token_h][token_w] -> out [n][out_ch][H][W] (the layout NormVQModel.decode_code returns)
int umgen_vq_decode(umgen_vq* e, int32_t n, const int64_t* codes, float* out) {
    if (!e || !codes || !out || n < 0) return UMGEN_E_INVALID;
    if (!e->finalized) return e->fail(UMGEN_E_STATE, "umgen_vq_finalize has not been called");
    const umgen_vq_config& cfg = e->cfg;
    const int L = cfg.n_levels;
    const long n_tok = (long)cfg.token_h * cfg.token_w;
    for (long i = 0; i < (long)n * n_tok; ++i)
        if (codes[i] < 0 || codes[i] >= cfg.n_embed) return e->fail(UMGEN_E_INVALID, "code %lld at flat index %ld is outside [0, %d)", (long long)codes[i], i, cfg.n_embed);
    VQCHK(e, hipSetDevice(cfg.device));
    for (int f = 0; f < n; ++f) {
        int H = cfg.token_h, W = cfg.token_w;
        VQCHK(e, hipMemcpyAsync(e->d_codes, codes + (long)f * n_tok, n_tok * sizeof(long long), hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(vq_embed_kernel, grid1d(n_tok * cfg.embed_dim), dim3(256), 0, e->stream, e->d_codes, e->emb, cfg.embed_dim, n_tok, e->h);
        conv(e, e->post_quant, e->h, H, W, e->t, false);                  // NormVQModel.decode: post_quant_conv
        conv(e, e->conv_in, e->t, H, W, e->x, false);                     // Decoder.forward
        res_block(e, e->mid1, H, W);
        attn_block(e, e->mid_attn, H, W);
        res_block(e, e->mid2, H, W);
        for (int lv = L - 1; lv >= 0; --lv) {
            const Level& u = e->up[lv];
            for (int b = 0; b <= cfg.num_res_blocks; ++b) {
                res_block(e, u.block[b], H, W);
                if (!u.attn.empty()) attn_block(e, u.attn[b], H, W);
            }
            if (u.has_up) {
                launch_upsample(e->stream, e->x, H, W, u.up.cin, e->h);
                H *= 2; W *= 2;
                conv(e, u.up, e->h, H, W, e->x, false);
            }
        }
        group_norm(e, e->norm_out, e->x, (long)H * W, true, e->h);
        conv(e, e->conv_out, e->h, H, W, e->t, false);
        launch_to_nchw(e->stream, e->t, (long)H * W, cfg.out_ch, e->conv_out.cout_pad, e->d_out);
        VQCHK(e, hipMemcpyAsync(out + (size_t)f * cfg.out_ch * H * W, e->d_out, (size_t)cfg.out_ch * H * W * 4, hipMemcpyDeviceToHost, e->stream));
        VQCHK(e, hipStreamSynchronize(e->stream));
    }
    VQCHK(e, hipGetLastError());
    return UMGEN_OK;
}

int umgen_vq_destroy(umgen_vq* e) {
    if (!e) return UMGEN_OK;
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    for (void* p : e->allocs) (void)hipFree(p);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return UMGEN_OK;
}

}  // extern "C"
